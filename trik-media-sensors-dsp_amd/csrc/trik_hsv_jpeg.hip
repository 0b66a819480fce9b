// trik_hsv_jpeg.hip -- the ov7670 JPEG encoder, JENC =
// trik/ov7670/jpeg_encoder/include/internal/jpeg_encoder_reference.hpp.  The
// reference codes one data unit (DU: an 8x8 block of one component) after the
// other through a sequential bit writer; here every stage is parallel over
// DUs, words or bytes, and the bytes are the same:
//
//  jpeg_block_kernel  one thread per DU: getBlock (JENC:734-752), the AAN
//                     transform and the quantisation (JENC:402-513) with the
//                     reference's int truncations and separately rounded
//                     double operations, the zigzag reorder; writes the 64
//                     coefficients, the bits of the DU's AC part and its DC.
//  jpeg_scan_kernel   one workgroup per frame: the DC difference against the
//                     previous DU of the component gives each DU's bit length;
//                     their exclusive scan is each DU's first bit.
//  jpeg_zero_kernel   zeroes the words of the unstuffed segment the frame uses.
//  jpeg_emit_kernel   one thread per DU: processDU's symbols (JENC:653-711)
//                     packed MSB first at the DU's bit offset.  A word inside
//                     the DU's span has one owner and is stored; the first and
//                     the last word are shared with the neighbours and are
//                     OR-ed in atomically.
//  jpeg_count_kernel  0xFF bytes per 1024-byte chunk of the unstuffed segment
//                     (the fill bits, JENC:838-847, OR-ed into its last byte
//                     on the fly: 8 of them when the segment ends aligned).
//  jpeg_sizes_kernel  one workgroup per frame: the chunks' exclusive scan and
//                     the stream's length.
//  jpeg_stuff_kernel  scatters every byte to its place after the header, a
//                     0x00 after each 0xFF (JENC:366-379), the header and EOI.
//                     A frame longer than the capacity is not written at all.
//
// No double operation here may be fused: the C674x rounds every multiply and
// add, and a fused multiply-add changes low bits that a truncation or the
// final rounding then turns into another coefficient.  Contraction is off for
// the whole file (and the Makefile compiles it with -ffp-contract=off).
#include <hip/hip_runtime.h>

#include "trik_hsv_internal.h"

#pragma clang fp contract(off)

namespace trik_hsv {

namespace {

constexpr int kDuBlock = 256;     // threads of the per-DU kernels
constexpr int kFrameBlock = 1024; // threads of the per-frame scans
constexpr int kChunkWords = kJpegChunkBytes / 4;
static_assert(kChunkWords == 256, "a chunk is one word per thread of a 256-thread workgroup");

// position in the zigzag scan of natural index i (T.81 figure A.6)
static __device__ const uint8_t kZigZag[64] = {0,  1,  5,  6,  14, 15, 27, 28, 2,  4,  7,  13, 16, 26, 29, 42,
                                               3,  8,  12, 17, 25, 30, 41, 43, 9,  11, 18, 24, 31, 40, 44, 53,
                                               10, 19, 23, 32, 39, 45, 52, 54, 20, 22, 33, 38, 46, 51, 55, 60,
                                               21, 34, 37, 47, 50, 56, 59, 61, 35, 36, 48, 49, 57, 58, 62, 63};

// One AAN pass over d[0], d[S], ..., d[7 S] (JENC:411-454 with S = 1, 459-502
// with S = 8): integer sums and differences, one double multiply or add per
// rotated term, every store truncated toward zero.
template <int S>
__device__ __forceinline__ void aan_pass(int* d) {
  const int t0 = d[0] + d[7 * S], t7 = d[0] - d[7 * S];
  const int t1 = d[1 * S] + d[6 * S], t6 = d[1 * S] - d[6 * S];
  const int t2 = d[2 * S] + d[5 * S], t5 = d[2 * S] - d[5 * S];
  const int t3 = d[3 * S] + d[4 * S], t4 = d[3 * S] - d[4 * S];
  int t10 = t0 + t3, t11 = t1 + t2, t12 = t1 - t2;
  const int t13 = t0 - t3;
  d[0] = t10 + t11;
  d[4 * S] = t10 - t11;
  const double z1 = (double)(t12 + t13) * 0.707106781;
  d[2 * S] = (int)((double)t13 + z1);
  d[6 * S] = (int)((double)t13 - z1);
  t10 = t4 + t5;
  t11 = t5 + t6;
  t12 = t6 + t7;
  const double z5 = (double)(t10 - t12) * 0.382683433;
  const double m2 = 0.541196100 * (double)t10;
  const double z2 = m2 + z5;
  const double m4 = 1.306562965 * (double)t12;
  const double z4 = m4 + z5;
  const double z3 = (double)t11 * 0.707106781;
  const double z11 = (double)t7 + z3, z13 = (double)t7 - z3;
  d[5 * S] = (int)(z13 + z2);
  d[3 * S] = (int)(z13 - z2);
  d[1 * S] = (int)(z11 + z4);
  d[7 * S] = (int)(z11 - z4);
}

__device__ __forceinline__ int bit_length(int v) {  // category (JENC:317-349): bit length of |v|
  return 32 - __clz(v < 0 ? -v : v);  // (__clz(0) is 32)
}

struct DuIndex {
  uint32_t frame, du, comp;
  int bx, by;
};
__device__ __forceinline__ DuIndex du_index(const JpegArgs& a, uint32_t gid) {
  DuIndex x;
  x.frame = gid / a.n_du;
  x.du = gid - x.frame * a.n_du;
  const uint32_t blk = x.du / (uint32_t)a.ncomp;
  x.comp = x.du - blk * (uint32_t)a.ncomp;
  x.by = (int)(blk / (uint32_t)a.blocks_w);
  x.bx = (int)(blk - (uint32_t)x.by * (uint32_t)a.blocks_w);
  return x;
}

__global__ __launch_bounds__(kDuBlock) void jpeg_block_kernel(JpegArgs a, JpegDivisors dv) {
  __shared__ uint8_t ac_len[2][256];
  for (int i = threadIdx.x; i < 512; i += kDuBlock) (&ac_len[0][0])[i] = (&a.huff->ac_len[0][0])[i];
  __syncthreads();
  const uint32_t gid = blockIdx.x * (uint32_t)kDuBlock + threadIdx.x;
  if (gid >= (uint32_t)a.n_frames * a.n_du) return;
  const DuIndex x = du_index(a, gid);
  const int t = x.comp ? 1 : 0;

  // the DU's pixels minus 128.  Y: the luma bytes.  U, V: pixel c takes pair
  // c / 2 of the chroma row, U its odd byte, V its even byte (JENC:745-748).
  int d[64];
  const int64_t ll = a.line_length;
  const uint8_t* p = frame_ptr(a, x.frame) + (x.comp ? ll * a.height : 0) +
                     (int64_t)x.by * 8 * ll + x.bx * 8;
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    const uint8_t* q = p + r * ll;  // (8 by + r < height, 8 bx + 7 < width <= line_length)
    uint32_t w0, w1;
    if (a.aligned4) {
      w0 = *reinterpret_cast<const uint32_t*>(q);
      w1 = *reinterpret_cast<const uint32_t*>(q + 4);
    } else {
      w0 = (uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16) | ((uint32_t)q[3] << 24);
      w1 = (uint32_t)q[4] | ((uint32_t)q[5] << 8) | ((uint32_t)q[6] << 16) | ((uint32_t)q[7] << 24);
    }
    if (x.comp == 1) {  // odd bytes, each twice
      w0 = ((w0 >> 8) & 0x00FF00FFu) * 0x0101u;
      w1 = ((w1 >> 8) & 0x00FF00FFu) * 0x0101u;
    } else if (x.comp == 2) {  // even bytes, each twice
      w0 = (w0 & 0x00FF00FFu) * 0x0101u;
      w1 = (w1 & 0x00FF00FFu) * 0x0101u;
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      d[8 * r + c] = (int)((w0 >> (8 * c)) & 0xFFu) - 128;
      d[8 * r + 4 + c] = (int)((w1 >> (8 * c)) & 0xFFu) - 128;
    }
  }
#pragma unroll
  for (int r = 0; r < 8; ++r) aan_pass<1>(d + 8 * r);
#pragma unroll
  for (int c = 0; c < 8; ++c) aan_pass<8>(d + c);

  // quantise (one multiply, round to nearest even: the reference's double2int)
  // and reorder: z[zigzag position] (JENC:505-510, 667-669)
  int z[64];
#pragma unroll
  for (int i = 0; i < 64; ++i) {
    const double f = t ? dv.fd[1][i] : dv.fd[0][i];
    z[kZigZag[i]] = __double2int_rn((double)d[i] * f);
  }

  uint32_t* out = reinterpret_cast<uint32_t*>(a.coeffs + (int64_t)gid * 64);
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    uint4 v;
    v.x = ((uint32_t)z[8 * i + 0] & 0xFFFFu) | ((uint32_t)z[8 * i + 1] << 16);
    v.y = ((uint32_t)z[8 * i + 2] & 0xFFFFu) | ((uint32_t)z[8 * i + 3] << 16);
    v.z = ((uint32_t)z[8 * i + 4] & 0xFFFFu) | ((uint32_t)z[8 * i + 5] << 16);
    v.w = ((uint32_t)z[8 * i + 6] & 0xFFFFu) | ((uint32_t)z[8 * i + 7] << 16);
    reinterpret_cast<uint4*>(out)[i] = v;
  }

  // the bits of the AC part (JENC:681-708): run / 16 ZRL codes, the run-size
  // code and the magnitude bits per non-zero coefficient, EOB after trailing zeros
  uint32_t bits = 0;
  int run = 0;
#pragma unroll
  for (int k = 1; k < 64; ++k) {
    // the coefficient as the emit pass will read it back (16 bits)
    const int v = (int)(int16_t)z[k];
    if (v == 0) {
      ++run;
    } else {
      const int cat = bit_length(v);
      bits += (uint32_t)(run >> 4) * ac_len[t][0xF0] + ac_len[t][(((run & 15) << 4) + cat) & 0xFF] + (uint32_t)cat;
      run = 0;
    }
  }
  if (run) bits += ac_len[t][0x00];
  a.info[gid] = bits | ((uint32_t)z[0] << 16);
}

// Inclusive scan of v over the NT threads of the workgroup; *total = the sum.
// Ends with a barrier, so it can be called again at once.
template <int NT>
__device__ __forceinline__ uint32_t block_scan(uint32_t v, uint32_t* wave_sums, uint32_t* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const uint32_t o = (uint32_t)__shfl_up((int)v, off, 64);
    if (lane >= off) v += o;
  }
  if (lane == 63) wave_sums[wave] = v;
  __syncthreads();
  uint32_t before = 0, all = 0;
#pragma unroll
  for (int w = 0; w < NT / 64; ++w) {
    const uint32_t s = wave_sums[w];
    if (w < wave) before += s;
    all += s;
  }
  __syncthreads();
  *total = all;
  return v + before;
}

__global__ __launch_bounds__(kFrameBlock) void jpeg_scan_kernel(JpegArgs a) {
  __shared__ uint32_t wave_sums[kFrameBlock / 64];
  __shared__ uint8_t dc_len[2][12];
  if (threadIdx.x < 24) (&dc_len[0][0])[threadIdx.x] = (&a.huff->dc_len[0][0])[threadIdx.x];
  __syncthreads();
  const uint32_t f = blockIdx.x;
  const uint32_t* info = a.info + (uint64_t)f * a.n_du;
  unsigned long long* bitoff = a.bitoff + (uint64_t)f * a.n_du;
  unsigned long long carry = 0;
  for (uint32_t base = 0; base < a.n_du; base += kFrameBlock) {
    const uint32_t i = base + threadIdx.x;
    uint32_t len = 0;
    if (i < a.n_du) {
      const uint32_t inf = info[i];
      // the predictor is the previous DU of the component, 0 at the frame's first block (JENC:820-822)
      const int prev = i >= (uint32_t)a.ncomp ? (int)(int16_t)(info[i - a.ncomp] >> 16) : 0;
      const int diff = (int)(int16_t)(inf >> 16) - prev;
      const int cat = min(bit_length(diff), 11);
      const int t = (i % (uint32_t)a.ncomp) ? 1 : 0;
      len = (inf & 0xFFFFu) + dc_len[t][cat] + (uint32_t)cat;
    }
    uint32_t tile = 0;
    const uint32_t incl = block_scan<kFrameBlock>(len, wave_sums, &tile);
    if (i < a.n_du) bitoff[i] = carry + incl - len;
    carry += tile;
  }
  if (threadIdx.x == 0) a.total[f] = carry;
}

// the bytes of a frame's unstuffed segment: its bits and 1..8 fill bits
__device__ __forceinline__ uint64_t segment_bytes(unsigned long long total_bits) { return total_bits / 8 + 1; }

__global__ __launch_bounds__(256) void jpeg_zero_kernel(JpegArgs a) {
  const uint32_t f = blockIdx.y;
  uint64_t n = a.total[f] / 32 + 2;  // the word of the last byte, and one more
  if (n > a.words_per_frame) n = a.words_per_frame;
  uint32_t* w = a.words + (uint64_t)f * a.words_per_frame;
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) w[i] = 0u;
}

// The sequential bit writer of one DU (writeBits, JENC:358-387, without the
// stuffing): bits gather MSB first in acc; a full word is flushed.
struct BitSink {
  uint32_t* words;
  uint64_t widx;
  unsigned long long acc;
  int nacc;
  bool first;
  __device__ __forceinline__ void put(uint32_t val, int len) {
    acc = (acc << len) | val;
    nacc += len;
    if (nacc >= 32) {
      nacc -= 32;
      const uint32_t w = (uint32_t)(acc >> nacc);
      if (first) {  // bits before the DU's first one belong to the DU before it
        atomicOr(&words[widx], w);
        first = false;
      } else {
        words[widx] = w;
      }
      ++widx;
      acc &= (1ull << nacc) - 1ull;
    }
  }
  __device__ __forceinline__ void finish() {
    if (nacc > 0) atomicOr(&words[widx], (uint32_t)(acc << (32 - nacc)));
  }
};

__device__ __forceinline__ uint32_t magnitude_bits(int v, int cat) {  // JENC:329-343
  return (uint32_t)(v > 0 ? v : (1 << cat) - 1 + v);
}

__global__ __launch_bounds__(kDuBlock) void jpeg_emit_kernel(JpegArgs a) {
  __shared__ uint16_t ac_code[2][256];
  __shared__ uint8_t ac_len[2][256];
  __shared__ uint16_t dc_code[2][12];
  __shared__ uint8_t dc_len[2][12];
  for (int i = threadIdx.x; i < 512; i += kDuBlock) {
    (&ac_code[0][0])[i] = (&a.huff->ac_code[0][0])[i];
    (&ac_len[0][0])[i] = (&a.huff->ac_len[0][0])[i];
  }
  if (threadIdx.x < 24) {
    (&dc_code[0][0])[threadIdx.x] = (&a.huff->dc_code[0][0])[threadIdx.x];
    (&dc_len[0][0])[threadIdx.x] = (&a.huff->dc_len[0][0])[threadIdx.x];
  }
  __syncthreads();
  const uint32_t gid = blockIdx.x * (uint32_t)kDuBlock + threadIdx.x;
  if (gid >= (uint32_t)a.n_frames * a.n_du) return;
  const DuIndex x = du_index(a, gid);
  const int t = x.comp ? 1 : 0;
  const unsigned long long pos = a.bitoff[gid];
  BitSink sink;
  sink.words = a.words + (uint64_t)x.frame * a.words_per_frame;
  sink.widx = pos >> 5;
  sink.acc = 0;
  sink.nacc = (int)(pos & 31);
  sink.first = true;

  const uint4* src = reinterpret_cast<const uint4*>(a.coeffs + (int64_t)gid * 64);
  int run = 0;
#pragma unroll 1
  for (int i = 0; i < 8; ++i) {
    const uint4 q = src[i];
    const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int v = (int)(int16_t)(w[j >> 1] >> (16 * (j & 1)));
      if (i == 0 && j == 0) {  // DC (JENC:670-679)
        const int prev = x.du >= (uint32_t)a.ncomp ? (int)(int16_t)(a.info[gid - a.ncomp] >> 16) : 0;
        const int diff = v - prev;
        const int cat = min(bit_length(diff), 11);
        sink.put(dc_code[t][cat], dc_len[t][cat]);
        if (cat) sink.put(magnitude_bits(diff, cat), cat);
      } else if (v == 0) {
        ++run;
      } else {  // JENC:692-705
        for (; run >= 16; run -= 16) sink.put(ac_code[t][0xF0], ac_len[t][0xF0]);
        const int cat = bit_length(v);
        const int sym = ((run << 4) + cat) & 0xFF;
        sink.put(ac_code[t][sym], ac_len[t][sym]);
        sink.put(magnitude_bits(v, cat) & ((1u << cat) - 1u), cat);
        run = 0;
      }
    }
  }
  if (run) sink.put(ac_code[t][0x00], ac_len[t][0x00]);  // EOB, unless coefficient 63 is non-zero
  sink.finish();
}

// Word widx of the frame's unstuffed segment of n_bytes bytes, byte 4 widx in
// its top byte, with the fill bits (ones up to the byte's end: 8 of them when
// the bits end aligned) in the last byte; 0 past the segment.
__device__ __forceinline__ uint32_t segment_word(const uint32_t* words, uint64_t widx, uint64_t n_bytes,
                                                 unsigned long long total_bits) {
  if (4 * widx >= n_bytes) return 0u;
  uint32_t w = words[widx];
  const uint64_t last = n_bytes - 1;
  if ((last >> 2) == widx) {
    const uint32_t fill = (1u << (8 - (int)(total_bits & 7))) - 1u;
    w |= fill << (24 - 8 * (int)(last & 3));
  }
  return w;
}

// 0xFF bytes among the word's bytes inside the segment
__device__ __forceinline__ uint32_t count_ff(uint32_t w, uint64_t widx, uint64_t n_bytes) {
  uint32_t n = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (4 * widx + k < n_bytes && ((w >> (24 - 8 * k)) & 0xFFu) == 0xFFu) ++n;
  return n;
}

__global__ __launch_bounds__(256) void jpeg_count_kernel(JpegArgs a) {
  __shared__ uint32_t wave_sums[4];
  const uint32_t f = blockIdx.y;
  const unsigned long long total = a.total[f];
  const uint64_t n_bytes = segment_bytes(total);
  const uint64_t chunks = (n_bytes + kJpegChunkBytes - 1) / kJpegChunkBytes;  // <= chunks_per_frame
  const uint32_t* words = a.words + (uint64_t)f * a.words_per_frame;
  for (uint64_t c = blockIdx.x; c < chunks; c += gridDim.x) {
    const uint64_t widx = c * kChunkWords + threadIdx.x;
    const uint32_t n = count_ff(segment_word(words, widx, n_bytes, total), widx, n_bytes);
    uint32_t sum = 0;
    (void)block_scan<256>(n, wave_sums, &sum);
    if (threadIdx.x == 0) a.chunk_ff[(uint64_t)f * a.chunks_per_frame + c] = sum;
  }
}

__global__ __launch_bounds__(kFrameBlock) void jpeg_sizes_kernel(JpegArgs a, int32_t header_size) {
  __shared__ uint32_t wave_sums[kFrameBlock / 64];
  const uint32_t f = blockIdx.x;
  const uint64_t n_bytes = segment_bytes(a.total[f]);
  const uint32_t chunks = (uint32_t)((n_bytes + kJpegChunkBytes - 1) / kJpegChunkBytes);
  uint32_t* ff = a.chunk_ff + (uint64_t)f * a.chunks_per_frame;
  uint32_t carry = 0;
  for (uint32_t base = 0; base < chunks; base += kFrameBlock) {
    const uint32_t i = base + threadIdx.x;
    const uint32_t n = i < chunks ? ff[i] : 0u;
    uint32_t tile = 0;
    const uint32_t incl = block_scan<kFrameBlock>(n, wave_sums, &tile);
    if (i < chunks) ff[i] = carry + incl - n;
    carry += tile;
  }
  // header, the segment with a 0x00 after every 0xFF, EOI
  if (threadIdx.x == 0) a.sizes[f] = (uint32_t)header_size + (uint32_t)n_bytes + carry + 2u;
}

__global__ __launch_bounds__(256) void jpeg_stuff_kernel(JpegArgs a, JpegHeader hd) {
  __shared__ uint32_t wave_sums[4];
  const uint32_t f = blockIdx.y;
  const uint32_t size = a.sizes[f];
  if (!a.out || (int64_t)size > a.out_capacity) return;  // sizes only, or the stream does not fit: nothing written
  uint8_t* out = a.out + (int64_t)f * a.out_stride;
  if (blockIdx.x == 0) {
    for (int i = threadIdx.x; i < hd.size; i += 256) out[i] = hd.bytes[i];
    if (threadIdx.x == 0) {
      out[size - 2] = 0xFF;
      out[size - 1] = 0xD9;
    }
  }
  const unsigned long long total = a.total[f];
  const uint64_t n_bytes = segment_bytes(total);
  const uint64_t chunks = (n_bytes + kJpegChunkBytes - 1) / kJpegChunkBytes;
  const uint32_t* words = a.words + (uint64_t)f * a.words_per_frame;
  const uint32_t* ff = a.chunk_ff + (uint64_t)f * a.chunks_per_frame;
  for (uint64_t c = blockIdx.x; c < chunks; c += gridDim.x) {
    const uint64_t widx = c * kChunkWords + threadIdx.x;
    const uint32_t w = segment_word(words, widx, n_bytes, total);
    const uint32_t n = count_ff(w, widx, n_bytes);
    uint32_t sum = 0;
    const uint32_t incl = block_scan<256>(n, wave_sums, &sum);
    // byte j of the segment goes to header + j + (0xFF bytes before it)
    uint8_t* dst = out + hd.size + 4 * widx + ff[c] + (incl - n);
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (4 * widx + k < n_bytes) {
        const uint32_t b = (w >> (24 - 8 * k)) & 0xFFu;
        *dst++ = (uint8_t)b;
        if (b == 0xFFu) *dst++ = 0;
      }
  }
}

}  // namespace

int launch_jpeg(const JpegArgs& a, const JpegDivisors& d, const JpegHeader& hd, hipStream_t s) {
  if (a.n_frames <= 0 || a.n_du == 0) return hipSuccess;
  const uint64_t dus = (uint64_t)a.n_frames * a.n_du;
  if (dus > 0x7FFFFFFFull) return hipErrorInvalidValue;
  const unsigned du_blocks = (unsigned)((dus + kDuBlock - 1) / kDuBlock);
  const unsigned per_frame = a.chunks_per_frame < 128u ? a.chunks_per_frame : 128u;
  const dim3 spread(per_frame, (unsigned)a.n_frames);
#define JPEG_LAUNCH(kernel, grid, block, ...)                      \
  do {                                                             \
    hipLaunchKernelGGL(kernel, grid, dim3(block), 0, s, __VA_ARGS__); \
    const hipError_t e = hipGetLastError();                        \
    if (e != hipSuccess) return e;                                 \
  } while (0)
  JPEG_LAUNCH(jpeg_block_kernel, dim3(du_blocks), kDuBlock, a, d);
  JPEG_LAUNCH(jpeg_scan_kernel, dim3((unsigned)a.n_frames), kFrameBlock, a);
  JPEG_LAUNCH(jpeg_zero_kernel, spread, 256, a);
  JPEG_LAUNCH(jpeg_emit_kernel, dim3(du_blocks), kDuBlock, a);
  JPEG_LAUNCH(jpeg_count_kernel, spread, 256, a);
  JPEG_LAUNCH(jpeg_sizes_kernel, dim3((unsigned)a.n_frames), kFrameBlock, a, hd.size);
  JPEG_LAUNCH(jpeg_stuff_kernel, spread, 256, a, hd);
#undef JPEG_LAUNCH
  return hipSuccess;
}

}  // namespace trik_hsv
