// trik_hsv_mask.hip -- the per-pixel detection mask as an output (DESIGN.md
// 4.16; trik_hsv_mask_batch): detectHsvPixel (WSEQ:171-179) of every pixel's
// s_rgb888hsv entry under range t of the pixel's frame, as one bit or one byte
// per pixel, a plane per range.  The ranges are six-tuples in device memory,
// shared by the batch or one set per frame, packed here by pack_range (the
// host's own definition); H, S, V are stripe_px::word_hsv's and the test is
// detect_packed: nothing of the arithmetic is restated, no table depends on a
// range.
//
// A workgroup takes a run of 8-pixel units of ONE frame (a multiple of the
// workgroup's 256 lanes, or the frame's last units).  Its lanes t < T pack the
// frame's ranges into LDS beside LUT43 / LUT255.  A lane then takes units u0 +
// lane, + 256, ...: one read of the unit, H, S and V of its 8 pixels once,
// whatever T is, and per range (its packed form in scalar registers) the 8
// results as bit i = pixel i of the unit.
//
//  mask_vec_kernel      input 16-byte aligned, output aligned to the store
//                       (mask_vec_ok).  Bits: width / 8 is a multiple of 4 and
//                       so is every run's first unit, so the four lanes of a
//                       quad hold bytes 4 q .. 4 q + 3 of one row: lane 4 q
//                       gathers them by three quad broadcasts and stores one
//                       32-bit word, 64 contiguous bytes per wave and range.
//                       Bytes: a lane stores its 8 bytes at once, 512
//                       contiguous bytes per wave and range.
//  mask_generic_kernel  every other placement: dword or byte loads
//                       (load_unit<.., 4> / <.., 1>), byte stores.
//
// Only mask bytes are stored, each once, by plain stores of whole values: pitch
// padding and the bytes between planes and between frames are never written.
#include <hip/hip_runtime.h>

#include "trik_hsv_internal.h"
#include "trik_hsv_pixel.h"
#include "trik_hsv_stripe_px.h"

// The vector kernel's stores: non-temporal (1) or plain (0); the A/B is
// profiles/mask/ab_nontemporal.txt.
#ifndef TRIK_HSV_MASK_NT
#define TRIK_HSV_MASK_NT 1
#endif

namespace trik_hsv {

namespace {

constexpr int kMkBlock = 256;
static_assert(kMkBlock == 256, "one lane per LUT entry; TRIK_HSV_MAX_RANGES lanes pack the ranges");
static_assert(TRIK_HSV_MAX_RANGES <= kMkBlock, "a lane per range packs it");
// workgroups a launch aims for (8 per CU, twice over) when the frames alone are fewer
constexpr int64_t kMkTargetBlocks = 4096;
// units a lane takes at least where the frame has them
constexpr int64_t kMkMinIters = 4;
// a launch holds fewer than 2^32 threads: larger batches go in several launches
constexpr int64_t kMkMaxLaunchBlocks = 0xFFFFFFFFll / kMkBlock;

struct MaskArgs : FrameView {
  int32_t n_ranges;
  int32_t segs;              // runs per frame
  uint32_t seg_units;        // units per run: a multiple of kMkBlock
  uint32_t units_per_frame;  // height * width / 8, a multiple of 16
  FastDiv units_per_row;     // width / 8, a multiple of 4
  const uint16_t* ranges;    // frame f's tuples at ranges + f * ranges_stride
  int64_t ranges_stride;     // uint16 elements; 0: one set for every frame
  uint8_t* out;
  int64_t out_frame_stride, out_plane_stride;
  int32_t out_row_pitch;
};

typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
template <typename T>
__device__ __forceinline__ void store_vec(uint8_t* p, T v) {
#if TRIK_HSV_MASK_NT
  __builtin_nontemporal_store(v, reinterpret_cast<T*>(p));
#else
  *reinterpret_cast<T*>(p) = v;
#endif
}

// the value lane `Q` of the caller's quad holds
template <int Q>
__device__ __forceinline__ uint32_t quad_bcast(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, Q * 0x55, 0xF, 0xF, false);  // quad_perm [Q, Q, Q, Q]
}

template <int LAYOUT, int ALIGN, int FORM, bool VEC>
__device__ __forceinline__ void mask_body(const MaskArgs& a) {
  __shared__ uint16_t l43[256], l255[256];
  __shared__ uint32_t pr_from[TRIK_HSV_MAX_RANGES], pr_to[TRIK_HSV_MAX_RANGES], pr_expect[TRIK_HSV_MAX_RANGES];
  const int tid = threadIdx.x;
  const uint32_t f = blockIdx.x / (uint32_t)a.segs, seg = blockIdx.x - f * (uint32_t)a.segs;
  const int T = a.n_ranges;

  // s_mult43_div, s_mult255_div (WSEQ:400-406) as frame_ranges_kernel builds
  // them, and this frame's ranges packed once
  l43[tid] = tid ? (uint16_t)((43u * 256u) / (uint32_t)tid) : (uint16_t)0;
  l255[tid] = tid ? (uint16_t)((255u * 256u) / (uint32_t)tid) : (uint16_t)0;
  if (tid < T) {
    const uint16_t* r = a.ranges + (int64_t)f * a.ranges_stride + 6 * tid;
    const PackedRange p = pack_range(r[0], r[1], r[2], r[3], r[4], r[5]);
    pr_from[tid] = p.from;
    pr_to[tid] = p.to;
    pr_expect[tid] = p.expect;
  }
  __syncthreads();

  const uint8_t* fr = frame_ptr(a, f);
  uint8_t* planes = a.out + (int64_t)f * a.out_frame_stride;  // plane 0 of the frame
  const uint32_t u0 = seg * a.seg_units, u1 = min(u0 + a.seg_units, a.units_per_frame);
  // u0, u1 and the units of a row are multiples of 4 and the stride one of 64:
  // a quad's lanes are in or out of an iteration together, with units 4 q ..
  // 4 q + 3 of one row
  for (uint32_t u = u0 + (uint32_t)tid; u < u1; u += kMkBlock) {
    const uint32_t row = fdiv(u, a.units_per_row), col = u - row * a.units_per_row.d;
    uint32_t w[4];
    load_unit<LAYOUT, ALIGN>(fr, a.height, a.line_length, (int)row, (int)col, w);
    uint32_t H[8], S[8], V[8];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const uint32_t wc = w[j] ^ 0xFF00FF00u;
      stripe_px::word_hsv<0>(w[j], wc, l43, l255, H[2 * j], S[2 * j], V[2 * j]);
      stripe_px::word_hsv<1>(w[j], wc, l43, l255, H[2 * j + 1], S[2 * j + 1], V[2 * j + 1]);
    }
    // the unit's byte (bits) or 8 bytes (bytes) of the row in plane 0
    uint8_t* dst = planes + (int64_t)row * a.out_row_pitch + (FORM == TRIK_HSV_MASK_BITS ? col : 8u * col);
    for (int t = 0; t < T; ++t, dst += a.out_plane_stride) {
      // the same in every lane: scalar registers
      PackedRange r;
      r.from = (uint32_t)__builtin_amdgcn_readfirstlane((int)pr_from[t]);
      r.to = (uint32_t)__builtin_amdgcn_readfirstlane((int)pr_to[t]);
      r.expect = (uint32_t)__builtin_amdgcn_readfirstlane((int)pr_expect[t]);
      if (FORM == TRIK_HSV_MASK_BITS) {
        uint32_t bits = 0;  // bit i: pixel 8 col + i, least significant first
#pragma unroll
        for (int i = 0; i < 8; ++i) bits |= detect_packed(H[i], S[i], V[i], r) ? 1u << i : 0u;
        if (VEC) {
          // byte k of the word: the unit of the quad's lane k
          const uint32_t word =
              bits | (quad_bcast<1>(bits) << 8) | (quad_bcast<2>(bits) << 16) | (quad_bcast<3>(bits) << 24);
          if ((tid & 3) == 0) store_vec<uint32_t>(dst, word);
        } else {
          dst[0] = (uint8_t)bits;
        }
      } else {
        uint32_t lo = 0, hi = 0;  // byte i: 0xFF where pixel 8 col + i is detected
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          lo |= detect_packed(H[i], S[i], V[i], r) ? 0xFFu << (8 * i) : 0u;
          hi |= detect_packed(H[4 + i], S[4 + i], V[4 + i], r) ? 0xFFu << (8 * i) : 0u;
        }
        if (VEC) {
          store_vec<u32x2>(dst, u32x2{lo, hi});
        } else {
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            dst[i] = (uint8_t)(lo >> (8 * i));
            dst[4 + i] = (uint8_t)(hi >> (8 * i));
          }
        }
      }
    }
  }
}

template <int LAYOUT, int FORM>
__global__ __launch_bounds__(kMkBlock) void mask_vec_kernel(MaskArgs a) {
  mask_body<LAYOUT, 16, FORM, true>(a);
}

// ALIGN 4: frames, stride and line length 4-byte aligned; 1: anything
template <int LAYOUT, int ALIGN, int FORM>
__global__ __launch_bounds__(kMkBlock) void mask_generic_kernel(MaskArgs a) {
  mask_body<LAYOUT, ALIGN, FORM, false>(a);
}

template <int LAYOUT, int FORM>
void launch_mask_form(bool vec, int align, unsigned blocks, hipStream_t s, const MaskArgs& a) {
  if (vec)
    hipLaunchKernelGGL((mask_vec_kernel<LAYOUT, FORM>), dim3(blocks), dim3(kMkBlock), 0, s, a);
  else if (align >= 4)
    hipLaunchKernelGGL((mask_generic_kernel<LAYOUT, 4, FORM>), dim3(blocks), dim3(kMkBlock), 0, s, a);
  else
    hipLaunchKernelGGL((mask_generic_kernel<LAYOUT, 1, FORM>), dim3(blocks), dim3(kMkBlock), 0, s, a);
}

template <int LAYOUT>
void launch_mask_layout(int form, bool vec, int align, unsigned blocks, hipStream_t s, const MaskArgs& a) {
  if (form == TRIK_HSV_MASK_BITS)
    launch_mask_form<LAYOUT, TRIK_HSV_MASK_BITS>(vec, align, blocks, s, a);
  else
    launch_mask_form<LAYOUT, TRIK_HSV_MASK_BYTES>(vec, align, blocks, s, a);
}

// the bits that must be zero for every frame address of the batch to be aligned
uintptr_t frame_align_bits(const TrikHsvFrameBatch& b) {
  uintptr_t bits = reinterpret_cast<uintptr_t>(b.frames) | (uintptr_t)b.line_length;
  if (b.n_frames > 1) bits |= (uintptr_t)b.frame_stride;  // (a single frame's stride is no address)
  return bits;
}

}  // namespace

// The vector kernel's condition: every 16-byte load address is 16-byte aligned
// (as launch_frame_ranges asks of its widest loads) and every store address a
// multiple of the store's width, 4 bytes for the bits and 8 for the bytes (the
// stride of a single frame or a single plane is no address).
bool mask_vec_ok(const TrikHsvFrameBatch& b, int n_ranges, const TrikHsvMaskOut& o) {
  uintptr_t bits = reinterpret_cast<uintptr_t>(o.out) | (uintptr_t)o.row_pitch;
  if (b.n_frames > 1) bits |= (uintptr_t)o.frame_stride;
  if (n_ranges > 1) bits |= (uintptr_t)o.plane_stride;
  const uintptr_t store = o.form == TRIK_HSV_MASK_BITS ? 4 : 8;
  return (frame_align_bits(b) & 15) == 0 && (bits & (store - 1)) == 0;
}

// b, the ranges' arguments and o validated, with n_frames, width and height > 0.
int launch_mask(const TrikHsvFrameBatch& b, const uint16_t* ranges, int n_ranges, int64_t ranges_stride,
                const TrikHsvMaskOut& o, hipStream_t s) {
  MaskArgs a = {frame_view(b)};
  if (b.n_frames <= 1) a.frame_stride = 0;  // (a single frame's stride is not validated)
  a.n_ranges = n_ranges;
  a.ranges = ranges;
  a.ranges_stride = ranges_stride;
  a.out = static_cast<uint8_t*>(o.out);
  a.out_frame_stride = b.n_frames <= 1 ? 0 : o.frame_stride;
  a.out_plane_stride = o.plane_stride;
  a.out_row_pitch = o.row_pitch;
  a.units_per_row = make_div((uint32_t)b.width / 8u);
  const int64_t units = (int64_t)b.height * (b.width / 8);  // < 2^27
  a.units_per_frame = (uint32_t)units;
  // runs: enough workgroups for the chip when the frames are few, each lane
  // with at least kMkMinIters units
  int64_t want = (kMkTargetBlocks + (int64_t)b.n_frames - 1) / b.n_frames;
  int64_t per_run = (units + want - 1) / want;
  if (per_run < kMkMinIters * kMkBlock) per_run = kMkMinIters * kMkBlock;
  per_run = (per_run + kMkBlock - 1) / kMkBlock * kMkBlock;
  a.seg_units = (uint32_t)per_run;
  a.segs = (int32_t)((units + per_run - 1) / per_run);
  const bool vec = mask_vec_ok(b, n_ranges, o);
  const int align = (frame_align_bits(b) & 3) == 0 ? 4 : 1;
  const int64_t per_launch = kMkMaxLaunchBlocks / a.segs;  // frames
  for (int64_t f0 = 0; f0 < b.n_frames; f0 += per_launch) {
    MaskArgs c = a;
    c.narrow(f0, b.n_frames - f0 < per_launch ? b.n_frames - f0 : per_launch);
    c.ranges = ranges + f0 * ranges_stride;
    c.out = a.out + f0 * a.out_frame_stride;
    const unsigned blocks = (unsigned)((int64_t)c.n_frames * a.segs);
    if (b.layout == TRIK_HSV_LAYOUT_YUYV)
      launch_mask_layout<TRIK_HSV_LAYOUT_YUYV>(o.form, vec, align, blocks, s, c);
    else
      launch_mask_layout<TRIK_HSV_LAYOUT_OV7670>(o.form, vec, align, blocks, s, c);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace trik_hsv
