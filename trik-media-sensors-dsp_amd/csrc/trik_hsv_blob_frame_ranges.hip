// trik_hsv_blob_frame_ranges.hip -- the multi-blob sensor's metapixel bitmaps
// with HSV ranges per frame, read from device memory (DESIGN.md 4.11;
// trik_hsv_blob_frame_ranges_batch).  BMB, CLU as in trik_hsv_blob.hip.
//
//  blob_meta_frame_ranges_kernel   table-free: no table depends on a range, so
//                        nothing is built per range set.  A wave takes a job: a
//                        run of 16-metapixel units of ONE frame.  Its lanes t <
//                        T read that frame's six-tuples and pack them
//                        (pack_range, the host's own definition); a range is
//                        then read out of lane t's registers into scalar ones
//                        (v_readlane) when it is tested.  Per unit, four lanes
//                        per metapixel, one per pixel row of it and 4 pixels
//                        each: one read of the frame and one H, S, V per pixel
//                        (stripe_px::word_hsv over the workgroup's LUT43 /
//                        LUT255, WSEQ:181-249) whatever T is -- the 12 values
//                        stay in registers across the loop over the groups of
//                        4 ranges (detect_packed, WSEQ:171-179), whose counts
//                        sit side by side in the byte lanes of one register
//                        (0..16 each: no carry crosses a lane; BMB:171-190),
//                        summed over the four rows with two xor-shuffles.  A
//                        bitmap byte is count > 2 (CLU:185-186).
//
// The clusterer (blob_ccl_kernel) then runs over the (frame, range) slots as
// for trik_hsv_blob_batch_ranges.
#include <hip/hip_runtime.h>

#include "trik_hsv_internal.h"
#include "trik_hsv_pixel.h"
#include "trik_hsv_stripe_px.h"

namespace trik_hsv {

namespace {

constexpr int kBfrBlock = 256;
constexpr int kBfrWaves = kBfrBlock / 64;
static_assert(kBfrBlock == 256, "one lane per LUT entry");
static_assert(TRIK_HSV_MAX_RANGES <= 64, "a wave's lanes hold a frame's packed ranges");
constexpr int kBfrUnit = 16;           // metapixels a wave takes per step: 64 lanes / 4 rows
constexpr int kBfrGroup = 4;           // ranges per register of counts
constexpr uint32_t kNeverExpect = 8u;  // detect_packed's `out` has 3 bits: no pixel matches
// jobs a launch aims for (8 waves per SIMD, twice over) when the frames alone are fewer
constexpr int64_t kBfrTargetJobs = 16384;

struct BlobFrameRangesArgs : FrameView {
  int32_t n_ranges;
  FastDiv per_row;         // bw
  uint32_t cells;          // bw * bh
  uint32_t units;          // ceil(cells / 16): a frame's units
  uint32_t job_units;      // units per job
  FastDiv jobs_per_frame;  // ceil(units / job_units)
  uint32_t jobs;           // n_frames * jobs_per_frame
  const uint16_t* ranges;  // [n_frames][n_ranges][6]
  uint8_t* meta;           // [n_frames][n_ranges][bh][bw]
};

// The two YUYV words (Y0 U Y1 V) of pixels 4 mc .. 4 mc + 3 of a row.  ALIGN 8:
// one 8-byte load (YUYV; the planes take a dword each, the widest a lane of 4
// pixels has); 4: dword loads; 1: bytes through fetch_yuv.  Every byte lies
// inside the row.
template <int LAYOUT, int ALIGN>
__device__ __forceinline__ void load_quad(const uint8_t* fr, int height, int line_length, int row, int mc,
                                          uint32_t& w0, uint32_t& w1) {
  if (ALIGN == 1) {
    uint32_t w[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      int y0, y1, u, v, u1, v1;
      fetch_yuv(fr, height, line_length, LAYOUT, row, 4 * mc + 2 * k, y0, u, v);
      fetch_yuv(fr, height, line_length, LAYOUT, row, 4 * mc + 2 * k + 1, y1, u1, v1);
      w[k] = (uint32_t)y0 | ((uint32_t)u << 8) | ((uint32_t)y1 << 16) | ((uint32_t)v << 24);
    }
    w0 = w[0];
    w1 = w[1];
  } else if (LAYOUT == TRIK_HSV_LAYOUT_YUYV) {
    const uint8_t* p = fr + (int64_t)row * line_length + (int64_t)mc * 8;
    if (ALIGN == 8) {
      const uint2 v = *reinterpret_cast<const uint2*>(p);
      w0 = v.x;
      w1 = v.y;
    } else {
      w0 = reinterpret_cast<const uint32_t*>(p)[0];
      w1 = reinterpret_cast<const uint32_t*>(p)[1];
    }
  } else {
    const uint8_t* py = fr + (int64_t)row * line_length + (int64_t)mc * 4;
    const uint8_t* pc = py + (int64_t)line_length * height;
    stripe_px::ov7670_words(*reinterpret_cast<const uint32_t*>(py), *reinterpret_cast<const uint32_t*>(pc), w0, w1);
  }
}

// The counts of NR ranges from range g0 on among the lane's 4 pixels, range
// g0 + k in byte lane k.  The ranges come out of the registers of lanes g0 + k
// (pf, pt, pe: the frame's packed ranges, one per lane); ranges past the
// frame's last never match.
template <int NR>
__device__ __forceinline__ uint32_t count_group(const uint32_t H[4], const uint32_t S[4], const uint32_t V[4],
                                                uint32_t pf, uint32_t pt, uint32_t pe, int g0, int T) {
  uint32_t cnt = 0;
#pragma unroll
  for (int k = 0; k < NR; ++k) {
    const bool live = g0 + k < T;         // (uniform)
    const int src = live ? g0 + k : g0;   // (g0 < T)
    PackedRange r;
    r.from = (uint32_t)__builtin_amdgcn_readlane((int)pf, src);
    r.to = (uint32_t)__builtin_amdgcn_readlane((int)pt, src);
    r.expect = live ? (uint32_t)__builtin_amdgcn_readlane((int)pe, src) : kNeverExpect;
#pragma unroll
    for (int px = 0; px < 4; ++px) cnt += detect_packed(H[px], S[px], V[px], r) ? (1u << (8 * k)) : 0u;
  }
  return cnt;
}

template <int LAYOUT, int ALIGN>
__global__ __launch_bounds__(kBfrBlock) void blob_meta_frame_ranges_kernel(BlobFrameRangesArgs a) {
  __shared__ uint16_t l43[256], l255[256];
  const int tid = threadIdx.x, lane = tid & 63;
  // s_mult43_div, s_mult255_div (WSEQ:400-406), as frame_ranges_kernel builds them
  l43[tid] = tid ? (uint16_t)((43u * 256u) / (uint32_t)tid) : (uint16_t)0;
  l255[tid] = tid ? (uint16_t)((255u * 256u) / (uint32_t)tid) : (uint16_t)0;
  __syncthreads();

  const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane(tid >> 6);
  const int T = a.n_ranges;
  const int rr = lane & 3;                    // the lane's pixel row of its metapixel
  const uint32_t q = (uint32_t)(lane >> 2);  // its metapixel of the unit
  const uint32_t bw = a.per_row.d;
  // jobs over the grid's waves; a job lies inside one frame, so all of this is wave-uniform
  for (uint32_t j = blockIdx.x * kBfrWaves + wave; j < a.jobs; j += gridDim.x * kBfrWaves) {
    const uint32_t f = fdiv(j, a.jobs_per_frame), part = j - f * a.jobs_per_frame.d;
    // lane t packs range t of this frame (lanes past T - 1: the last one again, never read)
    const uint16_t* six = a.ranges + ((int64_t)f * T + min(lane, T - 1)) * 6;
    const PackedRange p = pack_range(six[0], six[1], six[2], six[3], six[4], six[5]);
    const uint8_t* fr = frame_ptr(a, f);
    uint8_t* out = a.meta + (int64_t)f * T * a.cells;  // slot (f, 0)'s bitmap
    const uint32_t u0 = part * a.job_units, u1 = min(u0 + a.job_units, a.units);
    // the lane's 4 pixels of unit u (only a frame's last unit has lanes past
    // its end: they read its last metapixel and write nothing)
    auto load_unit = [&](uint32_t u, uint32_t& w0, uint32_t& w1) {
      const uint32_t remc = min(u * kBfrUnit + q, a.cells - 1);
      const uint32_t mr = fdiv(remc, a.per_row), mc = remc - mr * bw;
      load_quad<LAYOUT, ALIGN>(fr, a.height, a.line_length, (int)(4 * mr) + rr, (int)mc, w0, w1);
    };
    uint32_t n0, n1;  // the next unit's words, in flight while this unit is worked on
    load_unit(u0, n0, n1);
    for (uint32_t u = u0; u < u1; ++u) {
      const uint32_t rem = u * kBfrUnit + q;  // the metapixel, in the frame's raster order
      const bool valid = rem < a.cells;
      const uint32_t w0 = n0, w1 = n1;
      load_unit(min(u + 1, u1 - 1), n0, n1);  // (past the job's last unit: that unit again, unused)
      uint32_t H[4], S[4], V[4];
      stripe_px::word_hsv<0>(w0, w0 ^ 0xFF00FF00u, l43, l255, H[0], S[0], V[0]);
      stripe_px::word_hsv<1>(w0, w0 ^ 0xFF00FF00u, l43, l255, H[1], S[1], V[1]);
      stripe_px::word_hsv<0>(w1, w1 ^ 0xFF00FF00u, l43, l255, H[2], S[2], V[2]);
      stripe_px::word_hsv<1>(w1, w1 ^ 0xFF00FF00u, l43, l255, H[3], S[3], V[3]);
      // groups of 4 ranges; a last single range (one calibration per camera:
      // T = 1) takes the one-range form, a quarter of the tests
      for (int g0 = 0; g0 < T; g0 += kBfrGroup) {
        const int live = min(T - g0, kBfrGroup);  // (uniform)
        uint32_t cnt = live == 1 ? count_group<1>(H, S, V, p.from, p.to, p.expect, g0, T)
                                 : count_group<kBfrGroup>(H, S, V, p.from, p.to, p.expect, g0, T);
        cnt += __shfl_xor(cnt, 1, 64);
        cnt += __shfl_xor(cnt, 2, 64);
        if (rr == 0 && valid) {
#pragma unroll
          for (int k = 0; k < kBfrGroup; ++k)
            if (k < live) out[(int64_t)(g0 + k) * a.cells + rem] = ((cnt >> (8 * k)) & 0xFFu) > 2 ? 1 : 0;
        }
      }
    }
  }
}

template <int LAYOUT>
void launch_layout(int align, unsigned blocks, hipStream_t s, const BlobFrameRangesArgs& a) {
  if constexpr (LAYOUT == TRIK_HSV_LAYOUT_YUYV) {  // (the planes' widest load is the dword)
    if (align == 8) {
      hipLaunchKernelGGL((blob_meta_frame_ranges_kernel<LAYOUT, 8>), dim3(blocks), dim3(kBfrBlock), 0, s, a);
      return;
    }
  }
  if (align >= 4)
    hipLaunchKernelGGL((blob_meta_frame_ranges_kernel<LAYOUT, 4>), dim3(blocks), dim3(kBfrBlock), 0, s, a);
  else
    hipLaunchKernelGGL((blob_meta_frame_ranges_kernel<LAYOUT, 1>), dim3(blocks), dim3(kBfrBlock), 0, s, a);
}

}  // namespace

int launch_blob_meta_frame_ranges(const BlobArgs& b, const uint16_t* ranges, int n_ranges, hipStream_t s) {
  if (b.n_frames <= 0 || b.width <= 0 || b.height <= 0) return hipSuccess;
  const int bw = b.width >> 2, bh = b.height >> 2;
  const int64_t cells = (int64_t)bw * bh;
  if (cells <= 0 || cells >= (1ll << 31) - kBfrUnit || !ranges || !b.meta || n_ranges < 1 ||
      n_ranges > TRIK_HSV_MAX_RANGES)
    return hipErrorInvalidValue;
  BlobFrameRangesArgs a = {static_cast<const FrameView&>(b)};
  if (b.n_frames <= 1) a.frame_stride = 0;  // (a single frame's stride is not validated: it counts as aligned)
  a.n_ranges = n_ranges;
  a.per_row = make_div((uint32_t)bw);
  a.cells = (uint32_t)cells;
  a.units = (uint32_t)((cells + kBfrUnit - 1) / kBfrUnit);
  // jobs: whole frames when they alone fill the chip, else a frame in parts
  int64_t per_job = (int64_t)b.n_frames * a.units / kBfrTargetJobs;
  if (per_job < 1) per_job = 1;
  if (per_job > a.units) per_job = a.units;
  a.job_units = (uint32_t)per_job;
  const int64_t jpf = (a.units + per_job - 1) / per_job, jobs = jpf * b.n_frames;
  if (jobs >= (1ll << 31)) return hipErrorInvalidValue;
  a.jobs_per_frame = make_div((uint32_t)jpf);
  a.jobs = (uint32_t)jobs;
  a.ranges = ranges;
  a.meta = b.meta;
  // the widest load every address of the batch is aligned for (the chroma
  // plane lies height * line_length past the luma plane)
  const uintptr_t bits = reinterpret_cast<uintptr_t>(b.frames) | (uintptr_t)a.frame_stride | (uintptr_t)b.line_length;
  const bool yuyv = b.layout == TRIK_HSV_LAYOUT_YUYV;
  const int align = (bits & 3) != 0 ? 1 : (yuyv && (bits & 7) == 0 ? 8 : 4);
  const int64_t blocks = (jobs + kBfrWaves - 1) / kBfrWaves, most = 8LL * device_cus();
  const unsigned grid = (unsigned)(blocks < most ? blocks : most);
  if (yuyv)
    launch_layout<TRIK_HSV_LAYOUT_YUYV>(align, grid, s, a);
  else
    launch_layout<TRIK_HSV_LAYOUT_OV7670>(align, grid, s, a);
  return hipGetLastError();
}

}  // namespace trik_hsv
