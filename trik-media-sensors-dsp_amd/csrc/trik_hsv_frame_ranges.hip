// trik_hsv_frame_ranges.hip -- the batched object sensor with HSV ranges per
// frame, read from device memory.
//
//  frame_ranges_kernel   a workgroup takes a band of rows of ONE frame.  Its
//                        first lanes read the frame's six-tuples, pack them
//                        (pack_range, the host's own definition) and leave the
//                        packed ranges in LDS beside LUT43 / LUT255, which the
//                        workgroup builds itself.  Then, per group of 4 ranges
//                        (a last single range alone, in a pass of its own):
//                        the group's packed ranges go to scalar registers, the
//                        band is walked in units of 8 pixels of one row, H, S
//                        and V of every pixel are computed once (stripe_px::
//                        word_hsv, WSEQ:181-249) and tested against the 4 ranges
//                        (detect_packed, WSEQ:171-179).  A unit's N and sum of
//                        columns stay in 32 bits (8 pixels of one row; sum_y =
//                        row * N) and are widened to 64 bits before units are
//                        added; a wave reduction, a workgroup reduction through
//                        LDS and one 64-bit atomic per value end the group.
//                        Integer sums: any order gives the same result.
//  ranges_of_detect_kernel   centre/tolerance -> from/to (BMB:110-130), one
//                        lane per frame.
//
// No table depends on a range, so nothing is built per range set.
#include <hip/hip_runtime.h>

#include "trik_hsv_internal.h"
#include "trik_hsv_pixel.h"
#include "trik_hsv_stripe_px.h"
#include "trik_hsv_wave.h"

namespace trik_hsv {

namespace {

constexpr int kFrBlock = 256;
constexpr int kFrWaves = kFrBlock / 64;
static_assert(kFrBlock == 256, "one lane per LUT entry; TRIK_HSV_MAX_RANGES lanes pack the ranges");
constexpr int kFrGroup = 4;               // ranges tested per pass over the band
constexpr int kFrVals = 3 * kFrGroup;     // N, sum_x, sum_y per range
constexpr uint32_t kNeverExpect = 8u;     // detect_packed's `out` has 3 bits: no pixel matches
// workgroups a launch aims for (8 per CU) when the frames alone are fewer
constexpr int kFrTargetBlocks = 2048;
// a launch holds fewer than 2^32 threads: larger batches go in several launches
constexpr int64_t kFrMaxLaunchBlocks = 0xFFFFFFFFll / kFrBlock;

struct FrameRangesArgs : FrameView {
  int32_t n_ranges;
  int32_t segs, seg_rows;   // bands per frame, rows per band
  FastDiv units_per_row;    // width / 8
  const uint16_t* ranges;   // [n_frames][n_ranges][6]
  TrikHsvTargetSums* sums;  // [n_frames][n_ranges], zeroed
};

// One pass over the band for NR ranges from range g0 on (ranges past the
// frame's last never match): the lanes' 64-bit sums of N, sum_x and sum_y per
// range, reduced over the wave into red[wave].
template <int LAYOUT, int ALIGN, int NR>
__device__ __forceinline__ void band_pass(const FrameRangesArgs& a, const uint8_t* fr, int r0, uint32_t units, int g0,
                                          const uint16_t* l43, const uint16_t* l255, const uint32_t* pr_from,
                                          const uint32_t* pr_to, const uint32_t* pr_expect, uint64_t* red_wave) {
  const int tid = threadIdx.x, lane = tid & 63;
  // the ranges, the same in every lane: scalar registers
  PackedRange pr[NR];
#pragma unroll
  for (int k = 0; k < NR; ++k) {
    const bool live = g0 + k < a.n_ranges;  // (uniform)
    pr[k].from = (uint32_t)__builtin_amdgcn_readfirstlane((int)(live ? pr_from[g0 + k] : 0u));
    pr[k].to = (uint32_t)__builtin_amdgcn_readfirstlane((int)(live ? pr_to[g0 + k] : 0u));
    pr[k].expect = (uint32_t)__builtin_amdgcn_readfirstlane((int)(live ? pr_expect[g0 + k] : kNeverExpect));
  }
  uint64_t acc[3 * NR];
#pragma unroll
  for (int k = 0; k < 3 * NR; ++k) acc[k] = 0;

  for (uint32_t u = (uint32_t)tid; u < units; u += kFrBlock) {
    const uint32_t rr = fdiv(u, a.units_per_row);
    const int col = (int)(u - rr * a.units_per_row.d), row = r0 + (int)rr;
    uint32_t w[4];
    load_unit<LAYOUT, ALIGN>(fr, a.height, a.line_length, row, col, w);
    uint32_t cnt[NR], sxo[NR];  // this unit's detections and the sum of their offsets 0..7
#pragma unroll
    for (int k = 0; k < NR; ++k) cnt[k] = sxo[k] = 0u;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const uint32_t wc = w[j] ^ 0xFF00FF00u;
      uint32_t H[2], S[2], V[2];
      stripe_px::word_hsv<0>(w[j], wc, l43, l255, H[0], S[0], V[0]);
      stripe_px::word_hsv<1>(w[j], wc, l43, l255, H[1], S[1], V[1]);
#pragma unroll
      for (int px = 0; px < 2; ++px)
#pragma unroll
        for (int k = 0; k < NR; ++k) {
          const bool d = detect_packed(H[px], S[px], V[px], pr[k]);
          cnt[k] += d ? 1u : 0u;
          sxo[k] += d ? (uint32_t)(2 * j + px) : 0u;
        }
    }
    // 32-bit within the unit (8 pixels of one row), 64-bit from here on
#pragma unroll
    for (int k = 0; k < NR; ++k) {
      acc[3 * k + 0] += cnt[k];
      acc[3 * k + 1] += __umul24((uint32_t)(8 * col), cnt[k]) + sxo[k];  // <= 8 * 32767
      acc[3 * k + 2] += __umul24((uint32_t)row, cnt[k]);
    }
  }
#pragma unroll
  for (int k = 0; k < 3 * NR; ++k) {
    const uint64_t v = wave_sum(acc[k]);
    if (lane == 0) red_wave[k] = v;
  }
}

template <int LAYOUT, int ALIGN>
__global__ __launch_bounds__(kFrBlock) void frame_ranges_kernel(FrameRangesArgs a) {
  __shared__ uint16_t l43[256], l255[256];
  __shared__ uint32_t pr_from[TRIK_HSV_MAX_RANGES], pr_to[TRIK_HSV_MAX_RANGES], pr_expect[TRIK_HSV_MAX_RANGES];
  __shared__ uint64_t red[kFrWaves][kFrVals];
  const int tid = threadIdx.x, wave = tid >> 6;
  const int f = (int)(blockIdx.x / (uint32_t)a.segs), seg = (int)(blockIdx.x - (uint32_t)f * (uint32_t)a.segs);
  const int T = a.n_ranges;

  // s_mult43_div, s_mult255_div (WSEQ:400-406), and this frame's ranges packed once
  // (by a division per lane, not stage_luts: with the staged image the T = 1
  // pass measured 1 % slower, its loop's code unchanged but for registers)
  l43[tid] = tid ? (uint16_t)((43u * 256u) / (uint32_t)tid) : (uint16_t)0;
  l255[tid] = tid ? (uint16_t)((255u * 256u) / (uint32_t)tid) : (uint16_t)0;
  if (tid < T) {
    const uint16_t* r = a.ranges + ((int64_t)f * T + tid) * 6;
    const PackedRange p = pack_range(r[0], r[1], r[2], r[3], r[4], r[5]);
    pr_from[tid] = p.from;
    pr_to[tid] = p.to;
    pr_expect[tid] = p.expect;
  }
  __syncthreads();

  const uint8_t* fr = frame_ptr(a, f);
  const int r0 = seg * a.seg_rows;
  const int rows = min(a.seg_rows, a.height - r0);
  const uint32_t units = (uint32_t)rows * a.units_per_row.d;  // < 2^27

  // groups of 4 ranges, a pass each; a last single range (one calibration per
  // camera: T = 1) takes the one-range pass, which does a quarter of the tests
  for (int g0 = 0; g0 < T; g0 += kFrGroup) {
    const int live = min(T - g0, kFrGroup);  // (uniform)
    if (live == 1)
      band_pass<LAYOUT, ALIGN, 1>(a, fr, r0, units, g0, l43, l255, pr_from, pr_to, pr_expect, red[wave]);
    else
      band_pass<LAYOUT, ALIGN, kFrGroup>(a, fr, r0, units, g0, l43, l255, pr_from, pr_to, pr_expect, red[wave]);
    __syncthreads();
    if (tid < 3 * live) {
      uint64_t s = 0;
#pragma unroll
      for (int wv = 0; wv < kFrWaves; ++wv) s += red[wv][tid];
      if (s) {
        TrikHsvTargetSums* dst = a.sums + (int64_t)f * T + g0 + tid / 3;
        atomicAdd(reinterpret_cast<unsigned long long*>(&dst->points) + tid % 3, (unsigned long long)s);
      }
    }
    __syncthreads();  // red is rewritten by the next group
  }
}

// BMB:110-130 in int arithmetic: hue from/to = (hue -/+ tol) mod 360 (what
// makeValueWrap's loops reach), saturation and value clipped to 0..100.
__global__ __launch_bounds__(256) void ranges_of_detect_kernel(const uint16_t* detect, int n, uint16_t* ranges,
                                                               int n_ranges, int t) {
  const int i = (int)(blockIdx.x * 256u + threadIdx.x);
  if (i >= n) return;
  const uint16_t* d = detect + (int64_t)i * 6;
  uint16_t* o = ranges + ((int64_t)i * n_ranges + t) * 6;
  auto wrap = [](int v) {
    const int r = v % 360;
    return r < 0 ? r + 360 : r;
  };
  auto clip = [](int v) { return v < 0 ? 0 : (v > 100 ? 100 : v); };
  o[0] = (uint16_t)wrap((int)d[0] - (int)d[1]);
  o[1] = (uint16_t)wrap((int)d[0] + (int)d[1]);
  o[2] = (uint16_t)clip((int)d[2] - (int)d[3]);
  o[3] = (uint16_t)clip((int)d[2] + (int)d[3]);
  o[4] = (uint16_t)clip((int)d[4] - (int)d[5]);
  o[5] = (uint16_t)clip((int)d[4] + (int)d[5]);
}

template <int LAYOUT>
void launch_frame_ranges_layout(int align, unsigned blocks, hipStream_t s, const FrameRangesArgs& a) {
  if (align == 16)
    hipLaunchKernelGGL((frame_ranges_kernel<LAYOUT, 16>), dim3(blocks), dim3(kFrBlock), 0, s, a);
  else if (align == 4)
    hipLaunchKernelGGL((frame_ranges_kernel<LAYOUT, 4>), dim3(blocks), dim3(kFrBlock), 0, s, a);
  else
    hipLaunchKernelGGL((frame_ranges_kernel<LAYOUT, 1>), dim3(blocks), dim3(kFrBlock), 0, s, a);
}

}  // namespace

// sums (zeroed by the caller) of b's frames under ranges[f][0..n_ranges); b is
// a validated batch with width, height and n_frames > 0.
int launch_frame_ranges(const TrikHsvFrameBatch& b, const uint16_t* ranges, int n_ranges, TrikHsvTargetSums* sums,
                        hipStream_t s) {
  FrameRangesArgs a = {frame_view(b)};
  if (b.n_frames <= 1) a.frame_stride = 0;  // (a single frame's stride is not validated: it counts as aligned)
  a.n_ranges = n_ranges;
  a.units_per_row = make_div((uint32_t)b.width / 8u);
  // the widest load every address of the batch is aligned for
  const uintptr_t bits = reinterpret_cast<uintptr_t>(b.frames) | (uintptr_t)a.frame_stride | (uintptr_t)b.line_length;
  const int align = (bits & 15) == 0 ? 16 : ((bits & 3) == 0 ? 4 : 1);
  // bands: enough workgroups for the chip when the frames are few, each with
  // at least 4 units per lane
  const int64_t units = (int64_t)b.height * (b.width / 8);
  int64_t want = (kFrTargetBlocks + (int64_t)b.n_frames - 1) / b.n_frames;
  const int64_t most = units / (4 * kFrBlock);
  if (want > most) want = most;
  if (want > b.height) want = b.height;
  if (want < 1) want = 1;
  a.seg_rows = (int32_t)((b.height + want - 1) / want);
  a.segs = (b.height + a.seg_rows - 1) / a.seg_rows;
  const int64_t per_launch = kFrMaxLaunchBlocks / a.segs;  // frames
  for (int64_t f0 = 0; f0 < b.n_frames; f0 += per_launch) {
    FrameRangesArgs c = a;
    c.narrow(f0, b.n_frames - f0 < per_launch ? b.n_frames - f0 : per_launch);
    c.ranges = ranges + f0 * n_ranges * 6;
    c.sums = sums + f0 * n_ranges;
    const unsigned blocks = (unsigned)((int64_t)c.n_frames * a.segs);
    if (b.layout == TRIK_HSV_LAYOUT_YUYV)
      launch_frame_ranges_layout<TRIK_HSV_LAYOUT_YUYV>(align, blocks, s, c);
    else
      launch_frame_ranges_layout<TRIK_HSV_LAYOUT_OV7670>(align, blocks, s, c);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

int launch_ranges_of_detect(const uint16_t* detect, int n, uint16_t* ranges, int n_ranges, int t, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(ranges_of_detect_kernel, dim3(((unsigned)n + 255u) / 256u), dim3(256), 0, s, detect, n, ranges,
                     n_ranges, t);
  return hipGetLastError();
}

}  // namespace trik_hsv
