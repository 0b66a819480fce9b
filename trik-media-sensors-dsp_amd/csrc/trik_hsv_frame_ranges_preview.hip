// trik_hsv_frame_ranges_preview.hip -- the RGB565X previews with a range per
// frame, read from device memory: the bodies of
// trik_hsv_batch_preview and of the two line sensors' previews
// (trik_hsv_operator.hip) without a table.  No table depends on a range; a
// pixel is tested exactly, by one of two pixel tests:
//
//  HsvTest  the object sensor: H, S and V of every sampled pixel
//           (stripe_px::word_hsv, WSEQ:181-249) with LUT43 / LUT255 in 1 KiB of
//           LDS, against the frame's packed range (detect_packed, WSEQ:171-179).
//  ValTest  the line sensors (ov7670, LSEQ:283-291, 419-474; the webcam line
//           codec's process(), packed YUYV, LSEQW:232-269, 396-413): V alone,
//           the maximum of the three clamped colour bytes the preview computes
//           anyway (WSEQ:207-216), against the frame's two scaled bounds: no H,
//           no S, no LUT43 / LUT255 and no LDS.
//
// The frame index is wave-uniform in both kernels.  A wave takes one task at a
// time: 64 consecutive units of ONE frame (a frame of fewer units leaves lanes
// idle; a small frame is one task and the wave loops over frames).  The task's
// frame f comes from the wave's number, so the six-tuple's address is the same
// in every lane and the frame's range (and, for the line sensors, the low
// words of its sums) goes to scalar registers through readfirstlane, as in
// frame_ranges_kernel.  Tasks are handed out round robin over the grid's waves.
//
//  fr_preview_rows2_kernel   the 2:1 maps, preview_rows2_kernel's unit: 16
//                        bytes per plane, 8 output pixels (the odd pixel of
//                        each source pair), two nontemporal 8-byte stores, and
//                        the test's overlay in the same pass: the guide lines
//                        from guide_bits (HsvTest), or the window zeroing, the
//                        magenta thin lines, the band rows and the frame's
//                        target columns in preview_rows2_kernel<OVL>'s order
//                        (ValTest; the target line's output-column interval is
//                        formed once per task).  Eligibility: preview_rows2_ok,
//                        shared with launch_rows2.
//  fr_preview_gather_kernel  every other geometry, preview_gather_kernel's
//                        4-byte output groups through the inverse maps (in LDS
//                        as u16 when they fit; the line sensors' last_col
//                        carries the column window), zero for unmapped pixels
//                        and line padding, byte loads and stores when
//                        misaligned.
//
// The overlay kernels (unchanged) follow where the body did not draw:
// overlay_kernel (launch_preview_overlay) after either object-sensor body,
// line_overlay_kernel / the webcam line overlay after the line sensors' gather.
#include <hip/hip_runtime.h>

#include "trik_hsv_internal.h"
#include "trik_hsv_pixel.h"
#include "trik_hsv_preview_px.h"
#include "trik_hsv_stripe_px.h"

namespace trik_hsv {

namespace {

using namespace preview_px;

constexpr int kFpBlock = 256;                // 4 waves; 1 KiB of LUTs per workgroup
constexpr int kFpWaves = kFpBlock / 64;
constexpr int kFpBlocksPerCu = 8;            // the grid: 8 waves per SIMD
constexpr int kFpQ = 2;                      // gather: output groups per lane and task
constexpr int64_t kFpMapLdsBytes = 32 * 1024;  // gather: maps up to this size are staged in LDS

// The geometry a kernel reads.
struct FrPreviewGeom {
  const uint16_t* ranges;  // frame f's six-tuple at ranges + f * range_stride (entry t already added)
  uint32_t range_stride;   // 6 * n_ranges
  FastDiv segs;            // tasks per frame
  FastDiv per_row;         // units (2:1) or 4-byte groups (gather) per output row
  uint32_t per_frame;      // out_h * per_row.d
  uint32_t tasks;          // n_frames * segs.d, < 2^31
  uint32_t maps_lds;       // gather: the inverse maps are staged in LDS
};

// A pixel test supplies: kLuts (LUT43 / LUT255 staged in LDS), kLineOverlays
// (what the 2:1 kernel draws: the line sensors' overlays, else the guide
// bits), frame() (frame f's range in scalar registers, f wave-uniform) and
// px<PIX>() (RGB565X, write_px565's value, of pixel PIX of the YUYV-ordered
// word w: the clamped colour, or 0x00ffff when the pixel passes).
struct HsvTest {
  static constexpr bool kLuts = true, kLineOverlays = false;
  using Range = PackedRange;
  // (every lane reads the same 12 bytes, uint16 by uint16 -- the buffer is
  // only 2-byte aligned; packed by pack_range, the host's own definition)
  static __device__ __forceinline__ Range frame(const FrPreviewGeom& g, uint32_t f) {
    const uint16_t* r = g.ranges + (uint64_t)f * g.range_stride;
    const PackedRange p = pack_range(r[0], r[1], r[2], r[3], r[4], r[5]);
    PackedRange s;
    s.from = (uint32_t)__builtin_amdgcn_readfirstlane((int)p.from);
    s.to = (uint32_t)__builtin_amdgcn_readfirstlane((int)p.to);
    s.expect = (uint32_t)__builtin_amdgcn_readfirstlane((int)p.expect);
    return s;
  }
  template <int PIX>
  static __device__ __forceinline__ uint32_t px(uint32_t w, const uint16_t* l43, const uint16_t* l255,
                                                const Range& pr) {
    const uint32_t wc = w ^ 0xFF00FF00u;
    const PixelRgb c = stripe_px::rgb<PIX>(w, wc);
    uint32_t H, S, V;
    stripe_px::word_hsv<PIX>(w, wc, l43, l255, H, S, V);
    const uint32_t c565 = rgb565x_of(c);
    return detect_packed(H, S, V, pr) ? 0xFFE0u : c565;
  }
};

// The V window: lo <= V <= hi as (V - lo) <= span, unsigned.  An empty range
// (scaled from > to) becomes lo = 256, span = 0, which no byte passes.
struct VWindow {
  uint32_t lo, span;
};
struct ValTest {
  static constexpr bool kLuts = false, kLineOverlays = true;
  using Range = VWindow;
  // (every lane reads the same 4 bytes: entries 4 and 5, scaled by scale_val)
  static __device__ __forceinline__ Range frame(const FrPreviewGeom& g, uint32_t f) {
    const uint16_t* r = g.ranges + (uint64_t)f * g.range_stride;
    const uint32_t lo = scale_val(__builtin_amdgcn_readfirstlane((int32_t)r[4]));
    const uint32_t hi = scale_val(__builtin_amdgcn_readfirstlane((int32_t)r[5]));
    VWindow w;
    w.lo = lo <= hi ? lo : 256u;
    w.span = lo <= hi ? hi - lo : 0u;
    return w;
  }
  template <int PIX>
  static __device__ __forceinline__ uint32_t px(uint32_t w, const uint16_t*, const uint16_t*, const Range& vw) {
    const PixelRgb c = stripe_px::rgb<PIX>(w, w ^ 0xFF00FF00u);
    const uint32_t V = (uint32_t)max(c.r, max(c.g, c.b));
    const uint32_t c565 = rgb565x_of(c);
    return V - vw.lo <= vw.span ? 0xFFE0u : c565;
  }
};

// WIN: some output columns are outside the written window (the ov7670 line
// sensor's columns 5..W-5; the object sensor cannot reach one).  The band
// lines are the ov7670 line sensor's alone.
template <class Test, int LAYOUT, bool WIN>
__global__ __launch_bounds__(kFpBlock) void fr_preview_rows2_kernel(PreviewArgs a, FrPreviewGeom g) {
  static_assert(Test::kLineOverlays || !WIN, "the guide-bit form writes every output column");
  constexpr bool YUYV = LAYOUT == TRIK_HSV_LAYOUT_YUYV;
  constexpr bool BAND = !YUYV;
  constexpr int PX = kUnitPx;
  __shared__ uint16_t l43[Test::kLuts ? 256 : 1], l255[Test::kLuts ? 256 : 1];  // (no LDS when never touched)
  if (Test::kLuts) {
    stage_luts(l43, l255, threadIdx.x, kFpBlock);
    __syncthreads();
  }
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)((blockIdx.x * kFpBlock + threadIdx.x) >> 6));
  const uint32_t n_waves = gridDim.x * kFpWaves, gpr = g.per_row.d;
  const int64_t plane = (int64_t)a.height * a.line_length;
  for (uint32_t task = wave0; task < g.tasks; task += n_waves) {
    const uint32_t f = fdiv(task, g.segs), k = task - f * g.segs.d;
    const typename Test::Range range = Test::frame(g, f);
    // red columns [t_lo, t_hi] of this frame's target line, from the low words
    // of points and sumX: once per task
    uint32_t t_lo = 1u, t_hi = 0u;
    if (Test::kLineOverlays) {
      const uint32_t* ts = reinterpret_cast<const uint32_t*>(a.ovl_sums + f);
      const uint32_t n = (uint32_t)__builtin_amdgcn_readfirstlane((int)ts[0]);
      const uint32_t sx = (uint32_t)__builtin_amdgcn_readfirstlane((int)ts[2]);
      target_columns(a, n, sx, t_lo, t_hi);
    }
    const uint32_t u = 64u * k + lane;
    const bool live = u < g.per_frame;
    const uint32_t ul = live ? u : 0u;  // a lane with no unit re-reads the frame's first one and stores nothing
    const uint32_t r = fdiv(ul, g.per_row), q = ul - r * gpr;
    // (32-bit offsets and one 64-bit multiply-add per address: preview_rows2_ok
    // checks that strides and in-frame offsets fit 32 bits, rows 24)
    const uint8_t* src = a.frames + (uint64_t)f * (uint32_t)a.frame_stride +
                         (__umul24((uint32_t)a.rows2_first + 2u * r, (uint32_t)a.line_length) + (YUYV ? 32u : 16u) * q);
    uint32_t gbits = 0u;
    if (!Test::kLineOverlays) gbits = a.guide_bits[ul];  // [out_h][out_w / 8]: unit r * gpr + q
    const u32x4 w = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(src));
    // YUYV: the unit's second piece; ov7670: its chroma bytes
    const u32x4 wc = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(YUYV ? src + 16 : src + plane));
    const UnitWords uw = unit_words<YUYV>(w, wc);
    const bool band_row = Test::kLineOverlays && BAND && ((int32_t)r == a.ovl_band[0] || (int32_t)r == a.ovl_band[1]);
    uint32_t v[PX];
#pragma unroll
    for (int j = 0; j < PX; ++j) {
      const uint32_t c = PX * q + (uint32_t)j;                  // the pixel's output column
      v[j] = Test::template px<1>(uw.ws[j], l43, l255, range);  // the odd pixel: Y in byte 2
      if (Test::kLineOverlays) {
        if (WIN) v[j] = c >= (uint32_t)a.rows2_c0 && c < (uint32_t)a.rows2_c1 ? v[j] : 0u;
        line_overlay_px(a, c, band_row, t_lo, t_hi, &v[j]);
      } else {
        v[j] = (gbits >> j) & 1u ? kMagenta565 : v[j];  // a guide line's pixel (0xff00ff)
      }
    }
    if (live) {
      uint8_t* dst = a.previews + (uint64_t)f * (uint32_t)a.preview_stride +
                     (__umul24(r, (uint32_t)a.out_ll) + 2u * PX * q);
      store_unit(dst, v);
    }
  }
}

template <class Test, int LAYOUT, bool ALIGNED4>
__global__ __launch_bounds__(kFpBlock) void fr_preview_gather_kernel(PreviewArgs a, FrPreviewGeom g) {
  extern __shared__ __attribute__((aligned(16))) uint16_t maps[];  // [out_h] rows, then [out_w] columns (0xFFFF = -1)
  __shared__ uint16_t l43[Test::kLuts ? 256 : 1], l255[Test::kLuts ? 256 : 1];  // (no LDS when never touched)
  if (Test::kLuts) stage_luts(l43, l255, threadIdx.x, kFpBlock);
  if (g.maps_lds) {
    for (int i = threadIdx.x; i < a.out_h; i += kFpBlock) maps[i] = (uint16_t)a.last_row[i];
    for (int i = threadIdx.x; i < a.out_w; i += kFpBlock) maps[a.out_h + i] = (uint16_t)a.last_col[i];
  }
  if (Test::kLuts || g.maps_lds) __syncthreads();
  auto map_at = [&](const int32_t* mem, int off, int i) -> int {
    if (!g.maps_lds) return mem[i];
    const uint32_t v = maps[off + i];
    return v == 0xFFFFu ? -1 : (int)v;
  };
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)((blockIdx.x * kFpBlock + threadIdx.x) >> 6));
  const uint32_t n_waves = gridDim.x * kFpWaves, qpr = g.per_row.d;
  for (uint32_t task = wave0; task < g.tasks; task += n_waves) {
    const uint32_t f = fdiv(task, g.segs), k = task - f * g.segs.d;
    const typename Test::Range range = Test::frame(g, f);
    const uint8_t* fr = frame_ptr(a, f);
    // kFpQ output groups per lane, 64 apart, in phases (positions and maps,
    // frame loads, arithmetic, stores) so that a lane's loads are in flight
    // together; a lane past the frame's last group loads and stores nothing
    uint32_t rr[kFpQ], qq[kFpQ];
    bool ok[kFpQ];
    int sr[kFpQ], sc[kFpQ][2];
#pragma unroll
    for (int u = 0; u < kFpQ; ++u) {
      const uint32_t i = (k * kFpQ + (uint32_t)u) * 64u + lane;
      ok[u] = i < g.per_frame;
      const uint32_t il = ok[u] ? i : 0u;
      rr[u] = fdiv(il, g.per_row);
      qq[u] = il - rr[u] * qpr;
      sr[u] = ok[u] ? map_at(a.last_row, 0, (int)rr[u]) : -1;
#pragma unroll
      for (int p = 0; p < 2; ++p) {
        const int c = 2 * (int)qq[u] + p;
        sc[u][p] = ok[u] && c < a.out_w ? map_at(a.last_col, a.out_h, c) : -1;
      }
    }
    uint32_t w[kFpQ][2];  // each pixel as a YUYV word with its Y in byte 0
#pragma unroll
    for (int u = 0; u < kFpQ; ++u) {
#pragma unroll
      for (int p = 0; p < 2; ++p) {
        w[u][p] = 0u;
        if (sr[u] < 0 || sc[u][p] < 0) continue;
        w[u][p] = y_first(gather_word(fr, a, LAYOUT, ALIGNED4, sr[u], sc[u][p]), LAYOUT, ALIGNED4, sc[u][p]);
      }
    }
#pragma unroll
    for (int u = 0; u < kFpQ; ++u) {
      uint32_t v[2] = {0u, 0u};
#pragma unroll
      for (int p = 0; p < 2; ++p)
        if (sr[u] >= 0 && sc[u][p] >= 0) v[p] = Test::template px<0>(w[u][p], l43, l255, range);
      if (!ok[u]) continue;
      const uint32_t out = v[0] | (v[1] << 16);
      uint8_t* row = a.previews + (int64_t)f * a.preview_stride + (int64_t)rr[u] * a.out_ll;
      store_group(row, 4 * (int)qq[u], a.out_ll, ALIGNED4, out);
    }
  }
}

using FpKernel = void (*)(PreviewArgs, FrPreviewGeom);

// The task split and the launch: `per_frame` units of `per_row` a row,
// 64 * per_task of them a task.
int launch_tasks(FpKernel kern, const PreviewArgs& a, FrPreviewGeom g, int64_t per_row, int per_task, size_t lds,
                 hipStream_t s) {
  const int64_t per_frame = a.out_h * per_row, segs = (per_frame + 64 * per_task - 1) / (64 * per_task);
  g.per_row = make_div((uint32_t)per_row);
  g.per_frame = (uint32_t)per_frame;
  g.segs = make_div((uint32_t)segs);
  g.tasks = (uint32_t)(a.n_frames * segs);  // <= n_frames * per_frame < 2^31
  const int64_t blocks = ((int64_t)g.tasks + kFpWaves - 1) / kFpWaves, slots = (int64_t)kFpBlocksPerCu * device_cus();
  hipLaunchKernelGGL(kern, dim3((unsigned)(blocks < slots ? blocks : slots)), dim3(kFpBlock), lds, s, a, g);
  return hipGetLastError();
}

template <class Test>
int launch_gather(const PreviewArgs& a, FrPreviewGeom g, hipStream_t s) {
  const int64_t qpr = ((int64_t)a.out_ll + 3) / 4;
  if ((int64_t)a.n_frames * a.out_h * qpr >= (1ll << 31)) return hipErrorInvalidValue;
  // the maps in LDS when they fit and every source coordinate fits u16
  const int64_t map_bytes = 2LL * ((int64_t)a.out_w + a.out_h);
  g.maps_lds = a.width < 65535 && a.height < 65535 && map_bytes <= kFpMapLdsBytes ? 1u : 0u;
  static const FpKernel kerns[2][2] = {{fr_preview_gather_kernel<Test, TRIK_HSV_LAYOUT_YUYV, false>,
                                        fr_preview_gather_kernel<Test, TRIK_HSV_LAYOUT_YUYV, true>},
                                       {fr_preview_gather_kernel<Test, TRIK_HSV_LAYOUT_OV7670, false>,
                                        fr_preview_gather_kernel<Test, TRIK_HSV_LAYOUT_OV7670, true>}};
  const bool yuyv = a.layout == TRIK_HSV_LAYOUT_YUYV;
  return launch_tasks(kerns[yuyv ? 0 : 1][a.aligned4 ? 1 : 0], a, g, qpr, kFpQ, g.maps_lds ? (size_t)map_bytes : 0, s);
}

}  // namespace

int launch_frame_ranges_preview(const PreviewArgs& pa, const uint16_t* ranges, int n_ranges, int t,
                                const TrikHsvTargetSums* sums, int sums_pitch, hipStream_t s) {
  if (pa.n_frames <= 0 || pa.out_w <= 0 || pa.out_h <= 0) return hipSuccess;
  PreviewArgs a = pa;
  const bool yuyv = a.layout == TRIK_HSV_LAYOUT_YUYV;
  if (!yuyv && a.layout != TRIK_HSV_LAYOUT_OV7670) return hipErrorInvalidValue;
  FrPreviewGeom g = {};
  g.ranges = ranges + 6 * (int64_t)t;
  g.range_stride = 6u * (uint32_t)n_ranges;
  // The 2:1 kernel where launch_rows2 would run its own with the guide lines:
  // every output column written (no WIN form: the object sensor cannot reach
  // one) and the guide bits built; the gather otherwise.
  const bool win = a.rows2_c0 > 0 || a.rows2_c1 < a.out_w;
  int e;
  if (a.guide_bits && !win && preview_rows2_ok(a)) {
    a.guides_drawn = 1;
    e = launch_tasks(yuyv ? fr_preview_rows2_kernel<HsvTest, TRIK_HSV_LAYOUT_YUYV, false>
                          : fr_preview_rows2_kernel<HsvTest, TRIK_HSV_LAYOUT_OV7670, false>,
                     a, g, a.out_w / 8, 1, 0, s);
  } else {
    a.guides_drawn = 0;
    e = launch_gather<HsvTest>(a, g, s);
  }
  return e != hipSuccess ? e : launch_preview_overlay(a, sums, sums_pitch, s);
}

int launch_line_frame_ranges_preview(const PreviewArgs& pa, const uint16_t* ranges, const TrikHsvTargetSums* sums,
                                     hipStream_t s) {
  if (pa.n_frames <= 0 || pa.out_w <= 0 || pa.out_h <= 0) return hipSuccess;
  PreviewArgs a = pa;
  const bool yuyv = a.layout == TRIK_HSV_LAYOUT_YUYV;
  if (!yuyv && a.layout != TRIK_HSV_LAYOUT_OV7670) return hipErrorInvalidValue;
  FrPreviewGeom g = {};
  g.ranges = ranges;
  g.range_stride = 6u;
  // The 2:1 kernel where launch_line_preview would run preview_rows2_kernel
  // with the overlays in the same pass; the gather and line_overlay_kernel
  // otherwise.
  if (a.ovl_ok && preview_rows2_ok(a)) {
    a.ovl_sums = sums;
    const bool win = a.rows2_c0 > 0 || a.rows2_c1 < a.out_w;
    static const FpKernel kerns[2][2] = {{fr_preview_rows2_kernel<ValTest, TRIK_HSV_LAYOUT_YUYV, false>,
                                          fr_preview_rows2_kernel<ValTest, TRIK_HSV_LAYOUT_YUYV, true>},
                                         {fr_preview_rows2_kernel<ValTest, TRIK_HSV_LAYOUT_OV7670, false>,
                                          fr_preview_rows2_kernel<ValTest, TRIK_HSV_LAYOUT_OV7670, true>}};
    return launch_tasks(kerns[yuyv ? 0 : 1][win ? 1 : 0], a, g, a.out_w / 8, 1, 0, s);
  }
  const int e = launch_gather<ValTest>(a, g, s);
  if (e != hipSuccess) return e;
  return yuyv ? launch_wline_overlay(a, sums, s) : launch_line_overlay(a, sums, s);
}

}  // namespace trik_hsv
