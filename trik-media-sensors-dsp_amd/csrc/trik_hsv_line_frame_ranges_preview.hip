// trik_hsv_line_frame_ranges_preview.hip -- the two line sensors' RGB565X
// previews with a V range per frame, read from device memory:
// the body and overlays of trik_hsv_line_preview (ov7670, LSEQ:283-291,
// 419-474) and of the webcam line codec's process() (packed YUYV,
// LSEQW:232-269, 396-413) without a table.  A line sensor tests V alone, and V
// is the maximum of the three clamped colour bytes the preview computes anyway
// (WSEQ:207-216), so a pixel is the colour (stripe_px::rgb), one maximum and
// one window test against the frame's two scaled bounds: no H, no S, no
// LUT43 / LUT255 and no LDS.
//
// The task split is trik_hsv_preview_tasks.h's: a wave works inside one frame
// at a time, so frame f's bounds (entries 4 and 5 of its six-tuple, scaled by
// scale_val) and the low words of its sums go to scalar registers through
// readfirstlane.
//
//  lfr_preview_rows2_kernel   the 2:1 maps, preview_rows2_kernel's unit: 16
//                        bytes per plane, 8 output pixels, two nontemporal
//                        8-byte stores; the window zeroing, the magenta thin
//                        lines, the band rows and the frame's target columns in
//                        the same pass, in preview_rows2_kernel<OVL>'s order.
//                        The target line's output-column interval is formed
//                        once per task.  Eligibility: preview_rows2_ok and
//                        ovl_ok, as launch_line_preview's fused form.
//  lfr_preview_gather_kernel  every other geometry, fr_preview_gather_kernel's
//                        4-byte output groups through the inverse maps (whose
//                        last_col carries the column window), zero for unmapped
//                        pixels and line padding, byte loads and stores when
//                        misaligned; line_overlay_kernel (unchanged) follows.
#include <hip/hip_runtime.h>

#include "trik_hsv_internal.h"
#include "trik_hsv_pixel.h"
#include "trik_hsv_preview_tasks.h"
#include "trik_hsv_stripe_px.h"

namespace trik_hsv {

namespace {

// Frame f's V window in scalar registers: lo <= V <= hi as (V - lo) <= span,
// unsigned.  An empty range (scaled from > to) becomes lo = 256, span = 0,
// which no byte passes.  (f wave-uniform: every lane reads the same 4 bytes.)
struct VWindow {
  uint32_t lo, span;
};
__device__ __forceinline__ VWindow frame_window(const FrPreviewGeom& g, uint32_t f) {
  const uint16_t* r = g.ranges + (uint64_t)f * g.range_stride;
  const uint32_t lo = scale_val(__builtin_amdgcn_readfirstlane((int32_t)r[4]));
  const uint32_t hi = scale_val(__builtin_amdgcn_readfirstlane((int32_t)r[5]));
  VWindow w;
  w.lo = lo <= hi ? lo : 256u;
  w.span = lo <= hi ? hi - lo : 0u;
  return w;
}

// RGB565X (write_px565's value) of pixel PIX of the YUYV-ordered word w: the
// clamped colour, or 0x00ffff when V = max(R, G, B) lies in the window.
template <int PIX>
__device__ __forceinline__ uint32_t px565_of(uint32_t w, const VWindow& vw) {
  const PixelRgb c = stripe_px::rgb<PIX>(w, w ^ 0xFF00FF00u);
  const uint32_t V = (uint32_t)max(c.r, max(c.g, c.b));
  const uint32_t c565 = (((uint32_t)c.b << 8) & 0xF800u) | (((uint32_t)c.g << 3) & 0x07E0u) | ((uint32_t)c.r >> 3);
  return V - vw.lo <= vw.span ? 0xFFE0u : c565;
}

// WIN: some output columns are outside the written window (the ov7670 line
// sensor's columns 5..W-5).  The band lines are the ov7670 sensor's alone.
template <int LAYOUT, bool WIN>
__global__ __launch_bounds__(kFpBlock) void lfr_preview_rows2_kernel(PreviewArgs a, FrPreviewGeom g) {
  typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
  typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
  constexpr bool YUYV = LAYOUT == TRIK_HSV_LAYOUT_YUYV;
  constexpr bool BAND = !YUYV;
  constexpr int PX = 8;  // output pixels per unit
  constexpr uint32_t kRed = 0x001Fu, kMagenta = 0xF81Fu;  // RGB565X of 0xff0000, 0xff00ff
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)((blockIdx.x * kFpBlock + threadIdx.x) >> 6));
  const uint32_t n_waves = gridDim.x * kFpWaves, gpr = g.per_row.d;
  const int64_t plane = (int64_t)a.height * a.line_length;
  for (uint32_t task = wave0; task < g.tasks; task += n_waves) {
    const uint32_t f = fdiv(task, g.segs), k = task - f * g.segs.d;
    const VWindow vw = frame_window(g, f);
    // red columns [t_lo, t_hi] of this frame's target line (empty unless
    // points > 10), from the low words of points and sumX: once per task
    uint32_t t_lo = 1u, t_hi = 0u;
    {
      const uint32_t* ts = reinterpret_cast<const uint32_t*>(a.ovl_sums + f);
      const uint32_t n = (uint32_t)__builtin_amdgcn_readfirstlane((int)ts[0]);
      const uint32_t sx = (uint32_t)__builtin_amdgcn_readfirstlane((int)ts[2]);
      if (n > 10) {  // LSEQ:464-474: drawRgbTargetCenterLine(targetX), columns cx - 1 .. cx + 1
        const int32_t cx = (int32_t)(sx / n), wm = a.width - 1;
        const int32_t c0 = cx - 1 < 0 ? 0 : (cx - 1 > wm ? wm : cx - 1);
        const int32_t c1 = cx + 1 < 0 ? 0 : (cx + 1 > wm ? wm : cx + 1);
        // ovl_half: wi2wo[c] = c / 2 (the 2:1 maps), no dependent map loads
        t_lo = a.ovl_half ? (uint32_t)c0 >> 1 : a.wi2wo[c0];
        t_hi = a.ovl_half ? (uint32_t)c1 >> 1 : a.wi2wo[c1];
      }
    }
    const uint32_t u = 64u * k + lane;
    const bool live = u < g.per_frame;
    const uint32_t ul = live ? u : 0u;  // a lane with no unit re-reads the frame's first one and stores nothing
    const uint32_t r = fdiv(ul, g.per_row), q = ul - r * gpr;
    // (32-bit offsets and one 64-bit multiply-add per address: preview_rows2_ok
    // checks that strides and in-frame offsets fit 32 bits, rows 24)
    const uint8_t* src = a.frames + (uint64_t)f * (uint32_t)a.frame_stride +
                         (__umul24((uint32_t)a.rows2_first + 2u * r, (uint32_t)a.line_length) + (YUYV ? 32u : 16u) * q);
    const u32x4 w = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(src));
    // YUYV: the unit's second piece; ov7670: its chroma bytes
    const u32x4 wc = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(YUYV ? src + 16 : src + plane));
    uint32_t ws[PX];
    if (YUYV) {
      ws[0] = w.x; ws[1] = w.y; ws[2] = w.z; ws[3] = w.w;
      ws[4] = wc.x; ws[5] = wc.y; ws[6] = wc.z; ws[7] = wc.w;
    } else {  // the word (-, U, Y1, V) of output pixel 2d + j: luma byte 2j + 1, chroma bytes 2j, 2j + 1
      const uint32_t yy[4] = {w.x, w.y, w.z, w.w}, cc[4] = {wc.x, wc.y, wc.z, wc.w};
#pragma unroll
      for (int d = 0; d < 4; ++d) {
        ws[2 * d] = __builtin_amdgcn_perm(cc[d], yy[d], 0x0401050Cu);
        ws[2 * d + 1] = __builtin_amdgcn_perm(cc[d], yy[d], 0x0603070Cu);
      }
    }
    const bool band_row = BAND && ((int32_t)r == a.ovl_band[0] || (int32_t)r == a.ovl_band[1]);
    uint32_t v[PX];
#pragma unroll
    for (int j = 0; j < PX; ++j) {
      const uint32_t c = PX * q + (uint32_t)j;  // the pixel's output column
      v[j] = px565_of<1>(ws[j], vw);            // the odd pixel: Y in byte 2
      if (WIN) v[j] = c >= (uint32_t)a.rows2_c0 && c < (uint32_t)a.rows2_c1 ? v[j] : 0u;
      // thin lines (magenta) first, then the band and target lines (red) over them
      const bool mag = (int32_t)c == a.ovl_mag[0] || (int32_t)c == a.ovl_mag[1] || (int32_t)c == a.ovl_mag[2] ||
                       (int32_t)c == a.ovl_mag[3];
      const bool red = (BAND && band_row && (int32_t)c >= a.ovl_c_lo && (int32_t)c <= a.ovl_c_hi) ||
                       (c >= t_lo && c <= t_hi);
      v[j] = red ? kRed : (mag ? kMagenta : v[j]);
    }
    if (live) {
      uint8_t* dst = a.previews + (uint64_t)f * (uint32_t)a.preview_stride + (__umul24(r, (uint32_t)a.out_ll) + 2u * PX * q);
#pragma unroll
      for (int h = 0; h < PX / 4; ++h) {  // written once, not read back here: nontemporal
        u32x2 o;
        o.x = v[4 * h] | (v[4 * h + 1] << 16);
        o.y = v[4 * h + 2] | (v[4 * h + 3] << 16);
        __builtin_nontemporal_store(o, reinterpret_cast<u32x2*>(dst + 8 * h));
      }
    }
  }
}

template <int LAYOUT, bool ALIGNED4>
__global__ __launch_bounds__(kFpBlock) void lfr_preview_gather_kernel(PreviewArgs a, FrPreviewGeom g) {
  constexpr bool YUYV = LAYOUT == TRIK_HSV_LAYOUT_YUYV;
  extern __shared__ __attribute__((aligned(16))) uint16_t maps[];  // [out_h] rows, then [out_w] columns (0xFFFF = -1)
  if (g.maps_lds) {
    for (int i = threadIdx.x; i < a.out_h; i += kFpBlock) maps[i] = (uint16_t)a.last_row[i];
    for (int i = threadIdx.x; i < a.out_w; i += kFpBlock) maps[a.out_h + i] = (uint16_t)a.last_col[i];
    __syncthreads();
  }
  auto map_at = [&](const int32_t* mem, int off, int i) -> int {
    if (!g.maps_lds) return mem[i];
    const uint32_t v = maps[off + i];
    return v == 0xFFFFu ? -1 : (int)v;
  };
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)((blockIdx.x * kFpBlock + threadIdx.x) >> 6));
  const uint32_t n_waves = gridDim.x * kFpWaves, qpr = g.per_row.d;
  const int64_t ll = a.line_length;
  for (uint32_t task = wave0; task < g.tasks; task += n_waves) {
    const uint32_t f = fdiv(task, g.segs), k = task - f * g.segs.d;
    const VWindow vw = frame_window(g, f);
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
        if (YUYV && ALIGNED4) {
          w[u][p] = *reinterpret_cast<const uint32_t*>(fr + (int64_t)sr[u] * ll + 4 * (sc[u][p] >> 1));
          if (sc[u][p] & 1) w[u][p] = __builtin_amdgcn_perm(w[u][p], w[u][p], 0x03020102u);
        } else if (ALIGNED4) {
          // Y from the luma plane, the V, U byte pair as one u16 (OSEQ:343-387)
          const int64_t off = (int64_t)sr[u] * ll + sc[u][p];
          const uint32_t Y = fr[off];
          const uint32_t vu = *reinterpret_cast<const uint16_t*>(fr + ll * a.height + (off & ~(int64_t)1));
          w[u][p] = Y | ((vu >> 8) << 8) | ((vu & 0xFFu) << 24);
        } else {
          int Y, U, V;
          fetch_yuv(fr, a.height, a.line_length, LAYOUT, sr[u], sc[u][p], Y, U, V);
          w[u][p] = (uint32_t)Y | ((uint32_t)U << 8) | ((uint32_t)V << 24);
        }
      }
    }
#pragma unroll
    for (int u = 0; u < kFpQ; ++u) {
      uint32_t v[2] = {0u, 0u};
#pragma unroll
      for (int p = 0; p < 2; ++p)
        if (sr[u] >= 0 && sc[u][p] >= 0) v[p] = px565_of<0>(w[u][p], vw);
      if (!ok[u]) continue;
      const uint32_t out = v[0] | (v[1] << 16);
      uint8_t* row = a.previews + (int64_t)f * a.preview_stride + (int64_t)rr[u] * a.out_ll;
      const int b0 = 4 * (int)qq[u];
      if (ALIGNED4 && b0 + 4 <= a.out_ll) {
        __builtin_nontemporal_store(out, reinterpret_cast<uint32_t*>(row + b0));
      } else {
        for (int j = 0; j < 4 && b0 + j < a.out_ll; ++j) row[b0 + j] = (uint8_t)(out >> (8 * j));
      }
    }
  }
}

}  // namespace

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
    static const FpKernel kerns[2][2] = {
        {lfr_preview_rows2_kernel<TRIK_HSV_LAYOUT_YUYV, false>, lfr_preview_rows2_kernel<TRIK_HSV_LAYOUT_YUYV, true>},
        {lfr_preview_rows2_kernel<TRIK_HSV_LAYOUT_OV7670, false>, lfr_preview_rows2_kernel<TRIK_HSV_LAYOUT_OV7670, true>}};
    return launch_tasks(kerns[yuyv ? 0 : 1][win ? 1 : 0], a, g, a.out_w / 8, 1, 0, s);
  }
  const int64_t qpr = ((int64_t)a.out_ll + 3) / 4;
  if ((int64_t)a.n_frames * a.out_h * qpr >= (1ll << 31)) return hipErrorInvalidValue;
  // the maps in LDS when they fit and every source coordinate fits u16
  const int64_t map_bytes = 2LL * ((int64_t)a.out_w + a.out_h);
  g.maps_lds = a.width < 65535 && a.height < 65535 && map_bytes <= kFpMapLdsBytes ? 1u : 0u;
  static const FpKernel kerns[2][2] = {
      {lfr_preview_gather_kernel<TRIK_HSV_LAYOUT_YUYV, false>, lfr_preview_gather_kernel<TRIK_HSV_LAYOUT_YUYV, true>},
      {lfr_preview_gather_kernel<TRIK_HSV_LAYOUT_OV7670, false>, lfr_preview_gather_kernel<TRIK_HSV_LAYOUT_OV7670, true>}};
  const int e = launch_tasks(kerns[yuyv ? 0 : 1][a.aligned4 ? 1 : 0], a, g, qpr, kFpQ, g.maps_lds ? (size_t)map_bytes : 0, s);
  if (e != hipSuccess) return e;
  return yuyv ? launch_wline_overlay(a, sums, s) : launch_line_overlay(a, sums, s);
}

}  // namespace trik_hsv
