// trik_hsv_preview_px.h -- the pieces every RGB565X preview body is made of,
// each written once: the table previews (preview_rows2_kernel,
// preview_gather_kernel of trik_hsv_operator.hip) and the per-frame-range ones
// (trik_hsv_frame_ranges_preview.hip) differ in their task
// order and in how a pixel is tested, not in these.
//
//  the 2:1 unit    unit_words (two 16-byte pieces -> eight YUYV words, per
//                  layout), store_unit (eight pixels, two 8-byte stores)
//  the gather      gather_word, y_first (one pixel's YUYV word, Y in byte 0),
//                  store_group (a 4-byte output group with its byte tail)
//  line overlays   target_columns (LSEQ:464-474), line_overlay_px
//
// preview_rows2_kernel keeps its own text of unit_words, store_unit and
// line_overlay_px: with the calls its instruction schedule moves (DESIGN.md
// 4.13).  The forms of the parameters are part of what keeps every other
// caller's code as it was before these were shared: `aligned4` as the int it is
// in PreviewArgs (a bool parameter evaluates `!= 0` ahead of the short-circuit
// it stood in), and line_overlay_px's pixel through a plain pointer (a
// reference or a value lets the compiler form the selects before the caller's
// pixel loop is unrolled, and they then sink into the 16-bit packing).
#pragma once

#include <hip/hip_runtime.h>

#include "trik_hsv_internal.h"
#include "trik_hsv_pixel.h"

namespace trik_hsv {
namespace preview_px {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));

constexpr int kUnitPx = 8;  // output pixels per 2:1 unit
constexpr uint32_t kRed565 = 0x001Fu, kMagenta565 = 0xF81Fu;  // RGB565X (write_px565's value) of 0xff0000, 0xff00ff

// RGB565X of a clamped colour: R >> 3 | (G >> 2) << 5 | (B >> 3) << 11
__device__ __forceinline__ uint32_t rgb565x_of(const PixelRgb& c) {
  return (((uint32_t)c.b << 8) & 0xF800u) | (((uint32_t)c.g << 3) & 0x07E0u) | ((uint32_t)c.r >> 3);
}

// The eight YUYV-ordered words of a 2:1 unit, output pixel j in the odd pixel
// (Y in byte 2) of ws[j].  YUYV: w and wc are the unit's two 16-byte pieces;
// ov7670: w its 16 luma bytes, wc its 16 chroma bytes.
struct UnitWords {
  uint32_t ws[kUnitPx];
};
template <bool YUYV>
__device__ __forceinline__ UnitWords unit_words(u32x4 w, u32x4 wc) {
  constexpr int PX = kUnitPx;
  UnitWords o;
  if (YUYV) {
    o.ws[0] = w.x; o.ws[1] = w.y; o.ws[2] = w.z; o.ws[3] = w.w;
    o.ws[4] = wc.x; o.ws[5] = wc.y; o.ws[6] = wc.z; o.ws[7] = wc.w;
  } else {  // the word (-, U, Y1, V) of output pixel 2d + j: luma byte 2j + 1, chroma bytes 2j, 2j + 1
    const uint32_t yy[4] = {w.x, w.y, w.z, w.w}, cc[4] = {wc.x, wc.y, wc.z, wc.w};
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      o.ws[(2 * d) % PX] = __builtin_amdgcn_perm(cc[d], yy[d], 0x0401050Cu);
      o.ws[(2 * d + 1) % PX] = __builtin_amdgcn_perm(cc[d], yy[d], 0x0603070Cu);
    }
  }
  return o;
}

// A unit's eight RGB565X pixels to dst (8-byte aligned).  Nontemporal: the
// preview is written once and not read back here (630 MB per 4096 VGA frames;
// plain stores left back-to-back batches waiting on the write-backs: 0.51 ->
// 0.45-0.47 ms, scripts/ab/r05zc_preview_nt.py)
__device__ __forceinline__ void store_unit(uint8_t* dst, const uint32_t (&v)[kUnitPx]) {
#pragma unroll
  for (int h = 0; h < kUnitPx / 4; ++h) {
    u32x2 o;
    o.x = v[4 * h] | (v[4 * h + 1] << 16);
    o.y = v[4 * h + 2] | (v[4 * h + 3] << 16);
    __builtin_nontemporal_store(o, reinterpret_cast<u32x2*>(dst + 8 * h));
  }
}

// Source pixel (row, col), both mapped (>= 0), as a YUYV word for the gather:
// aligned packed YUYV gives the pixel pair's word as it lies in memory (y_first
// then brings an odd pixel's Y to byte 0); the other forms give Y in byte 0.
__device__ __forceinline__ uint32_t gather_word(const uint8_t* fr, const PreviewArgs& a, int layout, int aligned4,
                                                int row, int col) {
  const int64_t ll = a.line_length;
  if (layout == TRIK_HSV_LAYOUT_YUYV && aligned4) {
    return *reinterpret_cast<const uint32_t*>(fr + (int64_t)row * ll + 4 * (col >> 1));
  } else if (layout == TRIK_HSV_LAYOUT_OV7670 && aligned4) {
    // Y from the luma plane, the V, U byte pair as one u16 (OSEQ:343-387)
    const int64_t off = (int64_t)row * ll + col;
    const uint32_t Y = fr[off];
    const uint32_t vu = *reinterpret_cast<const uint16_t*>(fr + ll * a.height + (off & ~(int64_t)1));
    return Y | ((vu >> 8) << 8) | ((vu & 0xFFu) << 24);
  } else {
    int Y, U, V;
    fetch_yuv(fr, a.height, a.line_length, layout, row, col, Y, U, V);
    return (uint32_t)Y | ((uint32_t)U << 8) | ((uint32_t)V << 24);
  }
}
__device__ __forceinline__ uint32_t y_first(uint32_t w, int layout, int aligned4, int col) {
  if (layout == TRIK_HSV_LAYOUT_YUYV && aligned4 && (col & 1)) w = __builtin_amdgcn_perm(w, w, 0x03020102u);
  return w;
}

// The 4-byte output group at byte b0 of a preview row: one store, or bytes
// when misaligned or cut by the line's end (the line padding is written too).
__device__ __forceinline__ void store_group(uint8_t* row, int b0, int out_ll, int aligned4, uint32_t out) {
  if (aligned4 && b0 + 4 <= out_ll) {
    __builtin_nontemporal_store(out, reinterpret_cast<uint32_t*>(row + b0));  // (as the 2:1 kernels')
  } else {
    for (int j = 0; j < 4 && b0 + j < out_ll; ++j) row[b0 + j] = (uint8_t)(out >> (8 * j));
  }
}

// The line sensors' target line: output columns [t_lo, t_hi] of a frame with
// `n` points and sumX `sx` (their low words), empty (1, 0) unless n > 10.
__device__ __forceinline__ void target_columns(const PreviewArgs& a, uint32_t n, uint32_t sx, uint32_t& t_lo,
                                               uint32_t& t_hi) {
  t_lo = 1u;
  t_hi = 0u;
  if (n > 10) {  // LSEQ:464-474: drawRgbTargetCenterLine(targetX), columns cx - 1 .. cx + 1
    const int32_t cx = (int32_t)(sx / n), wm = a.width - 1;
    const int32_t c0 = cx - 1 < 0 ? 0 : (cx - 1 > wm ? wm : cx - 1);
    const int32_t c1 = cx + 1 < 0 ? 0 : (cx + 1 > wm ? wm : cx + 1);
    // ovl_half: wi2wo[c] = c / 2 (the 2:1 maps), no dependent map loads
    t_lo = a.ovl_half ? (uint32_t)c0 >> 1 : a.wi2wo[c0];
    t_hi = a.ovl_half ? (uint32_t)c1 >> 1 : a.wi2wo[c1];
  }
}

// Output column c's pixel under the line sensors' overlays: the thin lines
// (magenta) first, then the band and target lines (red) over them, else v.
__device__ __forceinline__ void line_overlay_px(const PreviewArgs& a, uint32_t c, bool band_row, uint32_t t_lo,
                                                uint32_t t_hi, uint32_t* v) {
  const bool mag = (int32_t)c == a.ovl_mag[0] || (int32_t)c == a.ovl_mag[1] || (int32_t)c == a.ovl_mag[2] ||
                   (int32_t)c == a.ovl_mag[3];
  const bool red = (band_row && (int32_t)c >= a.ovl_c_lo && (int32_t)c <= a.ovl_c_hi) || (c >= t_lo && c <= t_hi);
  *v = red ? kRed565 : (mag ? kMagenta565 : *v);
}

}  // namespace preview_px
}  // namespace trik_hsv
