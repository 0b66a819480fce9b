// trik_hsv_stripe_px.h -- the per-pixel arithmetic in its word form (pixel PIX
// of a YUYV word, branch-free on v_dot4 presums), each step written once:
// presum, clamp8_shift6 / rgb, hue_case, and word_hsv for kernels that need H,
// S, V.  On top of them the hot kernels' table addressing over the
// StripeTables image at LDS address 0 (phase1, sv_addr_only, v_addr,
// phase2_addr, combine).  The scalar form, the matrix constants and the LUT
// staging helper are trik_hsv_pixel.h's.
#pragma once

#include <hip/hip_runtime.h>

#include "trik_hsv_internal.h"
#include "trik_hsv_pixel.h"

namespace trik_hsv {
namespace stripe_px {

// LDS by absolute byte address.  The kernel has no static LDS, so its dynamic
// LDS (the StripeTables image) starts at address 0; addressing it through
// integer-derived address-space-3 pointers lets every table address be one
// VALU op (no symbol base to add).
typedef __attribute__((address_space(3))) const uint8_t* lds_u8_ptr;
typedef __attribute__((address_space(3))) const uint32_t* lds_u32_ptr;
__device__ __forceinline__ uint32_t lds_u32(uint32_t addr) { return *(lds_u32_ptr)(uintptr_t)addr; }
__device__ __forceinline__ uint32_t lds_u8(uint32_t addr) { return *(lds_u8_ptr)(uintptr_t)addr; }

// Presum CH of WSEQ:183-201 for pixel PIX of a YUYV word w
// (b0=Y0, b1=U, b2=Y1, b3=V), one v_dot4_u32_u8; wc = w ^ 0xFF00FF00 carries
// complemented chroma for the negative G weights (WSEQ:188-190).  The
// reference's _add2 keeps 16-bit lanes, so only bits 15:0 matter (B wraps for
// 27,136 triples).  PIX = kChromaTerms: Y weight 0 (the packed 16-bit forms
// add 74 Y themselves).  One call per channel: a caller keeps its own order
// of dot products and clamps, which the hot kernels' schedules follow.
enum { kR, kG, kB };
constexpr int kChromaTerms = -1;
template <int PIX, int CH>
__device__ __forceinline__ uint32_t presum(uint32_t w, uint32_t wc) {
  constexpr uint32_t kY = PIX < 0 ? 0u : (uint32_t)yuv::kY << (16 * PIX);
  constexpr uint32_t kG0c = (uint32_t)(yuv::kG0 - 255 * (yuv::kGU + yuv::kGV));  // -10939
  if (CH == kR) return __builtin_amdgcn_udot4(w, kY | ((uint32_t)yuv::kRV << 24), (uint32_t)yuv::kR0, false);
  if (CH == kG)
    return __builtin_amdgcn_udot4(wc, kY | ((uint32_t)yuv::kGU << 8) | ((uint32_t)yuv::kGV << 24), kG0c, false);
  return __builtin_amdgcn_udot4(w, kY | ((uint32_t)yuv::kBU << 8), (uint32_t)yuv::kB0, false);
}

// x = (int16)presum >> 6 clamped to [0, 255] (WSEQ:203-205): v_bfe_i32 + v_med3_i32
__device__ __forceinline__ int shift6(uint32_t s) { return ((int)(s << 16)) >> 22; }  // bits 15:6, sign from 15
__device__ __forceinline__ int clamp8_shift6(uint32_t s) {
  const int x = shift6(s);
  const int lo = x < 0 ? 0 : x;
  return lo > 255 ? 255 : lo;  // v_med3_i32
}
template <int PIX>
__device__ __forceinline__ PixelRgb rgb(uint32_t w, uint32_t wc) {
  PixelRgb p;
  p.r = clamp8_shift6(presum<PIX, kR>(w, wc));
  p.g = clamp8_shift6(presum<PIX, kG>(w, wc));
  p.b = clamp8_shift6(presum<PIX, kB>(w, wc));
  return p;
}

// The hue case select of WSEQ:226-246 (priority G > B > R on ties) as
// selects: h = base + LUT43[max - min] * diff.
__device__ __forceinline__ void hue_case(const PixelRgb& p, int mx, uint32_t& diff, uint32_t& base) {
  const bool eqG = mx == p.g, eqB = mx == p.b;
  const int dR = p.g - p.b, dG = p.b - p.r, dB = p.r - p.g;
  const int d = eqB ? dB : dR;
  diff = (uint32_t)(eqG ? dG : d);
  const uint32_t b = eqB ? (uint32_t)kHueBaseB : 0u;
  base = eqG ? (uint32_t)kHueBaseG : b;
}

// Phase 1 of the hot kernel for pixel PIX of a word: rgb, max, min
// (WSEQ:207-216), the hue case, and the LDS byte addresses of this pixel's
// LUT43[max - min] copy (per-bank replicated row, StripeTables::rows) and of
// its sat&val mask sv[max * 260 + min].
// Plain 32-bit code: on gfx950 this kernel's time follows its VALU
// instruction count (the 16-bit full-rate forms measured no faster in
// context, scripts/ubench/pixel_mix.hip), and the compiler schedules it and
// enforces the v_dot4 / VCC wait states itself.
struct Phase1 {
  uint32_t m43_addr, sv_addr, diff, base;
  uint32_t rgb888;  // the clamped pixel (the preview's colour); dead code where unused
  int r, g, b;      // its clamped channels (the 2:1 preview packs RGB565X from them)
};
constexpr int log2i(int v) { return v <= 1 ? 0 : 1 + log2i(v / 2); }
constexpr int kM43Shift = log2i(4 * kM43Copies);  // byte stride of one m43 entry's copies
constexpr int kHueShift = log2i(4 * kHueCopies);
static_assert((1 << kM43Shift) == 4 * kM43Copies && (1 << kHueShift) == 4 * kHueCopies, "pow2 copies");
template <int PIX>
__device__ __forceinline__ Phase1 phase1(uint32_t w, uint32_t wc, uint32_t m43_lane) {
  const PixelRgb c = rgb<PIX>(w, wc);
  const int mx = max(c.r, max(c.g, c.b));
  const int mn = min(c.r, min(c.g, c.b));
  Phase1 p;
  p.rgb888 = c.rgb888();
  p.r = c.r;
  p.g = c.g;
  p.b = c.b;
  p.m43_addr = ((uint32_t)(mx - mn) << kM43Shift) + m43_lane;
  p.sv_addr = __umul24((uint32_t)mx, (uint32_t)kSvStride) + (uint32_t)mn;
  hue_case(c, mx, p.diff, p.base);
  return p;
}

// H, S, V of pixel PIX of a YUYV word (WSEQ:181-249) with LUT43 / LUT255 from
// any address space: phase1 (its table addresses are dead code here), then
// the two LUT products (h mod 2^32, as the int product).
template <int PIX, typename L>
__device__ __forceinline__ void word_hsv(uint32_t w, uint32_t wc, const L* l43, const L* l255, uint32_t& H,
                                         uint32_t& S, uint32_t& V) {
  const Phase1 p = phase1<PIX>(w, wc, 0u);
  const int mx = max(p.r, max(p.g, p.b)), mn = min(p.r, min(p.g, p.b));
  const uint32_t h = p.base + (uint32_t)l43[mx - mn] * p.diff;
  H = (h >> 8) & 0xFFu;
  S = ((uint32_t)l255[mx] * (uint32_t)(mx - mn)) >> 8;
  V = (uint32_t)mx;
}

// The sat&val table address alone (ranges that accept every hue): clamp8 is
// monotone, so max and min of the clamped channels are the clamped max and min
// of the unclamped ones (two clamps per pixel instead of three).
template <int PIX>
__device__ __forceinline__ uint32_t sv_addr_only(uint32_t w, uint32_t wc) {
  const int r = shift6(presum<PIX, kR>(w, wc));  // v_bfe_i32 s, 6, 10
  const int g = shift6(presum<PIX, kG>(w, wc));
  const int b = shift6(presum<PIX, kB>(w, wc));
  const int mx = min(max(max(r, max(g, b)), 0), 255);
  const int mn = min(max(min(r, min(g, b)), 0), 255);
  return __umul24((uint32_t)mx, (uint32_t)kSvStride) + (uint32_t)mn;
}

// The value-only table address (ranges that accept every hue and every
// saturation): m = max(R', G', sext16(B')) of the unclamped presums,
// 4 * ((m >> 6) + 512) into a table of 1024 byte-spread value masks whose
// entries below 512 / above 767 hold V = 0 / V = 255 (the clamp).
template <int PIX>
__device__ __forceinline__ uint32_t v_addr(uint32_t w, uint32_t wc) {
  const int r = (int)presum<PIX, kR>(w, wc);  // int16 range
  const int g = (int)presum<PIX, kG>(w, wc);
  const int b = ((int)(presum<PIX, kB>(w, wc) << 16)) >> 16;
  const int m = max(r, max(g, b));
  return (uint32_t)(((m >> 6) + 512) << 2);
}

// Phase 2: h = base + m * diff (WSEQ:226-246; m < 2^14, |diff| < 2^8, so one
// v_mad_i32_i24), whose bits 15:8 (H) select the byte-spread hue mask (range t
// -> bit 8t); returns the LDS byte address of this lane's copy.
// (LLVM would fuse the multiply-add into a quarter-rate v_mad_u64_u32.)
__device__ __forceinline__ uint32_t phase2_addr(uint32_t m, const Phase1& p, uint32_t hue_lane) {
  uint32_t h;
  asm("v_mad_i32_i24 %0, %1, %2, %3" : "=v"(h) : "v"(m), "v"(p.diff), "v"(p.base));
  return (((h >> 8) & 0xFFu) << kHueShift) + hue_lane;
}

// Combine: spread sv's bit t to bit 8t (terms at t + 7s are disjoint for
// t, s < 4) and AND with the hue mask.
__device__ __forceinline__ uint32_t combine(uint32_t hue, uint32_t sv) {
  return hue & __umul24(sv, 0x00204081u);
}

// byte-spread mask -> bit mask (range t -> bit t): bit 8t lands on bit 24+t
__device__ __forceinline__ uint32_t pack_bits(uint32_t e) { return ((e * 0x01020408u) >> 24) & 0xFu; }

// ov7670 planes -> the two YUYV words of 4 pixels (OSEQ:360-373: U = odd
// chroma byte, V = even chroma byte): yy = Y0..Y3, cc = V0 U0 V1 U1.
__device__ __forceinline__ void ov7670_words(uint32_t yy, uint32_t cc, uint32_t& w0, uint32_t& w1) {
  w0 = __builtin_amdgcn_perm(cc, yy, 0x04010500u);
  w1 = __builtin_amdgcn_perm(cc, yy, 0x06030702u);
}

}  // namespace stripe_px

// The table-free kernels' unit load (trik_hsv_frame_ranges.hip,
// trik_hsv_mask.hip), the one definition:
// The four YUYV words (Y0 U Y1 V) of unit `col` (pixels 8 col .. 8 col + 7) of
// a row.  ALIGN 16: one 16-byte load (two 8-byte loads for the planes); 4:
// dword loads; 1: bytes through fetch_yuv.  Every byte lies inside the row.
template <int LAYOUT, int ALIGN>
__device__ __forceinline__ void load_unit(const uint8_t* fr, int height, int line_length, int row, int col,
                                          uint32_t w[4]) {
  if (ALIGN == 1) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      int y0, y1, u, v, u1, v1;
      fetch_yuv(fr, height, line_length, LAYOUT, row, 8 * col + 2 * k, y0, u, v);
      fetch_yuv(fr, height, line_length, LAYOUT, row, 8 * col + 2 * k + 1, y1, u1, v1);
      w[k] = (uint32_t)y0 | ((uint32_t)u << 8) | ((uint32_t)y1 << 16) | ((uint32_t)v << 24);
    }
  } else if (LAYOUT == TRIK_HSV_LAYOUT_YUYV) {
    const uint8_t* p = fr + (int64_t)row * line_length + (int64_t)col * 16;
    if (ALIGN == 16) {
      const uint4 v = *reinterpret_cast<const uint4*>(p);
      w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
    } else {
      const uint32_t* q = reinterpret_cast<const uint32_t*>(p);
      w[0] = q[0]; w[1] = q[1]; w[2] = q[2]; w[3] = q[3];
    }
  } else {
    const uint8_t* py = fr + (int64_t)row * line_length + (int64_t)col * 8;
    const uint8_t* pc = py + (int64_t)line_length * height;
    uint32_t y[2], c[2];
    if (ALIGN == 16) {
      const uint2 vy = *reinterpret_cast<const uint2*>(py);
      const uint2 vc = *reinterpret_cast<const uint2*>(pc);
      y[0] = vy.x; y[1] = vy.y; c[0] = vc.x; c[1] = vc.y;
    } else {
      y[0] = reinterpret_cast<const uint32_t*>(py)[0];
      y[1] = reinterpret_cast<const uint32_t*>(py)[1];
      c[0] = reinterpret_cast<const uint32_t*>(pc)[0];
      c[1] = reinterpret_cast<const uint32_t*>(pc)[1];
    }
    stripe_px::ov7670_words(y[0], c[0], w[0], w[1]);
    stripe_px::ov7670_words(y[1], c[1], w[2], w[3]);
  }
}

}  // namespace trik_hsv
