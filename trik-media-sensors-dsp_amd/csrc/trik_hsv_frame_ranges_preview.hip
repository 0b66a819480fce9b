// trik_hsv_frame_ranges_preview.hip -- the object sensor's RGB565X preview with
// an HSV range per frame, read from device memory: the body
// of trik_hsv_batch_preview (trik_hsv_operator.hip) without a table.  No table
// depends on a range: H, S and V of every sampled pixel are computed exactly
// (stripe_px::word_hsv, WSEQ:181-249) with LUT43 / LUT255 in 1 KiB of LDS and
// tested against the frame's packed range (detect_packed, WSEQ:171-179).
//
// The frame index is wave-uniform in both kernels.  A wave takes one task at a
// time: 64 consecutive units of ONE frame (a frame of fewer units leaves lanes
// idle; a small frame is one task and the wave loops over frames).  The task's
// frame f comes from the wave's number, so the six-tuple's address is the same
// in every lane; it is packed by pack_range (the host's own definition) and
// goes to scalar registers through readfirstlane, as in frame_ranges_kernel.
// Tasks are handed out round robin over the grid's waves.
//
//  fr_preview_rows2_kernel   the 2:1 maps, preview_rows2_kernel's unit: 16
//                        bytes per plane, 8 output pixels (the odd pixel of
//                        each source pair), two nontemporal 8-byte stores, the
//                        guide lines from guide_bits in the same pass.
//                        Eligibility: preview_rows2_ok, shared with launch_rows2.
//  fr_preview_gather_kernel  every other geometry, preview_gather_kernel's
//                        4-byte output groups through the inverse maps (in LDS
//                        as u16 when they fit), zero for unmapped pixels and
//                        line padding, byte loads and stores when misaligned.
//
// overlay_kernel (unchanged, launch_preview_overlay) follows either.
#include <hip/hip_runtime.h>

#include "trik_hsv_internal.h"
#include "trik_hsv_pixel.h"
#include "trik_hsv_stripe_px.h"

namespace trik_hsv {

namespace {

constexpr int kFpBlock = 256;                // 4 waves; 1 KiB of LUTs per workgroup
constexpr int kFpWaves = kFpBlock / 64;
constexpr int kFpBlocksPerCu = 8;            // the grid: 8 waves per SIMD
constexpr int kFpQ = 2;                      // gather: output groups per lane and task
constexpr int64_t kFpMapLdsBytes = 32 * 1024;  // gather: maps up to this size are staged in LDS

struct FrPreviewGeom {
  const uint16_t* ranges;  // frame f's six-tuple at ranges + f * range_stride (entry t already added)
  uint32_t range_stride;   // 6 * n_ranges
  FastDiv segs;            // tasks per frame
  FastDiv per_row;         // units (2:1) or 4-byte groups (gather) per output row
  uint32_t per_frame;      // out_h * per_row.d
  uint32_t tasks;          // n_frames * segs.d, < 2^31
  uint32_t maps_lds;       // gather: the inverse maps are staged in LDS
};

// Frame f's range in scalar registers (f wave-uniform: every lane reads the
// same 12 bytes, uint16 by uint16 -- the buffer is only 2-byte aligned).
__device__ __forceinline__ PackedRange frame_range(const FrPreviewGeom& g, uint32_t f) {
  const uint16_t* r = g.ranges + (uint64_t)f * g.range_stride;
  const PackedRange p = pack_range(r[0], r[1], r[2], r[3], r[4], r[5]);
  PackedRange s;
  s.from = (uint32_t)__builtin_amdgcn_readfirstlane((int)p.from);
  s.to = (uint32_t)__builtin_amdgcn_readfirstlane((int)p.to);
  s.expect = (uint32_t)__builtin_amdgcn_readfirstlane((int)p.expect);
  return s;
}

// RGB565X (write_px565's value) of pixel PIX of the YUYV-ordered word w: the
// clamped colour, or 0x00ffff when the pixel's exact H, S, V lie in the range.
template <int PIX>
__device__ __forceinline__ uint32_t px565_of(uint32_t w, const uint16_t* l43, const uint16_t* l255,
                                             const PackedRange& pr) {
  const uint32_t wc = w ^ 0xFF00FF00u;
  const PixelRgb c = stripe_px::rgb<PIX>(w, wc);
  uint32_t H, S, V;
  stripe_px::word_hsv<PIX>(w, wc, l43, l255, H, S, V);
  const uint32_t c565 = (((uint32_t)c.b << 8) & 0xF800u) | (((uint32_t)c.g << 3) & 0x07E0u) | ((uint32_t)c.r >> 3);
  return detect_packed(H, S, V, pr) ? 0xFFE0u : c565;
}

template <int LAYOUT>
__global__ __launch_bounds__(kFpBlock) void fr_preview_rows2_kernel(PreviewArgs a, FrPreviewGeom g) {
  typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
  typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
  constexpr bool YUYV = LAYOUT == TRIK_HSV_LAYOUT_YUYV;
  constexpr int PX = 8;  // output pixels per unit
  __shared__ uint16_t l43[256], l255[256];
  stage_luts(l43, l255, threadIdx.x, kFpBlock);
  __syncthreads();
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)((blockIdx.x * kFpBlock + threadIdx.x) >> 6));
  const uint32_t n_waves = gridDim.x * kFpWaves, gpr = g.per_row.d;
  const int64_t plane = (int64_t)a.height * a.line_length;
  for (uint32_t task = wave0; task < g.tasks; task += n_waves) {
    const uint32_t f = fdiv(task, g.segs), k = task - f * g.segs.d;
    const PackedRange pr = frame_range(g, f);
    const uint32_t u = 64u * k + lane;
    const bool live = u < g.per_frame;
    const uint32_t ul = live ? u : 0u;  // a lane with no unit re-reads the frame's first one and stores nothing
    const uint32_t r = fdiv(ul, g.per_row), q = ul - r * gpr;
    // (32-bit offsets and one 64-bit multiply-add per address: preview_rows2_ok
    // checks that strides and in-frame offsets fit 32 bits, rows 24)
    const uint8_t* src = a.frames + (uint64_t)f * (uint32_t)a.frame_stride +
                         (__umul24((uint32_t)a.rows2_first + 2u * r, (uint32_t)a.line_length) + (YUYV ? 32u : 16u) * q);
    const uint32_t gbits = a.guide_bits[ul];  // [out_h][out_w / 8]: unit r * gpr + q
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
    uint32_t v[PX];
#pragma unroll
    for (int j = 0; j < PX; ++j) {
      v[j] = px565_of<1>(ws[j], l43, l255, pr);  // the odd pixel: Y in byte 2
      v[j] = (gbits >> j) & 1u ? 0xF81Fu : v[j];  // a guide line's pixel (0xff00ff)
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
__global__ __launch_bounds__(kFpBlock) void fr_preview_gather_kernel(PreviewArgs a, FrPreviewGeom g) {
  constexpr bool YUYV = LAYOUT == TRIK_HSV_LAYOUT_YUYV;
  extern __shared__ __attribute__((aligned(16))) uint16_t maps[];  // [out_h] rows, then [out_w] columns (0xFFFF = -1)
  __shared__ uint16_t l43[256], l255[256];
  stage_luts(l43, l255, threadIdx.x, kFpBlock);
  if (g.maps_lds) {
    for (int i = threadIdx.x; i < a.out_h; i += kFpBlock) maps[i] = (uint16_t)a.last_row[i];
    for (int i = threadIdx.x; i < a.out_w; i += kFpBlock) maps[a.out_h + i] = (uint16_t)a.last_col[i];
  }
  __syncthreads();
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
    const PackedRange pr = frame_range(g, f);
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
        if (sr[u] >= 0 && sc[u][p] >= 0) v[p] = px565_of<0>(w[u][p], l43, l255, pr);
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

using FpKernel = void (*)(PreviewArgs, FrPreviewGeom);

// `per_frame` units of `per_row` a row, 64 * per_task of them a task
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
    e = launch_tasks(yuyv ? fr_preview_rows2_kernel<TRIK_HSV_LAYOUT_YUYV> : fr_preview_rows2_kernel<TRIK_HSV_LAYOUT_OV7670>,
                     a, g, a.out_w / 8, 1, 0, s);
  } else {
    a.guides_drawn = 0;
    const int64_t qpr = ((int64_t)a.out_ll + 3) / 4;
    if ((int64_t)a.n_frames * a.out_h * qpr >= (1ll << 31)) return hipErrorInvalidValue;
    // the maps in LDS when they fit and every source coordinate fits u16
    const int64_t map_bytes = 2LL * ((int64_t)a.out_w + a.out_h);
    g.maps_lds = a.width < 65535 && a.height < 65535 && map_bytes <= kFpMapLdsBytes ? 1u : 0u;
    static const FpKernel kerns[2][2] = {
        {fr_preview_gather_kernel<TRIK_HSV_LAYOUT_YUYV, false>, fr_preview_gather_kernel<TRIK_HSV_LAYOUT_YUYV, true>},
        {fr_preview_gather_kernel<TRIK_HSV_LAYOUT_OV7670, false>, fr_preview_gather_kernel<TRIK_HSV_LAYOUT_OV7670, true>}};
    e = launch_tasks(kerns[yuyv ? 0 : 1][a.aligned4 ? 1 : 0], a, g, qpr, kFpQ, g.maps_lds ? (size_t)map_bytes : 0, s);
  }
  return e != hipSuccess ? e : launch_preview_overlay(a, sums, sums_pitch, s);
}

}  // namespace trik_hsv
