// trik_hsv_convert.hip -- the reference's RGB888/HSV image as an output
// (DESIGN.md 4.15): convertImageYuyvToHsv's s_rgb888hsv entry of every pixel
// (WSEQ:251-284, OSEQ:343-387), in the reference's own 64-bit form or as three
// byte planes (H, S, V or R, G, B).  The arithmetic is stripe_px::rgb and
// stripe_px::word_hsv, nothing of it is restated here.
//
//  convert_vec_kernel      input and output 16-byte aligned (convert_vec_ok).
//                          The batch is one run of units (8 pixels of a row for
//                          the 64-bit form, 16 for the planes), a lane loads
//                          one unit with 16-byte loads.
//                          64-bit form: the wave's 256 YUYV words go through a
//                          lane transpose, so that in each of four steps lane L
//                          converts word 64 k + L and stores its two entries:
//                          16 bytes per lane, 1 KiB contiguous per store
//                          instruction (two spans where the wave crosses a row
//                          end, every span a multiple of 256 bytes).
//                          Planes: a lane converts its 16 pixels and stores 16
//                          bytes per plane, 1 KiB contiguous per instruction.
//  convert_generic_kernel  everything else: a lane per pixel through
//                          fetch_yuv, byte stores (one 8-byte store per entry
//                          where the entries are 8-byte aligned).
//
// Only pixel bytes are stored: pitch padding and the bytes between planes and
// between frames are never written.
#include <hip/hip_runtime.h>

#include "trik_hsv_internal.h"
#include "trik_hsv_pixel.h"
#include "trik_hsv_stripe_px.h"

// The vector kernel's stores are non-temporal: the image is never re-read by
// the kernel, and with plain stores (0) every form measured 2-8 % slower
// (profiles/convert/ab_nontemporal.txt).
#ifndef TRIK_HSV_CONVERT_NT
#define TRIK_HSV_CONVERT_NT 1
#endif

namespace trik_hsv {

namespace {

constexpr int kCvBlock = 256;
// a launch holds fewer than 2^32 threads: larger batches go in several launches
constexpr int64_t kCvMaxLaunchUnits = (0xFFFFFFFFll / kCvBlock) * kCvBlock;

struct ConvertArgs : FrameView {
  uint8_t* out;
  int64_t out_frame_stride, out_plane_stride;
  int32_t out_row_pitch;
  int32_t out_aligned8;  // generic kernel, 64-bit form: every entry is 8-byte aligned
  uint32_t units;        // of this launch: n_frames * units per frame
  FastDiv units_per_frame, units_per_row;
};

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void store16(uint8_t* p, uint32_t x, uint32_t y, uint32_t z, uint32_t w) {
  const u32x4 v = {x, y, z, w};
#if TRIK_HSV_CONVERT_NT
  __builtin_nontemporal_store(v, reinterpret_cast<u32x4*>(p));
#else
  *reinterpret_cast<u32x4*>(p) = v;
#endif
}

// unit u of the launch -> its frame, row and unit of the row
__device__ __forceinline__ void unit_pos(const ConvertArgs& a, uint32_t u, uint32_t& f, uint32_t& row, uint32_t& col) {
  f = fdiv(u, a.units_per_frame);
  const uint32_t q = u - f * a.units_per_frame.d;
  row = fdiv(q, a.units_per_row);
  col = q - row * a.units_per_row.d;
}

// The NW YUYV words (Y0 U Y1 V) of the unit of 2 NW pixels at `col` of a row,
// by 16-byte loads (8-byte ones for the planes of a 4-word unit).
template <int LAYOUT, int NW>
__device__ __forceinline__ void load_words(const ConvertArgs& a, uint32_t f, uint32_t row, uint32_t col,
                                           uint32_t w[NW]) {
  const uint8_t* fr = frame_ptr(a, f) + (int64_t)row * a.line_length;
  if (LAYOUT == TRIK_HSV_LAYOUT_YUYV) {
    const uint4* p = reinterpret_cast<const uint4*>(fr + (int64_t)col * (4 * NW));
#pragma unroll
    for (int k = 0; k < NW / 4; ++k) {
      const uint4 v = p[k];
      w[4 * k] = v.x; w[4 * k + 1] = v.y; w[4 * k + 2] = v.z; w[4 * k + 3] = v.w;
    }
  } else {
    const uint8_t* py = fr + (int64_t)col * (2 * NW);
    const uint8_t* pc = py + (int64_t)a.line_length * a.height;
    uint32_t y[NW / 2], c[NW / 2];
    if (NW == 4) {
      const uint2 vy = *reinterpret_cast<const uint2*>(py), vc = *reinterpret_cast<const uint2*>(pc);
      y[0] = vy.x; y[1] = vy.y; c[0] = vc.x; c[1] = vc.y;
    } else {
#pragma unroll
      for (int k = 0; k < NW / 8; ++k) {
        const uint4 vy = reinterpret_cast<const uint4*>(py)[k], vc = reinterpret_cast<const uint4*>(pc)[k];
        y[4 * k] = vy.x; y[4 * k + 1] = vy.y; y[4 * k + 2] = vy.z; y[4 * k + 3] = vy.w;
        c[4 * k] = vc.x; c[4 * k + 1] = vc.y; c[4 * k + 2] = vc.z; c[4 * k + 3] = vc.w;
      }
    }
#pragma unroll
    for (int k = 0; k < NW / 2; ++k) stripe_px::ov7670_words(y[k], c[k], w[2 * k], w[2 * k + 1]);
  }
}

// pixel PIX of word w: 0x00RRGGBB and 0x00VVSSHH (the two halves of the entry)
template <int PIX>
__device__ __forceinline__ void entry(uint32_t w, const uint16_t* l43, const uint16_t* l255, uint32_t& rgb,
                                      uint32_t& hsv) {
  const uint32_t wc = w ^ 0xFF00FF00u;
  uint32_t H, S, V;
  stripe_px::word_hsv<PIX>(w, wc, l43, l255, H, S, V);
  rgb = stripe_px::rgb<PIX>(w, wc).rgb888();
  hsv = (V << 16) | (S << 8) | H;
}

template <int LAYOUT, int FORM>
__global__ __launch_bounds__(kCvBlock) void convert_vec_kernel(ConvertArgs a) {
  __shared__ uint16_t l43[256], l255[256];
  const int tid = threadIdx.x, lane = tid & 63;
  if (FORM != TRIK_HSV_CONVERT_RGB_PLANES) {
    stage_luts(l43, l255, tid, kCvBlock);
    __syncthreads();
  }
  const uint32_t u = blockIdx.x * (uint32_t)kCvBlock + (uint32_t)tid;  // (the launch holds fewer than 2^32 lanes)

  if (FORM == TRIK_HSV_CONVERT_RGB888HSV) {
    // lane L's unit: words 4 L .. 4 L + 3 of the wave's 256 (zero past the batch's end)
    uint32_t w[4] = {0u, 0u, 0u, 0u};
    if (u < a.units) {
      uint32_t f, row, col;
      unit_pos(a, u, f, row, col);
      load_words<LAYOUT, 4>(a, f, row, col, w);
    }
    const uint32_t u0 = u - (uint32_t)lane;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      // word 64 k + L of the wave: word L % 4 of the unit lane 16 k + L / 4 holds
      // (every lane takes part in the exchange)
      const int src = 4 * (16 * k + (lane >> 2));
      uint32_t wk = 0u;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const uint32_t t = (uint32_t)__builtin_amdgcn_ds_bpermute(src, (int)w[c]);
        wk = (lane & 3) == c ? t : wk;
      }
      const uint32_t uk = u0 + (uint32_t)(16 * k + (lane >> 2));
      if (uk < a.units) {
        uint32_t f, row, col, rgb0, hsv0, rgb1, hsv1;
        unit_pos(a, uk, f, row, col);
        entry<0>(wk, l43, l255, rgb0, hsv0);
        entry<1>(wk, l43, l255, rgb1, hsv1);
        uint8_t* dst = a.out + (int64_t)f * a.out_frame_stride + (int64_t)row * a.out_row_pitch +
                       (int64_t)(8u * col + 2u * (uint32_t)(lane & 3)) * 8;
        store16(dst, hsv0, rgb0, hsv1, rgb1);
      }
    }
  } else {
    if (u >= a.units) return;
    uint32_t f, row, col;
    unit_pos(a, u, f, row, col);
    uint32_t w[8];
    load_words<LAYOUT, 8>(a, f, row, col, w);
    uint32_t p0[4] = {0u, 0u, 0u, 0u}, p1[4] = {0u, 0u, 0u, 0u}, p2[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      uint32_t rgb[2], hsv[2] = {0u, 0u};
      if (FORM == TRIK_HSV_CONVERT_HSV_PLANES) {
        entry<0>(w[j], l43, l255, rgb[0], hsv[0]);
        entry<1>(w[j], l43, l255, rgb[1], hsv[1]);
      } else {
        const uint32_t wc = w[j] ^ 0xFF00FF00u;
        rgb[0] = stripe_px::rgb<0>(w[j], wc).rgb888();
        rgb[1] = stripe_px::rgb<1>(w[j], wc).rgb888();
      }
#pragma unroll
      for (int px = 0; px < 2; ++px) {
        const int i = 2 * j + px, sh = 8 * (i & 3);
        // planes in the order of the form's name: H, S, V are bytes 0, 1, 2 of
        // 0x00VVSSHH; R, G, B are bytes 2, 1, 0 of 0x00RRGGBB
        const uint32_t e = FORM == TRIK_HSV_CONVERT_HSV_PLANES ? hsv[px] : __builtin_bswap32(rgb[px]) >> 8;
        p0[i >> 2] |= (e & 0xFFu) << sh;
        p1[i >> 2] |= ((e >> 8) & 0xFFu) << sh;
        p2[i >> 2] |= ((e >> 16) & 0xFFu) << sh;
      }
    }
    uint8_t* dst = a.out + (int64_t)f * a.out_frame_stride + (int64_t)row * a.out_row_pitch + (int64_t)col * 16;
    store16(dst, p0[0], p0[1], p0[2], p0[3]);
    store16(dst + a.out_plane_stride, p1[0], p1[1], p1[2], p1[3]);
    store16(dst + 2 * a.out_plane_stride, p2[0], p2[1], p2[2], p2[3]);
  }
}

// A lane per pixel (a unit is one pixel), any alignment.
template <int FORM>
__global__ __launch_bounds__(kCvBlock) void convert_generic_kernel(ConvertArgs a) {
  __shared__ uint16_t l43[256], l255[256];
  const int tid = threadIdx.x;
  if (FORM != TRIK_HSV_CONVERT_RGB_PLANES) {
    stage_luts(l43, l255, tid, kCvBlock);
    __syncthreads();
  }
  const uint32_t u = blockIdx.x * (uint32_t)kCvBlock + (uint32_t)tid;
  if (u >= a.units) return;
  uint32_t f, row, col;
  unit_pos(a, u, f, row, col);
  int Y, U, V;
  fetch_yuv(frame_ptr(a, f), a.height, a.line_length, a.layout, (int)row, (int)col, Y, U, V);
  const uint32_t w = (uint32_t)Y | ((uint32_t)U << 8) | ((uint32_t)Y << 16) | ((uint32_t)V << 24);
  uint32_t rgb, hsv = 0u;
  if (FORM == TRIK_HSV_CONVERT_RGB_PLANES)
    rgb = stripe_px::rgb<0>(w, w ^ 0xFF00FF00u).rgb888();
  else
    entry<0>(w, l43, l255, rgb, hsv);
  uint8_t* dst = a.out + (int64_t)f * a.out_frame_stride + (int64_t)row * a.out_row_pitch;
  if (FORM == TRIK_HSV_CONVERT_RGB888HSV) {
    dst += (int64_t)col * 8;
    if (a.out_aligned8) {
      *reinterpret_cast<uint2*>(dst) = make_uint2(hsv, rgb);
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        dst[k] = (uint8_t)(hsv >> (8 * k));
        dst[4 + k] = (uint8_t)(rgb >> (8 * k));
      }
    }
  } else {
    dst += col;
    const uint32_t e = FORM == TRIK_HSV_CONVERT_HSV_PLANES ? hsv : __builtin_bswap32(rgb) >> 8;
    dst[0] = (uint8_t)e;
    dst[a.out_plane_stride] = (uint8_t)(e >> 8);
    dst[2 * a.out_plane_stride] = (uint8_t)(e >> 16);
  }
}

template <int LAYOUT>
void launch_convert_vec(int form, unsigned blocks, hipStream_t s, const ConvertArgs& a) {
  if (form == TRIK_HSV_CONVERT_RGB888HSV)
    hipLaunchKernelGGL((convert_vec_kernel<LAYOUT, TRIK_HSV_CONVERT_RGB888HSV>), dim3(blocks), dim3(kCvBlock), 0, s, a);
  else if (form == TRIK_HSV_CONVERT_HSV_PLANES)
    hipLaunchKernelGGL((convert_vec_kernel<LAYOUT, TRIK_HSV_CONVERT_HSV_PLANES>), dim3(blocks), dim3(kCvBlock), 0, s, a);
  else
    hipLaunchKernelGGL((convert_vec_kernel<LAYOUT, TRIK_HSV_CONVERT_RGB_PLANES>), dim3(blocks), dim3(kCvBlock), 0, s, a);
}

void launch_convert_generic(int form, unsigned blocks, hipStream_t s, const ConvertArgs& a) {
  if (form == TRIK_HSV_CONVERT_RGB888HSV)
    hipLaunchKernelGGL((convert_generic_kernel<TRIK_HSV_CONVERT_RGB888HSV>), dim3(blocks), dim3(kCvBlock), 0, s, a);
  else if (form == TRIK_HSV_CONVERT_HSV_PLANES)
    hipLaunchKernelGGL((convert_generic_kernel<TRIK_HSV_CONVERT_HSV_PLANES>), dim3(blocks), dim3(kCvBlock), 0, s, a);
  else
    hipLaunchKernelGGL((convert_generic_kernel<TRIK_HSV_CONVERT_RGB_PLANES>), dim3(blocks), dim3(kCvBlock), 0, s, a);
}

}  // namespace

// The vector kernel's condition: every address a 16-byte load or store of it
// forms is 16-byte aligned (a single frame's strides are not addresses).
bool convert_vec_ok(const TrikHsvFrameBatch& b, const TrikHsvConvertOut& o) {
  uintptr_t bits = reinterpret_cast<uintptr_t>(b.frames) | (uintptr_t)b.line_length |
                   reinterpret_cast<uintptr_t>(o.out) | (uintptr_t)o.row_pitch;
  if (b.n_frames > 1) bits |= (uintptr_t)b.frame_stride | (uintptr_t)o.frame_stride;
  if (o.form != TRIK_HSV_CONVERT_RGB888HSV) bits |= (uintptr_t)o.plane_stride;
  return (bits & 15) == 0;
}

// b and o validated, with n_frames, width and height > 0.
int launch_convert(const TrikHsvFrameBatch& b, const TrikHsvConvertOut& o, hipStream_t s) {
  ConvertArgs a = {frame_view(b)};
  if (b.n_frames <= 1) a.frame_stride = 0;  // (a single frame's stride is not validated)
  a.out = static_cast<uint8_t*>(o.out);
  a.out_frame_stride = b.n_frames <= 1 ? 0 : o.frame_stride;
  a.out_plane_stride = o.plane_stride;
  a.out_row_pitch = o.row_pitch;
  a.out_aligned8 =
      ((reinterpret_cast<uintptr_t>(o.out) | (uintptr_t)a.out_frame_stride | (uintptr_t)o.row_pitch) & 7) == 0;
  const bool vec = convert_vec_ok(b, o);
  // pixels per unit: 8 or 16 for the vector kernel (width % 32 == 0), 1 for the generic one
  const uint32_t unit_px = !vec ? 1u : (o.form == TRIK_HSV_CONVERT_RGB888HSV ? 8u : 16u);
  a.units_per_row = make_div((uint32_t)b.width / unit_px);
  const uint32_t per_frame = (uint32_t)b.height * a.units_per_row.d;  // < 2^30
  a.units_per_frame = make_div(per_frame);
  const int64_t per_launch = kCvMaxLaunchUnits / per_frame;  // frames
  for (int64_t f0 = 0; f0 < b.n_frames; f0 += per_launch) {
    ConvertArgs c = a;
    c.narrow(f0, b.n_frames - f0 < per_launch ? b.n_frames - f0 : per_launch);
    c.out = a.out + f0 * a.out_frame_stride;
    c.units = (uint32_t)c.n_frames * per_frame;
    const unsigned blocks = (c.units + (uint32_t)kCvBlock - 1u) / (uint32_t)kCvBlock;
    if (!vec)
      launch_convert_generic(o.form, blocks, s, c);
    else if (b.layout == TRIK_HSV_LAYOUT_YUYV)
      launch_convert_vec<TRIK_HSV_LAYOUT_YUYV>(o.form, blocks, s, c);
    else
      launch_convert_vec<TRIK_HSV_LAYOUT_OV7670>(o.form, blocks, s, c);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace trik_hsv
