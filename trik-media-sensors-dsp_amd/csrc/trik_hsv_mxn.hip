// trik_hsv_mxn.hip -- the ov7670 MxN colour-grid sensor, MSEQ =
// trik/ov7670/mxn_sensor/include/internal/cv_ball_detector_seqpass.hpp:
//
//  mxn_hist_kernel     one workgroup per (frame, cell): the cell's 32x4x4 HSV
//                      histogram (MSEQ:411-452) and its winning bin.  The
//                      reference keeps the bin whose count first exceeds the
//                      running maximum in the cell's raster order.  The
//                      running maximum rises by one at a time, so the last bin
//                      to raise it is the first to reach the final maximum C,
//                      and a bin whose final count is C reaches C on its last
//                      pixel: the winner is, among the bins with count C, the
//                      one whose last pixel comes earliest.  Counts and last
//                      raster positions are kept per wave in LDS and combined
//                      at the end (counts add, positions max).  No floating
//                      point: the winner indexes the host-built colour table.
//  mxn_preview_kernel  the preview (MSEQ:328-366, 609-618) as a gather: output
//                      pixel (r', c') takes the last source row / column that
//                      maps onto it, then the colour of the highest-index cell
//                      whose clamped 20x20 square maps onto it (later cells
//                      overwrite earlier ones in the reference); never-written
//                      pixels and the line padding are zero (the zero fill of
//                      the glue).
#include <hip/hip_runtime.h>

#include "trik_hsv_internal.h"
#include "trik_hsv_pixel.h"
#include "trik_hsv_stripe_px.h"

namespace trik_hsv {

namespace {

constexpr int kMxnBlock = 256;
constexpr int kMxnWaves = kMxnBlock / 64;
constexpr int kMxnBins = 32 * 4 * 4;
// Rounds in which a wave adds all its lanes of one bin with a single LDS
// update; lanes left after them add one by one.  Scene frames put most of a
// cell into one or two bins (64 lanes on one LDS word would serialise);
// noise spreads over the bins and hardly collides.
constexpr int kMxnPeel = 2;

struct MxnGeom {
  FastDiv per_row;  // 4-pixel groups a cell row is walked in (the same for every cell)
  uint32_t total;   // groups per cell
};

// The histogram bin (H >> 3) << 4 | (S >> 6) << 2 | V >> 6 of one pixel given
// as a word with Y in byte 0, U in byte 1 and V in byte 3: MSEQ:191-249 in the
// word form (stripe_px::word_hsv, trik_hsv_stripe_px.h).
__device__ __forceinline__ uint32_t mxn_bin(uint32_t w, const uint16_t* l43, const uint16_t* l255) {
  uint32_t H, S, V;
  stripe_px::word_hsv<0>(w, w ^ 0xFF00FF00u, l43, l255, H, S, V);
  return ((H >> 3) << 4) | ((S >> 6) << 2) | (V >> 6);
}

// One pixel slot of a wave: lanes with `in` set add their bin (pos1 = raster
// position in the cell + 1).  Lanes are in raster order within a slot, so the
// highest lane of a bin holds the bin's last position of the slot.  In each
// round all lanes of one bin are added with a single LDS update.
__device__ __forceinline__ void mxn_vote(bool in, uint32_t bin, uint32_t pos1, uint32_t* cnt, uint32_t* lst,
                                         int lane) {
#pragma unroll
  for (int r = 0; r < kMxnPeel; ++r) {
    const uint64_t todo = __ballot(in);
    if (!todo) return;  // wave-uniform
    const int lead = __ffsll((unsigned long long)todo) - 1;
    const uint32_t b = (uint32_t)__builtin_amdgcn_readlane((int)bin, lead);
    const bool mine = in && bin == b;
    const uint64_t same = __ballot(mine);
    const int top = 63 - __clzll((long long)same);
    const uint32_t p = (uint32_t)__builtin_amdgcn_readlane((int)pos1, top);
    if (lane == lead) {
      atomicAdd(&cnt[b], (uint32_t)__popcll(same));
      atomicMax(&lst[b], p);
    }
    in = in && !mine;
  }
  if (in) {
    atomicAdd(&cnt[bin], 1u);
    atomicMax(&lst[bin], pos1);
  }
}

__global__ __launch_bounds__(kMxnBlock) void mxn_hist_kernel(MxnArgs a, MxnGeom g) {
  __shared__ uint32_t cnt[kMxnWaves][kMxnBins];
  __shared__ uint32_t lst[kMxnWaves][kMxnBins];  // last raster position + 1; 0: no pixel
  __shared__ uint16_t l43[256], l255[256];
  __shared__ uint32_t red_c[kMxnWaves];
  __shared__ unsigned long long red_k[kMxnWaves];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int cells = a.rows_m * a.cols_n;
  const int f = blockIdx.x / cells, k = blockIdx.x - f * cells;
  const int ci = k / a.cols_n, cj = k - ci * a.cols_n;
  const int r0 = ci * a.row_step, c0 = cj * a.col_step, c1 = c0 + a.col_step;
  for (int i = tid; i < kMxnWaves * kMxnBins; i += kMxnBlock) {
    (&cnt[0][0])[i] = 0u;
    (&lst[0][0])[i] = 0u;
  }
  stage_luts(l43, l255, tid, kMxnBlock);  // s_mult43_div, s_mult255_div (MSEQ:564-570)
  __syncthreads();

  // The cell's rows walked in aligned 4-pixel groups (frame columns 4g..4g+3,
  // one 32-bit load per plane); pixels of a group outside the cell's columns
  // are skipped.  A wave takes 64 consecutive groups in raster order.
  const int g0 = c0 >> 2;
  const uint8_t* fr = frame_ptr(a, f);
  const int64_t ll = a.line_length, cofs = ll * a.height;
  for (uint32_t q0 = (uint32_t)wave * 64u; q0 < g.total; q0 += kMxnWaves * 64u) {
    const uint32_t q = q0 + (uint32_t)lane;
    const uint32_t rr = fdiv(q, g.per_row);
    const int col4 = 4 * (g0 + (int)(q - rr * g.per_row.d));
    // (rr < row_step: r0 + rr < height; col4 < c1 <= width, width % 4 == 0: the group is inside the row)
    const bool ok = q < g.total && col4 < c1;
    uint32_t yw = 0u, cw = 0u;
    if (ok) {
      const uint8_t* yp = fr + (int64_t)(r0 + (int)rr) * ll + col4;
      if (a.aligned4) {
        yw = *reinterpret_cast<const uint32_t*>(yp);
        cw = *reinterpret_cast<const uint32_t*>(yp + cofs);
      } else {
        yw = (uint32_t)yp[0] | ((uint32_t)yp[1] << 8) | ((uint32_t)yp[2] << 16) | ((uint32_t)yp[3] << 24);
        const uint8_t* cp = yp + cofs;
        cw = (uint32_t)cp[0] | ((uint32_t)cp[1] << 8) | ((uint32_t)cp[2] << 16) | ((uint32_t)cp[3] << 24);
      }
    }
    // chroma bytes V0 U0 V1 U1 (V even, U odd: MSEQ:279-282); pixel j as Y | U << 8 | V << 24
    uint32_t bin[4];
    bin[0] = mxn_bin(__builtin_amdgcn_perm(cw, yw, 0x040c0500u), l43, l255);
    bin[1] = mxn_bin(__builtin_amdgcn_perm(cw, yw, 0x040c0501u), l43, l255);
    bin[2] = mxn_bin(__builtin_amdgcn_perm(cw, yw, 0x060c0702u), l43, l255);
    bin[3] = mxn_bin(__builtin_amdgcn_perm(cw, yw, 0x060c0703u), l43, l255);
    // the lane's pixels inside the cell's columns: j_lo <= j < j_hi
    const int j_lo = ok ? max(c0 - col4, 0) : 0, j_hi = ok ? min(c1 - col4, 4) : 0;
    const uint32_t pos0 = rr * (uint32_t)a.col_step + (uint32_t)(col4 - c0) + 1u;  // pos1 of pixel j: pos0 + j
#pragma unroll
    for (int j = 0; j < 4; ++j)
      mxn_vote(j >= j_lo && j < j_hi, bin[j], pos0 + (uint32_t)j, cnt[wave], lst[wave], lane);
  }
  __syncthreads();

  // C = the largest count; then the smallest last position among the bins at
  // C (positions are distinct; an empty cell has every bin at 0 and takes bin 0)
  uint32_t c[2], l[2];
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int b = tid + kMxnBlock * u;
    c[u] = 0u;
    l[u] = 0u;
#pragma unroll
    for (int w = 0; w < kMxnWaves; ++w) {
      c[u] += cnt[w][b];
      l[u] = max(l[u], lst[w][b]);
    }
  }
  uint32_t cmax = max(c[0], c[1]);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) cmax = max(cmax, (uint32_t)__shfl_xor((int)cmax, off, 64));
  if (lane == 0) red_c[wave] = cmax;
  __syncthreads();
  cmax = red_c[0];
#pragma unroll
  for (int w = 1; w < kMxnWaves; ++w) cmax = max(cmax, red_c[w]);
  unsigned long long key = ~0ull;
#pragma unroll
  for (int u = 0; u < 2; ++u)
    if (c[u] == cmax) {
      const unsigned long long k2 = ((unsigned long long)l[u] << 9) | (unsigned long long)(tid + kMxnBlock * u);
      key = k2 < key ? k2 : key;
    }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned long long o = __shfl_xor(key, off, 64);
    key = o < key ? o : key;
  }
  if (lane == 0) red_k[wave] = key;
  __syncthreads();
  if (tid == 0) {
    key = red_k[0];
#pragma unroll
    for (int w = 1; w < kMxnWaves; ++w) key = red_k[w] < key ? red_k[w] : key;
    const uint32_t winner = (uint32_t)key & (uint32_t)(kMxnBins - 1);
    a.colors[blockIdx.x] = (int32_t)a.table[winner];
    if (a.bins) a.bins[blockIdx.x] = (uint16_t)winner;
  }
}

// The highest cell index along one axis whose square [start, start + 19],
// each coordinate clamped to the image (MSEQ:355-366), maps onto output
// coordinate o, or -1.  The map is monotone, so the source coordinates that
// map onto o are one interval: the clamped square [lo, hi] meets it iff
// map[lo] <= o <= map[hi] and some coordinate maps onto o at all.
__device__ __forceinline__ int mxn_square_cell(int o, int n_cells, int step, int size, const uint32_t* map) {
  for (int i = n_cells - 1; i >= 0; --i) {
    const int lo = min(i * step, size - 1), hi = min(i * step + 19, size - 1);
    if ((int)map[lo] <= o && o <= (int)map[hi]) return i;
  }
  return -1;
}

__global__ __launch_bounds__(256) void mxn_preview_kernel(MxnPreviewArgs a, uint32_t blocks_per_row) {
  // a block: 256 two-byte units of one output row of one frame
  const uint32_t rb = blockIdx.x / blocks_per_row;
  const int x = (int)((blockIdx.x - rb * blocks_per_row) * 256u + threadIdx.x);
  const int f = (int)(rb / (uint32_t)a.out_h), ro = (int)(rb - (uint32_t)f * (uint32_t)a.out_h);
  if (2 * x >= a.out_ll) return;
  uint32_t v = 0u;
  if (x < a.out_w) {
    const int sr = a.last_row[ro], sc = a.last_col[x];
    if (sr >= 0 && sc >= 0) {
      int Y, U, V;
      fetch_yuv(frame_ptr(a, f), a.height, a.line_length, TRIK_HSV_LAYOUT_OV7670, sr, sc, Y,
                U, V);
      uint32_t rgb = pixel_rgb(Y, U, V).rgb888();
      const int ci = mxn_square_cell(ro, a.rows_m, a.row_step, a.height, a.hi2ho);
      const int cj = ci >= 0 ? mxn_square_cell(x, a.cols_n, a.col_step, a.width, a.wi2wo) : -1;
      if (cj >= 0) rgb = (uint32_t)a.colors[(int64_t)f * a.rows_m * a.cols_n + ci * a.cols_n + cj];
      v = ((rgb >> 19) & 0x001fu) | ((rgb >> 5) & 0x07e0u) | ((rgb << 8) & 0xf800u);  // write_px565
    }
  }
  uint8_t* dst = a.previews + (int64_t)f * a.preview_stride + (int64_t)ro * a.out_ll + 2 * x;
  dst[0] = (uint8_t)v;
  if (2 * x + 1 < a.out_ll) dst[1] = (uint8_t)(v >> 8);
}

}  // namespace

// A launch holds fewer than 2^32 threads (the grid size is a 32-bit thread
// count): larger batches go in several launches of whole frames.
constexpr int64_t kMaxLaunchBlocks = 0xFFFFFFFFll / 256;

int launch_mxn(const MxnArgs& a, hipStream_t s) {
  if (a.n_frames <= 0) return hipSuccess;
  const int64_t cells = (int64_t)a.rows_m * a.cols_n;
  MxnGeom g;
  // groups per cell row: ceil(col_step / 4), one more for a cell that starts inside a group
  const uint32_t gpr = a.col_step > 0 ? (uint32_t)(a.col_step + 3) / 4u + 1u : 1u;
  g.per_row = make_div(gpr);
  const uint64_t total = a.col_step > 0 ? (uint64_t)gpr * (uint32_t)a.row_step : 0u;
  if (total > 0x7FFFFFFFu) return hipErrorInvalidValue;
  g.total = (uint32_t)total;
  static_assert(kMxnBlock == 256, "kMaxLaunchBlocks");
  const int64_t per_launch = kMaxLaunchBlocks / cells;  // frames (cells <= 100)
  for (int64_t f0 = 0; f0 < a.n_frames; f0 += per_launch) {
    MxnArgs b = a;
    b.narrow(f0, a.n_frames - f0 < per_launch ? a.n_frames - f0 : per_launch);
    b.colors = a.colors + f0 * cells;
    if (a.bins) b.bins = a.bins + f0 * cells;
    hipLaunchKernelGGL(mxn_hist_kernel, dim3((unsigned)(b.n_frames * cells)), dim3(kMxnBlock), 0, s, b, g);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

int launch_mxn_preview(const MxnPreviewArgs& a, hipStream_t s) {
  if (a.n_frames <= 0 || a.out_h <= 0 || a.out_ll <= 0) return hipSuccess;
  const uint32_t bpr = (uint32_t)(((int64_t)a.out_ll + 1) / 2 + 255) / 256u;
  const int64_t per_frame = (int64_t)a.out_h * bpr;
  if (per_frame > kMaxLaunchBlocks) return hipErrorInvalidValue;
  const int64_t per_launch = kMaxLaunchBlocks / per_frame;
  for (int64_t f0 = 0; f0 < a.n_frames; f0 += per_launch) {
    MxnPreviewArgs b = a;
    b.narrow(f0, a.n_frames - f0 < per_launch ? a.n_frames - f0 : per_launch);
    b.colors = a.colors + f0 * a.rows_m * a.cols_n;
    b.previews = a.previews + f0 * a.preview_stride;
    hipLaunchKernelGGL(mxn_preview_kernel, dim3((unsigned)(b.n_frames * per_frame)), dim3(256), 0, s, b, bpr);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace trik_hsv
