// trik_hsv_autorange.hip -- deterministic autoDetectHsv of the ov7670 object
// sensor and the two line sensors (ODET, LDET, LDETW as in
// include/trik_hsv.h).
//
//  auto_exact_kernel  one workgroup per frame, three parts:
//   1. The detector's score histogram (ODET:200-227, LDET:215-240) in LDS: +1
//      per pixel of the positive zone, -2 per pixel of the negative zone, and
//      its start cell.  The reference raises max_value whenever a positive
//      increment lifts a cell's running value above it, in raster order with
//      the decrements interleaved.  In a row that holds positive pixels (a
//      band row) a cell's events come as left negatives, positives, right
//      negatives, so within the row its running value peaks right after its
//      last positive pixel:
//        peak_c(r) = value_c(before row r) - 2 leftneg_c(r) + pos_c(r).
//      With G the largest peak, the start cell is the cell of the earliest
//      (r, column of the cell's last positive pixel of row r) among the peaks
//      equal to G; no positive peak leaves max_value 0 and cell 0.  So the
//      rows before the band fold in one phase with plain LDS atomics; each
//      band row adds its left negatives and positives (and atomicMax of the
//      column per cell), a per-cell pass reads the peaks and then applies the
//      row's right negatives (counted aside meanwhile); the rows after the
//      band fold in one phase.  Two barriers per band row.
//   2. The exact search (when asked for): the weights score != 0 ? score :
//      -K0 as a prefix sum in LDS, every candidate box in O(1), the best by
//      one packed 64-bit key (L, then the tie rule) through an LDS atomicMax.
//   3. The reference's output scaling (auto_range_scale).
//  One shape for every geometry: the case list of tests/autorange_cases.py
//  reaches each phase (no band, band with and without side negatives).
#include <hip/hip_runtime.h>

#include "trik_hsv_internal.h"
#include "trik_hsv_pixel.h"

namespace trik_hsv {

namespace {

constexpr int kAutoBlock = 256;

// The histogram bin of pixel (row, col): (H >> 3) * 32 + (S >> 3) for the
// object kind, V for the line kinds (only the max channel is computed then).
template <bool OBJECT>
__device__ __forceinline__ int auto_cell(const uint8_t* fr, const AutoExactArgs& a, int row, int col,
                                         const uint16_t* l43, const uint16_t* l255) {
  int Y, U, V;
  fetch_yuv(fr, a.height, a.line_length, a.layout, row, col, Y, U, V);
  const PixelRgb p = pixel_rgb(Y, U, V);
  if (!OBJECT) return max(p.r, max(p.g, p.b));
  uint32_t H, S, Vv;
  pixel_hsv_bytes(p, l43, l255, H, S, Vv);
  return (int)(((H >> 3) << 5) | (S >> 3));
}

template <bool OBJECT>
__global__ __launch_bounds__(kAutoBlock) void auto_exact_kernel(AutoExactArgs a) {
  constexpr int kBins = OBJECT ? kAutoObjectBins : kAutoLineBins;
  constexpr int kPrefix = OBJECT ? 33 * 33 : 257;
  __shared__ int32_t hist[kBins];      // the running values
  __shared__ int32_t last_col[kBins];  // band row: the cell's last positive column, or -1
  __shared__ int32_t rneg[kBins];      // band row: the cell's right negatives
  __shared__ int32_t pre[kPrefix];     // the search's prefix sums
  __shared__ uint16_t l43[256], l255[256];
  __shared__ unsigned long long top;   // start cell, then the search: the best key
  __shared__ int32_t start_cell[2];    // cell, max_value
  const int f = blockIdx.x, tid = threadIdx.x;
  const int W = a.width, H = a.height;
  const uint8_t* fr = frame_ptr(a, f);
  for (int i = tid; i < kBins; i += kAutoBlock) {
    hist[i] = 0;
    last_col[i] = -1;
    rneg[i] = 0;
  }
  stage_luts(l43, l255, tid, kAutoBlock);
  if (tid == 0) {
    top = 0;
    start_cell[0] = 0;
    start_cell[1] = 0;
  }
  __syncthreads();

  // the positive pixels: columns [pc0, pc1) of the band rows [pr0, pr1)
  const int pc0 = max(a.pc_lo + 1, 0), pc1 = min(a.pc_hi, W);
  int pr0 = max(a.pr_lo + 1, 0), pr1 = min(a.pr_hi, H);
  if (pc0 >= pc1 || pr0 >= pr1) pr0 = pr1 = H;  // no positive pixel: every row folds below
  auto negative = [&](int row, int col) {
    return col < a.nc_lo || col > a.nc_hi || row < a.nr_lo || row > a.nr_hi;
  };
  // rows [r0, r1) without a positive pixel: the negatives alone, any order
  auto fold = [&](int r0, int r1) {
    if (r1 <= r0 || W <= 0) return;
    const int64_t n = (int64_t)(r1 - r0) * W;
    int row = r0 + tid / W, col = tid % W;
    const int dq = kAutoBlock / W, dr = kAutoBlock % W;
    for (int64_t i = tid; i < n; i += kAutoBlock) {
      if (negative(row, col)) atomicSub(&hist[auto_cell<OBJECT>(fr, a, row, col, l43, l255)], 2);
      col += dr;
      row += dq;
      if (col >= W) {
        col -= W;
        ++row;
      }
    }
  };
  fold(0, pr0);
  // the band: this thread's best peak (> 0), its scan position and its cell
  int best_g = 0, best_cell = 0;
  uint32_t best_pos = 0xFFFFFFFFu;
  for (int row = pr0; row < pr1; ++row) {
    for (int col = tid; col < W; col += kAutoBlock) {
      const bool pos = col >= pc0 && col < pc1;
      if (!pos && !negative(row, col)) continue;
      const int c = auto_cell<OBJECT>(fr, a, row, col, l43, l255);
      if (pos) {
        atomicAdd(&hist[c], 1);
        atomicMax(&last_col[c], col);
      } else if (col < pc0) {
        atomicSub(&hist[c], 2);
      } else {
        atomicAdd(&rneg[c], 1);
      }
    }
    __syncthreads();
    for (int c = tid; c < kBins; c += kAutoBlock) {
      const int lc = last_col[c];
      if (lc >= 0) {
        const int peak = hist[c];
        const uint32_t pos = (uint32_t)row * (uint32_t)W + (uint32_t)lc;
        if (peak > 0 && (peak > best_g || (peak == best_g && pos < best_pos))) {
          best_g = peak;
          best_pos = pos;
          best_cell = c;
        }
        last_col[c] = -1;
      }
      const int rn = rneg[c];
      if (rn) {
        hist[c] -= 2 * rn;
        rneg[c] = 0;
      }
    }
    __syncthreads();
  }
  fold(pr1, H);
  // the largest peak, then the earliest position (positions are distinct)
  const unsigned long long key = ((unsigned long long)(uint32_t)best_g << 32) | (0xFFFFFFFFu - best_pos);
  if (best_g > 0) atomicMax(&top, key);
  __syncthreads();
  if (best_g > 0 && top == key) {
    start_cell[0] = best_cell;
    start_cell[1] = best_g;
  }
  __syncthreads();
  const int sc = start_cell[0];
  if (a.scores)
    for (int i = tid; i < kBins; i += kAutoBlock) a.scores[(int64_t)f * kBins + i] = hist[i];
  if (a.start && tid == 0) {
    int32_t* st = a.start + (int64_t)f * 4;
    st[0] = OBJECT ? sc >> 5 : sc;
    st[1] = OBJECT ? sc & 31 : 0;
    st[2] = start_cell[1];
    st[3] = 0;
  }
  if (!a.out) return;

  // the search: weights, their prefix sums, every candidate
  constexpr int kK0 = OBJECT ? 2 : 1;
  if (tid == 0) top = 0;
  unsigned long long mine = 0;
  if (OBJECT) {
    // pre[(h + 1) * 33 + s + 1] = the weights of hues 0..h, saturations 0..s
    for (int i = tid; i < 33; i += kAutoBlock) {
      pre[i] = 0;
      pre[i * 33] = 0;
    }
    if (tid < 32) {
      int run = 0;
      for (int s = 0; s < 32; ++s) {
        const int v = hist[tid * 32 + s];
        run += v != 0 ? v : -kK0;
        pre[(tid + 1) * 33 + s + 1] = run;
      }
    }
    __syncthreads();
    if (tid < 32) {
      int run = 0;
      for (int h = 0; h < 32; ++h) {
        run += pre[(h + 1) * 33 + tid + 1];
        pre[(h + 1) * 33 + tid + 1] = run;
      }
    }
    __syncthreads();
    const int s_max = sc & 31, ns2 = 32 - s_max, total = (s_max + 1) * ns2 * 1024;
    auto rect = [&](int ha, int hb, int sa, int sb) {  // hues ha..hb, saturations sa..sb
      return pre[(hb + 1) * 33 + sb + 1] - pre[ha * 33 + sb + 1] - pre[(hb + 1) * 33 + sa] + pre[ha * 33 + sa];
    };
    for (int i = tid; i < total; i += kAutoBlock) {
      const int h2 = i & 31, h1 = (i >> 5) & 31, q = i >> 10, s1 = q / ns2, s2 = s_max + (q - s1 * ns2);
      int L, nh;
      if (h1 <= h2) {
        L = rect(h1, h2, s1, s2);
        nh = h2 - h1 + 1;
      } else {
        L = rect(h1, 31, s1, s2) + rect(0, h2, s1, s2);
        nh = 32 - h1 + h2 + 1;
      }
      const uint32_t cells = (uint32_t)(nh * (s2 - s1 + 1));
      const unsigned long long k = ((unsigned long long)((uint32_t)L + 0x80000000u) << 32) |
                                   ((1024u - cells) << 15) | ((uint32_t)(31 - h1) << 10) |
                                   ((uint32_t)(31 - s1) << 5) | (uint32_t)(31 - h2);
      mine = k > mine ? k : mine;
    }
  } else {
    // pre[v + 1] = the weights of values 0..v (an inclusive scan over the block)
    static_assert(kAutoBlock == kAutoLineBins, "one value per thread");
    const int v = hist[tid];
    int run = v != 0 ? v : -kK0;
    if (tid == 0) pre[0] = 0;
    pre[tid + 1] = run;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {
      const int add = tid >= d ? pre[tid + 1 - d] : 0;
      __syncthreads();
      run += add;
      pre[tid + 1] = run;
      __syncthreads();
    }
    const int v0 = tid;  // this thread's intervals start here
    for (int v1 = v0; v1 < 256; ++v1) {
      const int L = pre[v1 + 1] - pre[v0];
      const unsigned long long k = ((unsigned long long)((uint32_t)L + 0x80000000u) << 32) |
                                   ((uint32_t)(255 - (v1 - v0)) << 8) | (uint32_t)(255 - v0);
      mine = k > mine ? k : mine;
    }
  }
  atomicMax(&top, mine);
  __syncthreads();
  if (tid == 0) {
    const unsigned long long k = top;
    const int L = (int)((uint32_t)(k >> 32) - 0x80000000u);
    const uint32_t lo = (uint32_t)k;
    int h1, h2, s1, s2;
    if (OBJECT) {
      h1 = 31 - (int)((lo >> 10) & 31);
      s1 = 31 - (int)((lo >> 5) & 31);
      h2 = 31 - (int)(lo & 31);
      const int cells = 1024 - (int)(lo >> 15), nh = h1 <= h2 ? h2 - h1 + 1 : 32 - h1 + h2 + 1;
      s2 = s1 + cells / nh - 1;
    } else {
      h1 = 255 - (int)(lo & 255);
      h2 = h1 + 255 - (int)((lo >> 8) & 255);
      s1 = s2 = 0;
    }
    auto_range_scale(a.kind, h1, h2, s1, s2, a.out + (int64_t)f * 6);
    if (a.best) {
      int32_t* b = a.best + (int64_t)f * 5;
      b[0] = L;
      b[1] = h1;
      b[2] = h2;
      b[3] = s1;
      b[4] = s2;
    }
  }
}

}  // namespace

int launch_auto_exact(const AutoExactArgs& a, hipStream_t s) {
  if (a.n_frames <= 0) return hipSuccess;
  if (a.kind == TRIK_HSV_AUTO_OV7670_OBJECT)
    hipLaunchKernelGGL(auto_exact_kernel<true>, dim3((unsigned)a.n_frames), dim3(kAutoBlock), 0, s, a);
  else
    hipLaunchKernelGGL(auto_exact_kernel<false>, dim3((unsigned)a.n_frames), dim3(kAutoBlock), 0, s, a);
  return (int)hipGetLastError();
}

}  // namespace trik_hsv
