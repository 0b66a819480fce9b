// trik_hsv_edge.hip -- the ov7670 edge-line sensor, ESEQ =
// trik/ov7670/edge_line_sensor/include/internal/cv_ball_detector_seqpass.hpp.
// The three IMGLIB calls of ESEQ:179-232 are restated from TI's documented
// natural-C semantics:
//
//  IMG_sobel_3x3_8(in, out, w, h)   for i in 0 .. w*(h-2)-3, over the image as
//                       one linear array: H = -in[i] - 2in[i+1] - in[i+2] +
//                       in[i+2w] + 2in[i+2w+1] + in[i+2w+2], V = -in[i] + in[i+2]
//                       - 2in[i+w] + 2in[i+w+2] - in[i+2w] + in[i+2w+2],
//                       out[i+1] = min(|H| + |V|, 255).  Output (r, c) is the
//                       window whose top-left is (r, c-1); columns 0 and w-1 mix
//                       adjacent rows; out[0], out[w*(h-2)-1] and the last two
//                       rows are never written (0 here).
//  IMG_thr_gt2max_8     out = out > thr ? 255 : out; detected iff 255.
//  IMG_ycbcr422pl_to_rgb565   edge_rgb565 below.
//
//  edge_vec_kernel      the fast form: a lane owns 4Q columns and walks rows
//                       with a three-row window of the separable row terms
//                       s = a[c-1] + 2a[c] + a[c+1], d = a[c+1] - a[c-1] in
//                       packed 16-bit lanes (H = s(r+2) - s(r), V = d(r) +
//                       2d(r+1) + d(r+2)); the Y plane only, each byte once
//                       per row segment (+ 2 halo rows), column halos from the
//                       neighbour lanes.  One lane group spans a whole row, so
//                       the row's count and column sum are formed (and the
//                       column sum wrapped mod 65536) before rows are added.
//  edge_map_kernel      generic form (misaligned input, or the map asked for):
//                       one workgroup per row, the linear-array loop as
//                       written, wrap columns and zero bytes included.
//  edge_targets_kernel  OutArgs of ESEQ:397-417.
//  edge_preview_kernel  the preview by the inverse maps (ESEQ:236-249): the
//                       thresholded map as luma with the frame's chroma through
//                       edge_rgb565, then the target line (ESEQ:405).
#include <hip/hip_runtime.h>

#include "trik_hsv_internal.h"
#include "trik_hsv_wave.h"

namespace trik_hsv {

namespace {

constexpr int kEdgeBlock = 256;

// Byte i of the thresholded map of one frame (`in`: its Y plane, w * h bytes;
// last = w * (h - 2) - 3, the last window of the Sobel loop).
__device__ __forceinline__ uint32_t edge_byte(const uint8_t* in, int w, int64_t i, int64_t last, int thr) {
  const int64_t j = i - 1;  // out[j + 1] is window j
  if (j < 0 || j > last) return 0u;
  const uint8_t* p = in + j;
  const int a00 = p[0], a01 = p[1], a02 = p[2];
  const int a10 = p[w], a12 = p[w + 2];
  const int a20 = p[2 * w], a21 = p[2 * w + 1], a22 = p[2 * w + 2];
  const int H = -a00 - 2 * a01 - a02 + a20 + 2 * a21 + a22;
  const int V = -a00 + a02 - 2 * a10 + 2 * a12 - a20 + a22;
  const int O = min(abs(H) + abs(V), 255);
  return O > thr ? 255u : (uint32_t)O;
}

// IMG_ycbcr422pl_to_rgb565 of one pixel with the codec's coefficients
// {0x2000, 0x2BDD, -0x0AC5, -0x1658, 0x3770} (ESEQ:227-232): plain RGB565.
__device__ __forceinline__ uint32_t edge_rgb565(int y, int cb, int cr) {
  const int yt = 0x2000 * (y - 16);
  cb -= 128;
  cr -= 128;
  const int r = min(max((yt + 0x2BDD * cr) >> 13, 0), 255);
  const int g = min(max((yt - 0x0AC5 * cb - 0x1658 * cr) >> 13, 0), 255);
  const int b = min(max((yt + 0x3770 * cb) >> 13, 0), 255);
  return (uint32_t)(((r >> 3) << 11) | ((g >> 2) << 5) | (b >> 3));
}

// OutArgs of ESEQ:397-417 from a frame's sums; targetY is always the frame's
// top (m_targetY stays 0).
__device__ __forceinline__ TrikHsvTarget edge_target_of(const TrikHsvTargetSums& s, int width, int height) {
  TrikHsvTarget t = {0, 0, 0, 0};
  const uint32_t n = (uint32_t)s.points;
  if (n > 0) {
    const int32_t tx = (int32_t)((uint32_t)(int32_t)s.sum_x / n);
    const uint32_t radius = (uint32_t)ceilf(__fsqrt_rn(__fdiv_rn((float)n, 3.1415927f)));
    t.x = (int8_t)(((tx - width / 2) * 100 * 2) / width);
    t.y = (int8_t)(((0 - height / 2) * 100 * 2) / height);
    t.size = (uint8_t)((uint32_t)(radius * 100 * 4) / (uint32_t)(width + height));
  }
  return t;
}

// ---------------------------------------------------------------------------
// edge_vec_kernel.  A lane holds 4Q consecutive columns of one row (Q dwords)
// as 2Q packed pairs (lo half = the lower column).  With the bytes b[0 .. 4Q)
// and the neighbours' L = b[-1], R = b[4Q]:
//   a0[g] = (b[2g], b[2g+1])      m[g] = (b[2g-1], b[2g])      g = 0 .. 2Q
//   s[g] = m[g] + 2 a0[g] + m[g+1]     d[g] = m[g+1] - m[g]
// All of s, d, H, V, H +- V lie in int16.  |H| + |V| = max(|H+V|, |H-V|), and
// for 0 <= t <= 254, |x| > t iff (u16)(x + t) > 2t, so the pixel is detected
// (O > thr or O >= 255, i.e. |H| + |V| > t = min(thr, 254)) iff
// max_u16(H + t + V, H + t - V) > 2t: a saturating subtract of 2t, cut to the
// window mask (1 inside columns 16 .. W-16, ESEQ:196), is the detection flag.
// The window never takes a column whose stencil crosses a row end, so lane
// 0's L and the last lane's R (and those of idle lanes) are never used.
// Q is chosen per width so that a row's lanes fill a group of 16, 32 or 64
// (320 and 640 columns: Q = 5, 16 and 32 lanes); the next row's loads are in
// flight while a row is computed.
// ---------------------------------------------------------------------------
struct EdgeGeom {
  int32_t lanes_per_row;  // width / (4Q) <= 64
  int32_t group;          // lanes a row's group takes in a wave: 16, 32 or 64
  int32_t segs;           // row segments per frame
  int32_t seg_rows;       // output rows per segment
  int32_t t;              // min(threshold, 254)
};

template <int CTRL>
__device__ __forceinline__ uint32_t edge_dpp_add(uint32_t v) {
  return v + (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xf, 0xf, false);
}

// the sum over each aligned group of `group` lanes, in every lane of it
__device__ __forceinline__ uint32_t edge_group_sum(uint32_t v, int group) {
  v = edge_dpp_add<0xB1>(v);   // quad_perm [1, 0, 3, 2]
  v = edge_dpp_add<0x4E>(v);   // quad_perm [2, 3, 0, 1]
  v = edge_dpp_add<0x141>(v);  // row_half_mirror
  v = edge_dpp_add<0x140>(v);  // row_mirror
  if (group > 16) v += __shfl_xor(v, 16, 64);
  if (group > 32) v += __shfl_xor(v, 32, 64);
  return v;
}

template <int Q>
__device__ __forceinline__ void edge_load_row(const uint8_t* p, uint32_t (&D)[Q]) {
  if constexpr (Q % 2 == 0) {
#pragma unroll
    for (int u = 0; u < Q / 2; ++u) {
      typedef unsigned int v2 __attribute__((ext_vector_type(2)));
      const v2 y = __builtin_nontemporal_load(reinterpret_cast<const v2*>(p) + u);
      D[2 * u] = y.x;
      D[2 * u + 1] = y.y;
    }
  } else {
#pragma unroll
    for (int q = 0; q < Q; ++q) D[q] = __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(p) + q);
  }
}

template <int Q>
__global__ __launch_bounds__(kEdgeBlock) void edge_vec_kernel(EdgeArgs a, EdgeGeom g) {
  constexpr int G = 2 * Q;  // packed pairs per lane
  const int lane = threadIdx.x & 63;
  const int64_t wave = (int64_t)blockIdx.x * (kEdgeBlock / 64) + (threadIdx.x >> 6);
  const int gl = lane & (g.group - 1);
  const int64_t gid = wave * (64 / g.group) + lane / g.group;  // (frame, segment)
  const bool live_group = gid < (int64_t)a.n_frames * g.segs;
  const int64_t gidc = live_group ? gid : 0;
  const int f = (int)(gidc / g.segs), seg = (int)(gidc - (int64_t)f * g.segs);
  const int r0 = seg * g.seg_rows;
  const int out_rows = live_group ? min(a.height - 2, r0 + g.seg_rows) - r0 : 0;
  const int in_rows = live_group ? out_rows + 2 : 1;  // rows r0 .. r0 + out_rows + 1 <= height - 1
  const bool live = live_group && gl < g.lanes_per_row;
  const int w = a.width;
  const int c0 = live ? gl * 4 * Q : 0;  // (idle lanes read columns 0 .. 4Q-1 and count nothing)
  const uint8_t* p = frame_ptr(a, f) + (int64_t)r0 * w + c0;

  u16x2 mask[G], colpk[G];
#pragma unroll
  for (int i = 0; i < G; ++i) {
    const int c = c0 + 2 * i;
    mask[i] = u16x2{(unsigned short)(live && c >= 16 && c <= w - 16), (unsigned short)(live && c + 1 >= 16 && c + 1 <= w - 16)};
    colpk[i] = u16x2{(unsigned short)c, (unsigned short)(c + 1)};
  }
  const u16x2 tt = (u16x2)(unsigned short)g.t;
  const uint32_t t2 = (uint32_t)(2 * g.t) * 0x00010001u;

  u16x2 s1[G] = {}, s2t[G] = {}, d1[G] = {}, e1[G] = {};
  uint32_t n_sum = 0, x_sum = 0;
  const int iters = g.seg_rows + 2;  // uniform over the wave
  uint32_t Dn[Q];
  edge_load_row<Q>(p, Dn);
  for (int k = 0; k < iters; ++k) {
    uint32_t D[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) D[q] = Dn[q];
    p += k + 1 < in_rows ? w : 0;  // (past its rows a lane re-reads its last one)
    if (k + 1 < iters) edge_load_row<Q>(p, Dn);
    const uint32_t L = (uint32_t)__shfl_up((int)D[Q - 1], 1, 64);
    const uint32_t R = (uint32_t)__shfl_down((int)D[0], 1, 64);
    u16x2 m[G + 1], sc[G], dc[G];
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      m[2 * q] = __builtin_bit_cast(u16x2, __builtin_amdgcn_perm(D[q], q ? D[q - 1] : L, 0x0c040c03u));
      m[2 * q + 1] = __builtin_bit_cast(u16x2, __builtin_amdgcn_perm(0u, D[q], 0x0c020c01u));
    }
    m[G] = __builtin_bit_cast(u16x2, __builtin_amdgcn_perm(R, D[Q - 1], 0x0c040c03u));
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      const u16x2 lo = __builtin_bit_cast(u16x2, __builtin_amdgcn_perm(0u, D[q], 0x0c010c00u));
      const u16x2 hi = __builtin_bit_cast(u16x2, __builtin_amdgcn_perm(0u, D[q], 0x0c030c02u));
      sc[2 * q] = lo * (unsigned short)2 + m[2 * q] + m[2 * q + 1];
      sc[2 * q + 1] = hi * (unsigned short)2 + m[2 * q + 1] + m[2 * q + 2];
    }
#pragma unroll
    for (int i = 0; i < G; ++i) dc[i] = m[i + 1] - m[i];
    if (k >= 2) {  // output row r0 + k - 2 from input rows k-2 (s2t, in e1), k-1 (in e1) and k
      u16x2 nacc = {0, 0}, xacc = {0, 0};
#pragma unroll
      for (int i = 0; i < G; ++i) {
        const u16x2 ht = sc[i] - s2t[i];  // H + t
        const u16x2 ec = d1[i] + dc[i];
        const u16x2 v = e1[i] + ec;
        e1[i] = ec;
        const u16x2 mx = __builtin_elementwise_max((u16x2)(ht + v), (u16x2)(ht - v));
        uint32_t fl;
        asm("v_pk_sub_u16 %0, %1, %2 clamp\n\tv_pk_min_u16 %0, %0, %3"
            : "=&v"(fl)
            : "v"(__builtin_bit_cast(uint32_t, mx)), "v"(t2), "v"(__builtin_bit_cast(uint32_t, mask[i])));
        const u16x2 fm = __builtin_bit_cast(u16x2, fl);
        nacc += fm;
        xacc += fm * colpk[i];
      }
      const uint32_t nw = __builtin_bit_cast(uint32_t, nacc), xw = __builtin_bit_cast(uint32_t, xacc);
      // the row's part of this lane: column sum < 2^21 in the low bits, count < 2^11 above
      uint32_t val = ((xw & 0xffffu) + (xw >> 16)) | (((nw & 0xffffu) + (nw >> 16)) << 21);
      val = k - 2 < out_rows ? val : 0u;
      val = edge_group_sum(val, g.group);
      n_sum += val >> 21;
      x_sum += val & 0xffffu;  // targetPointsCol is a uint16_t (ESEQ:161)
    } else {
#pragma unroll
      for (int i = 0; i < G; ++i) e1[i] = d1[i] + dc[i];
    }
#pragma unroll
    for (int i = 0; i < G; ++i) {
      s2t[i] = s1[i] - tt;
      s1[i] = sc[i];
      d1[i] = dc[i];
    }
  }
  if (live_group && gl == 0) {
    TrikHsvTargetSums* d = a.sums + f;
    if (n_sum) atomicAdd(reinterpret_cast<unsigned long long*>(&d->points), (unsigned long long)n_sum);
    if (x_sum) atomicAdd(reinterpret_cast<unsigned long long*>(&d->sum_x), (unsigned long long)x_sum);
  }
}

// one workgroup per (frame, row): the map's bytes of that row and the row's sums
__global__ __launch_bounds__(kEdgeBlock) void edge_map_kernel(EdgeArgs a) {
  __shared__ uint32_t red[2][kEdgeBlock / 64];
  const int f = blockIdx.x / a.height, r = blockIdx.x - f * a.height;
  const uint8_t* in = frame_ptr(a, f);
  const int w = a.width;
  const int64_t last = (int64_t)w * (a.height - 2) - 3;
  uint32_t n = 0, sx = 0;
  for (int c = threadIdx.x; c < w; c += kEdgeBlock) {
    const uint32_t v = edge_byte(in, w, (int64_t)r * w + c, last, a.threshold);
    if (a.edges) a.edges[((int64_t)f * a.height + r) * w + c] = (uint8_t)v;
    if (v == 255u && c >= 16 && c <= w - 16) {  // ESEQ:196-199
      n += 1u;
      sx += (uint32_t)c;
    }
  }
  n = wave_sum(n);
  sx = wave_sum(sx);
  if ((threadIdx.x & 63) == 0) {
    red[0][threadIdx.x >> 6] = n;
    red[1][threadIdx.x >> 6] = sx;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    n = sx = 0;
#pragma unroll
    for (int i = 0; i < kEdgeBlock / 64; ++i) {
      n += red[0][i];
      sx += red[1][i];
    }
    n &= 0xffffu;  // both per-row accumulators are uint16_t (ESEQ:160-161)
    sx &= 0xffffu;
    TrikHsvTargetSums* d = a.sums + f;
    if (n) atomicAdd(reinterpret_cast<unsigned long long*>(&d->points), (unsigned long long)n);
    if (sx) atomicAdd(reinterpret_cast<unsigned long long*>(&d->sum_x), (unsigned long long)sx);
  }
}

__global__ void edge_targets_kernel(int n_frames, int width, int height, const TrikHsvTargetSums* sums,
                                    TrikHsvTarget* targets) {
  const int f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= n_frames) return;
  targets[f] = edge_target_of(sums[f], width, height);
}

__global__ __launch_bounds__(256) void edge_preview_kernel(EdgePreviewArgs a, uint32_t blocks_per_row) {
  // a block: 256 two-byte units of one output row of one frame
  const uint32_t rb = blockIdx.x / blocks_per_row;
  const int x = (int)((blockIdx.x - rb * blocks_per_row) * 256u + threadIdx.x);
  const int f = (int)(rb / (uint32_t)a.out_h), ro = (int)(rb - (uint32_t)f * (uint32_t)a.out_h);
  if (2 * x >= a.out_ll) return;
  uint32_t v = 0u;
  if (x < a.out_w) {
    const int sr = a.last_row[ro], sc = a.last_col[x];
    if (sr >= 0 && sc >= 0) {
      const int w = a.width, h = a.height;
      const uint8_t* in = frame_ptr(a, f);
      const int64_t i = (int64_t)sr * w + sc;
      const int y = (int)edge_byte(in, w, i, (int64_t)w * (h - 2) - 3, a.threshold);
      const uint8_t* cbcr = in + (int64_t)w * h + 2 * (i >> 1);  // cb = byte 2k, cr = byte 2k + 1 (ESEQ:166-173)
      v = edge_rgb565(y, cbcr[0], cbcr[1]);
      // drawRgbTargetCenterLine(targetX, height / 2, 0xff0000), ESEQ:405: the
      // row map is monotone, so the clamped rows [lo, hi] reach output row ro
      // iff hi2ho[lo] <= ro <= hi2ho[hi] (some source row maps onto ro: sr >= 0)
      const TrikHsvTargetSums s = a.sums[f];
      const uint32_t n = (uint32_t)s.points;
      if (n > 0) {
        const int32_t tx = (int32_t)((uint32_t)(int32_t)s.sum_x / n);
        const int col = tx < 0 ? 0 : (tx > w - 1 ? w - 1 : tx);
        const int lo = max(h / 2 - 99, 0), hi = min(h / 2 + 99, h - 1);
        if ((int)a.wi2wo[col] == x && (int)a.hi2ho[lo] <= ro && ro <= (int)a.hi2ho[hi]) v = 0x001fu;
      }
    }
  }
  uint8_t* dst = a.previews + (int64_t)f * a.preview_stride + (int64_t)ro * a.out_ll + 2 * x;
  dst[0] = (uint8_t)v;
  if (2 * x + 1 < a.out_ll) dst[1] = (uint8_t)(v >> 8);
}

}  // namespace

// Lanes and row segments for edge_vec_kernel; false: the generic kernel
// (frames or stride not 8-byte aligned, or a width past 64 lanes of 32 columns).
// q: dwords per lane, the candidate whose row fills its lane group best (the
// fewest dwords among equals).
static bool edge_geom(const EdgeArgs& a, EdgeGeom& g, int& q, int64_t& blocks) {
  const uintptr_t base = reinterpret_cast<uintptr_t>(a.frames);
  if (a.width % 8 || a.width > kEdgeMaxSide || a.height < 3 || base % 8 || (a.n_frames > 1 && a.frame_stride % 8))
    return false;
  q = 0;
  for (const int c : {2, 4, 5, 8}) {
    const int lanes = a.width / (4 * c);
    if (a.width % (4 * c) || lanes > 64) continue;
    const int group = lanes <= 16 ? 16 : (lanes <= 32 ? 32 : 64);
    if (!q || lanes * g.group > g.lanes_per_row * group) {
      q = c;
      g.lanes_per_row = lanes;
      g.group = group;
    }
  }
  if (!q) return false;
  const int gpw = 64 / g.group;  // groups per wave
  // row segments (2 halo rows each) only when the frames alone leave the chip underfilled
  const int out_rows = a.height - 2;
  const int max_segs = out_rows / 16 > 0 ? out_rows / 16 : 1;
  const int64_t want = (8192ll * gpw + a.n_frames - 1) / a.n_frames;
  const int segs = (int)(want < 1 ? 1 : (want > max_segs ? max_segs : want));
  g.seg_rows = (out_rows + segs - 1) / segs;
  g.segs = (out_rows + g.seg_rows - 1) / g.seg_rows;
  g.t = a.threshold < 254 ? a.threshold : 254;
  const int64_t waves = ((int64_t)a.n_frames * g.segs + gpw - 1) / gpw;
  blocks = (waves + kEdgeBlock / 64 - 1) / (kEdgeBlock / 64);
  return blocks <= 0x7FFFFFFF;
}

int launch_edge_targets(int n_frames, int width, int height, const TrikHsvTargetSums* sums, TrikHsvTarget* targets,
                        hipStream_t s) {
  if (n_frames <= 0 || !targets) return hipSuccess;
  hipLaunchKernelGGL(edge_targets_kernel, dim3((unsigned)((n_frames + 255) / 256)), dim3(256), 0, s, n_frames, width,
                     height, sums, targets);
  return hipGetLastError();
}

int launch_edge(const EdgeArgs& a, hipStream_t s) {
  if (a.n_frames <= 0 || a.width <= 0 || a.height <= 0) return hipSuccess;
  EdgeGeom g;
  int q = 0;
  int64_t blocks = 0;
  if (!a.edges && edge_geom(a, g, q, blocks)) {
    const dim3 grid((unsigned)blocks), block(kEdgeBlock);
    if (q == 2)
      hipLaunchKernelGGL(edge_vec_kernel<2>, grid, block, 0, s, a, g);
    else if (q == 4)
      hipLaunchKernelGGL(edge_vec_kernel<4>, grid, block, 0, s, a, g);
    else if (q == 5)
      hipLaunchKernelGGL(edge_vec_kernel<5>, grid, block, 0, s, a, g);
    else
      hipLaunchKernelGGL(edge_vec_kernel<8>, grid, block, 0, s, a, g);
  } else {
    blocks = (int64_t)a.n_frames * a.height;
    if (blocks > 0x7FFFFFFF) return hipErrorInvalidValue;
    hipLaunchKernelGGL(edge_map_kernel, dim3((unsigned)blocks), dim3(kEdgeBlock), 0, s, a);
  }
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  return launch_edge_targets(a.n_frames, a.width, a.height, a.sums, a.targets, s);
}

// A launch holds fewer than 2^32 threads: larger batches go in several
// launches of whole frames.
int launch_edge_preview(const EdgePreviewArgs& a, hipStream_t s) {
  if (a.n_frames <= 0 || a.out_h <= 0 || a.out_ll <= 0) return hipSuccess;
  constexpr int64_t kMaxBlocks = 0xFFFFFFFFll / 256;
  const uint32_t bpr = (uint32_t)(((int64_t)a.out_ll + 1) / 2 + 255) / 256u;
  const int64_t per_frame = (int64_t)a.out_h * bpr;
  if (per_frame > kMaxBlocks) return hipErrorInvalidValue;
  const int64_t per_launch = kMaxBlocks / per_frame;
  for (int64_t f0 = 0; f0 < a.n_frames; f0 += per_launch) {
    EdgePreviewArgs b = a;
    b.narrow(f0, a.n_frames - f0 < per_launch ? a.n_frames - f0 : per_launch);
    b.sums = a.sums + f0;
    b.previews = a.previews + f0 * a.preview_stride;
    hipLaunchKernelGGL(edge_preview_kernel, dim3((unsigned)(b.n_frames * per_frame)), dim3(256), 0, s, b, bpr);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace trik_hsv
