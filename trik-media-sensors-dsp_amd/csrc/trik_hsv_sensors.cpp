// trik_hsv_sensors.cpp -- the host side of the operator outputs (previews,
// line sensors, multi-blob sensor, auto range): the preview geometry, the
// kernel arguments, and one enqueue core per sensor, shared by process() and
// the batch API.
#include <string.h>

#include "trik_hsv_handle.h"

using namespace trik_hsv;

namespace {

// Scale maps of the preview (WSEQ:371-387) for this geometry, uploaded once.
// col_lo..col_hi: the source columns that write (the line sensor's window).
// A geometry change (rare) waits for the kernels still reading the old maps
// and for the upload (the staging is pageable and reused).
int32_t ensure_maps(TrikCvHandle* h, int w, int hgt, int ow, int oh, hipStream_t s, int col_lo = 0,
                    int col_hi = 0x7FFFFFFF) {
  if (h->d_maps && h->maps_key[0] == w && h->maps_key[1] == hgt && h->maps_key[2] == ow &&
      h->maps_key[3] == oh && h->maps_key[4] == col_lo && h->maps_key[5] == col_hi)
    return 0;
  const size_t n = (size_t)w + hgt + ow + oh;
  h->maps_users.wait_all();  // previous users done
  h->h_maps.assign(n ? n : 1, 0u);
  preview_maps(w, hgt, ow, oh, h->h_maps.data(), col_lo, col_hi);
  // the 2:1 maps (the defaults' 640x480 -> 320x240): preview_rows2_kernel
  bool rows2 = false;
  int c0 = 0, c1 = ow;
  {
    const uint32_t* last_row = h->h_maps.data() + w + hgt;
    const uint32_t* last_col = last_row + oh;
    rows2 = oh > 0 && ow > 0 && (int32_t)last_row[0] >= 0;
    for (int r = 0; rows2 && r < oh; ++r) rows2 = (int32_t)last_row[r] == (int32_t)last_row[0] + 2 * r;
    // the written columns: one window [c0, c1) with last_col[c] = 2c + 1, -1 outside
    while (c0 < ow && (int32_t)last_col[c0] < 0) ++c0;
    while (c1 > c0 && (int32_t)last_col[c1 - 1] < 0) --c1;
    for (int c = 0; rows2 && c < ow; ++c)
      rows2 = (c >= c0 && c < c1) ? (int32_t)last_col[c] == 2 * c + 1 : (int32_t)last_col[c] < 0;
    h->maps_rows2 = rows2 ? (int32_t)last_row[0] : -1;
  }
  h->maps_rows2_c0 = c0;
  h->maps_rows2_c1 = c1;
  // The object sensors' 8 guide lines (draw_guides, WSEQ:136-166,471-485) as
  // output pixels, one bit each, 8 per byte along a row, behind the maps: the
  // 2:1 row kernel writes them as it writes the preview, so the overlay only
  // draws the target circle.  The same points and clamping as Canvas::px.
  h->maps_guides = 0;
  if (rows2 && ow % 8 == 0 && w > 0 && hgt > 0) {
    const size_t gpr = (size_t)ow / 8, words = ((size_t)oh * gpr + 3) / 4;
    h->h_maps.resize(n + words, 0u);
    uint8_t* bits = reinterpret_cast<uint8_t*>(h->h_maps.data() + n);
    const uint32_t* wi2wo = h->h_maps.data();
    const uint32_t* hi2ho = wi2wo + w;
    const auto px = [&](int col, int row) {
      const int sc = col < 0 ? 0 : (col > w - 1 ? w - 1 : col);
      const int sr = row < 0 ? 0 : (row > hgt - 1 ? hgt - 1 : row);
      const uint32_t oc = wi2wo[sc], orow = hi2ho[sr];
      if (oc < (uint32_t)ow && orow < (uint32_t)oh) bits[orow * gpr + oc / 8] |= (uint8_t)(1u << (oc % 8));
    };
    const int step = hgt / 6, hh = hgt / 2, hw = w / 2;
    for (int k = 0; k < 8 * 100; ++k) {
      const int line = k / 100, adj = k % 100, off = (line & 3) < 2 ? ((line & 3) - 2) : ((line & 3) - 1);
      if (line < 4) {
        px(hw + off * step, hh - adj);
        px(hw + off * step, hh + adj);
      } else {
        px(hw - adj, hh + off * step);
        px(hw + adj, hh + off * step);
      }
    }
    h->maps_guides = 1;
  }
  const size_t total = h->h_maps.size();
  const int32_t rc = grow(h->d_maps, h->d_maps_cap, sizeof(uint32_t) * total);
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(h->d_maps, h->h_maps.data(), sizeof(uint32_t) * total, hipMemcpyHostToDevice, s));
  HIP_TRY(hipStreamSynchronize(s));  // h_maps is pageable and reused
  h->maps_key[0] = w; h->maps_key[1] = hgt; h->maps_key[2] = ow; h->maps_key[3] = oh;
  h->maps_key[4] = col_lo; h->maps_key[5] = col_hi;
  // the line overlays' output pixels (line_overlay_kernel, LSEQ:419-474): a
  // column map with steps of 0 or 1 sends any source interval to one interval
  const uint32_t* wi2wo = h->h_maps.data();
  const uint32_t* hi2ho = wi2wo + w;
  bool step1 = w > 0 && hgt > 0;
  for (int c = 1; step1 && c < w; ++c) step1 = wi2wo[c] - wi2wo[c - 1] <= 1u;
  h->maps_ovl_ok = step1 ? 1 : 0;
  bool half = step1;
  for (int c = 0; half && c < w; ++c) half = wi2wo[c] == (uint32_t)c >> 1;
  h->maps_ovl_half = half ? 1 : 0;
  if (step1) {
    const auto cl = [](int v, int n) { return v < 0 ? 0 : (v > n - 1 ? n - 1 : v); };
    const int hw = w / 2, hh = hgt / 2, step = 40;
    const int cols[4] = {hw - step, hw + step, hw - 2 * step, hw + 2 * step};
    for (int j = 0; j < 4; ++j) h->maps_ovl_mag[j] = (int32_t)wi2wo[cl(cols[j], w)];
    h->maps_ovl_band[0] = (int32_t)hi2ho[cl(hh, hgt)];
    h->maps_ovl_band[1] = (int32_t)hi2ho[cl(hh + 2 * step, hgt)];
    h->maps_ovl_c_lo = (int32_t)wi2wo[0];
    h->maps_ovl_c_hi = (int32_t)wi2wo[w - 1];
  }
  return 0;
}

// Where the previews go, with the handle's current maps (ensure_maps) for
// frames of w x hgt: wi2wo[w], hi2ho[hgt], last_row[out_h], last_col[out_w].
PreviewTarget preview_target(const TrikCvHandle* h, int w, int hgt, const PreviewDst& d) {
  PreviewTarget t = {d.out_w, d.out_h, d.out_ll, d.previews, d.stride};
  t.wi2wo = h->d_maps;
  t.hi2ho = t.wi2wo + w;
  t.last_row = reinterpret_cast<const int32_t*>(t.hi2ho + hgt);
  t.last_col = t.last_row + d.out_h;
  return t;
}

// The preview kernels' arguments on the handle's current maps.  The range is
// the all-zero one (the multi-blob preview detects by metapixel);
// preview_tables sets it wherever a range applies.
PreviewArgs preview_args(const TrikCvHandle* h, const TrikHsvFrameBatch& b, const PreviewDst& d) {
  PreviewArgs a = {frame_view(b), preview_target(h, b.width, b.height, d)};
  a.aligned4 = aligned4(b) && (reinterpret_cast<uintptr_t>(d.previews) & 3) == 0 &&
               (b.n_frames <= 1 || (d.stride & 3) == 0) && (d.out_ll & 3) == 0;
  a.rows2_first = h->maps_rows2;
  if (h->maps_guides) a.guide_bits = reinterpret_cast<const uint8_t*>(a.last_col + d.out_w);
  a.rows2_c0 = h->maps_rows2_c0;
  a.rows2_c1 = h->maps_rows2_c1;
  a.ovl_ok = h->maps_ovl_ok;
  a.ovl_half = h->maps_ovl_half;
  for (int j = 0; j < 4; ++j) a.ovl_mag[j] = h->maps_ovl_mag[j];
  a.ovl_band[0] = h->maps_ovl_band[0];
  a.ovl_band[1] = h->maps_ovl_band[1];
  a.ovl_c_lo = h->maps_ovl_c_lo;
  a.ovl_c_hi = h->maps_ovl_c_hi;
  return a;
}

// The preview's detection range compiled as a single-range table set.
int32_t preview_tables(TrikCvHandle* h, PreviewArgs& pa, const TRIK_VIDTRANSCODE_CV_InArgsAlg& range,
                       hipStream_t s, TableSet** set) {
  int32_t rc = acquire_tables(h, &range, 1, s, set);
  if (rc) return rc;
  pa.range = pack_range(range);
  pa.tables = (*set)->d_stripe;
  pa.hue_free = !(*set)->detect.empty() && (*set)->detect[0] != kDetectFull ? 1 : 0;
  return 0;
}

// LSEQ:391-414: hue and saturation bounds fixed at 0..255 (unscaled), value
// scaled as the object sensor's (scale_val, trik_hsv_internal.h).

// BitmapBuilder::run's range update (cv_bitmap_builder_reference.hpp:110-130):
// from/to around the centre (hue wraps, sat/val clip), scaled as the webcam's,
// then resetHsvRange (:62-77).
int wrap_value(int v, int adj, int lo, int hi) {  // makeValueWrap, stdcpp.hpp
  v += adj;
  while (v > hi) v -= hi - lo + 1;
  while (v < lo) v += hi - lo + 1;
  return v;
}
int clip_value(int v, int adj, int lo, int hi) {  // makeValueRange, stdcpp.hpp
  v += adj;
  return v > hi ? hi : (v < lo ? lo : v);
}

}  // namespace

// The line sensor's range in the object sensor's terms: hue 0..359 and
// saturation 0..100 scale to the full 0..255 bytes LSEQ:391-396 fixes.
TRIK_VIDTRANSCODE_CV_InArgsAlg trik_hsv::line_alg(int val_from, int val_to) {
  TRIK_VIDTRANSCODE_CV_InArgsAlg r;
  memset(&r, 0, sizeof r);
  r.detectHueFrom = 0;
  r.detectHueTo = 359;
  r.detectSatFrom = 0;
  r.detectSatTo = 100;
  r.detectValFrom = (uint8_t)val_from;
  r.detectValTo = (uint8_t)val_to;
  return r;
}

LineArgs trik_hsv::line_args(const TrikHsvFrameBatch& b, int val_from, int val_to, int band_start, int band_stop,
                             TrikHsvTargetSums* sums, TrikHsvTarget* targets) {
  LineArgs a = {frame_view(b)};
  a.val_lo = scale_val(val_from);
  a.val_hi = scale_val(val_to);
  a.band_start = band_start;
  a.band_stop = band_stop;
  a.sums = sums;
  a.targets = targets;
  return a;
}

TRIK_VIDTRANSCODE_CV_InArgsAlg trik_hsv::blob_range_args(const TRIK_VIDTRANSCODE_CV_OV7670_InArgsAlg& a) {
  TRIK_VIDTRANSCODE_CV_InArgsAlg r;
  memset(&r, 0, sizeof r);
  r.detectHueFrom = (uint16_t)wrap_value(a.detectHue, -(int)a.detectHueTol, 0, 359);
  r.detectHueTo = (uint16_t)wrap_value(a.detectHue, (int)a.detectHueTol, 0, 359);
  r.detectSatFrom = (uint8_t)clip_value(a.detectSat, -(int)a.detectSatTol, 0, 100);
  r.detectSatTo = (uint8_t)clip_value(a.detectSat, (int)a.detectSatTol, 0, 100);
  r.detectValFrom = (uint8_t)clip_value(a.detectVal, -(int)a.detectValTol, 0, 100);
  r.detectValTo = (uint8_t)clip_value(a.detectVal, (int)a.detectValTol, 0, 100);
  return r;  // then the same scaling and wrap packing (WSEQ:425-445 = BMB:62-77)
}

AutoRangeArgs trik_hsv::auto_range_args(const TrikHsvFrameBatch& b, uint16_t* out) {
  AutoRangeArgs a = {frame_view(b)};
  auto_range_zone(b.width, b.height, a.c_lo, a.c_hi, a.r_lo, a.r_hi);
  a.aligned4 = aligned4(b);
  a.out = out;
  return a;
}

AutoExactArgs trik_hsv::auto_exact_args(const TrikHsvFrameBatch& b, int kind, int32_t* scores, int32_t* start,
                                        uint16_t* out, int32_t* best) {
  AutoExactArgs a = {frame_view(b)};
  a.kind = kind;
  auto_exact_zone(a);
  a.scores = scores; a.start = start; a.out = out; a.best = best;
  return a;
}

namespace {

// Scratch for n frames of W x H.  Stream s waits (device side) for the
// handle's earlier multi-blob work on other streams, which used the same
// scratch; growing it (a larger batch) waits for that work on the host.
int32_t ensure_blob_scratch(TrikCvHandle* h, int n, int w, int hgt, hipStream_t s) {
  const size_t bw = (size_t)(w / 4), bh = (size_t)(hgt / 4), nn = (size_t)(n > 0 ? n : 1);
  const size_t ml = (size_t)blob_max_labels((int)bw, (int)bh);
  if (nn * (bw * bh > 0 ? bw * bh : 1) > h->d_meta_cap || nn * 3 * ml * sizeof(int32_t) > h->d_blob_stats_cap ||
      nn * 24 * sizeof(int32_t) > h->d_blob_top_cap || nn * 8 * sizeof(TrikHsvTarget) > h->d_blob_targets_cap)
    h->blob_users.wait_all();
  HIP_TRY(h->blob_users.order_after(s));
  int32_t r = grow(h->d_meta, h->d_meta_cap, nn * (bw * bh > 0 ? bw * bh : 1));
  // the clusterer's own statistics: zero when allocated, and every clusterer
  // launch leaves the labels it used zero again (blob_ccl_kernel).  The
  // capacity counts only once the zeroing is enqueued, and a failed clusterer
  // launch (which may leave labels non-zero) marks the buffer dirty: the next
  // call zeroes it whole.
  const size_t stats_bytes = nn * 3 * ml * sizeof(int32_t);
  if (!r && (stats_bytes > h->d_blob_stats_cap || h->blob_stats_dirty)) {
    if (stats_bytes > h->d_blob_stats_cap) r = grow(h->d_blob_stats, h->d_blob_stats_cap, stats_bytes);
    if (!r) {
      const hipError_t e = hipMemsetAsync(h->d_blob_stats, 0, h->d_blob_stats_cap, s);
      if (e != hipSuccess) {
        h->blob_stats_dirty = true;
        return fail(TRIK_IVIDTRANSCODE_EFAIL, std::string("hipMemsetAsync(blob stats): ") + hipGetErrorString(e));
      }
      h->blob_stats_dirty = false;
    }
  }
  if (!r) r = grow(h->d_blob_top, h->d_blob_top_cap, nn * 24 * sizeof(int32_t));
  if (!r) r = grow(h->d_blob_targets, h->d_blob_targets_cap, nn * 8 * sizeof(TrikHsvTarget));
  return r;
}

// Compiles the range's tables (cached per handle) and fills the kernel args.
int32_t blob_args(TrikCvHandle* h, const TrikHsvFrameBatch& b, const TRIK_VIDTRANSCODE_CV_InArgsAlg& range,
                  TrikHsvTarget* targets, int32_t* top, uint8_t* meta, uint16_t* labels, int32_t* n_labels,
                  hipStream_t s, BlobArgs& a, TableSet** set) {
  int32_t rc = acquire_tables(h, &range, 1, s, set);
  if (rc) return rc;
  a = {frame_view(b)};
  a.range = pack_range(range);
  a.tables = (*set)->d_stripe;
  a.aligned4 = aligned4(b);
  a.meta = meta ? meta : h->d_meta;
  a.labels = labels;
  a.stats = h->d_blob_stats;
  a.max_labels = (int32_t)blob_max_labels(b.width / 4, b.height / 4);
  a.targets = targets ? targets : h->d_blob_targets;
  a.top = top ? top : h->d_blob_top;
  a.n_labels = n_labels;
  return 0;
}

// The multi-blob sensor: the metapixel bitmap on the chroma-run tables of the
// sticky range when the hot-kernel setting allows it (AUTO: batches of at
// least TRIK_HSV_CHROMA_MIN_PIXELS whose exact-path share is low), else the
// stripe-arithmetic kernel inside launch_blob; then the clusterer.
int32_t run_blob(TrikCvHandle* h, BlobArgs& ba, TableSet& t, hipStream_t s) {
  const bool big = (int64_t)ba.n_frames * ba.width * ba.height >= (int64_t)TRIK_HSV_CHROMA_MIN_PIXELS;
  int32_t rc = 0;
  const HotPlan plan = plan_hot(h, t, 0, 1, big, h->hot.load() != TRIK_HSV_HOT_GENERIC && blob_chroma_ok(ba), s, &rc);
  if (rc) return rc;
  ba.meta_ready = 0;
  h->pending_set = nullptr;
  h->hot_groups.assign(1, TRIK_HSV_HOT_STRIPE);
  if (plan == kPlanChroma) {
    HIP_TRY(launch_blob_meta_chroma(ba, t.d_chroma, t.d_tables, s));
    ba.meta_ready = 1;
    h->hot_groups[0] = TRIK_HSV_HOT_CHROMA;
  } else if (plan == kPlanGated) {  // both bitmap kernels, the device runs one (see run_sums)
    BlobArgs bc = ba;
    bc.gate = ba.gate = &t.d_chroma[0].flagged_cost;
    bc.gate_max = ba.gate_max = kChromaMaxCost;
    bc.gate_le = 1;
    ba.gate_le = 0;
    HIP_TRY(launch_blob_meta_chroma(bc, t.d_chroma, t.d_tables, s));
    h->pending_set = &t;
    h->hot_groups[0] = -TRIK_HSV_HOT_STRIPE;
  }
  const int e = launch_blob(ba, s);
  if (e != hipSuccess) {
    h->blob_stats_dirty = true;  // (the clusterer may not have restored its statistics to zero)
    return fail(TRIK_IVIDTRANSCODE_EFAIL, std::string("launch_blob: ") + hipGetErrorString((hipError_t)e));
  }
  return 0;
}

}  // namespace

// ---------------------------------------------------------------------------
// One enqueue path per sensor
// ---------------------------------------------------------------------------
// the preview kernel writes every byte of each preview, zeros included (WFXNS:234)
int32_t trik_hsv::preview_core(TrikCvHandle* h, const TrikHsvFrameBatch& b,
                               const TRIK_VIDTRANSCODE_CV_InArgsAlg& range, const TrikHsvTargetSums* sums,
                               int sums_pitch, const PreviewDst& d, hipStream_t s) {
  int32_t rc = ensure_maps(h, b.width, b.height, d.out_w, d.out_h, s);
  if (rc) return rc;
  PreviewArgs pa = preview_args(h, b, d);
  TableSet* set = nullptr;
  rc = preview_tables(h, pa, range, s, &set);
  if (rc) return rc;
  HIP_TRY(launch_preview(pa, sums, sums_pitch, s));
  return note_uses(h, set, true, s);
}

// the handle lends its maps only: no table set is acquired, the ranges are read by the kernels
int32_t trik_hsv::frame_ranges_preview_core(TrikCvHandle* h, const TrikHsvFrameBatch& b, const uint16_t* ranges,
                                            int n_ranges, int t, const TrikHsvTargetSums* sums, int sums_pitch,
                                            const PreviewDst& d, hipStream_t s) {
  const int32_t rc = ensure_maps(h, b.width, b.height, d.out_w, d.out_h, s);
  if (rc) return rc;
  HIP_TRY(launch_frame_ranges_preview(preview_args(h, b, d), ranges, n_ranges, t, sums, sums_pitch, s));
  return note_uses(h, nullptr, true, s);
}

int32_t trik_hsv::line_preview_core(TrikCvHandle* h, const TrikHsvFrameBatch& b,
                                    const TRIK_VIDTRANSCODE_CV_InArgsAlg& table_range, int col_lo, int col_hi,
                                    int band, const TrikHsvTargetSums* sums, const PreviewDst& d, hipStream_t s) {
  int32_t rc = ensure_maps(h, b.width, b.height, d.out_w, d.out_h, s, col_lo, col_hi);
  if (rc) return rc;
  PreviewArgs pa = preview_args(h, b, d);
  TableSet* set = nullptr;
  rc = preview_tables(h, pa, table_range, s, &set);
  if (rc) return rc;
  HIP_TRY(launch_line_preview(pa, sums, band, s));
  return note_uses(h, set, true, s);
}

// the handle lends its maps only, with the layout's column window (LSEQ:283:
// columns 5..W-5; LSEQW:232: every column)
int32_t trik_hsv::line_frame_ranges_preview_core(TrikCvHandle* h, const TrikHsvFrameBatch& b,
                                                 const uint16_t* ranges, const TrikHsvTargetSums* sums,
                                                 const PreviewDst& d, hipStream_t s) {
  const bool ov7670 = b.layout == TRIK_HSV_LAYOUT_OV7670;
  const int32_t rc = ensure_maps(h, b.width, b.height, d.out_w, d.out_h, s, ov7670 ? 5 : 0,
                                 ov7670 ? b.width - 5 : 0x7FFFFFFF);
  if (rc) return rc;
  HIP_TRY(launch_line_frame_ranges_preview(preview_args(h, b, d), ranges, sums, s));
  return note_uses(h, nullptr, true, s);
}

int32_t trik_hsv::blob_core(TrikCvHandle* h, const TrikHsvFrameBatch& b,
                            const TRIK_VIDTRANSCODE_CV_InArgsAlg& range, TrikHsvTarget* targets, int32_t* top,
                            uint8_t* meta, uint16_t* labels, int32_t* n_labels, hipStream_t s, BlobArgs& ba) {
  int32_t r = ensure_blob_scratch(h, b.n_frames, b.width, b.height, s);
  if (r) return r;
  TableSet* set = nullptr;
  r = blob_args(h, b, range, targets, top, meta, labels, n_labels, s, ba, &set);
  if (r) return r;
  r = run_blob(h, ba, *set, s);
  if (r) return r;
  return note_uses(h, set, false, s, &h->blob_users);
}

// The multi-blob sensor for n_ranges ranges per frame.  A slot is one (frame,
// range) pair, s = f * n_ranges + t; the clusterer runs over slots as if they
// were frames.  The batch goes in chunks of whole frames of at most
// TRIK_HSV_BLOB_CHUNK_SLOTS slots (at least one frame), so the statistics
// scratch is that of a single-range call of as many frames.  Per chunk: one
// bitmap launch per group of 4 ranges (each reads the chunk's frames once),
// then one clusterer launch; all stream-ordered.
int32_t trik_hsv::blob_ranges_core(TrikCvHandle* h, const TrikHsvFrameBatch& b,
                                   const TRIK_VIDTRANSCODE_CV_InArgsAlg* ranges, int n_ranges,
                                   TrikHsvTarget* targets, int32_t* top, uint8_t* meta, uint16_t* labels,
                                   int32_t* n_labels, hipStream_t s) {
  const int chunk_frames = TRIK_HSV_BLOB_CHUNK_SLOTS / n_ranges > 1 ? TRIK_HSV_BLOB_CHUNK_SLOTS / n_ranges : 1;
  const int first = b.n_frames < chunk_frames ? b.n_frames : chunk_frames;
  int32_t r = ensure_blob_scratch(h, first * n_ranges, b.width, b.height, s);
  if (r) return r;
  TableSet* set = nullptr;
  r = acquire_tables(h, ranges, n_ranges, s, &set);
  if (r) return r;
  const int groups = (n_ranges + kRangesPerLaunch - 1) / kRangesPerLaunch;
  const int64_t cells = (int64_t)(b.width / 4) * (b.height / 4);
  h->pending_set = nullptr;
  h->hot_groups.assign((size_t)groups, TRIK_HSV_HOT_STRIPE);
  bool enqueued = false;
  for (int f0 = 0; f0 < b.n_frames && !r; f0 += chunk_frames) {
    const int nf = b.n_frames - f0 < chunk_frames ? b.n_frames - f0 : chunk_frames;
    const int64_t s0 = (int64_t)f0 * n_ranges;  // the chunk's first slot
    BlobArgs a = {frame_view(b, f0, nf)};
    a.range = pack_range(ranges[0]);
    a.aligned4 = aligned4(b);
    a.meta = meta ? meta + s0 * cells : h->d_meta;
    a.labels = labels ? labels + s0 * cells : nullptr;
    a.stats = h->d_blob_stats;
    a.max_labels = (int32_t)blob_max_labels(b.width / 4, b.height / 4);
    a.targets = targets + s0 * 8;
    a.top = top ? top + s0 * 24 : h->d_blob_top;
    a.n_labels = n_labels ? n_labels + s0 : nullptr;
    for (int g = 0; g < groups && !r; ++g) {
      const int left = n_ranges - g * kRangesPerLaunch;
      a.tables = set->d_stripe + g;
      const int e = launch_blob_meta_ranges(a, b.layout, n_ranges, g * kRangesPerLaunch,
                                            left < kRangesPerLaunch ? left : kRangesPerLaunch, s);
      if (e != hipSuccess)
        r = fail(TRIK_IVIDTRANSCODE_EFAIL,
                 std::string("launch_blob_meta_ranges: ") + hipGetErrorString((hipError_t)e));
      else
        enqueued = true;
    }
    if (r) break;
    a.tables = set->d_stripe;
    a.n_frames = nf * n_ranges;
    a.meta_ready = 1;
    const int e = launch_blob(a, s);
    if (e != hipSuccess) {
      h->blob_stats_dirty = true;  // (the clusterer may not have restored its statistics to zero)
      r = fail(TRIK_IVIDTRANSCODE_EFAIL, std::string("launch_blob: ") + hipGetErrorString((hipError_t)e));
    }
  }
  if (r) {  // what was enqueued still reads the tables and writes the scratch
    if (enqueued) {
      const std::string msg = last_error();
      (void)note_uses(h, set, false, s, &h->blob_users);
      return fail(r, msg);
    }
    return r;
  }
  return note_uses(h, set, false, s, &h->blob_users);
}

// The same with the ranges per frame, in device memory (ranges[f][t][6], never
// read on the host): the chunks of blob_ranges_core, each one table-free bitmap
// launch for all of its ranges, then the clusterer over its slots.  No table
// set is acquired and the hot-kernel report is left as it is; the handle lends
// its scratch alone.
int32_t trik_hsv::blob_frame_ranges_core(TrikCvHandle* h, const TrikHsvFrameBatch& b, const uint16_t* ranges,
                                         int n_ranges, TrikHsvTarget* targets, int32_t* top, uint8_t* meta,
                                         uint16_t* labels, int32_t* n_labels, hipStream_t s) {
  const int chunk_frames = TRIK_HSV_BLOB_CHUNK_SLOTS / n_ranges > 1 ? TRIK_HSV_BLOB_CHUNK_SLOTS / n_ranges : 1;
  const int first = b.n_frames < chunk_frames ? b.n_frames : chunk_frames;
  int32_t r = ensure_blob_scratch(h, first * n_ranges, b.width, b.height, s);
  if (r) return r;
  const int64_t cells = (int64_t)(b.width / 4) * (b.height / 4);
  bool enqueued = false;
  for (int f0 = 0; f0 < b.n_frames && !r; f0 += chunk_frames) {
    const int nf = b.n_frames - f0 < chunk_frames ? b.n_frames - f0 : chunk_frames;
    const int64_t s0 = (int64_t)f0 * n_ranges;  // the chunk's first slot
    BlobArgs a = {frame_view(b, f0, nf)};
    a.range = PackedRange{0, 0, 0};
    a.tables = nullptr;
    a.aligned4 = aligned4(b);
    a.meta = meta ? meta + s0 * cells : h->d_meta;
    a.labels = labels ? labels + s0 * cells : nullptr;
    a.stats = h->d_blob_stats;
    a.max_labels = (int32_t)blob_max_labels(b.width / 4, b.height / 4);
    a.targets = targets + s0 * 8;
    a.top = top ? top + s0 * 24 : h->d_blob_top;
    a.n_labels = n_labels ? n_labels + s0 : nullptr;
    int e = launch_blob_meta_frame_ranges(a, ranges + s0 * 6, n_ranges, s);  // the chunk's ranges
    if (e != hipSuccess) {
      r = fail(TRIK_IVIDTRANSCODE_EFAIL,
               std::string("launch_blob_meta_frame_ranges: ") + hipGetErrorString((hipError_t)e));
      break;
    }
    enqueued = true;
    a.n_frames = nf * n_ranges;
    a.meta_ready = 1;
    e = launch_blob(a, s);
    if (e != hipSuccess) {
      h->blob_stats_dirty = true;  // (the clusterer may not have restored its statistics to zero)
      r = fail(TRIK_IVIDTRANSCODE_EFAIL, std::string("launch_blob: ") + hipGetErrorString((hipError_t)e));
    }
  }
  if (r) {  // what was enqueued still writes the scratch
    if (enqueued) {
      const std::string msg = last_error();
      (void)note_uses(h, nullptr, false, s, &h->blob_users);
      return fail(r, msg);
    }
    return r;
  }
  return note_uses(h, nullptr, false, s, &h->blob_users);
}

std::string trik_hsv::mxn_grid_error(int64_t rows_m, int64_t cols_n) {
  if (rows_m < 1 || cols_n < 1 || rows_m * cols_n > 100)
    return "the MxN sensor takes widthM >= 1, heightN >= 1 and widthM * heightN <= 100";
  return "";
}

// GetImgColor2 of every cell (MSEQ:604-618); the steps are truncating
// divisions (MSEQ:587-588), pixels right of or below the last cell count nowhere
int32_t trik_hsv::mxn_core(TrikCvHandle* h, const TrikHsvFrameBatch& b, int rows_m, int cols_n, int32_t* colors,
                           uint16_t* bins, hipStream_t s) {
  if (!h->d_mxn_table) {  // once per handle; the host table is static
    uint32_t* t = nullptr;
    HIP_TRY(hipMalloc(&t, sizeof(uint32_t) * kMxnColors));
    hipError_t e = hipMemcpyAsync(t, mxn_color_table(), sizeof(uint32_t) * kMxnColors, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);  // later calls may run on other streams
    if (e != hipSuccess) {
      (void)hipFree(t);
      return fail(TRIK_IVIDTRANSCODE_EFAIL, std::string("MxN colour table upload: ") + hipGetErrorString(e));
    }
    h->d_mxn_table = t;
  }
  MxnArgs a = {frame_view(b)};
  a.rows_m = rows_m; a.cols_n = cols_n;
  a.row_step = b.height / rows_m;
  a.col_step = b.width / cols_n;
  a.aligned4 = aligned4(b);
  a.table = h->d_mxn_table;
  a.colors = colors;
  a.bins = bins;
  HIP_TRY(launch_mxn(a, s));
  return 0;
}

int32_t trik_hsv::mxn_preview_core(TrikCvHandle* h, const TrikHsvFrameBatch& b, int rows_m, int cols_n,
                                   const int32_t* colors, const PreviewDst& d, hipStream_t s) {
  int32_t rc = ensure_maps(h, b.width, b.height, d.out_w, d.out_h, s);
  if (rc) return rc;
  MxnPreviewArgs a = {frame_view(b), preview_target(h, b.width, b.height, d)};
  a.rows_m = rows_m; a.cols_n = cols_n;
  a.row_step = b.height / rows_m;
  a.col_step = b.width / cols_n;
  a.colors = colors;
  HIP_TRY(launch_mxn_preview(a, s));
  return note_uses(h, nullptr, true, s);
}

std::string trik_hsv::edge_geometry_error(int64_t width, int64_t height, int64_t line_length) {
  if (height > 0 && line_length != width)
    return "the edge-line sensor takes inputLineLength == inputWidth (the Sobel pass reads the Y plane as one "
           "linear array, ESEQ:179)";
  if (width > kEdgeMaxSide || height > kEdgeMaxSide) return "frame too large for the edge-line sensor (2048 x 2048)";
  return "";
}

EdgeArgs trik_hsv::edge_args(const TrikHsvFrameBatch& b, int threshold, TrikHsvTargetSums* sums,
                             TrikHsvTarget* targets, uint8_t* edges) {
  EdgeArgs a = {frame_view(b)};
  a.threshold = threshold;
  a.sums = sums;
  a.targets = targets;
  a.edges = edges;
  return a;
}

int32_t trik_hsv::edge_preview_core(TrikCvHandle* h, const TrikHsvFrameBatch& b, int threshold,
                                    const TrikHsvTargetSums* sums, const PreviewDst& d, hipStream_t s) {
  int32_t rc = ensure_maps(h, b.width, b.height, d.out_w, d.out_h, s);
  if (rc) return rc;
  EdgePreviewArgs a = {frame_view(b), preview_target(h, b.width, b.height, d)};
  a.threshold = threshold;
  a.sums = sums;
  HIP_TRY(launch_edge_preview(a, s));
  return note_uses(h, nullptr, true, s);
}

std::string trik_hsv::jpeg_geometry_error(int64_t width, int64_t height) {
  if (height % 8 != 0)
    return "the JPEG encoder takes height % 8 == 0 (the reference's block walk reads past the planes otherwise)";
  if (width > 65535 || height > 65535) return "the JPEG encoder takes width, height <= 65535 (SOF0 holds 16 bits)";
  // stream lengths are 32-bit (OutArgs size): header + worst-case segment, every byte stuffed, + EOI
  if ((width / 8) * (height / 8) * 3 * (kJpegMaxDuBits / 8) * 2 + kJpegMaxHeader + 4 > 0x7FFFFFFFll)
    return "the JPEG encoder's worst-case stream of this frame exceeds 2^31 bytes";
  return "";
}

namespace {

constexpr size_t kJpegScratchBudget = 256u << 20;  // scratch of one chunk of frames, unless one frame needs more

size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

// The scratch of one chunk of `frames` frames, as offsets into d_jpeg_scratch.
struct JpegScratch {
  size_t coeffs, info, bitoff, total, words, chunk_ff, bytes;
  uint64_t words_per_frame;
  uint32_t chunks_per_frame;
  JpegScratch(size_t frames, size_t n_du) {
    // a DU takes at most kJpegMaxDuBits bits; two more words for the fill
    // bits' byte and the zeroing's margin; whole chunks
    const uint64_t w = ((uint64_t)n_du * kJpegMaxDuBits + 31) / 32 + 2;
    chunks_per_frame = (uint32_t)((w * 4 + kJpegChunkBytes - 1) / kJpegChunkBytes);
    words_per_frame = (uint64_t)chunks_per_frame * (kJpegChunkBytes / 4);
    size_t o = 0;
    coeffs = o; o += align256(frames * n_du * 64 * sizeof(int16_t));
    info = o; o += align256(frames * n_du * sizeof(uint32_t));
    bitoff = o; o += align256(frames * n_du * sizeof(unsigned long long));
    total = o; o += align256(frames * sizeof(unsigned long long));
    words = o; o += align256(frames * words_per_frame * sizeof(uint32_t));
    chunk_ff = o; o += align256(frames * chunks_per_frame * sizeof(uint32_t));
    bytes = o;
  }
};

// Frames per chunk: as many as the budget holds, at least one, and within the
// launch limits (2^31 DUs per launch, 65535 in a grid's second dimension).
int64_t jpeg_chunk_frames(int64_t n_frames, size_t n_du) {
  const size_t one = JpegScratch(1, n_du).bytes;
  int64_t f = (int64_t)(kJpegScratchBudget / one);
  const int64_t by_du = (int64_t)(0x7FFFFFFFull / n_du);
  if (f > by_du) f = by_du;
  if (f > 32768) f = 32768;
  if (f > n_frames) f = n_frames;
  return f < 1 ? 1 : f;
}

}  // namespace

// JPGEncoder::encode of every frame (JENC:802-852).  The header is built on
// the host and travels as a kernel argument, like the divisor tables.
int32_t trik_hsv::jpeg_core(TrikCvHandle* h, const TrikHsvFrameBatch& b, int quality, bool bw, uint8_t* out,
                            int64_t out_stride, int64_t out_capacity, uint32_t* sizes, int16_t* coeffs,
                            hipStream_t s) {
  if (!h->d_jpeg_huff) {  // once per handle; the host table is static
    JpegHuffman* t = nullptr;
    HIP_TRY(hipMalloc(&t, sizeof(JpegHuffman)));
    hipError_t e = hipMemcpyAsync(t, jpeg_huffman(), sizeof(JpegHuffman), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);  // later calls may run on other streams
    if (e != hipSuccess) {
      (void)hipFree(t);
      return fail(TRIK_IVIDTRANSCODE_EFAIL, std::string("JPEG Huffman table upload: ") + hipGetErrorString(e));
    }
    h->d_jpeg_huff = t;
  }
  const int ncomp = bw ? 1 : 3;
  const size_t n_du = (size_t)(b.width / 8) * (size_t)(b.height / 8) * ncomp;
  const int64_t chunk = jpeg_chunk_frames(b.n_frames, n_du);
  const JpegScratch sc((size_t)chunk, n_du);
  if (sc.bytes > h->d_jpeg_scratch_cap) h->jpeg_users.wait_all();  // the buffer is replaced
  HIP_TRY(h->jpeg_users.order_after(s));
  int32_t r = grow(h->d_jpeg_scratch, h->d_jpeg_scratch_cap, sc.bytes);
  if (r) return r;

  JpegDivisors dv;
  JpegHeader hd;
  jpeg_divisors(quality, dv);
  jpeg_header(quality, bw, b.width, b.height, hd);
  JpegArgs all = {frame_view(b)};
  all.aligned4 = aligned4(b);
  all.ncomp = ncomp;
  all.blocks_w = b.width / 8;
  all.n_du = (uint32_t)n_du;
  all.huff = h->d_jpeg_huff;
  uint8_t* base = h->d_jpeg_scratch;
  all.coeffs = reinterpret_cast<int16_t*>(base + sc.coeffs);
  all.info = reinterpret_cast<uint32_t*>(base + sc.info);
  all.bitoff = reinterpret_cast<unsigned long long*>(base + sc.bitoff);
  all.total = reinterpret_cast<unsigned long long*>(base + sc.total);
  all.words = reinterpret_cast<uint32_t*>(base + sc.words);
  all.words_per_frame = sc.words_per_frame;
  all.chunk_ff = reinterpret_cast<uint32_t*>(base + sc.chunk_ff);
  all.chunks_per_frame = sc.chunks_per_frame;
  all.out_stride = out_stride;
  all.out_capacity = out_capacity;
  for (int64_t f0 = 0; f0 < b.n_frames; f0 += chunk) {
    JpegArgs a = all;
    a.narrow(f0, b.n_frames - f0 < chunk ? b.n_frames - f0 : chunk);
    a.out = out ? out + f0 * out_stride : nullptr;
    a.sizes = sizes + f0;
    HIP_TRY(launch_jpeg(a, dv, hd, s));
    if (coeffs)  // the verification output: the chunk's coefficients as the block kernel left them
      HIP_TRY(hipMemcpyAsync(coeffs + f0 * (int64_t)n_du * 64, a.coeffs,
                             (size_t)a.n_frames * n_du * 64 * sizeof(int16_t), hipMemcpyDeviceToDevice, s));
  }
  return note_uses(h, nullptr, false, s, &h->jpeg_users);
}

int32_t trik_hsv::blob_preview_core(TrikCvHandle* h, const TrikHsvFrameBatch& b, const uint8_t* meta,
                                    const int32_t* top, const PreviewDst& d, hipStream_t s) {
  int32_t rc = ensure_maps(h, b.width, b.height, d.out_w, d.out_h, s);
  if (rc) return rc;
  PreviewArgs pa = preview_args(h, b, d);
  pa.meta = meta;
  HIP_TRY(launch_preview_body(pa, s));
  HIP_TRY(launch_blob_overlay(pa, top, s));
  return note_uses(h, nullptr, true, s);
}
