// trik_hsv_handle.h -- the handle behind the C ABI and the host functions its
// translation units share.  Private and host only:
//   trik_hsv_handle.cpp   defaults, setup, create/delete/control, XDAIS tables
//   trik_hsv_hot.cpp      range-table cache and the hot-kernel choice
//   trik_hsv_sensors.cpp  the operator outputs' host side, one core per sensor
//   trik_hsv_process.cpp  Layer 1 TRIK_VIDTRANSCODE_CV_process
//   trik_hsv_batch.cpp    Layer 2 trik_hsv_* batch entry points
#pragma once

#include <atomic>
#include <hip/hip_runtime.h>

#include <mutex>
#include <string>
#include <vector>

#include "trik_hsv_internal.h"

// The algorithms behind a handle: the object sensor (BallDetector, webcam
// WSEQ and ov7670 OSEQ layouts) or the ov7670 line sensor (LineDetector,
// LSEQ = trik/ov7670/line_sensor/include/internal/cv_line_detector_seqpass.hpp;
// its glue trik/ov7670/line_sensor/src/vidtranscode_cv.cpp is WGLUE with
// YUV422P input and a 240x320 default output).
// kAlgoWLine: the webcam line sensor (LineDetector<YUV422, RGB565X> of
// trik/webcam/line_sensor/include/internal/cv_line_detector_seqpass.hpp --
// LSEQW -- with the webcam glue, a 240x320 default output as the line glues).
// kAlgoMxn: the ov7670 MxN colour-grid sensor (BallDetector<YUV422P, RGB565X>
// of trik/ov7670/mxn_sensor/include/internal/cv_ball_detector_seqpass.hpp --
// MSEQ -- behind the ov7670 object sensor's glue: YUV422P input, a 320x240
// default output).
// kAlgoJpeg: the ov7670 JPEG encoder (JPGEncoderWrapper<YUV422P, RGB565X> of
// trik/ov7670/jpeg_encoder/include/internal/cv_jpeg_encoder_wrapper_seqpass.hpp
// -- JWRAP -- over jpeg_encoder_reference.hpp -- JENC -- behind the same glue).
// kAlgoEdge: the ov7670 edge-line sensor (BallDetector<YUV422P, RGB565X> of
// trik/ov7670/edge_line_sensor/include/internal/cv_ball_detector_seqpass.hpp
// -- ESEQ -- behind the same glue; inputLineLength must equal inputWidth).
enum Algo { kAlgoBall = 0, kAlgoLine = 1, kAlgoBlob = 2, kAlgoWLine = 3, kAlgoMxn = 4, kAlgoJpeg = 5, kAlgoEdge = 6 };

// ---------------------------------------------------------------------------
// Handle
// ---------------------------------------------------------------------------
// Device buffers a handle shares between calls that may run on different
// streams: the last use on each stream is an event, so that a later call can
// make its stream wait for them (device side) or, before the buffer is
// rewritten, find out without blocking whether they have finished.
// One event per stream the handle has enqueued work on, recorded once per
// call after its last launch (an event record is a packet on the stream: one
// per call, not one per buffer).  A new stream takes over the event of one whose recorded work has
// completed once kMaxMarks streams are tracked, so the list stays bounded
// however many short-lived streams a caller cycles through.
constexpr size_t kMaxMarks = 16;
struct StreamMarks {
  std::vector<std::pair<hipStream_t, hipEvent_t>> marks;
  int32_t mark(hipStream_t s, hipEvent_t* out) {
    std::pair<hipStream_t, hipEvent_t>* slot = nullptr;
    for (auto& m : marks)
      if (m.first == s) {
        slot = &m;
        break;
      }
    if (!slot && marks.size() >= kMaxMarks)
      for (auto& m : marks)
        if (hipEventQuery(m.second) == hipSuccess) {
          m.first = s;
          slot = &m;
          break;
        }
    if (!slot) {
      hipEvent_t e = nullptr;
      // device-scope release, no system-scope fence: the marks order streams
      // of this device and tell the host that work has finished; none makes
      // device writes visible to the host (callers' copies do that).  With
      // the default system-scope fence a record cost ~5.7 us between two
      // back-to-back steps (L2 written back and invalidated:
      // profiles/r04/r04k_driver_cmd_timed_launches.txt).
      hipError_t r = hipEventCreateWithFlags(&e, hipEventDisableTiming | hipEventDisableSystemFence);
      if (r != hipSuccess) return (int32_t)r;
      marks.emplace_back(s, e);
      slot = &marks.back();
    }
    *out = slot->second;
    return (int32_t)hipEventRecord(slot->second, s);
  }
  void release() {
    for (auto& m : marks) {
      (void)hipEventSynchronize(m.second);
      (void)hipEventDestroy(m.second);
    }
    marks.clear();
  }
};

// The streams whose enqueued work reads or writes a buffer, each with the
// handle's event for that stream (StreamMarks, not owned here) recorded after
// that work.  The event may since have been recorded again, after later work:
// the tests below are conservative, never early.
struct StreamUses {
  std::vector<std::pair<hipStream_t, hipEvent_t>> uses;
  // the calling stream has (just) enqueued work on the buffer; e: its mark
  void note(hipStream_t s, hipEvent_t e) {
    bool found = false;
    size_t j = 0;
    for (size_t i = 0; i < uses.size(); ++i) {
      if (uses[i].first == s) {
        uses[i].second = e;
        found = true;
      } else if (uses[i].second == e) {
        continue;  // the event moved to stream s: that stream's work completed
      }
      uses[j++] = uses[i];
    }
    uses.resize(j);
    if (!found) uses.emplace_back(s, e);
  }
  // every recorded use has completed (non-blocking)
  bool idle() const {
    for (const auto& u : uses)
      if (hipEventQuery(u.second) != hipSuccess) return false;
    return true;
  }
  // stream s waits (device side) for the uses on other streams
  int32_t order_after(hipStream_t s) const {
    for (const auto& u : uses)
      if (u.first != s) {
        hipError_t r = hipStreamWaitEvent(s, u.second, 0);
        if (r != hipSuccess) return (int32_t)r;
      }
    return 0;
  }
  void wait_all() const {
    for (const auto& u : uses) (void)hipEventSynchronize(u.second);
  }
  void release() { uses.clear(); }
};

// Compiled range tables (device) for one range set, with the key (packed
// bounds) they were compiled from and their pinned staging.  A handle keeps a
// few of them (LRU), so that alternating range sets -- the batched sums, the
// preview's single range, the multi-blob sensor's sticky range -- do not
// recompile, and a new range set never overwrites tables a queued kernel is
// still reading: it takes a set whose uses have all completed.
struct TableSet {
  std::vector<uint32_t> key;  // empty: unused
  int groups_cap = 0;
  trik_hsv::RangeTables* d_tables = nullptr;
  trik_hsv::RangeTables* h_tables = nullptr;
  trik_hsv::StripeTables* d_stripe = nullptr;
  trik_hsv::StripeTables* h_stripe = nullptr;
  trik_hsv::ChromaTables* d_chroma = nullptr;  // built on first use per range set (chroma-run kernel)
  unsigned long long* h_cost = nullptr;    // pinned readback of each group's flagged_cost
  std::vector<uint8_t> detect;             // per group: detect_mode() of its ranges
  bool chroma_built = false;
  double chroma_share = -1.0;  // the builder's expected exact-path word share (max over groups), once read
  hipEvent_t ready = nullptr;       // uploads (and the chroma build) enqueued before it
  hipEvent_t cost_ready = nullptr;  // the flagged_cost readback enqueued before it
  StreamUses users;                 // kernels that read the set
  uint64_t tick = 0;                // last use (LRU)
  // AUTO's measured share per group: ChromaTables::flagged_words (the words
  // the chroma-run kernel's exact path resolved) read back every few
  // launches, over the words launched in between (Probe)
  struct Probe {
    uint64_t base = 0;          // the counter at the last landed readback
    bool have_base = false;
    uint64_t launched = 0;      // words launched on the chroma-run kernel since the last readback
    uint64_t in_flight = 0;     // those of the readback in flight
    // a gated launch (the device chose the kernel) since the last readback:
    // its words may or may not be in the counter, so that interval is not
    // measured (mixed) -- only the base moves
    bool mixed = false, in_flight_mixed = false;
    double measured = -1.0;     // flagged words / words between the last two readbacks
    int stripe_runs = 0;        // batches sent to the stripe kernel by the measured share
  };
  std::vector<Probe> probes;
  unsigned long long* h_words = nullptr;  // pinned [groups_cap]: the readback
  hipEvent_t words_ready = nullptr;
  bool words_pending = false;
  int chroma_runs = 0;  // calls with a chroma-run launch since the last readback
  void release() {
    users.wait_all();
    if (ready) (void)hipEventSynchronize(ready);
    if (words_ready) (void)hipEventSynchronize(words_ready);
    users.release();
    (void)hipFree(d_chroma);
    (void)hipHostFree(h_words);
    if (words_ready) (void)hipEventDestroy(words_ready);
    (void)hipHostFree(h_cost);
    (void)hipFree(d_tables);
    (void)hipHostFree(h_tables);
    (void)hipFree(d_stripe);
    (void)hipHostFree(h_stripe);
    if (ready) (void)hipEventDestroy(ready);
    if (cost_ready) (void)hipEventDestroy(cost_ready);
    *this = TableSet();
  }
  bool idle() const { return users.idle() && (!ready || hipEventQuery(ready) == hipSuccess); }
  // the exact-path share, once the readback has landed (-1 before)
  double share() {
    if (chroma_share < 0 && chroma_built && hipEventQuery(cost_ready) == hipSuccess) {
      double sh = 0.0;
      for (int g = 0; g < groups_cap; ++g) {
        const double v = (double)h_cost[g] / 4294967296.0;
        if (v > sh) sh = v;
      }
      chroma_share = sh;
    }
    return chroma_share;
  }
  // group g's own expected share (AUTO plans each group by its own tables),
  // or -1 while the builder's readback is in flight
  double group_share(int g) {
    if (!chroma_built || share() < 0) return -1.0;
    return (double)h_cost[g] / 4294967296.0;
  }
};
constexpr int kTableSets = 4;

struct TrikCvHandle {
  // XDAIS IALG_Obj: the framework's function table (algInit keeps it)
  TRIK_IALG_Obj ialg{};
  // false when the object lives in a framework-allocated IALG record
  // (algAlloc / algInit / algFree), true for TRIK_VIDTRANSCODE_CV_create
  bool owns_memory = true;
  int device = 0;
  int algo = kAlgoBall;
  // line sensor: the cross-point rows the previous run left (LSEQ:298 reads
  // m_hStart/m_hStop before LSEQ:449-450 sets them); set to the steady state
  // H/2, H/2+80 by setup (the reference leaves them uninitialised)
  int32_t line_band[2] = {0, 0};
  TRIK_VIDTRANSCODE_CV_Params params{};
  TRIK_VIDTRANSCODE_CV_DynamicParams dyn{};
  bool alg_ready = false;  // the reference's m_cvAlgorithm is set (WGLUE:302)
  int layout = TRIK_HSV_LAYOUT_YUYV;
  int in_w = 0, in_h = 0, in_ll = 0;
  int out_w = 0, out_h = 0, out_ll = 0;
  std::mutex mu;

  // compiled range tables (device), LRU over the range sets in use
  TableSet sets[kTableSets];
  uint64_t tick = 0;
  TableSet* sums_set = nullptr;  // the set of the last batched-sums call (trik_hsv_chroma_share)
  // hot-kernel choice for this handle (trik_hsv_set_hot_kernel) and the
  // kernel each range group of its last hot call ran (negative: the device
  // chose between the chroma-run kernel and -kind by the group's cost, the
  // share not being known yet; pending_set holds the costs), resolved by
  // trik_hsv_last_hot_kernel
  std::atomic<int> hot{TRIK_HSV_HOT_AUTO};
  std::atomic<int> reserved_cus{0};  // trik_hsv_set_reserved_cus
  // trik_hsv_set_auto_detect: 1 = process() of the ov7670 object sensor and
  // the line sensors answers InArgs autoDetectHsv with the exact search
  std::atomic<int> auto_detect{0};
  std::vector<int8_t> hot_groups;
  TableSet* pending_set = nullptr;

  // preview geometry: scale maps for maps_key = {W, H, out_w, out_h}
  uint32_t* d_maps = nullptr;
  size_t d_maps_cap = 0;
  int maps_key[6] = {-1, -1, -1, -1, -1, -1};
  int32_t maps_rows2 = -1;  // first source row when the maps are the 2:1 ones, else -1
  int32_t maps_guides = 0;  // the guide lines' output bits follow the maps (2:1 maps)
  int32_t maps_rows2_c0 = 0, maps_rows2_c1 = 0;  // the output columns the 2:1 maps write
  // the line sensors' overlay geometry on these maps (PreviewArgs::ovl_*)
  int32_t maps_ovl_half = 0, maps_ovl_ok = 0, maps_ovl_mag[4] = {-1, -1, -1, -1}, maps_ovl_band[2] = {-1, -1};
  int32_t maps_ovl_c_lo = 0, maps_ovl_c_hi = -1;
  std::vector<uint32_t> h_maps;
  StreamUses maps_users;

  // process() staging
  hipStream_t stream = nullptr;
  uint8_t* d_preview = nullptr;
  size_t d_preview_cap = 0;
  uint16_t* d_auto = nullptr;
  uint8_t* d_frame = nullptr;
  size_t d_frame_cap = 0;
  TrikHsvTargetSums* d_sums = nullptr;
  TrikHsvTarget* d_targets = nullptr;

  // the chroma-run kernel's fused step: per-workgroup partial totals and the
  // last-workgroup counter, per-frame accumulators and unit-done counts (all
  // zero between launches), shared by this handle's calls
  unsigned long long* d_wg_part = nullptr;
  uint32_t* d_wg_cnt = nullptr;
  unsigned long long* d_frame_acc = nullptr;  // [frames][16]: 12 sums, the unit count
  int64_t frame_acc_cap = 0;  // frames
  StreamUses fused_users;
  // the chroma-run kernel's sink for its past-the-end loads (KernelArgs::tail):
  // kChromaTailSink bytes, allocated once on first use, never resized
  uint8_t* d_tail_sink = nullptr;

  // ov7670 multi-blob sensor: BitmapBuilder's sticky range (uninitialised in
  // the reference before the first setHsvRange; zero here) and scratch
  TRIK_VIDTRANSCODE_CV_InArgsAlg blob_range{};  // as webcam-form bounds (all zero at first)
  uint8_t* d_meta = nullptr;
  size_t d_meta_cap = 0;
  int32_t* d_blob_stats = nullptr;
  size_t d_blob_stats_cap = 0;
  bool blob_stats_dirty = false;  // zeroed whole by the next call (a failed clusterer launch)
  int32_t* d_blob_top = nullptr;
  size_t d_blob_top_cap = 0;
  TrikHsvTarget* d_blob_targets = nullptr;
  size_t d_blob_targets_cap = 0;
  StreamUses blob_users;  // calls that wrote the multi-blob scratch
  // MxN sensor: the colour table's device copy (uploaded once, then only
  // read) and process()'s cell colours (used on the handle's stream only)
  uint32_t* d_mxn_table = nullptr;
  int32_t* d_mxn_colors = nullptr;
  // JPEG encoder: the Huffman tables' device copy (uploaded once, then only
  // read), the pipeline's scratch for one chunk of frames (jpeg_core) and
  // process()'s stream length (used on the handle's stream only)
  trik_hsv::JpegHuffman* d_jpeg_huff = nullptr;
  uint8_t* d_jpeg_scratch = nullptr;
  size_t d_jpeg_scratch_cap = 0;
  uint32_t* d_jpeg_size = nullptr;
  StreamUses jpeg_users;  // calls that wrote the JPEG scratch
  StreamMarks marks;     // the events the StreamUses lists point at (freed last)
};

// Everything below is internal to the library's own translation units.
#pragma GCC visibility push(hidden)
namespace trik_hsv {

// The calling thread's last-error slot (one object, trik_hsv_handle.cpp).
inline int32_t fail(int32_t code, const std::string& msg) { return set_error(code, msg); }
const std::string& last_error();

#define HIP_TRY(expr)                                                                  \
  do {                                                                                 \
    hipError_t e_ = (hipError_t)(expr);                                                \
    if (e_ != hipSuccess)                                                              \
      return fail(TRIK_IVIDTRANSCODE_EFAIL, std::string(#expr) + ": " + hipGetErrorString(e_)); \
  } while (0)

inline void set_bit(int32_t& word, int bit) { word |= (int32_t)(1u << bit); }

// A call runs on the handle's device (one thread may drive several GPUs, one
// handle each); the caller's current device is restored after.
struct DeviceGuard {
  int prev = -1;
  explicit DeviceGuard(int dev) {
    int cur = 0;
    if (hipGetDevice(&cur) == hipSuccess && cur != dev && hipSetDevice(dev) == hipSuccess) prev = cur;
  }
  ~DeviceGuard() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
};

// A device buffer of at least `bytes`: kept when large enough, else replaced.
template <typename T>
int32_t grow(T*& p, size_t& cap, size_t bytes) {
  if (bytes <= cap) return 0;
  (void)hipFree(p);
  p = nullptr;
  cap = 0;
  HIP_TRY(hipMalloc(&p, bytes));
  cap = bytes;
  return 0;
}

// The kernels' aligned4 flag: frames, frame stride and line length 4-byte aligned.
inline bool aligned4(const TrikHsvFrameBatch& b) {
  return (reinterpret_cast<uintptr_t>(b.frames) & 3) == 0 && (b.n_frames <= 1 || (b.frame_stride & 3) == 0) &&
         (b.line_length & 3) == 0;
}

// trik_hsv_handle.cpp
std::string validate_batch(const TrikHsvFrameBatch* b);

// trik_hsv_hot.cpp: the range-table cache and the hot-kernel choice
int32_t acquire_tables(TrikCvHandle* h, const TRIK_VIDTRANSCODE_CV_InArgsAlg* ranges, int n, hipStream_t s,
                       TableSet** out);
// How the hot kernel is chosen for one launch: CHROMA / STRIPE decided on the
// host, or GATED: both launched, the device picks by the builder's cost.
enum HotPlan { kPlanStripe, kPlanChroma, kPlanGated };
HotPlan plan_hot(TrikCvHandle* h, TableSet& t, int g, int groups, bool big, bool chroma_ok, hipStream_t s,
                 int32_t* rc);
// Record that the work just enqueued on s reads `set` (and the preview maps,
// and `extra`): one event record on s for the call.
int32_t note_uses(TrikCvHandle* h, TableSet* set, bool maps, hipStream_t s, StreamUses* extra = nullptr);
// The outputs of a full step (process_batch): sums written whole (not added),
// targets and the per-target batch totals when not NULL.
struct StepOut {
  TrikHsvTarget* targets = nullptr;
  TrikHsvTargetSums* totals = nullptr;
};
int32_t run_sums(TrikCvHandle* h, const TrikHsvFrameBatch* b, const TRIK_VIDTRANSCODE_CV_InArgsAlg* ranges, int n,
                 TrikHsvTargetSums* sums, uint8_t* masks, hipStream_t s, const StepOut* step = nullptr);

// trik_hsv_sensors.cpp: the operator outputs.  The cores run with the handle's
// mutex held, its device current and their arguments validated; each is the
// one enqueue sequence of its sensor, for process() and the batch API alike.
TRIK_VIDTRANSCODE_CV_InArgsAlg line_alg(int val_from, int val_to);
LineArgs line_args(const TrikHsvFrameBatch& b, int val_from, int val_to, int band_start, int band_stop,
                   TrikHsvTargetSums* sums, TrikHsvTarget* targets);
TRIK_VIDTRANSCODE_CV_InArgsAlg blob_range_args(const TRIK_VIDTRANSCODE_CV_OV7670_InArgsAlg& a);
AutoRangeArgs auto_range_args(const TrikHsvFrameBatch& b, uint16_t* out);
// the exact-search detectors (kind and geometry validated: auto_exact_error)
AutoExactArgs auto_exact_args(const TrikHsvFrameBatch& b, int kind, int32_t* scores, int32_t* start, uint16_t* out,
                              int32_t* best);
// Where a preview call writes: the previews' geometry, the device buffer and
// the bytes from one frame's preview to the next.
struct PreviewDst {
  int32_t out_w, out_h, out_ll;
  uint8_t* previews;
  int64_t stride;
};
// the object sensor's preview: body, guide lines and the circle from sums
int32_t preview_core(TrikCvHandle* h, const TrikHsvFrameBatch& b, const TRIK_VIDTRANSCODE_CV_InArgsAlg& range,
                     const TrikHsvTargetSums* sums, int sums_pitch, const PreviewDst& d, hipStream_t s);
// the same preview with frame f's range at ranges + (f * n_ranges + t) * 6 in
// device memory (no table set; the hot-kernel report is left as it is)
int32_t frame_ranges_preview_core(TrikCvHandle* h, const TrikHsvFrameBatch& b, const uint16_t* ranges, int n_ranges,
                                  int t, const TrikHsvTargetSums* sums, int sums_pitch, const PreviewDst& d,
                                  hipStream_t s);
// a line sensor's preview: source columns col_lo..col_hi write, the tables are
// table_range's; band = 1 draws the ov7670 line sensor's band lines
int32_t line_preview_core(TrikCvHandle* h, const TrikHsvFrameBatch& b,
                          const TRIK_VIDTRANSCODE_CV_InArgsAlg& table_range, int col_lo, int col_hi, int band,
                          const TrikHsvTargetSums* sums, const PreviewDst& d, hipStream_t s);
// a line sensor's preview (b.layout: ov7670 with its column window and band
// lines, or the webcam line sensor on YUYV) with frame f's V bounds at ranges +
// 6 f + 4 in device memory (no table set; the hot-kernel report is left as it is)
int32_t line_frame_ranges_preview_core(TrikCvHandle* h, const TrikHsvFrameBatch& b, const uint16_t* ranges,
                                       const TrikHsvTargetSums* sums, const PreviewDst& d, hipStream_t s);
// the multi-blob sensor; NULL outputs go to the handle's scratch (ba tells where)
int32_t blob_core(TrikCvHandle* h, const TrikHsvFrameBatch& b, const TRIK_VIDTRANSCODE_CV_InArgsAlg& range,
                  TrikHsvTarget* targets, int32_t* top, uint8_t* meta, uint16_t* labels, int32_t* n_labels,
                  hipStream_t s, BlobArgs& ba);
// the same for n_ranges ranges per frame, on either layout; outputs by slot
// (frame * n_ranges + range), in chunks of TRIK_HSV_BLOB_CHUNK_SLOTS slots
int32_t blob_ranges_core(TrikCvHandle* h, const TrikHsvFrameBatch& b, const TRIK_VIDTRANSCODE_CV_InArgsAlg* ranges,
                         int n_ranges, TrikHsvTarget* targets, int32_t* top, uint8_t* meta, uint16_t* labels,
                         int32_t* n_labels, hipStream_t s);
// the same with the ranges per frame, in device memory [n_frames][n_ranges][6]
// (no table set; the hot-kernel report is left as it is)
int32_t blob_frame_ranges_core(TrikCvHandle* h, const TrikHsvFrameBatch& b, const uint16_t* ranges, int n_ranges,
                               TrikHsvTarget* targets, int32_t* top, uint8_t* meta, uint16_t* labels,
                               int32_t* n_labels, hipStream_t s);
// its preview: set metapixels, guide lines, target marks
int32_t blob_preview_core(TrikCvHandle* h, const TrikHsvFrameBatch& b, const uint8_t* meta, const int32_t* top,
                          const PreviewDst& d, hipStream_t s);

// the MxN sensor: cell colours (and winning bins when not NULL) of rows_m x
// cols_n cells per frame; rows_m, cols_n validated by the caller (mxn_grid_error)
int32_t mxn_core(TrikCvHandle* h, const TrikHsvFrameBatch& b, int rows_m, int cols_n, int32_t* colors,
                 uint16_t* bins, hipStream_t s);
// its preview: every source pixel, then the cells' 20x20 squares in cell order
int32_t mxn_preview_core(TrikCvHandle* h, const TrikHsvFrameBatch& b, int rows_m, int cols_n, const int32_t* colors,
                         const PreviewDst& d, hipStream_t s);
// "" when 1 <= rows_m, 1 <= cols_n and rows_m * cols_n <= 100 (OutArgs holds
// 100 colours; the reference does not check)
std::string mxn_grid_error(int64_t rows_m, int64_t cols_n);

// the JPEG encoder: frame i's stream to out + i * out_stride when it fits
// out_capacity (out NULL: sizes only), its length to sizes[i], the quantised
// coefficients to coeffs when not NULL; the geometry validated by the caller
// (jpeg_geometry_error).  Batches go through the handle's scratch in chunks
// of frames (jpeg_chunk_frames).
int32_t jpeg_core(TrikCvHandle* h, const TrikHsvFrameBatch& b, int quality, bool bw, uint8_t* out,
                  int64_t out_stride, int64_t out_capacity, uint32_t* sizes, int16_t* coeffs, hipStream_t s);
// "" when the encoder takes the frame: height % 8 == 0 (the reference's block
// walk reads past the planes otherwise), both sides at most 65535 (SOF0), and a
// worst-case stream below 2^31 bytes
std::string jpeg_geometry_error(int64_t width, int64_t height);

// the edge-line sensor: "" when the geometry is one it takes (line_length ==
// width, both sides <= kEdgeMaxSide; the reference's statics hold 320 x 240)
std::string edge_geometry_error(int64_t width, int64_t height, int64_t line_length);
EdgeArgs edge_args(const TrikHsvFrameBatch& b, int threshold, TrikHsvTargetSums* sums, TrikHsvTarget* targets,
                   uint8_t* edges);
// its preview: the thresholded map through IMG_ycbcr422pl_to_rgb565 with the
// frame's chroma, every source pixel, then the target line (ESEQ:226-249, 405)
int32_t edge_preview_core(TrikCvHandle* h, const TrikHsvFrameBatch& b, int threshold, const TrikHsvTargetSums* sums,
                          const PreviewDst& d, hipStream_t s);

}  // namespace trik_hsv
#pragma GCC visibility pop
