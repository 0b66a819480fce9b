// trik_hsv_hot.cpp -- the handle's range-table cache and the hot-kernel
// choice (AUTO's planner and its probes), with the batched sums they serve.
#include "trik_hsv_handle.h"

using namespace trik_hsv;

namespace {

// The last call's gated groups (hot_groups[g] = -partner: AUTO's choice made
// on the device from the builder cost) resolved from that cost, which was
// copied back without a host wait: waits for the copy.  Runs when the answer
// is asked for and before the pending set's slot is reused.
void resolve_pending(TrikCvHandle* h) {
  TableSet* t = h->pending_set;
  if (!t) return;
  (void)hipEventSynchronize(t->cost_ready);
  for (size_t g = 0; g < h->hot_groups.size(); ++g)
    if (h->hot_groups[g] < 0)
      h->hot_groups[g] = (int8_t)(g < (size_t)t->groups_cap && t->h_cost[g] <= kChromaMaxCost ? TRIK_HSV_HOT_CHROMA
                                                                                             : -h->hot_groups[g]);
  h->pending_set = nullptr;
}

}  // namespace

// The tables for ranges[0..n), stream-ordered on s: a cached set (s waits
// for its uploads, device side), or a set compiled now into a slot whose
// earlier uses have completed -- found without blocking (hipEventQuery);
// only when all kTableSets sets are still in use does the host wait for the
// least recently used one.
int32_t trik_hsv::acquire_tables(TrikCvHandle* h, const TRIK_VIDTRANSCODE_CV_InArgsAlg* ranges, int n,
                                 hipStream_t s, TableSet** out) {
  std::vector<uint32_t> key;
  key.reserve(3 * n + 1);
  key.push_back((uint32_t)n);
  for (int i = 0; i < n; ++i) {
    const PackedRange p = pack_range(ranges[i]);
    key.push_back(p.from); key.push_back(p.to); key.push_back(p.expect);
  }
  for (TableSet& t : h->sets)
    if (!t.key.empty() && t.key == key) {
      if (t.ready) HIP_TRY(hipStreamWaitEvent(s, t.ready, 0));
      t.tick = ++h->tick;
      *out = &t;
      return 0;
    }
  TableSet* v = nullptr;
  for (TableSet& t : h->sets)
    if (t.key.empty()) { v = &t; break; }
  if (!v)
    for (TableSet& t : h->sets)
      if (t.idle() && (!v || t.tick < v->tick)) v = &t;
  if (!v) {  // every set is in use: wait for the least recently used one
    for (TableSet& t : h->sets)
      if (!v || t.tick < v->tick) v = &t;
    v->users.wait_all();
    if (v->ready) HIP_TRY(hipEventSynchronize(v->ready));
  }
  if (h->pending_set == v) resolve_pending(h);  // (its costs are about to be overwritten)
  if (h->sums_set == v) h->sums_set = nullptr;
  const int groups = (n + kRangesPerLaunch - 1) / kRangesPerLaunch;
  if (groups > v->groups_cap) {
    v->release();
    HIP_TRY(hipMalloc(&v->d_tables, sizeof(RangeTables) * groups));
    HIP_TRY(hipHostMalloc(&v->h_tables, sizeof(RangeTables) * groups, hipHostMallocDefault));
    HIP_TRY(hipMalloc(&v->d_stripe, sizeof(StripeTables) * groups));
    HIP_TRY(hipHostMalloc(&v->h_stripe, sizeof(StripeTables) * groups, hipHostMallocDefault));
    HIP_TRY(hipHostMalloc(&v->h_cost, sizeof(unsigned long long) * groups, hipHostMallocDefault));
    HIP_TRY(hipHostMalloc(&v->h_words, sizeof(unsigned long long) * groups, hipHostMallocDefault));
    HIP_TRY(hipEventCreateWithFlags(&v->words_ready, hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&v->ready, hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&v->cost_ready, hipEventDisableTiming));
    v->groups_cap = groups;
  }
  v->key.clear();  // invalid until the uploads are enqueued
  // the set's earlier uploads and readers have finished (idle), so its pinned
  // staging and device tables may be rewritten
  v->detect.assign(groups, kDetectFull);
  // the tables: built on the device from the packed ranges (no table crosses
  // PCIe: a host-built upload went through the copy engine, whose hand-offs
  // with the compute queue cost tens of microseconds); the per-value tests
  // are also compiled on the host, for detect_mode
  TableBuildArgs ta = {};
  ta.n_ranges = n;
  for (int i = 0; i < n && groups <= kTableGroups; ++i) {
    const PackedRange p = pack_range(ranges[i]);
    ta.from[i] = p.from;
    ta.to[i] = p.to;
    ta.expect[i] = p.expect;
  }
  for (int g = 0; g < groups; ++g) {
    const int cnt = n - g * kRangesPerLaunch < kRangesPerLaunch ? n - g * kRangesPerLaunch : kRangesPerLaunch;
    if (groups <= kTableGroups) {
      compile_tables_head(ranges + g * kRangesPerLaunch, cnt, &v->h_tables[g]);
    } else {  // (more than 64 ranges: compiled on the host, uploaded below)
      compile_tables(ranges + g * kRangesPerLaunch, cnt, &v->h_tables[g]);
      compile_stripe_tables(v->h_tables[g], cnt, &v->h_stripe[g]);
    }
    v->detect[g] = (uint8_t)detect_mode(v->h_tables[g], cnt);
  }
  if (groups == 0) {
  } else if (groups <= kTableGroups) {
    HIP_TRY(launch_compile_tables(ta, groups, v->d_tables, v->d_stripe, s));
  } else {
    HIP_TRY(hipMemcpyAsync(v->d_tables, v->h_tables, sizeof(RangeTables) * groups, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(v->d_stripe, v->h_stripe, sizeof(StripeTables) * groups, hipMemcpyHostToDevice, s));
  }
  HIP_TRY(hipEventRecord(v->ready, s));
  v->key.swap(key);
  v->chroma_built = false;
  v->chroma_share = -1.0;
  if (v->words_pending) (void)hipEventSynchronize(v->words_ready);
  v->words_pending = false;
  v->probes.assign(groups, TableSet::Probe());
  v->chroma_runs = 0;
  v->tick = ++h->tick;
  *out = v;
  return 0;
}

namespace {

// The chroma-run kernel's tables for the set's range groups, built on the
// device from the uploaded RangeTables (stream-ordered on s).  The builder's
// expected exact-path cost is copied back into pinned memory without waiting:
// TableSet::share() reads it once it has landed.
int32_t ensure_chroma(TableSet& t, int groups, hipStream_t s) {
  if (t.chroma_built) return 0;
  if (!t.d_chroma) HIP_TRY(hipMalloc(&t.d_chroma, sizeof(ChromaTables) * t.groups_cap));
  for (int g = 0; g < groups; ++g) {
    HIP_TRY(build_chroma_tables(t.d_tables + g, t.d_chroma + g, s));
    HIP_TRY(hipMemcpyAsync(&t.h_cost[g], &t.d_chroma[g].flagged_cost, sizeof(unsigned long long),
                           hipMemcpyDeviceToHost, s));
  }
  for (int g = groups; g < t.groups_cap; ++g) t.h_cost[g] = 0;
  HIP_TRY(hipEventRecord(t.cost_ready, s));
  HIP_TRY(hipEventRecord(t.ready, s));  // later users on other streams wait for the build too
  t.chroma_built = true;
  t.chroma_share = -1.0;
  return 0;
}

// Batches AUTO keeps on the stripe kernel for a group whose measured share
// is too high before it tries the chroma-run kernel again (re-measuring), and
// AUTO chroma-run launches between readbacks of the measured share.
constexpr int kReprobeAfter = 32;
constexpr int kProbeEvery = 8;

// The measured shares, once their readback has landed (non-blocking).
void poll_measured(TableSet& t) {
  if (!t.words_pending || hipEventQuery(t.words_ready) != hipSuccess) return;
  for (size_t g = 0; g < t.probes.size(); ++g) {
    TableSet::Probe& p = t.probes[g];
    const uint64_t v = t.h_words[g];
    if (p.have_base && p.in_flight > 0 && !p.in_flight_mixed)
      p.measured = (double)(v - p.base) / (double)p.in_flight;
    p.base = v;
    p.have_base = true;
    p.in_flight = 0;
    p.in_flight_mixed = false;
  }
  t.words_pending = false;
}

}  // namespace

HotPlan trik_hsv::plan_hot(TrikCvHandle* h, TableSet& t, int g, int groups, bool big, bool chroma_ok, hipStream_t s,
                           int32_t* rc) {
  *rc = 0;
  const int choice = h->hot.load();
  if (!chroma_ok || !(choice == TRIK_HSV_HOT_CHROMA || (choice == TRIK_HSV_HOT_AUTO && big))) return kPlanStripe;
  *rc = ensure_chroma(t, groups, s);
  if (*rc) return kPlanStripe;
  if (choice == TRIK_HSV_HOT_CHROMA) return kPlanChroma;
  const double sh = t.group_share(g);
  if (sh < 0) return kPlanGated;  // the share is still in flight: no host wait
  if (sh > TRIK_HSV_CHROMA_MAX_SHARE) return kPlanStripe;
  // the input's own share, measured on earlier batches: input that
  // concentrates on the chromas the tables describe worst (their windows and
  // exceptions) goes to the stripe kernel, with a chroma-run batch now and
  // then to see whether it still does
  TableSet::Probe& p = t.probes[g];
  if (p.measured > TRIK_HSV_CHROMA_MAX_SHARE && ++p.stripe_runs <= kReprobeAfter) return kPlanStripe;
  p.stripe_runs = 0;
  return kPlanChroma;
}

namespace {

// After a call's launches: AUTO chroma-run words counted, and every
// kProbeEvery such launches (or right after a re-probe) the groups' exact-path
// word counters read back into pinned memory without a host wait.
int32_t probe_measured(TableSet& t, bool reprobe, hipStream_t s) {
  if (t.chroma_runs == 0 || t.words_pending) return 0;
  bool want = reprobe || t.chroma_runs >= kProbeEvery;
  for (const TableSet::Probe& p : t.probes) want = want || !p.have_base;
  if (!want) return 0;
  const size_t n = t.probes.size();
  for (size_t g = 0; g < n; ++g)
    HIP_TRY(hipMemcpyAsync(&t.h_words[g], &t.d_chroma[g].flagged_words, sizeof(unsigned long long),
                           hipMemcpyDeviceToHost, s));
  HIP_TRY(hipEventRecord(t.words_ready, s));
  for (TableSet::Probe& p : t.probes) {
    p.in_flight = p.launched;
    p.in_flight_mixed = p.mixed;
    p.launched = 0;
    p.mixed = false;
  }
  t.words_pending = true;
  t.chroma_runs = 0;
  return 0;
}

// The fused step's scratch, allocated on first use: one slot of 12 totals per
// CU and the last-workgroup counter; per frame a 128-byte line holding its 12
// accumulators and its unit-done count.  All zeroed once; every launch leaves
// them zero.  A larger batch reallocates the per-frame part (after the
// launches still using it: the caller ordered s after them).
int32_t ensure_fused_scratch(TrikCvHandle* h, int64_t n_frames, hipStream_t s) {
  if (!h->d_wg_part) {
    const size_t parts = (size_t)device_cus() * 12;
    void* p = nullptr;
    HIP_TRY(hipMalloc(&p, sizeof(unsigned long long) * parts + 16));
    h->d_wg_part = static_cast<unsigned long long*>(p);
    h->d_wg_cnt = reinterpret_cast<uint32_t*>(h->d_wg_part + parts);
    HIP_TRY(hipMemsetAsync(h->d_wg_cnt, 0, 16, s));
  }
  if (n_frames > h->frame_acc_cap) {
    if (h->d_frame_acc) {
      HIP_TRY(hipStreamSynchronize(s));
      (void)hipFree(h->d_frame_acc);
      h->d_frame_acc = nullptr;
      h->frame_acc_cap = 0;
    }
    const int64_t cap = n_frames < 1024 ? 1024 : n_frames;
    const size_t bytes = (size_t)cap * 128;
    void* p = nullptr;
    HIP_TRY(hipMalloc(&p, bytes));
    HIP_TRY(hipMemsetAsync(p, 0, bytes, s));
    h->d_frame_acc = static_cast<unsigned long long*>(p);
    h->frame_acc_cap = cap;
  }
  return 0;
}

}  // namespace

int32_t trik_hsv::note_uses(TrikCvHandle* h, TableSet* set, bool maps, hipStream_t s, StreamUses* extra) {
  hipEvent_t e = nullptr;
  int32_t r = h->marks.mark(s, &e);
  if (r) return fail(TRIK_IVIDTRANSCODE_EFAIL, std::string("hipEventRecord: ") + hipGetErrorString((hipError_t)r));
  if (set) set->users.note(s, e);
  if (maps) h->maps_users.note(s, e);
  if (extra) extra->note(s, e);
  return 0;
}

// The hot kernel(s) over the batch: one launch per group of <= 4 ranges.
// Without `step` the kernels ADD into sums (the caller zeroes it).  With it
// the call is a full step: when every group runs the chroma-run kernel and the
// batch gives each workgroup whole frames (chroma_fused_ok), each launch
// zeroes its sums and writes its targets and totals itself (the fused step,
// one launch per group); otherwise sums are zeroed first and the epilogue and
// totals kernels follow.
int32_t trik_hsv::run_sums(TrikCvHandle* h, const TrikHsvFrameBatch* b,
                           const TRIK_VIDTRANSCODE_CV_InArgsAlg* ranges, int n, TrikHsvTargetSums* sums,
                           uint8_t* masks, hipStream_t s, const StepOut* step) {
  TableSet* t = nullptr;
  int32_t rc = acquire_tables(h, ranges, n, s, &t);
  if (rc) return rc;
  h->sums_set = t;
  const bool empty = b->n_frames == 0 || b->width == 0 || b->height == 0;
  const int groups = (n + kRangesPerLaunch - 1) / kRangesPerLaunch;
  const bool big = (int64_t)b->n_frames * b->width * b->height >= (int64_t)TRIK_HSV_CHROMA_MIN_PIXELS;
  FrameView frames = frame_view(*b);
  if (b->n_frames <= 1) frames.frame_stride = 0;  // (not validated then; the launchers test its alignment)
  std::vector<KernelArgs> args(empty ? 0 : groups, KernelArgs{frames});
  std::vector<HotPlan> plans(args.size(), kPlanStripe);
  bool fused = step != nullptr && !masks && !empty;
  poll_measured(*t);
  bool reprobe = false;
  for (size_t g = 0; g < args.size(); ++g) {
    KernelArgs& a = args[g];
    a.n_ranges = n - (int)g * kRangesPerLaunch < kRangesPerLaunch ? n - (int)g * kRangesPerLaunch : kRangesPerLaunch;
    a.range_offset = (int)g * kRangesPerLaunch;
    a.sums_ranges = n;
    a.tables = t->d_tables + g;
    a.stripe_tables = t->d_stripe + g;
    a.detect_mode = t->detect[g];
    a.sums = sums;
    a.masks = masks;
    a.mask_shift = (int)g * kRangesPerLaunch;
    // the chroma-run kernel for large batches, the stripe kernel otherwise;
    // the generic kernel takes misaligned inputs and rows wider than 8192 pixels
    // value-only groups (every range accepts every hue and saturation) run
    // the stripe kernel's value form under AUTO at any batch size: it beats
    // the chroma-run kernel there and needs no table build
    const bool was_measured_stripe = g < t->probes.size() && t->probes[g].stripe_runs > 0;
    plans[g] = plan_hot(h, *t, (int)g, groups, big && t->detect[g] != kDetectV,
                        h->hot.load() != TRIK_HSV_HOT_GENERIC && chroma_geometry_ok(a), s, &rc);
    if (rc) return rc;
    reprobe = reprobe || (was_measured_stripe && plans[g] == kPlanChroma);
    fused = fused && plans[g] == kPlanChroma && chroma_fused_ok(a);
  }
  if (fused) {
    HIP_TRY(h->fused_users.order_after(s));
    rc = ensure_fused_scratch(h, b->n_frames, s);
    if (rc) return rc;
  }
  bool any_chroma = false;
  for (HotPlan p : plans) any_chroma = any_chroma || p != kPlanStripe;
  if (any_chroma && !h->d_tail_sink) {  // (its contents are never used: zeroed once for tidiness)
    void* p = nullptr;
    HIP_TRY(hipMalloc(&p, (size_t)kChromaTailSink));
    HIP_TRY(hipMemsetAsync(p, 0, (size_t)kChromaTailSink, s));
    h->d_tail_sink = static_cast<uint8_t*>(p);
  }
  for (KernelArgs& a : args) {
    a.tail = h->d_tail_sink;
    a.tail_bytes = h->d_tail_sink ? kChromaTailSink : 0;
    a.reserved_cus = h->reserved_cus.load();
  }
  if (step && !fused && b->n_frames > 0 && sums)  // (frames of zero width or height: zero sums)
    HIP_TRY(hipMemsetAsync(sums, 0, sizeof(TrikHsvTargetSums) * (size_t)b->n_frames * n, s));
  bool gated = false, chroma_ran = false;
  // (an empty batch launches nothing and keeps the last call's answer)
  if (!args.empty()) {
    h->hot_groups.assign(groups, 0);
    h->pending_set = nullptr;  // (set again as soon as a group is gated)
  }
  for (size_t g = 0; g < args.size(); ++g) {
    KernelArgs& a = args[g];
    const HotPlan plan = plans[g];
    int e = hipErrorNotSupported;
    if (plan == kPlanChroma) {
      if (fused) {
        a.fused = 1;
        a.targets = step->targets;
        a.totals = step->totals;
        a.wg_part = h->d_wg_part;
        a.wg_cnt = h->d_wg_cnt;
        a.frame_acc = h->d_frame_acc;
      }
      e = launch_chroma(a, t->d_chroma + g, masks != nullptr, s);
      if (e == hipSuccess) {
        h->hot_groups[g] = TRIK_HSV_HOT_CHROMA;
        // every chroma-run launch adds to the group's flagged_words (forced or
        // AUTO), so every one counts its words: the two sides of the share
        t->probes[g].launched += (uint64_t)a.n_frames * (uint64_t)(a.width / 2) * (uint64_t)a.height;
        chroma_ran = true;
      }
    } else if (plan == kPlanGated) {
      // AUTO's rule on the device: the chroma-run kernel runs while this
      // group's cost is at most kChromaMaxCost, its partner otherwise -- the
      // stripe kernel, or the generic kernel where the stripe kernel's
      // geometry does not take the batch (rows wider than 8192 pixels), with
      // the same gate: exactly one of the two adds into the sums
      KernelArgs ac = a, as = a;
      ac.gate = as.gate = &t->d_chroma[g].flagged_cost;
      ac.gate_max = as.gate_max = kChromaMaxCost;
      ac.gate_le = 1;
      as.gate_le = 0;
      e = launch_chroma(ac, t->d_chroma + g, masks != nullptr, s);
      if (e == hipSuccess) {
        int partner = TRIK_HSV_HOT_STRIPE;
        e = launch_stripe(as, masks != nullptr, s);
        if (e == hipErrorNotSupported) {
          partner = TRIK_HSV_HOT_GENERIC;
          e = launch_reduce(as, masks != nullptr, s);
        }
        HIP_TRY(e);  // never an ungated launch after a gated one
        h->hot_groups[g] = (int8_t)-partner;
        h->pending_set = t;  // at once: a later group's error return leaves it consistent
        t->probes[g].mixed = true;
        gated = true;
        continue;
      }
    }
    if (e == hipErrorNotSupported && h->hot.load() != TRIK_HSV_HOT_GENERIC) {
      e = launch_stripe(a, masks != nullptr, s);
      if (e == hipSuccess) h->hot_groups[g] = TRIK_HSV_HOT_STRIPE;
    }
    if (e == hipErrorNotSupported) {
      e = launch_reduce(a, masks != nullptr, s);
      if (e == hipSuccess) h->hot_groups[g] = TRIK_HSV_HOT_GENERIC;
    }
    HIP_TRY(e);
  }
  // (an empty batch keeps the last call's answer, gated groups included)
  if (!args.empty()) h->pending_set = gated ? t : nullptr;
  if (chroma_ran) ++t->chroma_runs;  // once per call, whichever groups ran it
  if (!masks) {
    rc = probe_measured(*t, reprobe, s);
    if (rc) return rc;
  }
  if (step && !fused) {  // the epilogue and the totals as kernels of their own
    if (step->targets) HIP_TRY(launch_targets(*b, n, sums, step->targets, s));
    if (step->totals) HIP_TRY(launch_totals(b->n_frames > 0 ? b->n_frames : 0, n, sums, step->totals, s));
  }
  return note_uses(h, t, false, s, fused ? &h->fused_users : nullptr);
}

// ---------------------------------------------------------------------------
// The hot-kernel setting and what the last call ran
// ---------------------------------------------------------------------------
extern "C" int32_t trik_hsv_set_hot_kernel(TRIK_VIDTRANSCODE_CV_Handle h, int32_t kind) {
  if (!h || kind < TRIK_HSV_HOT_AUTO || kind > TRIK_HSV_HOT_GENERIC) return -1;
  return h->hot.exchange(kind);
}

extern "C" int32_t trik_hsv_set_reserved_cus(TRIK_VIDTRANSCODE_CV_Handle h, int32_t n) {
  if (!h || n < 0 || n > 32) return -1;
  return h->reserved_cus.exchange(n);
}

extern "C" int32_t trik_hsv_last_hot_kernel(TRIK_VIDTRANSCODE_CV_Handle h) {
  if (!h) return 0;
  std::lock_guard<std::mutex> lock(h->mu);
  {
    DeviceGuard dg(h->device);
    resolve_pending(h);
  }
  int kind = 0;
  for (int8_t k : h->hot_groups) {
    if (!k) continue;
    kind = kind == 0 || kind == k ? k : TRIK_HSV_HOT_MIXED;
  }
  return kind;
}

extern "C" int32_t trik_hsv_chroma_share(TRIK_VIDTRANSCODE_CV_Handle h, double* share) {
  if (!h || !share) return fail(TRIK_IVIDTRANSCODE_EFAIL, "NULL handle or share");
  std::lock_guard<std::mutex> lock(h->mu);
  DeviceGuard dg(h->device);
  TableSet* t = h->sums_set;
  *share = -1.0;
  if (t && t->chroma_built) {
    HIP_TRY(hipEventSynchronize(t->cost_ready));
    *share = t->share();
  }
  return 0;
}

extern "C" int32_t trik_hsv_chroma_measured_share(TRIK_VIDTRANSCODE_CV_Handle h, double* share) {
  if (!h || !share) return fail(TRIK_IVIDTRANSCODE_EFAIL, "NULL handle or share");
  std::lock_guard<std::mutex> lock(h->mu);
  DeviceGuard dg(h->device);
  TableSet* t = h->sums_set;
  *share = -1.0;
  if (!t) return 0;
  if (t->words_pending) HIP_TRY(hipEventSynchronize(t->words_ready));
  poll_measured(*t);
  for (const TableSet::Probe& p : t->probes)
    if (p.measured > *share) *share = p.measured;
  return 0;
}
