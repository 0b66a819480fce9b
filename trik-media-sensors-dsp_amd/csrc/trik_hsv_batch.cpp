// trik_hsv_batch.cpp -- Layer 2 of the C ABI: the batched device API
// (trik_hsv_*), each entry point its argument checks and then the shared
// enqueue path (run_sums, or the sensor's core in trik_hsv_sensors.cpp).
#include <math.h>
#include <string.h>

#include "trik_hsv_handle.h"

using namespace trik_hsv;

namespace {

// A device buffer handed to a batched call must be device-accessible memory
// of the handle's device ("" if so).
std::string device_buffer_error(const void* p, int dev, const char* what) {
  if (!p) return "";
  hipPointerAttribute_t at;
  if (hipPointerGetAttributes(&at, p) != hipSuccess) {
    (void)hipGetLastError();
    return std::string(what) + " is not device-accessible memory";
  }
  if (at.type == hipMemoryTypeUnregistered)
    return std::string(what) + " is pageable host memory, not device-accessible memory";
  if (at.type == hipMemoryTypeDevice && at.device != dev)
    return std::string(what) + " is on device " + std::to_string(at.device) + ", the handle on device " +
           std::to_string(dev);
  return "";
}

// The batch's frames and the output buffer live on the handle's device.
int32_t check_device(TRIK_VIDTRANSCODE_CV_Handle h, const TrikHsvFrameBatch* b, const void* out) {
  if (!b || b->n_frames <= 0) return 0;
  DeviceGuard dg(h->device);
  std::string e = device_buffer_error(b->frames, h->device, "frames");
  if (e.empty()) e = device_buffer_error(out, h->device, "the output buffer");
  return e.empty() ? 0 : fail(TRIK_IVIDTRANSCODE_EFAIL, e);
}

int32_t check_batch(const TrikHsvFrameBatch* b) {
  const std::string e = validate_batch(b);
  return e.empty() ? 0 : fail(TRIK_IVIDTRANSCODE_EFAIL, e);
}

int32_t check_handle_batch(TRIK_VIDTRANSCODE_CV_Handle h, const TrikHsvFrameBatch* b) {
  if (!h) return fail(TRIK_IVIDTRANSCODE_EFAIL, "handle is NULL");
  return check_batch(b);
}

int32_t check_common(TRIK_VIDTRANSCODE_CV_Handle h, const TrikHsvFrameBatch* b,
                     const TRIK_VIDTRANSCODE_CV_InArgsAlg* ranges, int32_t n, const void* sums) {
  int32_t rc = check_handle_batch(h, b);
  if (rc) return rc;
  if (n < 1 || n > TRIK_HSV_MAX_RANGES || !ranges)
    return fail(TRIK_IVIDTRANSCODE_EFAIL, "n_ranges must be 1..64");
  if (!sums && b->n_frames > 0) return fail(TRIK_IVIDTRANSCODE_EFAIL, "sums is NULL");
  return check_device(h, b, sums);
}

// "ov7670 layout required": sensor names the caller in the message.
int32_t check_ov7670(const TrikHsvFrameBatch* b, const char* sensor) {
  if (b->layout == TRIK_HSV_LAYOUT_OV7670) return 0;
  return fail(TRIK_IVIDTRANSCODE_EFAIL, std::string("the ") + sensor + " sensor takes the ov7670 layout (YUV422P)");
}

// Handle and batch, then the layout, of an ov7670 sensor's entry point.
int32_t check_ov7670_call(TRIK_VIDTRANSCODE_CV_Handle h, const TrikHsvFrameBatch* b, const char* sensor) {
  const int32_t rc = check_handle_batch(h, b);
  return rc ? rc : check_ov7670(b, sensor);
}

int64_t preview_bytes(const PreviewDst& d) { return (int64_t)d.out_h * d.out_ll; }

// The last checks of a preview entry point before the lock: the preview-output
// geometry d.  `buffers`: every buffer the call needs is there.  The object
// sensor's call (ball) also checks its sums_pitch and words its errors itself.
int32_t check_preview_out(const TrikHsvFrameBatch* b, const PreviewDst& d, bool buffers, bool ball = false,
                          int32_t sums_pitch = 1) {
  if (d.out_w < 0 || d.out_h < 0 || d.out_ll < 2 * d.out_w || sums_pitch < 1)
    return fail(TRIK_IVIDTRANSCODE_EFAIL, std::string("preview geometry: need out_line_length >= 2*out_width") +
                                              (ball ? ", sums_pitch >= 1" : ""));
  if (b->n_frames > 1 && d.stride < preview_bytes(d))
    return fail(TRIK_IVIDTRANSCODE_EFAIL, "preview_stride smaller than one preview");
  if (b->n_frames > 0 && preview_bytes(d) > 0 && !buffers)
    return fail(TRIK_IVIDTRANSCODE_EFAIL, ball ? "previews is NULL" : "NULL buffer");
  return 0;
}

// A preview entry point after its checks: with the handle locked and its device
// current, nothing when there is no frame or no preview byte; else the
// previews checked as memory of that device, then `enqueue`.
template <typename Enqueue>
int32_t locked_preview(TRIK_VIDTRANSCODE_CV_Handle h, const TrikHsvFrameBatch* b, const PreviewDst& d,
                       Enqueue enqueue) {
  std::lock_guard<std::mutex> lock(h->mu);
  DeviceGuard dg(h->device);
  if (b->n_frames == 0 || preview_bytes(d) == 0) return 0;
  const int32_t rc = check_device(h, b, d.previews);
  return rc ? rc : enqueue();
}

// Frames without pixels write no preview pixel: the zero fill alone.
int32_t zero_previews(const TrikHsvFrameBatch* b, const PreviewDst& d, hipStream_t s) {
  for (int32_t f = 0; f < b->n_frames; ++f)
    HIP_TRY(hipMemsetAsync(d.previews + (int64_t)f * (b->n_frames > 1 ? d.stride : 0), 0, (size_t)preview_bytes(d), s));
  return 0;
}

// Frames without pixels hold no blob: every slot's targets (and top, n_labels) zero.
int32_t zero_blob_outputs(TrikHsvTarget* targets, int32_t* top, int32_t* n_labels, size_t slots, hipStream_t s) {
  HIP_TRY(hipMemsetAsync(targets, 0, sizeof(TrikHsvTarget) * 8 * slots, s));
  if (top) HIP_TRY(hipMemsetAsync(top, 0, sizeof(int32_t) * 24 * slots, s));
  if (n_labels) HIP_TRY(hipMemsetAsync(n_labels, 0, sizeof(int32_t) * slots, s));
  return 0;
}

}  // namespace

extern "C" int32_t trik_hsv_batch_sums(TRIK_VIDTRANSCODE_CV_Handle h, const TrikHsvFrameBatch* b,
                                       const TRIK_VIDTRANSCODE_CV_InArgsAlg* ranges, int32_t n,
                                       TrikHsvTargetSums* sums, void* stream) {
  int32_t rc = check_common(h, b, ranges, n, sums);
  if (rc) return rc;
  std::lock_guard<std::mutex> lock(h->mu);
  DeviceGuard dg(h->device);
  return run_sums(h, b, ranges, n, sums, nullptr, static_cast<hipStream_t>(stream));
}

extern "C" int32_t trik_hsv_batch_totals(int32_t n_frames, int32_t n_ranges, const TrikHsvTargetSums* sums,
                                         TrikHsvTargetSums* totals, void* stream) {
  if (n_frames < 0 || n_ranges < 1 || n_ranges > TRIK_HSV_MAX_RANGES)
    return fail(TRIK_IVIDTRANSCODE_EFAIL, "batch_totals: need n_frames >= 0 and n_ranges 1..64");
  if (!totals || (n_frames > 0 && !sums)) return fail(TRIK_IVIDTRANSCODE_EFAIL, "batch_totals: NULL buffer");
  HIP_TRY(launch_totals(n_frames, n_ranges, sums, totals, static_cast<hipStream_t>(stream)));
  return 0;
}

extern "C" int32_t trik_hsv_batch_targets(const TrikHsvFrameBatch* b, int32_t n,
                                          const TrikHsvTargetSums* sums, TrikHsvTarget* targets,
                                          void* stream) {
  // only the geometry matters here (no frame bytes are read)
  if (!b) return fail(TRIK_IVIDTRANSCODE_EFAIL, "batch is NULL");
  if (b->n_frames < 0 || b->width <= 0 || b->height <= 0 || b->width > 32767 || b->height > 32767)
    return fail(TRIK_IVIDTRANSCODE_EFAIL, "batch_targets: need n_frames >= 0 and 0 < width, height <= 32767");
  if (n < 1 || n > TRIK_HSV_MAX_RANGES) return fail(TRIK_IVIDTRANSCODE_EFAIL, "n_ranges must be 1..64");
  if (b->n_frames > 0 && (!sums || !targets)) return fail(TRIK_IVIDTRANSCODE_EFAIL, "NULL buffer");
  HIP_TRY(launch_targets(*b, n, sums, targets, static_cast<hipStream_t>(stream)));
  return 0;
}

extern "C" int32_t trik_hsv_process_batch(TRIK_VIDTRANSCODE_CV_Handle h, const TrikHsvFrameBatch* b,
                                          const TRIK_VIDTRANSCODE_CV_InArgsAlg* ranges, int32_t n,
                                          TrikHsvTargetSums* sums, TrikHsvTarget* targets,
                                          void* stream) {
  int32_t rc = check_common(h, b, ranges, n, sums);
  if (rc) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  std::lock_guard<std::mutex> lock(h->mu);
  DeviceGuard dg(h->device);
  StepOut step;
  step.targets = targets;
  return run_sums(h, b, ranges, n, sums, nullptr, s, &step);
}

extern "C" int32_t trik_hsv_process_batch_totals(TRIK_VIDTRANSCODE_CV_Handle h, const TrikHsvFrameBatch* b,
                                                 const TRIK_VIDTRANSCODE_CV_InArgsAlg* ranges, int32_t n,
                                                 TrikHsvTargetSums* sums, TrikHsvTarget* targets,
                                                 TrikHsvTargetSums* totals, void* stream) {
  int32_t rc = check_common(h, b, ranges, n, sums);
  if (rc) return rc;
  if (!totals) return fail(TRIK_IVIDTRANSCODE_EFAIL, "totals is NULL");
  hipStream_t s = static_cast<hipStream_t>(stream);
  std::lock_guard<std::mutex> lock(h->mu);
  DeviceGuard dg(h->device);
  rc = check_device(h, b, totals);
  if (rc) return rc;
  StepOut step;
  step.targets = targets;
  step.totals = totals;
  return run_sums(h, b, ranges, n, sums, nullptr, s, &step);
}

extern "C" int32_t trik_hsv_batch_masks(TRIK_VIDTRANSCODE_CV_Handle h, const TrikHsvFrameBatch* b,
                                        const TRIK_VIDTRANSCODE_CV_InArgsAlg* ranges, int32_t n,
                                        uint8_t* masks, TrikHsvTargetSums* sums, void* stream) {
  int32_t rc = check_common(h, b, ranges, n, sums);
  if (rc) return rc;
  if (n > 8) return fail(TRIK_IVIDTRANSCODE_EFAIL, "mask mode supports at most 8 ranges");
  if (!masks && b->n_frames > 0) return fail(TRIK_IVIDTRANSCODE_EFAIL, "masks is NULL");
  std::lock_guard<std::mutex> lock(h->mu);
  DeviceGuard dg(h->device);
  return run_sums(h, b, ranges, n, sums, masks, static_cast<hipStream_t>(stream));
}

extern "C" int32_t trik_hsv_batch_preview(TRIK_VIDTRANSCODE_CV_Handle h, const TrikHsvFrameBatch* b,
                                          const TRIK_VIDTRANSCODE_CV_InArgsAlg* range,
                                          const TrikHsvTargetSums* sums, int32_t sums_pitch,
                                          int32_t out_width, int32_t out_height,
                                          int32_t out_line_length, uint8_t* previews,
                                          int64_t preview_stride, void* stream) {
  const PreviewDst d = {out_width, out_height, out_line_length, previews, preview_stride};
  int32_t rc = check_common(h, b, range, 1, sums);
  if (!rc) rc = check_preview_out(b, d, previews != nullptr, true, sums_pitch);
  if (rc) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  return locked_preview(h, b, d, [&] { return preview_core(h, *b, *range, sums, sums_pitch, d, s); });
}

extern "C" int32_t trik_hsv_batch_auto_range(const TrikHsvFrameBatch* b, uint16_t* out, void* stream) {
  int32_t rc = check_batch(b);
  if (rc) return rc;
  if (!out && b->n_frames > 0) return fail(TRIK_IVIDTRANSCODE_EFAIL, "out is NULL");
  HIP_TRY(launch_auto_range(auto_range_args(*b, out), static_cast<hipStream_t>(stream)));
  return 0;
}

namespace {

// The batch, then the kind against its layout and the side cap.
int32_t check_auto_exact(const TrikHsvFrameBatch* b, int32_t kind) {
  const int32_t rc = check_batch(b);
  if (rc) return rc;
  const std::string e = auto_exact_error(kind, b->layout, b->width, b->height);
  return e.empty() ? 0 : fail(TRIK_IVIDTRANSCODE_EFAIL, e);
}

}  // namespace

extern "C" int32_t trik_hsv_auto_scores(const TrikHsvFrameBatch* b, int32_t kind, int32_t* scores, int32_t* start,
                                        void* stream) {
  const int32_t rc = check_auto_exact(b, kind);
  if (rc) return rc;
  if (b->n_frames > 0 && (!scores || !start)) return fail(TRIK_IVIDTRANSCODE_EFAIL, "auto_scores: NULL buffer");
  HIP_TRY(launch_auto_exact(auto_exact_args(*b, kind, scores, start, nullptr, nullptr),
                            static_cast<hipStream_t>(stream)));
  return 0;
}

extern "C" int32_t trik_hsv_batch_auto_range_exact(const TrikHsvFrameBatch* b, int32_t kind, uint16_t* out,
                                                   int32_t* best, void* stream) {
  const int32_t rc = check_auto_exact(b, kind);
  if (rc) return rc;
  if (b->n_frames > 0 && !out) return fail(TRIK_IVIDTRANSCODE_EFAIL, "out is NULL");
  HIP_TRY(launch_auto_exact(auto_exact_args(*b, kind, nullptr, nullptr, out, best),
                            static_cast<hipStream_t>(stream)));
  return 0;
}

extern "C" int32_t trik_hsv_auto_range_of(int32_t kind, int32_t h1, int32_t h2, int32_t s1, int32_t s2,
                                          uint16_t out[6]) {
  if (!out) return fail(TRIK_IVIDTRANSCODE_EFAIL, "auto_range_of: out is NULL");
  if (kind == TRIK_HSV_AUTO_OV7670_OBJECT) {
    if (h1 < 0 || h1 > 31 || h2 < 0 || h2 > 31 || s1 < 0 || s2 > 31 || s1 > s2)
      return fail(TRIK_IVIDTRANSCODE_EFAIL, "auto_range_of: need 0 <= h1, h2 <= 31 and 0 <= s1 <= s2 <= 31");
  } else if (kind == TRIK_HSV_AUTO_OV7670_LINE || kind == TRIK_HSV_AUTO_WEBCAM_LINE) {
    if (h1 < 0 || h2 > 255 || h1 > h2) return fail(TRIK_IVIDTRANSCODE_EFAIL, "auto_range_of: need 0 <= v0 <= v1 <= 255");
  } else {
    return fail(TRIK_IVIDTRANSCODE_EFAIL, "auto range: unknown kind " + std::to_string(kind));
  }
  auto_range_scale(kind, h1, h2, s1, s2, out);
  return 0;
}

extern "C" int32_t trik_hsv_set_auto_detect(TRIK_VIDTRANSCODE_CV_Handle h, int32_t mode) {
  if (!h) {
    fail(TRIK_IVIDTRANSCODE_EFAIL, "handle is NULL");
    return -1;
  }
  if (h->algo != kAlgoBlob && h->algo != kAlgoLine && h->algo != kAlgoWLine) {
    fail(TRIK_IVIDTRANSCODE_EFAIL, "set_auto_detect: only the ov7670 object sensor and the line sensors take it");
    return -1;
  }
  if (mode != 0 && mode != 1) {
    fail(TRIK_IVIDTRANSCODE_EFAIL, "set_auto_detect: mode must be 0 or 1");
    return -1;
  }
  return h->auto_detect.exchange(mode);
}

extern "C" int32_t trik_hsv_line_batch(const TrikHsvFrameBatch* b, int32_t val_from, int32_t val_to,
                                       int32_t band_start, int32_t band_stop, TrikHsvTargetSums* sums,
                                       TrikHsvTarget* targets, void* stream) {
  int32_t rc = check_batch(b);
  if (!rc) rc = check_ov7670(b, "line");
  if (rc) return rc;
  if (b->n_frames > 0 && !sums) return fail(TRIK_IVIDTRANSCODE_EFAIL, "sums is NULL");
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (b->n_frames == 0) return 0;
  HIP_TRY(hipMemsetAsync(sums, 0, sizeof(TrikHsvTargetSums) * (size_t)b->n_frames, s));
  if (b->width == 0 || b->height == 0) {
    if (targets) HIP_TRY(hipMemsetAsync(targets, 0, sizeof(TrikHsvTarget) * (size_t)b->n_frames, s));
    return 0;
  }
  HIP_TRY(launch_line(line_args(*b, val_from, val_to, band_start, band_stop, sums, targets), s));
  return 0;
}

extern "C" int32_t trik_hsv_line_frame_ranges_batch(const TrikHsvFrameBatch* b, const uint16_t* ranges,
                                                    int32_t band_start, int32_t band_stop, TrikHsvTargetSums* sums,
                                                    TrikHsvTarget* targets, void* stream) {
  const int32_t rc = check_batch(b);
  if (rc) return rc;
  if (b->n_frames > 0 && !ranges) return fail(TRIK_IVIDTRANSCODE_EFAIL, "ranges is NULL");
  if (b->n_frames > 0 && !sums) return fail(TRIK_IVIDTRANSCODE_EFAIL, "sums is NULL");
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (b->n_frames == 0) return 0;
  HIP_TRY(hipMemsetAsync(sums, 0, sizeof(TrikHsvTargetSums) * (size_t)b->n_frames, s));
  if (b->width == 0 || b->height == 0) {
    if (targets) HIP_TRY(hipMemsetAsync(targets, 0, sizeof(TrikHsvTarget) * (size_t)b->n_frames, s));
    return 0;
  }
  LineArgs a = line_args(*b, 0, 0, band_start, band_stop, sums, targets);
  a.ranges = ranges;  // read by the kernels, never here
  HIP_TRY(launch_line(a, s));
  return 0;
}

extern "C" int32_t trik_hsv_line_scale_val(int32_t percent) { return (int32_t)scale_val(percent); }

extern "C" int32_t trik_hsv_frame_ranges_batch(const TrikHsvFrameBatch* b, const uint16_t* ranges, int32_t n,
                                               TrikHsvTargetSums* sums, TrikHsvTarget* targets, void* stream) {
  int32_t rc = check_batch(b);
  if (rc) return rc;
  if (n < 1 || n > TRIK_HSV_MAX_RANGES) return fail(TRIK_IVIDTRANSCODE_EFAIL, "n_ranges must be 1..64");
  if (b->n_frames > 0 && !ranges) return fail(TRIK_IVIDTRANSCODE_EFAIL, "ranges is NULL");
  if (b->n_frames > 0 && !sums) return fail(TRIK_IVIDTRANSCODE_EFAIL, "sums is NULL");
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (b->n_frames == 0) return 0;
  const size_t slots = (size_t)b->n_frames * (size_t)n;
  HIP_TRY(hipMemsetAsync(sums, 0, sizeof(TrikHsvTargetSums) * slots, s));
  if (b->width == 0 || b->height == 0) {
    if (targets) HIP_TRY(hipMemsetAsync(targets, 0, sizeof(TrikHsvTarget) * slots, s));
    return 0;
  }
  HIP_TRY(launch_frame_ranges(*b, ranges, n, sums, s));
  if (targets) HIP_TRY(launch_targets(*b, n, sums, targets, s));
  return 0;
}

extern "C" int32_t trik_hsv_convert_batch(const TrikHsvFrameBatch* b, const TrikHsvConvertOut* o, void* stream) {
  if (!o) return fail(TRIK_IVIDTRANSCODE_EFAIL, "convert_batch: out is NULL");
  const int32_t rc = check_batch(b);
  if (rc) return rc;
  if (o->form != TRIK_HSV_CONVERT_RGB888HSV && o->form != TRIK_HSV_CONVERT_HSV_PLANES &&
      o->form != TRIK_HSV_CONVERT_RGB_PLANES)
    return fail(TRIK_IVIDTRANSCODE_EFAIL, "convert_batch: unknown form " + std::to_string(o->form));
  if (b->n_frames > 0 && !b->frames) return fail(TRIK_IVIDTRANSCODE_EFAIL, "frames is NULL");
  if (b->n_frames > 0 && !o->out) return fail(TRIK_IVIDTRANSCODE_EFAIL, "convert_batch: out->out is NULL");
  const bool planes = o->form != TRIK_HSV_CONVERT_RGB888HSV;
  if (o->row_pitch < (planes ? 1 : 8) * (int64_t)b->width)
    return fail(TRIK_IVIDTRANSCODE_EFAIL, "convert_batch: row_pitch shorter than a row (8*width, or width for planes)");
  const int64_t image = (int64_t)b->height * o->row_pitch;
  if (planes && o->plane_stride < image)
    return fail(TRIK_IVIDTRANSCODE_EFAIL, "convert_batch: plane_stride smaller than a plane (height*row_pitch)");
  // (plane_stride >= 0 here, and below 2^62 or the sum would not be below frame_stride)
  if (planes ? o->plane_stride > (INT64_MAX - image) / 2 || o->frame_stride < 2 * o->plane_stride + image
             : o->frame_stride < image)
    return fail(TRIK_IVIDTRANSCODE_EFAIL, "convert_batch: frame_stride smaller than a frame's output");
  if (b->n_frames == 0 || b->width == 0 || b->height == 0) return 0;  // nothing is written
  HIP_TRY(launch_convert(*b, *o, static_cast<hipStream_t>(stream)));
  return 0;
}

extern "C" int32_t trik_hsv_mask_batch(const TrikHsvFrameBatch* b, const uint16_t* ranges, int32_t n,
                                       int64_t ranges_stride, const TrikHsvMaskOut* o, void* stream) {
  if (!o) return fail(TRIK_IVIDTRANSCODE_EFAIL, "mask_batch: out is NULL");
  const int32_t rc = check_batch(b);
  if (rc) return rc;
  if (o->form != TRIK_HSV_MASK_BITS && o->form != TRIK_HSV_MASK_BYTES)
    return fail(TRIK_IVIDTRANSCODE_EFAIL, "mask_batch: unknown form " + std::to_string(o->form));
  if (n < 1 || n > TRIK_HSV_MAX_RANGES) return fail(TRIK_IVIDTRANSCODE_EFAIL, "mask_batch: n_ranges must be 1..64");
  if (ranges_stride != 0 && ranges_stride < 6 * (int64_t)n)
    return fail(TRIK_IVIDTRANSCODE_EFAIL, "mask_batch: ranges_frame_stride must be 0 (shared) or at least 6*n_ranges");
  if (b->n_frames > 0 && !b->frames) return fail(TRIK_IVIDTRANSCODE_EFAIL, "frames is NULL");
  if (b->n_frames > 0 && !ranges) return fail(TRIK_IVIDTRANSCODE_EFAIL, "mask_batch: ranges is NULL");
  if (b->n_frames > 0 && !o->out) return fail(TRIK_IVIDTRANSCODE_EFAIL, "mask_batch: out->out is NULL");
  if (o->row_pitch < (o->form == TRIK_HSV_MASK_BITS ? b->width / 8 : b->width))
    return fail(TRIK_IVIDTRANSCODE_EFAIL, "mask_batch: row_pitch shorter than a row (width/8 for bits, width for bytes)");
  const int64_t image = (int64_t)b->height * o->row_pitch;
  if (o->plane_stride < image)
    return fail(TRIK_IVIDTRANSCODE_EFAIL, "mask_batch: plane_stride smaller than a plane (height*row_pitch)");
  // (plane_stride >= 0 here; the product is kept below 2^63)
  if (o->plane_stride > (INT64_MAX - image) / n || o->frame_stride < (n - 1) * o->plane_stride + image)
    return fail(TRIK_IVIDTRANSCODE_EFAIL, "mask_batch: frame_stride smaller than a frame's planes");
  if (b->n_frames == 0 || b->width == 0 || b->height == 0) return 0;  // nothing is written
  HIP_TRY(launch_mask(*b, ranges, n, ranges_stride, *o, static_cast<hipStream_t>(stream)));
  return 0;
}

extern "C" int32_t trik_hsv_ranges_of_detect(const uint16_t* detect, int32_t n, uint16_t* ranges, int32_t n_ranges,
                                             int32_t t, void* stream) {
  if (n < 0) return fail(TRIK_IVIDTRANSCODE_EFAIL, "ranges_of_detect: n < 0");
  if (n_ranges < 1 || n_ranges > TRIK_HSV_MAX_RANGES)
    return fail(TRIK_IVIDTRANSCODE_EFAIL, "ranges_of_detect: n_ranges must be 1..64");
  if (t < 0 || t >= n_ranges) return fail(TRIK_IVIDTRANSCODE_EFAIL, "ranges_of_detect: t must be 0..n_ranges-1");
  if (n > 0 && (!detect || !ranges)) return fail(TRIK_IVIDTRANSCODE_EFAIL, "ranges_of_detect: NULL buffer");
  HIP_TRY(launch_ranges_of_detect(detect, n, ranges, n_ranges, t, static_cast<hipStream_t>(stream)));
  return 0;
}

extern "C" int32_t trik_hsv_frame_ranges_preview(TRIK_VIDTRANSCODE_CV_Handle h, const TrikHsvFrameBatch* b,
                                                 const uint16_t* ranges, int32_t n, int32_t t,
                                                 const TrikHsvTargetSums* sums, int32_t sums_pitch,
                                                 int32_t out_width, int32_t out_height, int32_t out_line_length,
                                                 uint8_t* previews, int64_t preview_stride, void* stream) {
  const PreviewDst d = {out_width, out_height, out_line_length, previews, preview_stride};
  int32_t rc = check_handle_batch(h, b);
  if (rc) return rc;
  if (n < 1 || n > TRIK_HSV_MAX_RANGES) return fail(TRIK_IVIDTRANSCODE_EFAIL, "n_ranges must be 1..64");
  if (t < 0 || t >= n) return fail(TRIK_IVIDTRANSCODE_EFAIL, "frame_ranges_preview: t must be 0..n_ranges-1");
  if (b->n_frames > 0 && !ranges) return fail(TRIK_IVIDTRANSCODE_EFAIL, "ranges is NULL");
  if (b->n_frames > 0 && !sums) return fail(TRIK_IVIDTRANSCODE_EFAIL, "sums is NULL");
  rc = check_device(h, b, sums);
  if (!rc) rc = check_preview_out(b, d, previews != nullptr, true, sums_pitch);
  if (rc) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  return locked_preview(h, b, d, [&] {
    // (the pointer's kind is asked of the runtime; its bytes are read by the kernels alone)
    const std::string e = device_buffer_error(ranges, h->device, "ranges");
    if (!e.empty()) return fail(TRIK_IVIDTRANSCODE_EFAIL, e);
    return frame_ranges_preview_core(h, *b, ranges, n, t, sums, sums_pitch, d, s);
  });
}

extern "C" int32_t trik_hsv_line_preview(TRIK_VIDTRANSCODE_CV_Handle h, const TrikHsvFrameBatch* b,
                                         int32_t val_from, int32_t val_to, const TrikHsvTargetSums* sums,
                                         int32_t out_width, int32_t out_height, int32_t out_line_length,
                                         uint8_t* previews, int64_t preview_stride, void* stream) {
  const PreviewDst d = {out_width, out_height, out_line_length, previews, preview_stride};
  int32_t rc = check_ov7670_call(h, b, "line");
  if (!rc) rc = check_preview_out(b, d, previews && sums);
  if (rc) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  return locked_preview(h, b, d, [&] {
    return line_preview_core(h, *b, line_alg(val_from, val_to), 5, b->width - 5, 1, sums, d, s);
  });
}

extern "C" int32_t trik_hsv_line_frame_ranges_preview(TRIK_VIDTRANSCODE_CV_Handle h, const TrikHsvFrameBatch* b,
                                                      const uint16_t* ranges, const TrikHsvTargetSums* sums,
                                                      int32_t out_width, int32_t out_height, int32_t out_line_length,
                                                      uint8_t* previews, int64_t preview_stride, void* stream) {
  const PreviewDst d = {out_width, out_height, out_line_length, previews, preview_stride};
  int32_t rc = check_handle_batch(h, b);  // (either layout: it picks the line sensor)
  if (rc) return rc;
  if (b->n_frames > 0 && !ranges) return fail(TRIK_IVIDTRANSCODE_EFAIL, "ranges is NULL");
  if (b->n_frames > 0 && !sums) return fail(TRIK_IVIDTRANSCODE_EFAIL, "sums is NULL");
  rc = check_preview_out(b, d, true);
  if (rc) return rc;
  if (b->n_frames > 0 && preview_bytes(d) > 0 && !previews) return fail(TRIK_IVIDTRANSCODE_EFAIL, "previews is NULL");
  rc = check_device(h, b, sums);
  if (rc) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  return locked_preview(h, b, d, [&] {
    // (the pointer's kind is asked of the runtime; its bytes are read by the kernels alone)
    const std::string e = device_buffer_error(ranges, h->device, "ranges");
    if (!e.empty()) return fail(TRIK_IVIDTRANSCODE_EFAIL, e);
    return line_frame_ranges_preview_core(h, *b, ranges, sums, d, s);
  });
}

extern "C" int32_t trik_hsv_blob_batch(TRIK_VIDTRANSCODE_CV_Handle h, const TrikHsvFrameBatch* b,
                                       const TRIK_VIDTRANSCODE_CV_OV7670_InArgsAlg* hsv, TrikHsvTarget* targets,
                                       int32_t* top, uint8_t* meta, uint16_t* labels, int32_t* n_labels,
                                       void* stream) {
  int32_t r = check_ov7670_call(h, b, "multi-blob");
  if (r) return r;
  if (!hsv) return fail(TRIK_IVIDTRANSCODE_EFAIL, "hsv is NULL");
  if (b->width % 32 || b->height % 4) return fail(TRIK_IVIDTRANSCODE_EFAIL, "width % 32 / height % 4");
  if (b->width > 8192 || blob_max_labels(b->width / 4, b->height / 4) > 30000)
    return fail(TRIK_IVIDTRANSCODE_EFAIL, "frame too large for the multi-blob sensor");
  if (b->n_frames > 0 && !targets) return fail(TRIK_IVIDTRANSCODE_EFAIL, "targets is NULL");
  hipStream_t s = static_cast<hipStream_t>(stream);
  std::lock_guard<std::mutex> lock(h->mu);
  DeviceGuard dg(h->device);
  if (b->n_frames == 0) return 0;
  r = check_device(h, b, targets);
  if (r) return r;
  if (b->width == 0 || b->height == 0) return zero_blob_outputs(targets, top, n_labels, (size_t)b->n_frames, s);
  BlobArgs ba;
  return blob_core(h, *b, blob_range_args(*hsv), targets, top, meta, labels, n_labels, s, ba);
}

extern "C" int32_t trik_hsv_blob_batch_ranges(TRIK_VIDTRANSCODE_CV_Handle h, const TrikHsvFrameBatch* b,
                                              const TRIK_VIDTRANSCODE_CV_InArgsAlg* ranges, int32_t n,
                                              TrikHsvTarget* targets, int32_t* top, uint8_t* meta,
                                              uint16_t* labels, int32_t* n_labels, void* stream) {
  int32_t r = check_handle_batch(h, b);  // (either layout; width % 32, height % 4)
  if (r) return r;
  if (n < 1 || n > TRIK_HSV_MAX_RANGES || !ranges) return fail(TRIK_IVIDTRANSCODE_EFAIL, "n_ranges must be 1..64");
  if (b->width > 8192 || blob_max_labels(b->width / 4, b->height / 4) > 30000)
    return fail(TRIK_IVIDTRANSCODE_EFAIL, "frame too large for the multi-blob sensor");
  if (b->n_frames > 0 && !targets) return fail(TRIK_IVIDTRANSCODE_EFAIL, "targets is NULL");
  hipStream_t s = static_cast<hipStream_t>(stream);
  std::lock_guard<std::mutex> lock(h->mu);
  DeviceGuard dg(h->device);
  if (b->n_frames == 0) return 0;
  r = check_device(h, b, targets);
  if (r) return r;
  if (b->width == 0 || b->height == 0)
    return zero_blob_outputs(targets, top, n_labels, (size_t)b->n_frames * (size_t)n, s);
  return blob_ranges_core(h, *b, ranges, n, targets, top, meta, labels, n_labels, s);
}

extern "C" int32_t trik_hsv_blob_frame_ranges_batch(TRIK_VIDTRANSCODE_CV_Handle h, const TrikHsvFrameBatch* b,
                                                    const uint16_t* ranges, int32_t n, TrikHsvTarget* targets,
                                                    int32_t* top, uint8_t* meta, uint16_t* labels,
                                                    int32_t* n_labels, void* stream) {
  int32_t r = check_handle_batch(h, b);  // (either layout; width % 32, height % 4)
  if (r) return r;
  if (n < 1 || n > TRIK_HSV_MAX_RANGES) return fail(TRIK_IVIDTRANSCODE_EFAIL, "n_ranges must be 1..64");
  if (b->width > 8192 || blob_max_labels(b->width / 4, b->height / 4) > 30000)
    return fail(TRIK_IVIDTRANSCODE_EFAIL, "frame too large for the multi-blob sensor");
  if (b->n_frames > 0 && !targets) return fail(TRIK_IVIDTRANSCODE_EFAIL, "targets is NULL");
  if (b->n_frames > 0 && !ranges) return fail(TRIK_IVIDTRANSCODE_EFAIL, "ranges is NULL");
  if (b->n_frames == 0) return 0;  // (nothing is touched, the handle included)
  hipStream_t s = static_cast<hipStream_t>(stream);
  std::lock_guard<std::mutex> lock(h->mu);
  DeviceGuard dg(h->device);
  r = check_device(h, b, targets);
  if (r) return r;
  const std::string e = device_buffer_error(ranges, h->device, "ranges");  // (its attributes: never its bytes)
  if (!e.empty()) return fail(TRIK_IVIDTRANSCODE_EFAIL, e);
  if (b->width == 0 || b->height == 0)
    return zero_blob_outputs(targets, top, n_labels, (size_t)b->n_frames * (size_t)n, s);
  return blob_frame_ranges_core(h, *b, ranges, n, targets, top, meta, labels, n_labels, s);
}

// BMB:110-130 on the host: the centre/tolerance range in the from/to form
extern "C" int32_t trik_hsv_blob_range_of(const TRIK_VIDTRANSCODE_CV_OV7670_InArgsAlg* hsv,
                                          TRIK_VIDTRANSCODE_CV_InArgsAlg* out) {
  if (!hsv || !out) return fail(TRIK_IVIDTRANSCODE_EFAIL, "blob_range_of: NULL argument");
  *out = blob_range_args(*hsv);
  return 0;
}

extern "C" int32_t trik_hsv_blob_preview(TRIK_VIDTRANSCODE_CV_Handle h, const TrikHsvFrameBatch* b,
                                         const uint8_t* meta, const int32_t* top, int32_t out_width,
                                         int32_t out_height, int32_t out_line_length, uint8_t* previews,
                                         int64_t preview_stride, void* stream) {
  const PreviewDst d = {out_width, out_height, out_line_length, previews, preview_stride};
  int32_t rc = check_ov7670_call(h, b, "multi-blob");
  if (!rc) rc = check_preview_out(b, d, previews && meta && top);
  if (rc) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  return locked_preview(h, b, d, [&] { return blob_preview_core(h, *b, meta, top, d, s); });
}

extern "C" int32_t trik_hsv_mxn_batch(TRIK_VIDTRANSCODE_CV_Handle h, const TrikHsvFrameBatch* b, int32_t rows_m,
                                      int32_t cols_n, int32_t* colors, uint16_t* bins, void* stream) {
  int32_t r = check_ov7670_call(h, b, "MxN");
  if (r) return r;
  const std::string e = mxn_grid_error(rows_m, cols_n);
  if (!e.empty()) return fail(TRIK_IVIDTRANSCODE_EFAIL, e);
  if (b->n_frames > 0 && !colors) return fail(TRIK_IVIDTRANSCODE_EFAIL, "colors is NULL");
  hipStream_t s = static_cast<hipStream_t>(stream);
  std::lock_guard<std::mutex> lock(h->mu);
  DeviceGuard dg(h->device);
  if (b->n_frames == 0) return 0;
  r = check_device(h, b, colors);
  if (r) return r;
  if (b->width == 0 || b->height == 0) {  // every cell is empty: bin (0, 0, 0), colour 0
    const size_t cells = (size_t)b->n_frames * rows_m * cols_n;
    HIP_TRY(hipMemsetAsync(colors, 0, sizeof(int32_t) * cells, s));
    if (bins) HIP_TRY(hipMemsetAsync(bins, 0, sizeof(uint16_t) * cells, s));
    return 0;
  }
  return mxn_core(h, *b, rows_m, cols_n, colors, bins, s);
}

extern "C" int32_t trik_hsv_mxn_preview(TRIK_VIDTRANSCODE_CV_Handle h, const TrikHsvFrameBatch* b, int32_t rows_m,
                                        int32_t cols_n, const int32_t* colors, int32_t out_width,
                                        int32_t out_height, int32_t out_line_length, uint8_t* previews,
                                        int64_t preview_stride, void* stream) {
  int32_t rc = check_ov7670_call(h, b, "MxN");
  if (rc) return rc;
  const std::string e = mxn_grid_error(rows_m, cols_n);
  if (!e.empty()) return fail(TRIK_IVIDTRANSCODE_EFAIL, e);
  const PreviewDst d = {out_width, out_height, out_line_length, previews, preview_stride};
  rc = check_preview_out(b, d, previews && colors);
  if (rc) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  return locked_preview(h, b, d, [&] {
    if (b->width == 0 || b->height == 0) return zero_previews(b, d, s);
    return mxn_preview_core(h, *b, rows_m, cols_n, colors, d, s);
  });
}

extern "C" uint32_t trik_hsv_mxn_color(int32_t h_bin, int32_t s_bin, int32_t v_bin) {
  if (h_bin < 0 || h_bin > 31 || s_bin < 0 || s_bin > 3 || v_bin < 0 || v_bin > 3) {
    fail(TRIK_IVIDTRANSCODE_EFAIL, "mxn_color: bins are h 0..31, s 0..3, v 0..3");
    return 0;
  }
  return mxn_color_table()[(h_bin << 4) | (s_bin << 2) | v_bin];
}

extern "C" int32_t trik_hsv_edge_batch(const TrikHsvFrameBatch* b, int32_t threshold, TrikHsvTargetSums* sums,
                                       TrikHsvTarget* targets, uint8_t* edges, void* stream) {
  int32_t rc = check_batch(b);
  if (!rc) rc = check_ov7670(b, "edge-line");
  if (rc) return rc;
  const std::string e = edge_geometry_error(b->width, b->height, b->line_length);
  if (!e.empty()) return fail(TRIK_IVIDTRANSCODE_EFAIL, e);
  if (threshold < 0 || threshold > 255) return fail(TRIK_IVIDTRANSCODE_EFAIL, "edge_batch: threshold must be 0..255");
  if (b->n_frames > 0 && !sums) return fail(TRIK_IVIDTRANSCODE_EFAIL, "sums is NULL");
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (b->n_frames == 0) return 0;
  HIP_TRY(hipMemsetAsync(sums, 0, sizeof(TrikHsvTargetSums) * (size_t)b->n_frames, s));
  if (b->width == 0 || b->height == 0) {
    if (targets) HIP_TRY(hipMemsetAsync(targets, 0, sizeof(TrikHsvTarget) * (size_t)b->n_frames, s));
    return 0;
  }
  HIP_TRY(launch_edge(edge_args(*b, threshold, sums, targets, edges), s));
  return 0;
}

extern "C" int32_t trik_hsv_edge_preview(TRIK_VIDTRANSCODE_CV_Handle h, const TrikHsvFrameBatch* b,
                                         int32_t threshold, const TrikHsvTargetSums* sums, int32_t out_width,
                                         int32_t out_height, int32_t out_line_length, uint8_t* previews,
                                         int64_t preview_stride, void* stream) {
  int32_t rc = check_ov7670_call(h, b, "edge-line");
  if (rc) return rc;
  const std::string e = edge_geometry_error(b->width, b->height, b->line_length);
  if (!e.empty()) return fail(TRIK_IVIDTRANSCODE_EFAIL, e);
  if (threshold < 0 || threshold > 255)
    return fail(TRIK_IVIDTRANSCODE_EFAIL, "edge_preview: threshold must be 0..255");
  const PreviewDst d = {out_width, out_height, out_line_length, previews, preview_stride};
  rc = check_preview_out(b, d, previews && sums);
  if (rc) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  return locked_preview(h, b, d, [&] {
    if (b->width == 0 || b->height == 0) return zero_previews(b, d, s);
    return edge_preview_core(h, *b, threshold, sums, d, s);
  });
}

// ESEQ:397-417 on the host, as edge_targets_kernel on the device
extern "C" int32_t trik_hsv_edge_targets(const TrikHsvTargetSums* sums, int32_t width, int32_t height,
                                         TrikHsvTarget* target) {
  if (!sums || !target) return fail(TRIK_IVIDTRANSCODE_EFAIL, "edge_targets: NULL argument");
  if (width <= 0 || height <= 0 || width > kEdgeMaxSide || height > kEdgeMaxSide)
    return fail(TRIK_IVIDTRANSCODE_EFAIL, "edge_targets: need 0 < width, height <= 2048");
  TrikHsvTarget t = {0, 0, 0, 0};
  const uint32_t n = (uint32_t)sums->points;
  if (n > 0) {
    const int32_t tx = (int32_t)((uint32_t)(int32_t)sums->sum_x / n);
    const uint32_t radius = (uint32_t)ceilf(sqrtf((float)n / 3.1415927f));
    t.x = (int8_t)(((tx - width / 2) * 100 * 2) / width);
    t.y = (int8_t)(((0 - height / 2) * 100 * 2) / height);
    t.size = (uint8_t)((uint32_t)(radius * 100 * 4) / (uint32_t)(width + height));
  }
  *target = t;
  return 0;
}

extern "C" int32_t trik_hsv_jpeg_batch(TRIK_VIDTRANSCODE_CV_Handle h, const TrikHsvFrameBatch* b, int32_t quality,
                                       int32_t black_and_white, uint8_t* out, int64_t out_stride,
                                       int64_t out_capacity, uint32_t* sizes, int16_t* coeffs, void* stream) {
  int32_t r = check_ov7670_call(h, b, "JPEG");
  if (r) return r;
  const std::string e = jpeg_geometry_error(b->width, b->height);
  if (!e.empty()) return fail(TRIK_IVIDTRANSCODE_EFAIL, e);
  if (out_capacity < 0 || (out && b->n_frames > 1 && out_stride < out_capacity))
    return fail(TRIK_IVIDTRANSCODE_EFAIL, "jpeg_batch: need out_capacity >= 0 and out_stride >= out_capacity");
  if (b->n_frames > 0 && !sizes) return fail(TRIK_IVIDTRANSCODE_EFAIL, "sizes is NULL");
  hipStream_t s = static_cast<hipStream_t>(stream);
  std::lock_guard<std::mutex> lock(h->mu);
  DeviceGuard dg(h->device);
  if (b->n_frames == 0) return 0;
  r = check_device(h, b, sizes);
  if (r) return r;
  std::string de = device_buffer_error(out, h->device, "out");
  if (de.empty()) de = device_buffer_error(coeffs, h->device, "coeffs");
  if (!de.empty()) return fail(TRIK_IVIDTRANSCODE_EFAIL, de);
  if (b->width == 0 || b->height == 0) {  // the reference encodes nothing (JWRAP:67): empty streams
    HIP_TRY(hipMemsetAsync(sizes, 0, sizeof(uint32_t) * (size_t)b->n_frames, s));
    return 0;
  }
  return jpeg_core(h, *b, quality, black_and_white != 0, out, out_stride, out_capacity, sizes, coeffs, s);
}

extern "C" int32_t trik_hsv_jpeg_header(int32_t quality, int32_t black_and_white, int32_t width, int32_t height,
                                        uint8_t* out, int32_t capacity) {
  if (width < 0 || height < 0 || width > 65535 || height > 65535) {
    fail(TRIK_IVIDTRANSCODE_EFAIL, "jpeg_header: need 0 <= width, height <= 65535 (SOF0 holds 16 bits)");
    return 0;
  }
  JpegHeader hd;
  jpeg_header(quality, black_and_white != 0, width, height, hd);
  if (out && capacity >= hd.size) memcpy(out, hd.bytes, (size_t)hd.size);
  return hd.size;
}

extern "C" int32_t trik_hsv_synth(const TrikHsvFrameBatch* b, int32_t first_frame, int32_t kind,
                                  uint64_t seed, void* stream) {
  int32_t rc = check_batch(b);
  if (rc) return rc;
  if (kind != 0 && kind != 1) return fail(TRIK_IVIDTRANSCODE_EFAIL, "kind must be 0 or 1");
  HIP_TRY(launch_synth(*b, const_cast<uint8_t*>(static_cast<const uint8_t*>(b->frames)), first_frame,
                       kind, seed, static_cast<hipStream_t>(stream)));
  return 0;
}
