// trik_hsv_process.cpp -- Layer 1 TRIK_VIDTRANSCODE_CV_process: the XDAIS
// shell (WFXNS:174-264), the frame's staging on the handle's stream, and one
// function per sensor that enqueues through the sensor's core
// (trik_hsv_sensors.cpp), as the batch API does.
#include <limits.h>
#include <string.h>

#include "trik_hsv_handle.h"

using namespace trik_hsv;

namespace {

// The caller's preview buffer; bytes = 0: no preview stream to write.
struct PreviewOut {
  int8_t* ptr;
  size_t bytes;
};

// Where the sensors' cores write the run's preview: d_preview, in the handle's
// output geometry.
PreviewDst preview_dst(const TrikCvHandle* h, const PreviewOut& pv) {
  return {h->out_w, h->out_h, h->out_ll, h->d_preview, (int64_t)pv.bytes};
}

// The frame staged as a batch of one on the handle's stream (created on first
// use), with d_sums zeroed, d_targets allocated and d_preview large enough.
int32_t stage_frame(TrikCvHandle* h, const void* src, size_t preview_bytes, TrikHsvFrameBatch& b) {
  const size_t fb = (size_t)h->in_h * h->in_ll * (h->layout == TRIK_HSV_LAYOUT_OV7670 ? 2 : 1);
  if (!h->stream) HIP_TRY(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
  int32_t r = grow(h->d_frame, h->d_frame_cap, fb);
  if (!r) r = grow(h->d_preview, h->d_preview_cap, preview_bytes);
  if (r) return r;
  if (!h->d_sums) HIP_TRY(hipMalloc(&h->d_sums, sizeof(TrikHsvTargetSums)));
  if (!h->d_targets) HIP_TRY(hipMalloc(&h->d_targets, sizeof(TrikHsvTarget)));
  HIP_TRY(hipMemcpyAsync(h->d_frame, src, fb, hipMemcpyHostToDevice, h->stream));
  b = {h->d_frame, (int64_t)fb, 1, h->in_w, h->in_h, h->in_ll, h->layout};
  HIP_TRY(hipMemsetAsync(h->d_sums, 0, sizeof(TrikHsvTargetSums), h->stream));
  return 0;
}

// The end of every sensor's run: the preview its core enqueued into d_preview
// copied to the caller, n targets read back, and the stream synchronised.
int32_t read_back(TrikCvHandle* h, const PreviewOut& pv, const TrikHsvTarget* d_targets, TrikHsvTarget* t, int n) {
  if (pv.bytes) HIP_TRY(hipMemcpyAsync(pv.ptr, h->d_preview, pv.bytes, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipMemcpyAsync(t, d_targets, sizeof(TrikHsvTarget) * n, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return 0;
}

void set_target(TRIK_VIDTRANSCODE_CV_OutArgsAlg& oa, const TrikHsvTarget& t) {
  oa.targetX = t.x; oa.targetY = t.y; oa.targetSize = t.size;
}

// BallDetector::run (WSEQ:412-508)
int32_t process_ball(TrikCvHandle* h, const TrikHsvFrameBatch& b, const PreviewOut& pv,
                     const TRIK_VIDTRANSCODE_CV_InArgsAlg& ia, TRIK_VIDTRANSCODE_CV_OutArgsAlg& oa) {
  int32_t r = run_sums(h, &b, &ia, 1, h->d_sums, nullptr, h->stream);
  if (r) return r;
  HIP_TRY(launch_targets(b, 1, h->d_sums, h->d_targets, h->stream));
  uint16_t detect[6] = {0, 0, 0, 0, 0, 0};
  const bool auto_detect = ia.autoDetectHsv != 0;
  if (auto_detect) {  // WSEQ:455-462
    if (!h->d_auto) HIP_TRY(hipMalloc(&h->d_auto, 6 * sizeof(uint16_t)));
    HIP_TRY(launch_auto_range(auto_range_args(b, h->d_auto), h->stream));
    HIP_TRY(hipMemcpyAsync(detect, h->d_auto, sizeof detect, hipMemcpyDeviceToHost, h->stream));
  }
  if (pv.bytes) {  // the preview stream (WSEQ:316-354, 471-494)
    r = preview_core(h, b, ia, h->d_sums, 1, preview_dst(h, pv), h->stream);
    if (r) return r;
  }
  TrikHsvTarget t;
  r = read_back(h, pv, h->d_targets, &t, 1);
  if (r) return r;
  set_target(oa, t);
  if (auto_detect) {  // OutArgs.detect* are written only when autoDetectHsv is set (WSEQ:455-462)
    oa.detectHue = detect[0]; oa.detectHueTolerance = detect[1];
    oa.detectSat = detect[2]; oa.detectSatTolerance = detect[3];
    oa.detectVal = detect[4]; oa.detectValTolerance = detect[5];
  }
  return 0;
}

// The three sensors below ignore autoDetectHsv and leave OutArgs.detect*
// untouched by default: their range detectors are simulated annealings seeded
// by srand(time(NULL)) (the webcam line sensor's cv_hsv_range_detector.hpp:200)
// -- not reproducible.  With trik_hsv_set_auto_detect(handle, 1) a set
// autoDetectHsv is answered by the exact maximum of the detector's own
// objective over its bit-exact score histogram (trik_hsv_autorange.hip,
// DESIGN.md 4.9): deterministic, never worse by the reference's measure.
struct AutoDetect {
  bool on = false;
  uint16_t detect[6] = {0, 0, 0, 0, 0, 0};
};

// Enqueues the exact search of the staged frame and its readback when the
// handle's mode and InArgs ask for it; the caller's read_back synchronises.
int32_t enqueue_auto_detect(TrikCvHandle* h, const TrikHsvFrameBatch& b, int kind, int32_t auto_detect_hsv,
                            AutoDetect& ad) {
  ad.on = auto_detect_hsv != 0 && h->auto_detect.load() == 1;
  if (!ad.on) return 0;
  const std::string e = auto_exact_error(kind, b.layout, b.width, b.height);
  if (!e.empty()) return fail(TRIK_IVIDTRANSCODE_EFAIL, e);
  if (!h->d_auto) HIP_TRY(hipMalloc(&h->d_auto, 6 * sizeof(uint16_t)));
  HIP_TRY(launch_auto_exact(auto_exact_args(b, kind, nullptr, nullptr, h->d_auto, nullptr), h->stream));
  HIP_TRY(hipMemcpyAsync(ad.detect, h->d_auto, sizeof ad.detect, hipMemcpyDeviceToHost, h->stream));
  return 0;
}

template <typename OutArgsAlg>
void set_detect(OutArgsAlg& oa, const AutoDetect& ad) {
  if (!ad.on) return;
  oa.detectHue = ad.detect[0]; oa.detectHueTolerance = ad.detect[1];
  oa.detectSat = ad.detect[2]; oa.detectSatTolerance = ad.detect[3];
  oa.detectVal = ad.detect[4]; oa.detectValTolerance = ad.detect[5];
}

// LineDetector::run, LSEQ:376-476
int32_t process_line(TrikCvHandle* h, const TrikHsvFrameBatch& b, const PreviewOut& pv,
                     const TRIK_VIDTRANSCODE_CV_InArgsAlg& ia, TRIK_VIDTRANSCODE_CV_OutArgsAlg& oa) {
  HIP_TRY(launch_line(line_args(b, ia.detectValFrom, ia.detectValTo, h->line_band[0], h->line_band[1], h->d_sums,
                                h->d_targets), h->stream));
  AutoDetect ad;
  int32_t r = enqueue_auto_detect(h, b, TRIK_HSV_AUTO_OV7670_LINE, ia.autoDetectHsv, ad);
  if (r) return r;
  if (pv.bytes) {  // preview: window columns only, then the overlays
    r = line_preview_core(h, b, line_alg(ia.detectValFrom, ia.detectValTo), 5, h->in_w - 5, 1, h->d_sums,
                          preview_dst(h, pv), h->stream);
    if (r) return r;
  }
  TrikHsvTarget t;
  r = read_back(h, pv, h->d_targets, &t, 1);
  if (r) return r;
  set_target(oa, t);
  set_detect(oa, ad);
  h->line_band[0] = h->in_h / 2;  // LSEQ:449-450, read by the next run
  h->line_band[1] = h->in_h / 2 + 80;
  return 0;
}

// webcam LineDetector::run, LSEQW:330-420
int32_t process_wline(TrikCvHandle* h, const TrikHsvFrameBatch& b, const PreviewOut& pv,
                      const TRIK_VIDTRANSCODE_CV_InArgsAlg& ia, TRIK_VIDTRANSCODE_CV_OutArgsAlg& oa) {
  // hue and saturation fixed to the full bytes, V from InArgs (LSEQW:345-351)
  const TRIK_VIDTRANSCODE_CV_InArgsAlg wr = line_alg(ia.detectValFrom, ia.detectValTo);
  int32_t r = run_sums(h, &b, &wr, 1, h->d_sums, nullptr, h->stream);
  if (r) return r;
  HIP_TRY(launch_wline_targets(1, h->in_w, h->in_h, h->d_sums, h->d_targets, h->stream));
  AutoDetect ad;
  r = enqueue_auto_detect(h, b, TRIK_HSV_AUTO_WEBCAM_LINE, ia.autoDetectHsv, ad);
  if (r) return r;
  if (pv.bytes) {  // every pixel (LSEQW:232-269), then the thin and target lines
    r = line_preview_core(h, b, wr, 0, 0x7FFFFFFF, 0, h->d_sums, preview_dst(h, pv), h->stream);
    if (r) return r;
  }
  TrikHsvTarget t;
  r = read_back(h, pv, h->d_targets, &t, 1);
  if (r) return r;
  set_target(oa, t);
  set_detect(oa, ad);
  return 0;
}

// BallDetector<YUV422P>::run, OSEQ:516-602
int32_t process_blob(TrikCvHandle* h, const TrikHsvFrameBatch& b, const PreviewOut& pv,
                     const TRIK_VIDTRANSCODE_CV_OV7670_InArgsAlg& ia, TRIK_VIDTRANSCODE_CV_OV7670_OutArgsAlg& oa) {
  if (ia.setHsvRange) h->blob_range = blob_range_args(ia);  // BMB:110-130
  BlobArgs ba;
  int32_t r = blob_core(h, b, h->blob_range, nullptr, nullptr, nullptr, nullptr, nullptr, h->stream, ba);
  if (r) return r;
  AutoDetect ad;  // OSEQ:537-544
  r = enqueue_auto_detect(h, b, TRIK_HSV_AUTO_OV7670_OBJECT, ia.autoDetectHsv, ad);
  if (r) return r;
  if (pv.bytes) {  // preview: set metapixels, guide lines, target marks
    r = blob_preview_core(h, b, ba.meta, ba.top, preview_dst(h, pv), h->stream);
    if (r) return r;
  }
  TrikHsvTarget t[8];
  r = read_back(h, pv, ba.targets, t, 8);
  if (r) return r;
  for (int i = 0; i < 8; ++i) {
    oa.target[i].x = t[i].x;
    oa.target[i].y = t[i].y;
    oa.target[i].size = t[i].size;
  }
  set_detect(oa, ad);
  return 0;
}

// BallDetector<YUV422P>::run of the MxN sensor, MSEQ:576-621.  outColor past
// widthM * heightN is left as the caller had it.
int32_t process_mxn(TrikCvHandle* h, const TrikHsvFrameBatch& b, const PreviewOut& pv, int rows_m, int cols_n,
                    TRIK_VIDTRANSCODE_CV_MXN_OutArgsAlg& oa) {
  const int cells = rows_m * cols_n;
  if (!h->d_mxn_colors) HIP_TRY(hipMalloc(&h->d_mxn_colors, sizeof(int32_t) * 100));
  int32_t r = mxn_core(h, b, rows_m, cols_n, h->d_mxn_colors, nullptr, h->stream);
  if (r) return r;
  if (pv.bytes) {  // preview: every pixel, then the cells' squares
    r = mxn_preview_core(h, b, rows_m, cols_n, h->d_mxn_colors, preview_dst(h, pv), h->stream);
    if (r) return r;
  }
  int32_t colors[100];
  if (pv.bytes) HIP_TRY(hipMemcpyAsync(pv.ptr, h->d_preview, pv.bytes, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipMemcpyAsync(colors, h->d_mxn_colors, sizeof(int32_t) * cells, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  memcpy(oa.outColor, colors, sizeof(int32_t) * cells);
  return 0;
}

// BallDetector<YUV422P>::run of the edge-line sensor, ESEQ:365-420: every
// InArgs field is ignored (the threshold is the codec's 50, ESEQ:183), the
// detect* OutArgs are left untouched.
int32_t process_edge(TrikCvHandle* h, const TrikHsvFrameBatch& b, const PreviewOut& pv,
                     TRIK_VIDTRANSCODE_CV_OutArgsAlg& oa) {
  constexpr int kThreshold = 50;
  HIP_TRY(launch_edge(edge_args(b, kThreshold, h->d_sums, h->d_targets, nullptr), h->stream));
  int32_t r = 0;
  if (pv.bytes) {
    r = edge_preview_core(h, b, kThreshold, h->d_sums, preview_dst(h, pv), h->stream);
    if (r) return r;
  }
  TrikHsvTarget t;
  r = read_back(h, pv, h->d_targets, &t, 1);
  if (r) return r;
  set_target(oa, t);
  return 0;
}

// JPGEncoderWrapper::run, JWRAP:52-77: the stream into the caller's output
// buffer (`out`, `cap` bytes; NULL: no output stream, the size alone) and its
// length into OutArgs.  A stream longer than the buffer fails the run with
// nothing of it written (the reference writes on past the buffer).
int32_t process_jpeg(TrikCvHandle* h, const TrikHsvFrameBatch& b, int8_t* out, int64_t cap, int quality, bool bw,
                     TRIK_VIDTRANSCODE_CV_JPEG_OutArgsAlg& oa) {
  if (!h->d_jpeg_size) HIP_TRY(hipMalloc(&h->d_jpeg_size, sizeof(uint32_t)));
  int32_t r = jpeg_core(h, b, quality, bw, out ? h->d_preview : nullptr, cap, cap, h->d_jpeg_size, nullptr,
                        h->stream);
  if (r) return r;
  uint32_t size = 0;
  HIP_TRY(hipMemcpyAsync(&size, h->d_jpeg_size, sizeof size, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  if (out) {
    if ((int64_t)size > cap)
      return fail(TRIK_IVIDTRANSCODE_EFAIL, "the JPEG stream (" + std::to_string(size) +
                                                " bytes) is longer than the output buffer");
    HIP_TRY(hipMemcpyAsync(out, h->d_preview, size, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
  }
  oa.size = size;
  return 0;
}

// The algorithm's run on a checked frame: the targets cleared, then a frame
// of non-zero size staged and taken through the handle's sensor.
int32_t run_sensor(TrikCvHandle* h, const void* frame, const PreviewOut& pv, int64_t out_cap,
                   const TRIK_VIDTRANSCODE_CV_InArgs* in_args, TRIK_VIDTRANSCODE_CV_OutArgs* out_args) {
  TRIK_VIDTRANSCODE_CV_OutArgsAlg& oa = out_args->alg;
  auto* ia7 = reinterpret_cast<const TRIK_VIDTRANSCODE_CV_OV7670_InArgs*>(in_args);
  auto* oa7 = reinterpret_cast<TRIK_VIDTRANSCODE_CV_OV7670_OutArgs*>(out_args);
  if (h->algo == kAlgoMxn) {
    // The grid is checked here, the reference does not (0 divides by zero,
    // more than 100 cells overrun outColor): an invalid one fails the run.
    const auto& im = reinterpret_cast<const TRIK_VIDTRANSCODE_CV_MXN_InArgs*>(in_args)->alg;
    auto& om = reinterpret_cast<TRIK_VIDTRANSCODE_CV_MXN_OutArgs*>(out_args)->alg;
    const std::string e = mxn_grid_error(im.widthM, im.heightN);
    if (!e.empty()) return fail(TRIK_IVIDTRANSCODE_EFAIL, e);
    if (h->in_w <= 0 || h->in_h <= 0) {  // every cell is empty: bin (0, 0, 0)
      for (int k = 0; k < im.widthM * im.heightN; ++k) om.outColor[k] = (int32_t)mxn_color_table()[0];
      return 0;
    }
    DeviceGuard dg(h->device);
    TrikHsvFrameBatch b;
    const int32_t r = stage_frame(h, frame, pv.bytes, b);
    return r ? r : process_mxn(h, b, pv, im.widthM, im.heightN, om);
  }
  if (h->algo == kAlgoJpeg) {
    const auto& ij = reinterpret_cast<const TRIK_VIDTRANSCODE_CV_JPEG_InArgs*>(in_args)->alg;
    auto& oj = reinterpret_cast<TRIK_VIDTRANSCODE_CV_JPEG_OutArgs*>(out_args)->alg;
    if (h->in_w <= 0 || h->in_h <= 0) return 0;  // nothing is encoded, size is left untouched (JWRAP:67)
    // The block walk is checked here, the reference does not (a height that
    // is no multiple of 8 reads past both planes): such a frame fails the run.
    const std::string e = jpeg_geometry_error(h->in_w, h->in_h);
    if (!e.empty()) return fail(TRIK_IVIDTRANSCODE_EFAIL, e);
    DeviceGuard dg(h->device);
    TrikHsvFrameBatch b;
    // (the stream is staged in d_preview: the caller's whole buffer is its capacity)
    const int64_t cap = pv.ptr && out_cap > 0 ? out_cap : 0;
    const int32_t r = stage_frame(h, frame, (size_t)cap, b);
    return r ? r : process_jpeg(h, b, pv.ptr, cap, ij.jpgImageQuality, ij.ifBlackAndWhite != 0, oj);
  }
  if (h->algo == kAlgoBlob)
    memset(oa7->alg.target, 0, sizeof oa7->alg.target);  // OSEQ:563
  else {
    oa.targetX = 0; oa.targetY = 0; oa.targetSize = 0;
  }
  if (h->in_w <= 0 || h->in_h <= 0) return 0;
  DeviceGuard dg(h->device);
  TrikHsvFrameBatch b;
  const int32_t r = stage_frame(h, frame, pv.bytes, b);
  if (r) return r;
  switch (h->algo) {
    case kAlgoBlob: return process_blob(h, b, pv, ia7->alg, oa7->alg);
    case kAlgoLine: return process_line(h, b, pv, in_args->alg, oa);
    case kAlgoWLine: return process_wline(h, b, pv, in_args->alg, oa);
    case kAlgoEdge: return process_edge(h, b, pv, oa);
    default: return process_ball(h, b, pv, in_args->alg, oa);
  }
}

}  // namespace

extern "C" int32_t TRIK_VIDTRANSCODE_CV_process(TRIK_VIDTRANSCODE_CV_Handle h,
                                                TRIK_XDM1_BufDesc* in_bufs,
                                                TRIK_XDM_BufDesc* out_bufs,
                                                TRIK_VIDTRANSCODE_CV_InArgs* in_args,
                                                TRIK_VIDTRANSCODE_CV_OutArgs* out_args) {
  if (!h || !in_bufs || !out_bufs || !in_args || !out_args)
    return fail(TRIK_IVIDTRANSCODE_EFAIL, "NULL argument");
  std::lock_guard<std::mutex> lock(h->mu);
  // the ov7670 object sensor, the MxN sensor and the JPEG encoder have their own InArgs / OutArgs
  const bool blob = h->algo == kAlgoBlob, mxn = h->algo == kAlgoMxn, jpeg = h->algo == kAlgoJpeg;
  const int32_t in_want = blob   ? (int32_t)sizeof(TRIK_VIDTRANSCODE_CV_OV7670_InArgs)
                          : mxn  ? (int32_t)sizeof(TRIK_VIDTRANSCODE_CV_MXN_InArgs)
                          : jpeg ? (int32_t)sizeof(TRIK_VIDTRANSCODE_CV_JPEG_InArgs)
                                 : (int32_t)sizeof(TRIK_VIDTRANSCODE_CV_InArgs);
  const int32_t out_want = blob   ? (int32_t)sizeof(TRIK_VIDTRANSCODE_CV_OV7670_OutArgs)
                           : mxn  ? (int32_t)sizeof(TRIK_VIDTRANSCODE_CV_MXN_OutArgs)
                           : jpeg ? (int32_t)sizeof(TRIK_VIDTRANSCODE_CV_JPEG_OutArgs)
                                  : (int32_t)sizeof(TRIK_VIDTRANSCODE_CV_OutArgs);
  if (in_args->base.size != in_want ||  // WFXNS:192-197
      out_args->base.size != out_want) {
    set_bit(out_args->base.extendedError, TRIK_XDM_UNSUPPORTEDPARAM_BIT);
    return fail(TRIK_IVIDTRANSCODE_EUNSUPPORTED, "InArgs/OutArgs size mismatch");
  }
  if (in_bufs->numBufs != 1 || out_bufs->numBufs < h->params.base.numOutputStreams) {  // :199-204
    set_bit(out_args->base.extendedError, TRIK_XDM_UNSUPPORTEDPARAM_BIT);
    return fail(TRIK_IVIDTRANSCODE_EFAIL, "buffer count");
  }
  TRIK_XDM1_SingleBufDesc* in = &in_bufs->descs[0];
  if (!in->buf || in_args->base.numBytes < 0 || in_args->base.numBytes > in->bufSize) {  // :207-214
    set_bit(out_args->base.extendedError, TRIK_XDM_UNSUPPORTEDPARAM_BIT);
    return fail(TRIK_IVIDTRANSCODE_EFAIL, "input buffer");
  }
  set_bit(in->accessMask, TRIK_XDM_ACCESSMODE_READ);  // :216-221
  out_args->base.bitsConsumed = in_args->base.numBytes * CHAR_BIT;
  out_args->base.decodedPictureType = -1;       // IVIDEO_NA_PICTURE
  out_args->base.decodedPictureStructure = -1;  // IVIDEO_CONTENTTYPE_NA
  out_args->base.decodedHeight = h->dyn.inputHeight;
  out_args->base.decodedWidth = h->dyn.inputWidth;
  const int64_t in_size = in_args->base.numBytes;

  TRIK_XDM1_SingleBufDesc* out = nullptr;
  int8_t* out_ptr = nullptr;
  int64_t out_size = 0;
  if (h->params.base.numOutputStreams == 1) {  // :226-235
    out = &out_args->base.encodedBuf[0];
    out->buf = out_bufs->bufs ? out_bufs->bufs[0] : nullptr;
    out->bufSize = out_bufs->bufSizes ? out_bufs->bufSizes[0] : 0;
    out->accessMask = 0;
    out_ptr = out->buf;
    out_size = out->bufSize;
    if (out_ptr && out_size > 0) memset(out_ptr, 0, (size_t)out_size);
  }

  // trikCvProceedImage + BallDetector::run (WGLUE:291-320, WSEQ:412-508)
  int32_t rc = TRIK_IVIDTRANSCODE_EOK;
  std::string why;
  if (!h->alg_ready) {
    rc = TRIK_IVIDTRANSCODE_EFAIL; why = "CV algorithm not created";
  } else if ((int64_t)h->in_h * h->in_ll > in_size ||
             (h->layout == TRIK_HSV_LAYOUT_OV7670 && 2LL * h->in_h * h->in_ll > in_size)) {
    rc = TRIK_IVIDTRANSCODE_EFAIL; why = "input buffer smaller than the image";  // WSEQ:415-416
  } else if ((int64_t)h->out_h * h->out_ll > out_size) {
    rc = TRIK_IVIDTRANSCODE_EFAIL; why = "output buffer smaller than the preview";  // WSEQ:417-418
  }
  if (rc == TRIK_IVIDTRANSCODE_EOK) {
    const int64_t out_cap = out_size;  // the caller's buffer (the JPEG encoder's capacity)
    out_size = (int64_t)h->out_h * h->out_ll;  // WSEQ:419
    const PreviewOut pv = {out_ptr, out_ptr && out_size > 0 ? (size_t)out_size : 0};
    if (run_sensor(h, in->buf, pv, out_cap, in_args, out_args)) { rc = TRIK_IVIDTRANSCODE_EFAIL; why = last_error(); }
  }
  if (rc != TRIK_IVIDTRANSCODE_EOK) {
    set_bit(out_args->base.extendedError, TRIK_XDM_CORRUPTEDDATA_BIT);  // WFXNS:243-247
    return fail(rc, why);
  }
  if (out) {  // WFXNS:249-259
    out->bufSize = (int32_t)out_size;
    set_bit(out->accessMask, TRIK_XDM_ACCESSMODE_WRITE);
    out_args->base.bitsGenerated[0] = out->bufSize * CHAR_BIT;
    out_args->base.encodedPictureType[0] = out_args->base.decodedPictureType;
    out_args->base.encodedPictureStructure[0] = out_args->base.decodedPictureStructure;
    out_args->base.outputID[0] = in_args->base.inputID;
    out_args->base.inputFrameSkipTranscodeFlag[0] = 0;
  }
  out_args->base.outBufsInUseFlag = 0;
  return TRIK_IVIDTRANSCODE_EOK;
}
