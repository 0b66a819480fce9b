// trik_hsv_handle.cpp -- the handle of the C ABI of libtrik_hsv.so (declared
// in include/trik_hsv.h): defaults, setup, create/delete/control and the XDAIS
// function tables.
//
// Layer 1 restates the reference's XDAIS codec shell and handle glue:
//   WFXNS trik/webcam/object_sensor/src/vidtranscode_cv_fxns.c
//   WGLUE trik/webcam/object_sensor/src/vidtranscode_cv.cpp
// with per-handle state (the reference keeps its image buffers and LUT
// pointers in process-wide statics, WSEQ:23-26,63-64) and the pixel work on
// the GPU.  Layer 2 (trik_hsv_*) is the batched device API the GPU work sits
// behind.  No C++ exception escapes any entry point.
#include <string.h>

#include <new>

#include "trik_hsv_handle.h"

using namespace trik_hsv;

namespace {
thread_local std::string g_last_error;
}  // namespace

// The last-error slot of the calling thread, for every translation unit
// (trik_hsv_group.cpp reports its workers' errors on the caller's thread).
int32_t trik_hsv::set_error(int32_t code, const std::string& msg) {
  g_last_error = msg;
  return code;
}
const std::string& trik_hsv::last_error() { return g_last_error; }

extern "C" const char* trik_hsv_version(void) { return "trik-hsv-mi355x 0.1.0 (gfx950)"; }

extern "C" const char* trik_hsv_last_error(void) { return g_last_error.c_str(); }

std::string trik_hsv::validate_batch(const TrikHsvFrameBatch* b) {
  if (!b) return "batch is NULL";
  if (b->n_frames < 0) return "n_frames < 0";
  if (b->width < 0 || b->height < 0 || b->width % 32 != 0 || b->height % 4 != 0)
    return "geometry: need width % 32 == 0, height % 4 == 0, both >= 0 (WSEQ:365-369)";
  if (b->width > 32767 || b->height > 32767) return "geometry: width/height exceed int16 (WINT:32)";
  if (b->layout != TRIK_HSV_LAYOUT_YUYV && b->layout != TRIK_HSV_LAYOUT_OV7670) return "unknown layout";
  const int64_t row = b->layout == TRIK_HSV_LAYOUT_YUYV ? 2LL * b->width : (int64_t)b->width;
  if (b->height > 0 && b->line_length < row) return "line_length shorter than a row";
  const int64_t fb = (int64_t)b->height * b->line_length * (b->layout == TRIK_HSV_LAYOUT_OV7670 ? 2 : 1);
  if (b->n_frames > 1 && b->frame_stride < fb) return "frame_stride shorter than a frame";
  if (b->n_frames > 0 && fb > 0 && !b->frames) return "frames is NULL";
  return "";
}

namespace {

const char k_version[] = "1.00.00.00";  // WFXNS:75

// WGLUE:153-184.  The ov7670 glues (object sensor: trik/ov7670/object_sensor/
// src/vidtranscode_cv.cpp:80,157; line sensor :153-184) are the webcam glue
// with formatInput = YUV422P.
TRIK_VIDTRANSCODE_CV_Params default_params(int32_t format_input) {
  return {{(int32_t)sizeof(TRIK_VIDTRANSCODE_CV_Params),
           1,
           format_input,
           {TRIK_VIDTRANSCODE_CV_VIDEO_FORMAT_RGB565X, TRIK_VIDTRANSCODE_CV_VIDEO_FORMAT_UNKNOWN},
           480, 640, 60000, -1,
           {480, -1},
           {640, -1},
           {-1, -1},
           {-1, -1},
           1 /* XDM_BYTE */}};
}

TRIK_VIDTRANSCODE_CV_DynamicParams default_dynamic_params(int algo) {  // WGLUE:205-266
  TRIK_VIDTRANSCODE_CV_DynamicParams d;
  memset(&d, 0, sizeof d);
  d.base.size = (int32_t)sizeof(TRIK_VIDTRANSCODE_CV_DynamicParams);
  d.base.readHeaderOnlyFlag = 0;
  d.base.keepInputResolutionFlag[0] = 0;
  d.base.keepInputResolutionFlag[1] = 1;
  const bool line = algo == kAlgoLine || algo == kAlgoWLine;
  d.base.outputHeight[0] = line ? 320 : 240;  // the line glues (:214,218) swap them
  d.base.outputWidth[0] = line ? 240 : 320;
  d.base.keepInputFrameRateFlag[0] = d.base.keepInputFrameRateFlag[1] = 1;
  d.base.inputFrameRate = -1;
  d.base.outputFrameRate[0] = d.base.outputFrameRate[1] = -1;
  d.base.targetBitRate[0] = d.base.targetBitRate[1] = -1;
  d.base.keepInputGOPFlag[0] = d.base.keepInputGOPFlag[1] = 1;
  d.base.intraFrameInterval[0] = d.base.intraFrameInterval[1] = 1;
  d.base.forceFrame[0] = d.base.forceFrame[1] = -1;  // IVIDEO_NA_FRAME
  d.inputHeight = -1;
  d.inputWidth = -1;
  d.inputLineLength = -1;
  d.outputLineLength[0] = d.outputLineLength[1] = -1;
  return d;
}

// The handle's device resources, freed; the object stays valid (null
// pointers, no streams), so that this may run twice.
void free_resources(TrikCvHandle* h) {
  DeviceGuard dg(h->device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  for (TableSet& t : h->sets) t.release();
  h->maps_users.wait_all();
  h->maps_users.release();
  h->blob_users.wait_all();
  h->blob_users.release();
  h->jpeg_users.wait_all();
  h->jpeg_users.release();
  h->fused_users.wait_all();
  h->fused_users.release();
  h->marks.release();
  (void)hipFree(h->d_wg_part);
  (void)hipFree(h->d_frame_acc);
  (void)hipFree(h->d_tail_sink);
  (void)hipFree(h->d_frame);
  (void)hipFree(h->d_maps);
  (void)hipFree(h->d_preview);
  (void)hipFree(h->d_auto);
  (void)hipFree(h->d_sums);
  (void)hipFree(h->d_targets);
  (void)hipFree(h->d_meta);
  (void)hipFree(h->d_blob_stats);
  (void)hipFree(h->d_blob_top);
  (void)hipFree(h->d_blob_targets);
  (void)hipFree(h->d_mxn_table);
  (void)hipFree(h->d_mxn_colors);
  (void)hipFree(h->d_jpeg_huff);
  (void)hipFree(h->d_jpeg_scratch);
  (void)hipFree(h->d_jpeg_size);
  if (h->stream) (void)hipStreamDestroy(h->stream);
  h->stream = nullptr;
  h->d_frame = nullptr; h->d_frame_cap = 0;
  h->d_maps = nullptr; h->d_maps_cap = 0;
  h->maps_key[0] = -1;
  h->d_preview = nullptr; h->d_preview_cap = 0;
  h->d_auto = nullptr;
  h->d_sums = nullptr;
  h->d_targets = nullptr;
  h->d_meta = nullptr; h->d_meta_cap = 0;
  h->d_blob_stats = nullptr; h->d_blob_stats_cap = 0;
  h->d_blob_top = nullptr; h->d_blob_top_cap = 0;
  h->d_blob_targets = nullptr; h->d_blob_targets_cap = 0;
  h->d_mxn_table = nullptr; h->d_mxn_colors = nullptr;
  h->d_jpeg_huff = nullptr; h->d_jpeg_size = nullptr;
  h->d_jpeg_scratch = nullptr; h->d_jpeg_scratch_cap = 0;
  h->d_wg_part = nullptr; h->d_wg_cnt = nullptr;
  h->d_frame_acc = nullptr; h->frame_acc_cap = 0;
  h->d_tail_sink = nullptr;
  h->sums_set = h->pending_set = nullptr;
  h->alg_ready = false;
}

void release(TrikCvHandle* h) {
  if (!h) return;
  free_resources(h);
  if (h->owns_memory)
    delete h;
  else
    h->~TrikCvHandle();  // the framework releases the record (algFree)
}

// handleSetupImageDesc + createCVAlgorithm + BallDetector::setup
// (WGLUE:52-145, WSEQ:358-410).
int32_t setup_image_desc(TrikCvHandle* h) {
  h->alg_ready = false;
  const TRIK_IVIDTRANSCODE_Params& p = h->params.base;
  if (p.numOutputStreams != 0 && p.numOutputStreams != 1)  // WGLUE:96-101
    return fail(TRIK_IALG_EFAIL, "invalid number of output streams");
  const int in_fmt = p.formatInput;
  const int in_w = h->dyn.inputWidth > 0 ? h->dyn.inputWidth : 0;  // WGLUE:106-109
  const int in_h = h->dyn.inputHeight > 0 ? h->dyn.inputHeight : 0;
  const int in_ll = h->dyn.inputLineLength > 0 ? h->dyn.inputLineLength : 0;
  int out_fmt = TRIK_VIDTRANSCODE_CV_VIDEO_FORMAT_UNKNOWN, out_w = 0, out_h = 0, out_ll = 0;
  if (p.numOutputStreams == 1) {  // WGLUE:111-117
    out_fmt = p.formatOutput[0];
    out_w = h->dyn.base.outputWidth[0] > 0 ? h->dyn.base.outputWidth[0] : 0;
    out_h = h->dyn.base.outputHeight[0] > 0 ? h->dyn.base.outputHeight[0] : 0;
    out_ll = h->dyn.outputLineLength[0] > 0 ? h->dyn.outputLineLength[0] : 0;
  }
  if (in_w > p.maxWidthInput || in_h > p.maxHeightInput ||  // WGLUE:126-135
      (p.numOutputStreams == 1 && (out_w > p.maxWidthOutput[0] || out_h > p.maxHeightOutput[0])))
    return fail(TRIK_IALG_EFAIL, "invalid image dimensions");
  // IF_IN_OUT_FORMAT dispatch (WGLUE:76-84): BallDetector<YUV422, RGB565X>
  // (webcam) and BallDetector<YUV422P, RGB565X> (ov7670 object sensor).  With
  // no output stream the preview format is UNKNOWN; the reference then finds
  // no algorithm, this build accepts it (no preview to write).
  const bool out_ok = out_fmt == TRIK_VIDTRANSCODE_CV_VIDEO_FORMAT_RGB565X ||
                      (p.numOutputStreams == 0 && out_fmt == TRIK_VIDTRANSCODE_CV_VIDEO_FORMAT_UNKNOWN);
  int layout;
  if (h->algo == kAlgoBlob &&
      (in_w > 8192 || blob_max_labels(in_w / 4, in_h / 4) > 30000))  // uint16 labels, LDS
    return fail(TRIK_IALG_EFAIL, "CV algorithm setup failed: frame too large for the multi-blob sensor");
  if ((h->algo == kAlgoBall || h->algo == kAlgoWLine) && in_fmt == TRIK_VIDTRANSCODE_CV_VIDEO_FORMAT_YUV422 &&
      out_ok)
    layout = TRIK_HSV_LAYOUT_YUYV;
  else if (h->algo != kAlgoWLine && in_fmt == TRIK_VIDTRANSCODE_CV_VIDEO_FORMAT_YUV422P &&
           out_ok)  // ov7670 line: YUV422P only; webcam line: YUV422 only
    layout = TRIK_HSV_LAYOUT_OV7670;
  else
    return fail(TRIK_IALG_EFAIL, "cannot create CV algorithm for this format pair");
  if (in_w % 32 != 0 || in_h % 4 != 0 || in_w > 32767 || in_h > 32767)  // WSEQ:365-369
    return fail(TRIK_IALG_EFAIL, "CV algorithm setup failed: width % 32 / height % 4");
  const int row = layout == TRIK_HSV_LAYOUT_YUYV ? 2 * in_w : in_w;
  if (in_h > 0 && in_ll < row)
    return fail(TRIK_IALG_EFAIL, "CV algorithm setup failed: inputLineLength shorter than a row");
  if (h->algo == kAlgoEdge) {  // the reference does not check: its Sobel pass assumes lineLength == width
    const std::string e = edge_geometry_error(in_w, in_h, in_ll);
    if (!e.empty()) return fail(TRIK_IALG_EFAIL, "CV algorithm setup failed: " + e);
  }
  h->layout = layout;
  h->in_w = in_w; h->in_h = in_h; h->in_ll = in_ll;
  h->out_w = out_w; h->out_h = out_h; h->out_ll = out_ll;
  h->line_band[0] = in_h / 2;
  h->line_band[1] = in_h / 2 + 80;
  h->alg_ready = true;
  return TRIK_IALG_EOK;
}

int32_t setup_dynamic(TrikCvHandle* h, const TRIK_VIDTRANSCODE_CV_DynamicParams* d) {
  h->dyn = d ? *d : default_dynamic_params(h->algo);  // WGLUE:271-274
  return setup_image_desc(h);
}

}  // namespace

// ---------------------------------------------------------------------------
// Layer 1: XDAIS-shaped quartet (process: trik_hsv_process.cpp)
// ---------------------------------------------------------------------------
extern "C" TRIK_IVIDTRANSCODE_Fxns TRIK_VIDTRANSCODE_CV_FXNS, TRIK_VIDTRANSCODE_CV_OV7670_FXNS,
    TRIK_VIDTRANSCODE_CV_LINE_FXNS, TRIK_VIDTRANSCODE_CV_WEBCAM_LINE_FXNS, TRIK_VIDTRANSCODE_CV_MXN_FXNS,
    TRIK_VIDTRANSCODE_CV_JPEG_FXNS, TRIK_VIDTRANSCODE_CV_EDGE_LINE_FXNS;

static const TRIK_IALG_Fxns* table_of(int algo) {
  switch (algo) {
    case kAlgoLine: return &TRIK_VIDTRANSCODE_CV_LINE_FXNS.ialg;
    case kAlgoBlob: return &TRIK_VIDTRANSCODE_CV_OV7670_FXNS.ialg;
    case kAlgoWLine: return &TRIK_VIDTRANSCODE_CV_WEBCAM_LINE_FXNS.ialg;
    case kAlgoMxn: return &TRIK_VIDTRANSCODE_CV_MXN_FXNS.ialg;
    case kAlgoJpeg: return &TRIK_VIDTRANSCODE_CV_JPEG_FXNS.ialg;
    case kAlgoEdge: return &TRIK_VIDTRANSCODE_CV_EDGE_LINE_FXNS.ialg;
    default: return &TRIK_VIDTRANSCODE_CV_FXNS.ialg;
  }
}

// A failed init: a handle of TRIK_VIDTRANSCODE_CV_create is deleted; one in
// a framework record keeps a valid object without device resources, because
// the framework calls algFree on it next (TI's ALG_create does), which
// destroys it once.
static void init_failed(TrikCvHandle* h) {
  if (h->owns_memory)
    release(h);
  else
    free_resources(h);
}

// trikCvHandleInit + SetupParams + SetupDynamicParams (WFXNS:146-166) on a
// constructed object; init_failed on failure.
static int32_t init_handle(TrikCvHandle* h, int algo, const TRIK_VIDTRANSCODE_CV_Params* params) {
  if (hipGetDevice(&h->device) != hipSuccess) {
    init_failed(h);
    return fail(TRIK_IALG_EFAIL, "no HIP device");
  }
  h->algo = algo;
  // (the webcam line sensor's glue has the webcam object sensor's Params)
  h->params = params ? *params
                     : default_params(algo == kAlgoLine || algo == kAlgoBlob || algo == kAlgoMxn || algo == kAlgoJpeg ||
                                              algo == kAlgoEdge
                                          ? TRIK_VIDTRANSCODE_CV_VIDEO_FORMAT_YUV422P
                                          : TRIK_VIDTRANSCODE_CV_VIDEO_FORMAT_YUV422);  // WGLUE:188-191
  const int32_t rc = setup_dynamic(h, nullptr);      // WFXNS:158-163
  if (rc != TRIK_IALG_EOK) {
    init_failed(h);
    return rc;
  }
  return TRIK_IALG_EOK;
}

static int32_t create_handle(int algo, const TRIK_VIDTRANSCODE_CV_Params* params,
                             TRIK_VIDTRANSCODE_CV_Handle* out_handle) {
  if (!out_handle) return fail(TRIK_IALG_EFAIL, "out_handle is NULL");
  *out_handle = nullptr;
  TrikCvHandle* h = new (std::nothrow) TrikCvHandle();
  if (!h) return fail(TRIK_IALG_EFAIL, "out of memory");
  h->ialg.fxns = table_of(algo);
  const int32_t rc = init_handle(h, algo, params);
  if (rc == TRIK_IALG_EOK) *out_handle = h;
  return rc;
}

extern "C" int32_t TRIK_VIDTRANSCODE_CV_create(const TRIK_VIDTRANSCODE_CV_Params* params,
                                               TRIK_VIDTRANSCODE_CV_Handle* out_handle) {
  return create_handle(kAlgoBall, params, out_handle);
}

extern "C" int32_t TRIK_VIDTRANSCODE_CV_create_line(const TRIK_VIDTRANSCODE_CV_Params* params,
                                                    TRIK_VIDTRANSCODE_CV_Handle* out_handle) {
  return create_handle(kAlgoLine, params, out_handle);
}

extern "C" int32_t TRIK_VIDTRANSCODE_CV_create_webcam_line(const TRIK_VIDTRANSCODE_CV_Params* params,
                                                           TRIK_VIDTRANSCODE_CV_Handle* out_handle) {
  return create_handle(kAlgoWLine, params, out_handle);
}

extern "C" int32_t TRIK_VIDTRANSCODE_CV_create_ov7670(const TRIK_VIDTRANSCODE_CV_Params* params,
                                                      TRIK_VIDTRANSCODE_CV_Handle* out_handle) {
  return create_handle(kAlgoBlob, params, out_handle);
}

extern "C" int32_t TRIK_VIDTRANSCODE_CV_create_mxn(const TRIK_VIDTRANSCODE_CV_Params* params,
                                                   TRIK_VIDTRANSCODE_CV_Handle* out_handle) {
  return create_handle(kAlgoMxn, params, out_handle);
}

extern "C" int32_t TRIK_VIDTRANSCODE_CV_create_jpeg(const TRIK_VIDTRANSCODE_CV_Params* params,
                                                    TRIK_VIDTRANSCODE_CV_Handle* out_handle) {
  return create_handle(kAlgoJpeg, params, out_handle);
}

extern "C" int32_t TRIK_VIDTRANSCODE_CV_create_edge_line(const TRIK_VIDTRANSCODE_CV_Params* params,
                                                         TRIK_VIDTRANSCODE_CV_Handle* out_handle) {
  return create_handle(kAlgoEdge, params, out_handle);
}

extern "C" int32_t TRIK_VIDTRANSCODE_CV_delete(TRIK_VIDTRANSCODE_CV_Handle handle) {
  if (!handle) return fail(TRIK_IALG_EFAIL, "handle is NULL");
  release(handle);
  return TRIK_IALG_EOK;
}

extern "C" int32_t TRIK_VIDTRANSCODE_CV_control(TRIK_VIDTRANSCODE_CV_Handle h, int32_t cmd,
                                                TRIK_VIDTRANSCODE_CV_DynamicParams* dyn,
                                                TRIK_IVIDTRANSCODE_Status* status) {
  if (!h || !status) return fail(TRIK_IVIDTRANSCODE_EFAIL, "handle or status is NULL");
  std::lock_guard<std::mutex> lock(h->mu);
  int32_t rc = TRIK_IVIDTRANSCODE_EFAIL;
  status->data.accessMask &= ~((1 << TRIK_XDM_ACCESSMODE_READ) | (1 << TRIK_XDM_ACCESSMODE_WRITE));
  switch (cmd) {  // WFXNS:285-331
    case TRIK_XDM_GETSTATUS:
    case TRIK_XDM_GETBUFINFO:
      status->extendedError = 0;
      status->bufInfo.minNumInBufs = 1;
      status->bufInfo.minNumOutBufs = 1;
      status->bufInfo.minInBufSize[0] = 0;
      status->bufInfo.minOutBufSize[0] = 0;
      set_bit(status->data.accessMask, TRIK_XDM_ACCESSMODE_WRITE);
      rc = TRIK_IVIDTRANSCODE_EOK;
      break;
    case TRIK_XDM_SETPARAMS:
      if (dyn && dyn->base.size == (int32_t)sizeof(TRIK_VIDTRANSCODE_CV_DynamicParams))
        rc = setup_dynamic(h, dyn);
      else
        rc = fail(TRIK_IVIDTRANSCODE_EUNSUPPORTED, "SETPARAMS: dynamic params size mismatch");
      break;
    case TRIK_XDM_RESET:
    case TRIK_XDM_SETDEFAULT:
      rc = setup_dynamic(h, nullptr);
      break;
    case TRIK_XDM_FLUSH:
      rc = TRIK_IVIDTRANSCODE_EOK;
      break;
    case TRIK_XDM_GETVERSION:
      if (status->data.buf && status->data.bufSize >= (int32_t)sizeof k_version) {
        memcpy(status->data.buf, k_version, sizeof k_version);
        set_bit(status->data.accessMask, TRIK_XDM_ACCESSMODE_WRITE);
        rc = TRIK_IVIDTRANSCODE_EOK;
      } else {
        rc = fail(TRIK_IVIDTRANSCODE_EFAIL, "GETVERSION: buffer too small");
      }
      break;
    default:
      rc = fail(TRIK_IVIDTRANSCODE_EFAIL, "unsupported control command");
  }
  return rc;
}

// ---------------------------------------------------------------------------
// Layer 1b: the XDAIS IALG functions and function tables (WFXNS:20-166)
// ---------------------------------------------------------------------------
// algAlloc / algFree: one persistent external record for the object (the
// reference's second record, C64x+ on-chip fast RAM, has no use here)
static int32_t object_record(TRIK_IALG_MemRec mem_tab[], void* base) {
  mem_tab[0].size = (uint32_t)sizeof(TrikCvHandle);
  mem_tab[0].alignment = (int32_t)alignof(TrikCvHandle);
  mem_tab[0].space = TRIK_IALG_EXTERNAL;
  mem_tab[0].attrs = TRIK_IALG_PERSIST;
  mem_tab[0].base = base;
  return 1;  // records in use
}

static int32_t ialg_alloc(const TRIK_IALG_Params*, TRIK_IALG_Fxns**, TRIK_IALG_MemRec mem_tab[]) {
  if (!mem_tab) return fail(TRIK_IALG_EFAIL, "algAlloc: mem_tab is NULL");
  return object_record(mem_tab, nullptr);
}

// algInit: the object is constructed in the framework's record; the fxns
// word the framework stored there is kept
static int32_t ialg_init(int algo, TRIK_IALG_Handle alg, const TRIK_IALG_MemRec mem_tab[], const TRIK_IALG_Params* params) {
  if (!alg || !mem_tab || mem_tab[0].base != (void*)alg)
    return fail(TRIK_IALG_EFAIL, "algInit: the handle must be mem_tab[0].base");
  if (mem_tab[0].size < sizeof(TrikCvHandle) || (reinterpret_cast<uintptr_t>(alg) % alignof(TrikCvHandle)))
    return fail(TRIK_IALG_EFAIL, "algInit: mem_tab[0] smaller or less aligned than algAlloc asked");
  if (params && params->size != (int32_t)sizeof(TRIK_VIDTRANSCODE_CV_Params))
    return fail(TRIK_IALG_EFAIL, "algInit: params size mismatch");
  const TRIK_IALG_Fxns* fxns = alg->fxns;
  TrikCvHandle* h = new (alg) TrikCvHandle();
  h->ialg.fxns = fxns ? fxns : table_of(algo);
  h->owns_memory = false;
  return init_handle(h, algo, reinterpret_cast<const TRIK_VIDTRANSCODE_CV_Params*>(params));
}

template <int kAlgo>  // each function table's own algInit
static int32_t ialg_init_as(TRIK_IALG_Handle a, const TRIK_IALG_MemRec* m, TRIK_IALG_Handle, const TRIK_IALG_Params* p) {
  return ialg_init(kAlgo, a, m, p);
}

// algFree: the object is destroyed; its record is returned for the framework
static int32_t ialg_free(TRIK_IALG_Handle alg, TRIK_IALG_MemRec mem_tab[]) {
  if (!alg || !mem_tab) return fail(TRIK_IALG_EFAIL, "algFree: NULL argument");
  TrikCvHandle* h = reinterpret_cast<TrikCvHandle*>(alg);
  if (h->owns_memory) return fail(TRIK_IALG_EFAIL, "algFree: handle made by TRIK_VIDTRANSCODE_CV_create");
  release(h);
  return object_record(mem_tab, alg);
}

static int32_t xdais_process(TRIK_IALG_Handle alg, TRIK_XDM1_BufDesc* in, TRIK_XDM_BufDesc* out,
                             TRIK_IVIDTRANSCODE_InArgs* in_args, TRIK_IVIDTRANSCODE_OutArgs* out_args) {
  return TRIK_VIDTRANSCODE_CV_process(reinterpret_cast<TRIK_VIDTRANSCODE_CV_Handle>(alg), in, out,
                                      reinterpret_cast<TRIK_VIDTRANSCODE_CV_InArgs*>(in_args),
                                      reinterpret_cast<TRIK_VIDTRANSCODE_CV_OutArgs*>(out_args));
}

static int32_t xdais_control(TRIK_IALG_Handle alg, int32_t cmd, TRIK_VIDTRANSCODE_CV_DynamicParams* dyn,
                             TRIK_IVIDTRANSCODE_Status* status) {
  return TRIK_VIDTRANSCODE_CV_control(reinterpret_cast<TRIK_VIDTRANSCODE_CV_Handle>(alg), cmd, dyn, status);
}

// WFXNS:20-29: module ID, activate, alloc, control, deactivate, free, init,
// moved, numAlloc (NULL => IALG_MAXMEMRECS)
#define TRIK_IALGFXNS(self, init) {&self, nullptr, ialg_alloc, nullptr, nullptr, ialg_free, init, nullptr, nullptr}

extern "C" {
TRIK_IVIDTRANSCODE_Fxns TRIK_VIDTRANSCODE_CV_FXNS = {
    TRIK_IALGFXNS(TRIK_VIDTRANSCODE_CV_FXNS, ialg_init_as<kAlgoBall>), xdais_process, xdais_control};
TRIK_IALG_Fxns TRIK_VIDTRANSCODE_CV_IALG = TRIK_IALGFXNS(TRIK_VIDTRANSCODE_CV_FXNS, ialg_init_as<kAlgoBall>);
TRIK_IVIDTRANSCODE_Fxns TRIK_VIDTRANSCODE_CV_OV7670_FXNS = {
    TRIK_IALGFXNS(TRIK_VIDTRANSCODE_CV_OV7670_FXNS, ialg_init_as<kAlgoBlob>), xdais_process, xdais_control};
TRIK_IVIDTRANSCODE_Fxns TRIK_VIDTRANSCODE_CV_LINE_FXNS = {
    TRIK_IALGFXNS(TRIK_VIDTRANSCODE_CV_LINE_FXNS, ialg_init_as<kAlgoLine>), xdais_process, xdais_control};
TRIK_IVIDTRANSCODE_Fxns TRIK_VIDTRANSCODE_CV_WEBCAM_LINE_FXNS = {
    TRIK_IALGFXNS(TRIK_VIDTRANSCODE_CV_WEBCAM_LINE_FXNS, ialg_init_as<kAlgoWLine>), xdais_process, xdais_control};
TRIK_IVIDTRANSCODE_Fxns TRIK_VIDTRANSCODE_CV_MXN_FXNS = {
    TRIK_IALGFXNS(TRIK_VIDTRANSCODE_CV_MXN_FXNS, ialg_init_as<kAlgoMxn>), xdais_process, xdais_control};
TRIK_IVIDTRANSCODE_Fxns TRIK_VIDTRANSCODE_CV_JPEG_FXNS = {
    TRIK_IALGFXNS(TRIK_VIDTRANSCODE_CV_JPEG_FXNS, ialg_init_as<kAlgoJpeg>), xdais_process, xdais_control};
TRIK_IVIDTRANSCODE_Fxns TRIK_VIDTRANSCODE_CV_EDGE_LINE_FXNS = {
    TRIK_IALGFXNS(TRIK_VIDTRANSCODE_CV_EDGE_LINE_FXNS, ialg_init_as<kAlgoEdge>), xdais_process, xdais_control};
}

extern "C" int32_t TRIK_VIDTRANSCODE_CV_alloc(const TRIK_IALG_Params* params, TRIK_IALG_Fxns** parent_fxns,
                                              TRIK_IALG_MemRec mem_tab[]) {
  return ialg_alloc(params, parent_fxns, mem_tab);
}

extern "C" int32_t TRIK_VIDTRANSCODE_CV_initObj(TRIK_IALG_Handle alg, const TRIK_IALG_MemRec mem_tab[],
                                                TRIK_IALG_Handle parent, const TRIK_IALG_Params* params) {
  return ialg_init_as<kAlgoBall>(alg, mem_tab, parent, params);
}

extern "C" int32_t TRIK_VIDTRANSCODE_CV_free(TRIK_IALG_Handle alg, TRIK_IALG_MemRec mem_tab[]) {
  return ialg_free(alg, mem_tab);
}
