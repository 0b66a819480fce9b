/*
 * trik_hsv.h -- C ABI of the MI355X-native TRIK HSV-threshold + centroid path.
 *
 * Drop-in boundary for the reference's object-sensor codec.  All paths below
 * are relative to the reference checkout (trikset/trik-media-sensors-dsp):
 *   WPUB   trik/webcam/object_sensor/trik_vidtranscode_cv.h
 *   OPUB   trik/ov7670/object_sensor/trik_vidtranscode_cv.h
 *   WFXNS  trik/webcam/object_sensor/src/vidtranscode_cv_fxns.c
 *   WGLUE  trik/webcam/object_sensor/src/vidtranscode_cv.cpp
 *   WINT   trik/webcam/object_sensor/include/internal/vidtranscode_cv.h
 *   WSEQ   trik/webcam/object_sensor/include/internal/cv_ball_detector_seqpass.hpp
 *
 * Two layers:
 *  1. The XDAIS-shaped quartet create / control / process / delete.  It keeps
 *     the reference's struct field order, argument meaning and return codes
 *     (TI's xdas.h / ialg.h / xdm.h / ividtranscode.h are not in this image,
 *     so the base structs are restated here with 32-bit XDAS_Int32 fields;
 *     sizes are this ABI's, documented in INTEGRATION.md).  process() takes a
 *     host frame, like the reference's ARM->DSP call.
 *  2. A batched device API (trik_hsv_*) that the quartet sits on: N frames
 *     resident in HBM, T HSV ranges, per-frame per-range results.  This is
 *     where the HIP kernels run.
 *
 * No torch or HIP types cross this ABI: device buffers and streams are plain
 * pointers (a hipStream_t passed as void*; NULL = the null stream).
 * Errors are return codes; no C++ exception crosses it.
 */
#ifndef TRIK_HSV_H_
#define TRIK_HSV_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------- */
/* Return codes and XDM constants (TI ialg.h / xdm.h values)               */
/* ---------------------------------------------------------------------- */
#define TRIK_IALG_EOK 0                   /* IALG_EOK */
#define TRIK_IALG_EFAIL (-1)              /* IALG_EFAIL */
#define TRIK_IVIDTRANSCODE_EOK 0          /* IVIDTRANSCODE_EOK */
#define TRIK_IVIDTRANSCODE_EFAIL (-1)     /* IVIDTRANSCODE_EFAIL */
#define TRIK_IVIDTRANSCODE_EUNSUPPORTED (-3) /* IVIDTRANSCODE_EUNSUPPORTED */

/* XDM_CmdId (control commands used at WFXNS:285-330) */
#define TRIK_XDM_GETSTATUS 0
#define TRIK_XDM_SETPARAMS 1
#define TRIK_XDM_RESET 2
#define TRIK_XDM_SETDEFAULT 3
#define TRIK_XDM_FLUSH 4
#define TRIK_XDM_GETBUFINFO 5
#define TRIK_XDM_GETVERSION 6

/* extendedError bits set by XDM_SETUNSUPPORTEDPARAM / XDM_SETCORRUPTEDDATA */
#define TRIK_XDM_CORRUPTEDDATA_BIT 11
#define TRIK_XDM_UNSUPPORTEDPARAM_BIT 14
/* accessMask bits (XDM_SETACCESSMODE_READ / _WRITE) */
#define TRIK_XDM_ACCESSMODE_READ 0
#define TRIK_XDM_ACCESSMODE_WRITE 1

#define TRIK_XDM_CUSTOMENUMBASE 0x100     /* XDM_CUSTOMENUMBASE (TI xdm.h) */
#define TRIK_IVIDTRANSCODE_MAXOUTSTREAMS 2
#define TRIK_XDM_MAX_IO_BUFFERS 16

/* TRIK_VIDTRANSCODE_CV_VideoFormat, WPUB:21-29 and OPUB:21-32 */
typedef enum TRIK_VIDTRANSCODE_CV_VideoFormat {
  TRIK_VIDTRANSCODE_CV_VIDEO_FORMAT_UNKNOWN = 0,
  TRIK_VIDTRANSCODE_CV_VIDEO_FORMAT_RGB888 = TRIK_XDM_CUSTOMENUMBASE,
  TRIK_VIDTRANSCODE_CV_VIDEO_FORMAT_RGB565,
  TRIK_VIDTRANSCODE_CV_VIDEO_FORMAT_RGB565X,
  TRIK_VIDTRANSCODE_CV_VIDEO_FORMAT_YUV444,
  TRIK_VIDTRANSCODE_CV_VIDEO_FORMAT_YUV422,  /* packed YUYV (webcam) */
  TRIK_VIDTRANSCODE_CV_VIDEO_FORMAT_YUV422P  /* Y plane + chroma plane (ov7670) */
} TRIK_VIDTRANSCODE_CV_VideoFormat;

/* ---------------------------------------------------------------------- */
/* XDAIS-mirror structs                                                    */
/* ---------------------------------------------------------------------- */

/* IVIDTRANSCODE_Params, field order from the initialiser at WGLUE:153-184. */
typedef struct TRIK_IVIDTRANSCODE_Params {
  int32_t size;
  int32_t numOutputStreams;
  int32_t formatInput;
  int32_t formatOutput[TRIK_IVIDTRANSCODE_MAXOUTSTREAMS];
  int32_t maxHeightInput;
  int32_t maxWidthInput;
  int32_t maxFrameRateInput;
  int32_t maxBitRateInput;
  int32_t maxHeightOutput[TRIK_IVIDTRANSCODE_MAXOUTSTREAMS];
  int32_t maxWidthOutput[TRIK_IVIDTRANSCODE_MAXOUTSTREAMS];
  int32_t maxFrameRateOutput[TRIK_IVIDTRANSCODE_MAXOUTSTREAMS];
  int32_t maxBitRateOutput[TRIK_IVIDTRANSCODE_MAXOUTSTREAMS];
  int32_t dataEndianness;
} TRIK_IVIDTRANSCODE_Params;

/* TRIK_VIDTRANSCODE_CV_Params, WPUB:32-34 */
typedef struct TRIK_VIDTRANSCODE_CV_Params {
  TRIK_IVIDTRANSCODE_Params base;
} TRIK_VIDTRANSCODE_CV_Params;

/* IVIDTRANSCODE_DynamicParams, field order from WGLUE:205-258. */
typedef struct TRIK_IVIDTRANSCODE_DynamicParams {
  int32_t size;
  int32_t readHeaderOnlyFlag;
  int32_t keepInputResolutionFlag[TRIK_IVIDTRANSCODE_MAXOUTSTREAMS];
  int32_t outputHeight[TRIK_IVIDTRANSCODE_MAXOUTSTREAMS];
  int32_t outputWidth[TRIK_IVIDTRANSCODE_MAXOUTSTREAMS];
  int32_t keepInputFrameRateFlag[TRIK_IVIDTRANSCODE_MAXOUTSTREAMS];
  int32_t inputFrameRate;
  int32_t outputFrameRate[TRIK_IVIDTRANSCODE_MAXOUTSTREAMS];
  int32_t targetBitRate[TRIK_IVIDTRANSCODE_MAXOUTSTREAMS];
  int32_t rateControl[TRIK_IVIDTRANSCODE_MAXOUTSTREAMS];
  int32_t keepInputGOPFlag[TRIK_IVIDTRANSCODE_MAXOUTSTREAMS];
  int32_t intraFrameInterval[TRIK_IVIDTRANSCODE_MAXOUTSTREAMS];
  int32_t interFrameInterval[TRIK_IVIDTRANSCODE_MAXOUTSTREAMS];
  int32_t forceFrame[TRIK_IVIDTRANSCODE_MAXOUTSTREAMS];
  int32_t frameSkipTranscodeFlag[TRIK_IVIDTRANSCODE_MAXOUTSTREAMS];
} TRIK_IVIDTRANSCODE_DynamicParams;

/* TRIK_VIDTRANSCODE_CV_DynamicParams, WPUB:37-45 */
typedef struct TRIK_VIDTRANSCODE_CV_DynamicParams {
  TRIK_IVIDTRANSCODE_DynamicParams base;
  int32_t inputHeight;
  int32_t inputWidth;
  int32_t inputLineLength;
  int32_t outputLineLength[TRIK_IVIDTRANSCODE_MAXOUTSTREAMS];
} TRIK_VIDTRANSCODE_CV_DynamicParams;

/* TRIK_VIDTRANSCODE_CV_InArgsAlg, WPUB:48-56 (XDAS_Bool restated as int32) */
typedef struct TRIK_VIDTRANSCODE_CV_InArgsAlg {
  uint16_t detectHueFrom; /* [0..359] */
  uint16_t detectHueTo;   /* [0..359]; From > To wraps through 0 (WSEQ:439-445) */
  uint8_t detectSatFrom;  /* [0..100] */
  uint8_t detectSatTo;
  uint8_t detectValFrom;  /* [0..100] */
  uint8_t detectValTo;
  int32_t autoDetectHsv;  /* fill OutArgsAlg.detect* (WSEQ:455-462); detection unchanged */
} TRIK_VIDTRANSCODE_CV_InArgsAlg;

/* IVIDTRANSCODE_InArgs base fields used at WFXNS:192-224 */
typedef struct TRIK_IVIDTRANSCODE_InArgs {
  int32_t size;
  int32_t numBytes;
  int32_t inputID;
} TRIK_IVIDTRANSCODE_InArgs;

typedef struct TRIK_VIDTRANSCODE_CV_InArgs { /* WPUB:58-61 */
  TRIK_IVIDTRANSCODE_InArgs base;
  TRIK_VIDTRANSCODE_CV_InArgsAlg alg;
} TRIK_VIDTRANSCODE_CV_InArgs;

/* TRIK_VIDTRANSCODE_CV_OutArgsAlg, WPUB:64-74 */
typedef struct TRIK_VIDTRANSCODE_CV_OutArgsAlg {
  int8_t targetX;    /* [-100..100] */
  int8_t targetY;    /* [-100..100] */
  uint8_t targetSize; /* [0..100] */
  uint16_t detectHue;
  uint16_t detectHueTolerance;
  uint16_t detectSat;
  uint16_t detectSatTolerance;
  uint16_t detectVal;
  uint16_t detectValTolerance;
} TRIK_VIDTRANSCODE_CV_OutArgsAlg;

/* The ov7670 object sensor's InArgsAlg (OPUB:51-60): a centre and tolerance
 * per channel, applied when setHsvRange is set and kept until the next set
 * (BitmapBuilder, cv_bitmap_builder_reference.hpp:110-130). */
typedef struct TRIK_VIDTRANSCODE_CV_OV7670_InArgsAlg {
  int32_t setHsvRange;
  uint16_t detectHue;    /* [0..359] */
  uint16_t detectHueTol; /* [0..359] */
  uint8_t detectSat;     /* [0..100] */
  uint8_t detectSatTol;
  uint8_t detectVal;     /* [0..100] */
  uint8_t detectValTol;
  int32_t autoDetectHsv; /* ignored unless trik_hsv_set_auto_detect(handle, 1) */
} TRIK_VIDTRANSCODE_CV_OV7670_InArgsAlg;

typedef struct TRIK_VIDTRANSCODE_CV_OV7670_InArgs { /* OPUB:62-65 */
  TRIK_IVIDTRANSCODE_InArgs base;
  TRIK_VIDTRANSCODE_CV_OV7670_InArgsAlg alg;
} TRIK_VIDTRANSCODE_CV_OV7670_InArgs;

/* XDAS_Target, OPUB:67-71 */
typedef struct TRIK_XDAS_Target {
  int8_t x;     /* [-100..100] */
  int8_t y;     /* [-100..100] */
  uint8_t size; /* [0..100] */
} TRIK_XDAS_Target;

/* The ov7670 object sensor's OutArgsAlg, OPUB:73-81 */
typedef struct TRIK_VIDTRANSCODE_CV_OV7670_OutArgsAlg {
  TRIK_XDAS_Target target[8];
  uint16_t detectHue;
  uint16_t detectHueTolerance;
  uint16_t detectSat;
  uint16_t detectSatTolerance;
  uint16_t detectVal;
  uint16_t detectValTolerance;
} TRIK_VIDTRANSCODE_CV_OV7670_OutArgsAlg;

/* The ov7670 MxN colour-grid sensor's InArgsAlg and OutArgsAlg (MPUB =
 * trik/ov7670/mxn_sensor/trik_vidtranscode_cv.h:49-67), field names as the
 * reference's.  The names are crossed there (its run() assigns widthM to the
 * grid's height and heightN to its width): widthM is the number of cell ROWS
 * (a cell is inputHeight / widthM rows high), heightN the number of cell
 * COLUMNS (inputWidth / heightN columns wide).  outColor[i * heightN + j] is
 * the 0x00RRGGBB colour of the cell in row i, column j. */
typedef struct TRIK_VIDTRANSCODE_CV_MXN_InArgsAlg {
  int32_t widthM;  /* cell rows */
  int32_t heightN; /* cell columns */
} TRIK_VIDTRANSCODE_CV_MXN_InArgsAlg;

typedef struct TRIK_VIDTRANSCODE_CV_MXN_OutArgsAlg {
  int32_t outColor[100];
} TRIK_VIDTRANSCODE_CV_MXN_OutArgsAlg;

/* The ov7670 JPEG encoder's InArgsAlg and OutArgsAlg (JPUB = trik/ov7670/
 * jpeg_encoder/trik_vidtranscode_cv.h:49-67), field names as the reference's.
 * XDAS_Bool is a 32-bit int.  jpgImageQuality is clamped to 1..100 by the
 * encoder (0 encodes as 1, 101..255 as 100); size is the stream's length in
 * bytes. */
typedef struct TRIK_VIDTRANSCODE_CV_JPEG_InArgsAlg {
  uint8_t jpgImageQuality;
  int32_t ifBlackAndWhite; /* non-zero: the luma plane alone, one component */
} TRIK_VIDTRANSCODE_CV_JPEG_InArgsAlg;

typedef struct TRIK_VIDTRANSCODE_CV_JPEG_OutArgsAlg {
  uint32_t size;
} TRIK_VIDTRANSCODE_CV_JPEG_OutArgsAlg;

/* XDM1_SingleBufDesc */
typedef struct TRIK_XDM1_SingleBufDesc {
  int8_t* buf;
  int32_t bufSize;
  int32_t accessMask;
} TRIK_XDM1_SingleBufDesc;

/* XDM1_BufDesc (process input, WFXNS:199-214) */
typedef struct TRIK_XDM1_BufDesc {
  int32_t numBufs;
  TRIK_XDM1_SingleBufDesc descs[TRIK_XDM_MAX_IO_BUFFERS];
} TRIK_XDM1_BufDesc;

/* XDM_BufDesc (process output, WFXNS:200,228-230) */
typedef struct TRIK_XDM_BufDesc {
  int8_t** bufs;
  int32_t numBufs;
  int32_t* bufSizes;
} TRIK_XDM_BufDesc;

/* IVIDTRANSCODE_OutArgs base fields written at WFXNS:195-261 */
typedef struct TRIK_IVIDTRANSCODE_OutArgs {
  int32_t size;
  int32_t extendedError;
  int32_t bitsConsumed;
  int32_t decodedPictureType;
  int32_t decodedPictureStructure;
  int32_t decodedHeight;
  int32_t decodedWidth;
  TRIK_XDM1_SingleBufDesc encodedBuf[TRIK_IVIDTRANSCODE_MAXOUTSTREAMS];
  int32_t bitsGenerated[TRIK_IVIDTRANSCODE_MAXOUTSTREAMS];
  int32_t encodedPictureType[TRIK_IVIDTRANSCODE_MAXOUTSTREAMS];
  int32_t encodedPictureStructure[TRIK_IVIDTRANSCODE_MAXOUTSTREAMS];
  int32_t outputID[TRIK_IVIDTRANSCODE_MAXOUTSTREAMS];
  int32_t inputFrameSkipTranscodeFlag[TRIK_IVIDTRANSCODE_MAXOUTSTREAMS];
  int32_t outBufsInUseFlag;
} TRIK_IVIDTRANSCODE_OutArgs;

typedef struct TRIK_VIDTRANSCODE_CV_OutArgs { /* WPUB:76-79 */
  TRIK_IVIDTRANSCODE_OutArgs base;
  TRIK_VIDTRANSCODE_CV_OutArgsAlg alg;
} TRIK_VIDTRANSCODE_CV_OutArgs;

typedef struct TRIK_VIDTRANSCODE_CV_OV7670_OutArgs { /* OPUB:83-86 */
  TRIK_IVIDTRANSCODE_OutArgs base;
  TRIK_VIDTRANSCODE_CV_OV7670_OutArgsAlg alg;
} TRIK_VIDTRANSCODE_CV_OV7670_OutArgs;

typedef struct TRIK_VIDTRANSCODE_CV_MXN_InArgs { /* MPUB:54-57 */
  TRIK_IVIDTRANSCODE_InArgs base;
  TRIK_VIDTRANSCODE_CV_MXN_InArgsAlg alg;
} TRIK_VIDTRANSCODE_CV_MXN_InArgs;

typedef struct TRIK_VIDTRANSCODE_CV_MXN_OutArgs { /* MPUB:64-67 */
  TRIK_IVIDTRANSCODE_OutArgs base;
  TRIK_VIDTRANSCODE_CV_MXN_OutArgsAlg alg;
} TRIK_VIDTRANSCODE_CV_MXN_OutArgs;

typedef struct TRIK_VIDTRANSCODE_CV_JPEG_InArgs { /* JPUB:54-57 */
  TRIK_IVIDTRANSCODE_InArgs base;
  TRIK_VIDTRANSCODE_CV_JPEG_InArgsAlg alg;
} TRIK_VIDTRANSCODE_CV_JPEG_InArgs;

typedef struct TRIK_VIDTRANSCODE_CV_JPEG_OutArgs { /* JPUB:64-67 */
  TRIK_IVIDTRANSCODE_OutArgs base;
  TRIK_VIDTRANSCODE_CV_JPEG_OutArgsAlg alg;
} TRIK_VIDTRANSCODE_CV_JPEG_OutArgs;

/* XDM1_AlgBufInfo subset filled by GETSTATUS/GETBUFINFO (WFXNS:287-297) */
typedef struct TRIK_XDM1_AlgBufInfo {
  int32_t minNumInBufs;
  int32_t minNumOutBufs;
  int32_t minInBufSize[TRIK_XDM_MAX_IO_BUFFERS];
  int32_t minOutBufSize[TRIK_XDM_MAX_IO_BUFFERS];
} TRIK_XDM1_AlgBufInfo;

/* IVIDTRANSCODE_Status */
typedef struct TRIK_IVIDTRANSCODE_Status {
  int32_t size;
  int32_t extendedError;
  TRIK_XDM1_SingleBufDesc data;
  TRIK_XDM1_AlgBufInfo bufInfo;
} TRIK_IVIDTRANSCODE_Status;

typedef struct TrikCvHandle* TRIK_VIDTRANSCODE_CV_Handle;

/* ---------------------------------------------------------------------- */
/* Layer 1: XDAIS-shaped quartet                                           */
/* ---------------------------------------------------------------------- */

/* Replaces TRIK_VIDTRANSCODE_CV_alloc + _initObj (WFXNS:85-102, 146-166) as
 * driven by Codec Engine's VIDTRANSCODE_create.  params == NULL takes the
 * defaults of WGLUE:153-184 (YUV422 in, RGB565X out, 640x480 max; the cap is
 * a parameter, not a static buffer size, here).  The handle binds to the
 * calling thread's current HIP device.  Returns IALG_EOK / IALG_EFAIL. */
int32_t TRIK_VIDTRANSCODE_CV_create(const TRIK_VIDTRANSCODE_CV_Params* params,
                                    TRIK_VIDTRANSCODE_CV_Handle* out_handle);

/* The same quartet for the ov7670 line sensor's codec (its own DSP server in
 * the reference: trik/ov7670/line_sensor, LineDetector<YUV422P, RGB565X> of
 * include/internal/cv_line_detector_seqpass.hpp -- LSEQ below).  params ==
 * NULL takes that glue's defaults (YUV422P in, RGB565X out; default dynamic
 * output 240 wide x 320 high as its src/vidtranscode_cv.cpp:214,218).
 * control/process/delete are the functions below; process() then runs
 * LineDetector::run (LSEQ:376-476): V-range detection in columns 5..W-5,
 * cross points over rows H/2..H/2+80, its preview overlays; OutArgs.targetY
 * is the cross size.  autoDetectHsv is ignored (the line sensor's detector is
 * seeded by srand(time(NULL))) unless trik_hsv_set_auto_detect asks for the
 * exact search. */
int32_t TRIK_VIDTRANSCODE_CV_create_line(const TRIK_VIDTRANSCODE_CV_Params* params,
                                         TRIK_VIDTRANSCODE_CV_Handle* out_handle);

/* The quartet for the webcam line sensor's codec (trik/webcam/line_sensor,
 * LineDetector<YUV422, RGB565X> of include/internal/
 * cv_line_detector_seqpass.hpp -- LSEQW).  params == NULL takes the webcam
 * glue's defaults (YUV422 = packed YUYV in, RGB565X out; default dynamic
 * output 240 wide x 320 high).  process() runs LineDetector::run (LSEQW:
 * 330-420): the range (H 0..359, S 0..100, V detectValFrom..detectValTo)
 * over every pixel; when more than 10 pixels match, targetX = ((x - W/2) *
 * 200) / W of the mean column, targetY = 0, targetSize = N * 100 / (W * H);
 * the preview is every pixel (matches white) with magenta lines at columns
 * W/2 +- 40 and +- 80 and a red 3-column line at the mean column.
 * autoDetectHsv is ignored (its detector is seeded by srand(time(NULL)))
 * unless trik_hsv_set_auto_detect asks for the exact search. */
int32_t TRIK_VIDTRANSCODE_CV_create_webcam_line(const TRIK_VIDTRANSCODE_CV_Params* params,
                                                TRIK_VIDTRANSCODE_CV_Handle* out_handle);

/* The quartet for the ov7670 object sensor's codec (trik/ov7670/object_sensor:
 * BallDetector<YUV422P, RGB565X> of include/internal/
 * cv_ball_detector_seqpass.hpp:516-602 -- OSEQ -- with its BitmapBuilder and
 * Clusterizer).  params == NULL takes that glue's defaults (YUV422P in,
 * RGB565X out).  process() then takes TRIK_VIDTRANSCODE_CV_OV7670_InArgs and
 * TRIK_VIDTRANSCODE_CV_OV7670_OutArgs (size fields checked): the sticky HSV
 * range, the 4x4 metapixel bitmap, the clusterer and up to 8 targets by
 * size, and the preview (set metapixels as 0x00ffff, guide lines, a 3x3 red
 * mark per target).  Frames up to 2048x2048 (the reference: 640x480). */
int32_t TRIK_VIDTRANSCODE_CV_create_ov7670(const TRIK_VIDTRANSCODE_CV_Params* params,
                                           TRIK_VIDTRANSCODE_CV_Handle* out_handle);

/* The quartet for the ov7670 MxN colour-grid sensor's codec (trik/ov7670/
 * mxn_sensor: BallDetector<YUV422P, RGB565X> of include/internal/
 * cv_ball_detector_seqpass.hpp -- MSEQ -- behind the ov7670 object sensor's
 * glue).  params == NULL takes that glue's defaults (YUV422P in, RGB565X
 * out).  process() then takes TRIK_VIDTRANSCODE_CV_MXN_InArgs and
 * TRIK_VIDTRANSCODE_CV_MXN_OutArgs (size fields checked).  The frame is split
 * into widthM rows x heightN columns of cells (steps are truncating
 * divisions; pixels right of or below the last cell belong to no cell); each
 * cell's pixels are counted in a 32 x 4 x 4 histogram of (H >> 3, S >> 6,
 * V >> 6), the bin that first reaches the largest count in the cell's raster
 * order wins, and outColor[k] is that bin's colour (trik_hsv_mxn_color).
 * outColor past widthM * heightN is left untouched.  The preview is every
 * source pixel through the scale maps, then a 20 x 20 square of each cell's
 * colour at the cell's top-left corner, in cell order (MSEQ:328-366, 609-618).
 * The one divergence: the reference does not check the grid (0 divides by
 * zero, more than 100 cells overrun outColor, widthM is cut to 8 bits); here
 * widthM < 1, heightN < 1 or widthM * heightN > 100 makes process() return
 * IVIDTRANSCODE_EFAIL with nothing written to outColor. */
int32_t TRIK_VIDTRANSCODE_CV_create_mxn(const TRIK_VIDTRANSCODE_CV_Params* params,
                                        TRIK_VIDTRANSCODE_CV_Handle* out_handle);

/* The quartet for the ov7670 JPEG encoder's codec (trik/ov7670/jpeg_encoder:
 * JPGEncoderWrapper<YUV422P, RGB565X> of include/internal/
 * cv_jpeg_encoder_wrapper_seqpass.hpp -- JWRAP -- over JPGEncoder of
 * jpeg_encoder_reference.hpp -- JENC -- behind the ov7670 object sensor's
 * glue).  params == NULL takes that glue's defaults (YUV422P in, "RGB565X"
 * out).  process() then takes TRIK_VIDTRANSCODE_CV_JPEG_InArgs and
 * TRIK_VIDTRANSCODE_CV_JPEG_OutArgs (size fields checked).  The output
 * buffer, declared RGB565X, receives a baseline JFIF stream: SOI, APP0, DQT,
 * SOF0, DHT, SOS (607 bytes in colour, 324 in black and white), the
 * entropy-coded 8x8 blocks in raster order (Y, U, V per block; colour is
 * declared 4:4:4 with each chroma sample repeated for two pixels), fill bits
 * and EOI -- the reference's bytes, its truncating fp64 AAN transform, its
 * 8 fill bits on an aligned end and its unwritten undefined Huffman symbols
 * included.  OutArgs.alg.size is the stream's length.  process() keeps the
 * wrapper's two buffer checks (the input holds the image, the output buffer
 * holds outputHeight * outputLineLength bytes: JWRAP:55-58).  Without an
 * output stream the size alone is reported; with a zero width or height
 * nothing is encoded and size is left untouched (JWRAP:67).  The divergences:
 *  - a height that is no multiple of 8: the reference's block walk reads the
 *    chroma plane as luma and past the buffer as chroma; here process()
 *    returns IVIDTRANSCODE_EFAIL with nothing written;
 *  - a stream longer than the output buffer: the reference writes on past
 *    it; here process() returns IVIDTRANSCODE_EFAIL with none of the stream
 *    written (the buffer keeps the shell's zero fill);
 *  - a width or height above 65535 is rejected (SOF0 holds 16 bits; setup
 *    already rejects sides above 32767);
 *  - both planes are checked against the input buffer, as for every ov7670
 *    codec here. */
int32_t TRIK_VIDTRANSCODE_CV_create_jpeg(const TRIK_VIDTRANSCODE_CV_Params* params,
                                         TRIK_VIDTRANSCODE_CV_Handle* out_handle);

/* The quartet for the ov7670 edge-line sensor's codec (trik/ov7670/
 * edge_line_sensor: BallDetector<YUV422P, RGB565X> of include/internal/
 * cv_ball_detector_seqpass.hpp -- ESEQ -- behind the ov7670 object sensor's
 * glue; its Harris block is not compiled).  params == NULL takes that glue's
 * defaults (YUV422P in, RGB565X out, a 320x240 output).  process() takes the
 * webcam object sensor's InArgs and OutArgs; every InArgs field is ignored and
 * the detect* OutArgs are left untouched.  The Y plane goes through
 * IMG_sobel_3x3_8 and IMG_thr_gt2max_8 (threshold 50), restated from TI's
 * documented natural-C semantics over the plane as one linear array of
 * width * height bytes: byte i + 1 of the map is min(|H| + |V|, 255) of the
 * 3x3 window whose first byte is i, for i in 0 .. width * (height - 2) - 3,
 * then 255 where that exceeds the threshold.  So map (r, c) is the window
 * with top-left (r, c - 1), columns 0 and width - 1 mix adjacent rows, and
 * byte 0, byte width * (height - 2) - 1 and the last two rows are never
 * written.  A pixel is detected iff its map byte is 255; per row, the count
 * and the column sum over columns 16 .. width - 16 are uint16_t (they wrap
 * mod 65536, the column sum from width 384) and are added to the frame's
 * totals (ESEQ:189-205).  OutArgs (ESEQ:397-417, all 0 without a detected
 * pixel): targetX from the mean column, targetY the frame's top (-100: the
 * row sum stays 0), targetSize from ceil(sqrtf(points / pi)).  The preview
 * (ESEQ:226-249, 405): IMG_ycbcr422pl_to_rgb565 of the map as luma with the
 * frame's chroma (cb = chroma byte 2k, cr = byte 2k + 1 of pixel pair k),
 * stored as native uint16 RGB565 -- not the byte order of the other codecs'
 * previews --, every source pixel through the scale maps, then a line of
 * value 0x001f at the mean column over rows height / 2 +- 99 (clamped).
 * process() keeps this library's two-plane input check and its output-size
 * check.  The divergences:
 *  - inputLineLength != inputWidth is rejected by SETPARAMS (the reference
 *    takes it and reads the padded plane as if it were dense);
 *  - the never-written map bytes are always 0, the state of a fresh instance
 *    (the reference keeps the map in a static, so an instance resized
 *    downward sees stale bytes of earlier, larger frames);
 *  - frames up to 2048 x 2048 are taken (the reference's statics hold
 *    320 x 240 and larger frames overrun them);
 *  - the chroma split's read of a further width * height bytes past the
 *    frame (ESEQ:169) is not made. */
int32_t TRIK_VIDTRANSCODE_CV_create_edge_line(const TRIK_VIDTRANSCODE_CV_Params* params,
                                              TRIK_VIDTRANSCODE_CV_Handle* out_handle);

/* Replaces TRIK_VIDTRANSCODE_CV_free (WFXNS:114-136). */
int32_t TRIK_VIDTRANSCODE_CV_delete(TRIK_VIDTRANSCODE_CV_Handle handle);

/* Replaces TRIK_VIDTRANSCODE_CV_process (WFXNS:174-264).  One host frame in
 * (in_bufs->descs[0]), targetX/Y/Size out in out_args->alg (and detect* when
 * autoDetectHsv is set).  With numOutputStreams == 1 the RGB565X preview is
 * rendered into out_bufs->bufs[0] (see trik_hsv_batch_preview);
 * numOutputStreams == 0 is accepted and writes nothing.  Returns IVIDTRANSCODE_EOK / _EFAIL /
 * _EUNSUPPORTED with the reference's extendedError bits. */
int32_t TRIK_VIDTRANSCODE_CV_process(TRIK_VIDTRANSCODE_CV_Handle handle,
                                     TRIK_XDM1_BufDesc* in_bufs, TRIK_XDM_BufDesc* out_bufs,
                                     TRIK_VIDTRANSCODE_CV_InArgs* in_args,
                                     TRIK_VIDTRANSCODE_CV_OutArgs* out_args);

/* Replaces TRIK_VIDTRANSCODE_CV_control (WFXNS:272-334): GETSTATUS,
 * GETBUFINFO, SETPARAMS (re-runs setup, WGLUE:202-286), RESET/SETDEFAULT,
 * FLUSH, GETVERSION ("1.00.00.00"). */
int32_t TRIK_VIDTRANSCODE_CV_control(TRIK_VIDTRANSCODE_CV_Handle handle, int32_t cmd,
                                     TRIK_VIDTRANSCODE_CV_DynamicParams* dyn_params,
                                     TRIK_IVIDTRANSCODE_Status* status);

/* ---------------------------------------------------------------------- */
/* Layer 1b: the XDAIS function tables (WFXNS:20-66, 85-166)               */
/* ---------------------------------------------------------------------- */
/* What a Codec-Engine-style framework binds: IALG_Fxns + IVIDTRANSCODE_Fxns,
 * restated from TI XDAIS ialg.h / ividtranscode.h (absent here; Int/Uns are
 * 32-bit on the C64x+, so int32_t/uint32_t).  The framework calls algAlloc
 * for the memory records, allocates them, stores the table in the object's
 * first word (IALG_Obj.fxns), calls algInit, then process/control through
 * the table, then algFree and releases the records.  The object IS a
 * TRIK_VIDTRANSCODE_CV_Handle: the table's process/control are the quartet's
 * process/control, and TRIK_VIDTRANSCODE_CV_create/_delete are the same
 * alloc + init / free with the library owning the memory. */
typedef enum TRIK_IALG_MemAttrs { TRIK_IALG_SCRATCH = 0, TRIK_IALG_PERSIST = 1, TRIK_IALG_WRITEONCE = 2 } TRIK_IALG_MemAttrs;
#define TRIK_IALG_MXTRN 0x0010 /* ialg.h: external memory space bit */
#define TRIK_IALG_DARAM0 0
#define TRIK_IALG_EXTERNAL (TRIK_IALG_MXTRN + 1)

typedef struct TRIK_IALG_MemRec {
  uint32_t size;      /* Uns */
  int32_t alignment;  /* Int: 0 = any */
  int32_t space;      /* IALG_MemSpace */
  int32_t attrs;      /* IALG_MemAttrs */
  void* base;
} TRIK_IALG_MemRec;

struct TRIK_IALG_Fxns;
typedef struct TRIK_IALG_Obj {
  const struct TRIK_IALG_Fxns* fxns;
} TRIK_IALG_Obj;
typedef TRIK_IALG_Obj* TRIK_IALG_Handle;

/* IALG_Params: the codec's TRIK_VIDTRANSCODE_CV_Params (its first field is the size). */
typedef struct TRIK_IALG_Params {
  int32_t size;
} TRIK_IALG_Params;

typedef struct TRIK_IALG_Fxns {
  const void* implementationId;
  void (*algActivate)(TRIK_IALG_Handle);
  int32_t (*algAlloc)(const TRIK_IALG_Params*, struct TRIK_IALG_Fxns**, TRIK_IALG_MemRec*);
  int32_t (*algControl)(TRIK_IALG_Handle, int32_t, void*);
  void (*algDeactivate)(TRIK_IALG_Handle);
  int32_t (*algFree)(TRIK_IALG_Handle, TRIK_IALG_MemRec*);
  int32_t (*algInit)(TRIK_IALG_Handle, const TRIK_IALG_MemRec*, TRIK_IALG_Handle, const TRIK_IALG_Params*);
  void (*algMoved)(TRIK_IALG_Handle, const TRIK_IALG_MemRec*, TRIK_IALG_Handle, const TRIK_IALG_Params*);
  int32_t (*algNumAlloc)(void);
} TRIK_IALG_Fxns;

/* IVIDTRANSCODE_Fxns.  in_args / out_args: the codec's InArgs / OutArgs
 * (size fields checked), as IVIDTRANSCODE_InArgs* / _OutArgs* in TI's. */
typedef struct TRIK_IVIDTRANSCODE_Fxns {
  TRIK_IALG_Fxns ialg;
  int32_t (*process)(TRIK_IALG_Handle, TRIK_XDM1_BufDesc*, TRIK_XDM_BufDesc*, TRIK_IVIDTRANSCODE_InArgs*,
                     TRIK_IVIDTRANSCODE_OutArgs*);
  int32_t (*control)(TRIK_IALG_Handle, int32_t, TRIK_VIDTRANSCODE_CV_DynamicParams*, TRIK_IVIDTRANSCODE_Status*);
} TRIK_IVIDTRANSCODE_Fxns;

/* The webcam object sensor's tables (WFXNS:36-66); IALG is the same table
 * as FXNS.ialg (the reference aliases the two symbols on TI toolchains and
 * duplicates them elsewhere, as here).  The other six codecs of this library
 * (one DSP server each in the reference, all named TRIK_VIDTRANSCODE_CV_FXNS
 * there): the ov7670 object sensor, the ov7670 line sensor, the webcam line
 * sensor, the ov7670 MxN sensor, the ov7670 JPEG encoder and the ov7670
 * edge-line sensor. */
extern TRIK_IVIDTRANSCODE_Fxns TRIK_VIDTRANSCODE_CV_FXNS;
extern TRIK_IALG_Fxns TRIK_VIDTRANSCODE_CV_IALG;
extern TRIK_IVIDTRANSCODE_Fxns TRIK_VIDTRANSCODE_CV_OV7670_FXNS;
extern TRIK_IVIDTRANSCODE_Fxns TRIK_VIDTRANSCODE_CV_LINE_FXNS;
extern TRIK_IVIDTRANSCODE_Fxns TRIK_VIDTRANSCODE_CV_WEBCAM_LINE_FXNS;
extern TRIK_IVIDTRANSCODE_Fxns TRIK_VIDTRANSCODE_CV_MXN_FXNS;
extern TRIK_IVIDTRANSCODE_Fxns TRIK_VIDTRANSCODE_CV_JPEG_FXNS;
extern TRIK_IVIDTRANSCODE_Fxns TRIK_VIDTRANSCODE_CV_EDGE_LINE_FXNS;

/* The webcam object sensor's IALG functions (WFXNS:85-166), also reachable
 * through the tables.  alloc asks for one persistent external record (the
 * object; the reference's second record is C64x+ on-chip fast RAM, which
 * has no use here) and returns the record count; initObj constructs the
 * object in that record (keeping the framework's fxns word) and runs the
 * setup of WFXNS:146-166; free destroys it and returns the record for the
 * framework to release. */
int32_t TRIK_VIDTRANSCODE_CV_alloc(const TRIK_IALG_Params* params, TRIK_IALG_Fxns** parent_fxns,
                                   TRIK_IALG_MemRec mem_tab[]);
int32_t TRIK_VIDTRANSCODE_CV_initObj(TRIK_IALG_Handle handle, const TRIK_IALG_MemRec mem_tab[],
                                     TRIK_IALG_Handle parent, const TRIK_IALG_Params* params);
int32_t TRIK_VIDTRANSCODE_CV_free(TRIK_IALG_Handle handle, TRIK_IALG_MemRec mem_tab[]);

/* ---------------------------------------------------------------------- */
/* Layer 2: batched device API                                             */
/* ---------------------------------------------------------------------- */

#define TRIK_HSV_LAYOUT_YUYV 0   /* packed Y0 U Y1 V, row = 2*W bytes (WSEQ:251-284) */
#define TRIK_HSV_LAYOUT_OV7670 1 /* Y plane rows + chroma plane rows; U = odd, V = even
                                    chroma byte (OSEQ:343-387) */

/* N frames in device memory: frame i starts at frames + i * frame_stride.
 * One frame is height * line_length bytes (YUYV) or 2 * height * line_length
 * (ov7670, chroma plane right after the luma plane).  Geometry rules of
 * WSEQ:365-369: width % 32 == 0, height % 4 == 0, both >= 0; line_length >=
 * 2*width (YUYV) or >= width (ov7670). */
typedef struct TrikHsvFrameBatch {
  const void* frames;
  int64_t frame_stride;
  int32_t n_frames;
  int32_t width;
  int32_t height;
  int32_t line_length;
  int32_t layout;
} TrikHsvFrameBatch;

/* Per frame per range: the reference's m_targetPoints / m_targetX / m_targetY
 * (WSEQ:56-58, accumulated at WSEQ:350-352), widened to 64 bits. */
typedef struct TrikHsvTargetSums {
  int64_t points;
  int64_t sum_x;
  int64_t sum_y;
} TrikHsvTargetSums;

/* Per frame per range: OutArgsAlg.targetX/targetY/targetSize (WSEQ:486-505). */
typedef struct TrikHsvTarget {
  int8_t x;
  int8_t y;
  uint8_t size;
  uint8_t reserved;
} TrikHsvTarget;

#define TRIK_HSV_MAX_RANGES 64

const char* trik_hsv_version(void);
/* Message of the last failed call on this thread ("" if none). */
const char* trik_hsv_last_error(void);

/* Full batched process: zero sums, detect + reduce, epilogue.
 * sums_dev: [n_frames][n_ranges] TrikHsvTargetSums (device).
 * targets_dev: [n_frames][n_ranges] TrikHsvTarget (device) or NULL.
 * Returns 0 or TRIK_IVIDTRANSCODE_EFAIL (see trik_hsv_last_error()). */
int32_t trik_hsv_process_batch(TRIK_VIDTRANSCODE_CV_Handle handle, const TrikHsvFrameBatch* batch,
                               const TRIK_VIDTRANSCODE_CV_InArgsAlg* ranges, int32_t n_ranges,
                               TrikHsvTargetSums* sums_dev, TrikHsvTarget* targets_dev,
                               void* hip_stream);

/* The full batched step: as trik_hsv_process_batch, plus the per-target
 * batch totals (totals_dev[r] = the sum over the frames of sums_dev[f][r], as
 * trik_hsv_batch_totals).  Where the chroma-run kernel runs, each group of
 * <= 4 ranges is ONE launch: the kernel writes every frame's sums and targets
 * as the frame completes and the totals at its end (scratch held by the
 * handle); otherwise the same outputs come from the separate kernels.
 * totals_dev: [n_ranges] TrikHsvTargetSums (device, not NULL). */
int32_t trik_hsv_process_batch_totals(TRIK_VIDTRANSCODE_CV_Handle handle, const TrikHsvFrameBatch* batch,
                                      const TRIK_VIDTRANSCODE_CV_InArgsAlg* ranges, int32_t n_ranges,
                                      TrikHsvTargetSums* sums_dev, TrikHsvTarget* targets_dev,
                                      TrikHsvTargetSums* totals_dev, void* hip_stream);

/* Detect + reduce only; ADDS into sums_dev (caller zeroes it).  This is the
 * hot kernel, one launch per group of <= 4 ranges. */
int32_t trik_hsv_batch_sums(TRIK_VIDTRANSCODE_CV_Handle handle, const TrikHsvFrameBatch* batch,
                            const TRIK_VIDTRANSCODE_CV_InArgsAlg* ranges, int32_t n_ranges,
                            TrikHsvTargetSums* sums_dev, void* hip_stream);

/* Hot-kernel selection of one handle for its trik_hsv_batch_sums /
 * _process_batch / _masks / _blob_batch calls and process() (tests and A/B
 * runs; other handles are not affected).  TRIK_HSV_HOT_AUTO (the default)
 * picks, per group of 4 ranges, the chroma-run kernel for batches of at
 * least TRIK_HSV_CHROMA_MIN_PIXELS pixels whose geometry it takes when the
 * group's tables send at most TRIK_HSV_CHROMA_MAX_SHARE of the words to its
 * exact path (see trik_hsv_chroma_share), the stripe kernel otherwise -- always for a
 * group of ranges that accepts every hue and saturation (value bands), which
 * the stripe kernel tests by value alone; all kernels give the same results.
 * The first batch with a new range set is not held up by that
 * share: both kernels are enqueued and the device runs the one the rule picks.
 * Returns the previous setting, or -1 for a NULL handle or an unknown kind. */
#define TRIK_HSV_HOT_AUTO 0
#define TRIK_HSV_HOT_STRIPE 1
#define TRIK_HSV_HOT_CHROMA 2
#define TRIK_HSV_HOT_GENERIC 3
#define TRIK_HSV_HOT_MIXED 4 /* trik_hsv_last_hot_kernel: the call's range groups ran different kernels */
#define TRIK_HSV_CHROMA_MIN_PIXELS (32 * 640 * 480)
#define TRIK_HSV_CHROMA_MAX_SHARE 0.27 /* the measured crossover (profiles/r05/r05p_adversarial_4096.txt) */
int32_t trik_hsv_set_hot_kernel(TRIK_VIDTRANSCODE_CV_Handle handle, int32_t kind);
/* The chroma-run kernel's expected exact-path word share (uniform input) for
 * the handle's current batched-sums range set (the maximum over its groups of
 * 4 ranges), or -1 when its tables are not built.  Waits for the builder's
 * readback if it is still in flight.  Returns 0 or TRIK_IVIDTRANSCODE_EFAIL. */
int32_t trik_hsv_chroma_share(TRIK_VIDTRANSCODE_CV_Handle handle, double* share);
/* The share of words the chroma-run kernel's exact path actually resolved on
 * the handle's recent batches of that range set that ran it (the maximum over
 * its groups; -1 before two readbacks have landed; intervals with a batch on
 * which the device chose the kernel are not measured).  AUTO reads the kernel's
 * counter back every few launches without waiting and sends a group whose
 * measured share exceeds TRIK_HSV_CHROMA_MAX_SHARE -- input concentrated on
 * the chromas its tables describe worst -- to the stripe kernel, trying the
 * chroma-run kernel again every 32 batches.  Waits for a readback in flight. */
int32_t trik_hsv_chroma_measured_share(TRIK_VIDTRANSCODE_CV_Handle handle, double* share);
/* The kernel the handle's last hot call ran (TRIK_HSV_HOT_STRIPE, _CHROMA or
 * _GENERIC; TRIK_HSV_HOT_MIXED when its groups of 4 ranges ran different
 * kernels; 0 before any; a call with an empty batch launches nothing and
 * leaves the answer unchanged).  When the device chose (see above) this waits for
 * the builder's readback. */
int32_t trik_hsv_last_hot_kernel(TRIK_VIDTRANSCODE_CV_Handle handle);
/* CUs the chroma-run hot kernel leaves free (0 by default): its grid is one
 * 160-KiB-LDS workgroup per CU the stream may use, so a kernel on another
 * stream (the per-step all-reduce of the totals over RCCL, multi-GPU) waits
 * for a CU to free up unless some stay free.  n CUs fewer: ~n/256 slower at
 * MI355X's 256 CUs; results are identical.  0 <= n <= 32; returns the
 * previous setting, or -1 for a NULL handle or an n out of range.  A stream
 * created with a CU mask (hipExtStreamCreateWithCUMask) is sized to its mask
 * where the runtime reports it. */
int32_t trik_hsv_set_reserved_cus(TRIK_VIDTRANSCODE_CV_Handle handle, int32_t n);

/* Epilogue only: sums_dev -> targets_dev for an n_frames x n_ranges grid. */
int32_t trik_hsv_batch_targets(const TrikHsvFrameBatch* batch, int32_t n_ranges,
                               const TrikHsvTargetSums* sums_dev, TrikHsvTarget* targets_dev,
                               void* hip_stream);

/* Verification mode of the hot kernel: also writes the per-pixel detection
 * mask (bit t = range t, n_ranges <= 8) to masks_dev[n_frames][height][width]
 * and adds into sums_dev.  Not used on the timed path. */
int32_t trik_hsv_batch_masks(TRIK_VIDTRANSCODE_CV_Handle handle, const TrikHsvFrameBatch* batch,
                             const TRIK_VIDTRANSCODE_CV_InArgsAlg* ranges, int32_t n_ranges,
                             uint8_t* masks_dev, TrikHsvTargetSums* sums_dev, void* hip_stream);

/* The operator's preview stream for N frames and one range (SURVEY 8(f)
 * row 2): each preview (out_height rows of out_line_length bytes at
 * previews_dev + i * preview_stride) is zero-filled (WFXNS:234), then written
 * as proceedImageHsv does -- RGB565X (B5 G6 R5, R in the low bits) of every
 * source pixel through the truncated scale maps, last writer wins, detected
 * pixels as 0x00ffff (WSEQ:316-354, 371-387) -- and overlaid with the guide
 * lines and the target circle (WSEQ:66-166, 471-494).  The circle uses
 * sums_dev[i * sums_pitch] (this range's sums of frame i, e.g. from
 * trik_hsv_process_batch with sums_pitch = n_ranges). */
int32_t trik_hsv_batch_preview(TRIK_VIDTRANSCODE_CV_Handle handle, const TrikHsvFrameBatch* batch,
                               const TRIK_VIDTRANSCODE_CV_InArgsAlg* range,
                               const TrikHsvTargetSums* sums_dev, int32_t sums_pitch,
                               int32_t out_width, int32_t out_height, int32_t out_line_length,
                               uint8_t* previews_dev, int64_t preview_stride, void* hip_stream);

/* autoDetectHsv for N frames: HsvRangeDetector::detect
 * (trik/webcam/object_sensor/include/internal/cv_hsv_range_detector.hpp:
 * 88-198, zone scale 6 as WSEQ:32).  out_dev[i][6] = detectHue,
 * detectHueTolerance, detectSat, detectSatTolerance, detectVal,
 * detectValTolerance (uint16), as OutArgsAlg receives them. */
int32_t trik_hsv_batch_auto_range(const TrikHsvFrameBatch* batch, uint16_t* out_dev, void* hip_stream);

/* Deterministic autoDetectHsv of the ov7670 object sensor and the two line
 * sensors.  Their detectors (ODET = trik/ov7670/object_sensor/
 * include/internal/cv_hsv_range_detector.hpp; LDET, LDETW = the copies under
 * trik/ov7670/line_sensor and trik/webcam/line_sensor) build a signed score
 * histogram of the whole frame (+1 per pixel of the positive zone, -2 per
 * pixel of the negative zone), remember a start cell, and then anneal from a
 * clock seed towards the box (interval) that maximises
 * sum(score != 0 ? score : -K0).  The histogram and the start cell are
 * reproduced bit for bit; the annealing is replaced by the exact maximum of
 * the same objective under a fixed tie rule; the output scaling is the
 * reference's.
 *   kind                          layout  bins                 K0
 *   TRIK_HSV_AUTO_OV7670_OBJECT   ov7670  32 x 32 [H>>3][S>>3]  2   (ODET:200-227)
 *   TRIK_HSV_AUTO_OV7670_LINE     ov7670  256 [V]               1   (LDET:215-240)
 *   TRIK_HSV_AUTO_WEBCAM_LINE     YUYV    256 [V]               1   (LDETW:215-240)
 * Each call fails (trik_hsv_last_error()) and writes nothing for an unknown
 * kind, a layout that is not the kind's, or a side above 2048. */
#define TRIK_HSV_AUTO_OV7670_OBJECT 0
#define TRIK_HSV_AUTO_OV7670_LINE 1
#define TRIK_HSV_AUTO_WEBCAM_LINE 2
#define TRIK_HSV_AUTO_MAX_SIDE 2048

/* The deterministic half, for a caller with a search of their own:
 *   scores_dev  [N][1024] int32 (object kind, bin h * 32 + s) or [N][256]: the
 *               final histogram;
 *   start_dev   [N][4] int32: the start cell's h (or v), its s (or 0), the
 *               detector's max_value, 0.  The start cell is the cell whose
 *               running value first reaches the largest value any cell holds
 *               right after one of its positive pixels, in raster order;
 *               (0, 0) with max_value 0 when no such value is positive (the
 *               line detectors leave the cell uninitialised there). */
int32_t trik_hsv_auto_scores(const TrikHsvFrameBatch* batch, int32_t kind, int32_t* scores_dev, int32_t* start_dev,
                             void* hip_stream);

/* The whole detector with the exact search:
 *   out_dev   [N][6] uint16: detectHue, detectHueTolerance, detectSat,
 *             detectSatTolerance, detectVal, detectValTolerance;
 *   best_dev  optional [N][5] int32: the maximum L and its box h1, h2, s1, s2
 *             (line kinds: v0, v1, 0, 0).
 * Object kind: over h1, h2 in 0..31 (h1 > h2 wraps through 31 -> 0), s1 in
 * 0..s_start, s2 in s_start..31 -- every state the annealing can visit --
 * the largest m_foo (ODET:109-153); ties go to the fewest cells, then the
 * smallest h1, then the smallest s1, then the smallest h2.  Line kinds: over
 * 0 <= v0 <= v1 <= 255 the largest F (LDET:137-163); ties go to the shortest
 * interval, then the smallest v0. */
int32_t trik_hsv_batch_auto_range_exact(const TrikHsvFrameBatch* batch, int32_t kind, uint16_t* out_dev,
                                        int32_t* best_dev, void* hip_stream);

/* The detectors' output scaling of a box (ODET:271-293; LDET:280-303, LDETW
 * the same with (v1 + 1) - 1 for v1 + 1): fp32 products truncated to int
 * (uint8_t for the line kinds' bounds).  Line kinds take v0, v1 as h1, h2 and
 * ignore s1, s2.  Needs 0 <= h1, h2 <= 31 and 0 <= s1 <= s2 <= 31, or 0 <= v0
 * <= v1 <= 255.  Host code, no GPU call; the device path gives the same. */
int32_t trik_hsv_auto_range_of(int32_t kind, int32_t h1, int32_t h2, int32_t s1, int32_t s2, uint16_t out[6]);

/* autoDetectHsv of the ov7670 object sensor's, the ov7670 line sensor's and
 * the webcam line sensor's process().  Mode 0 (the default): InArgs
 * autoDetectHsv is ignored and OutArgs detect* are left untouched.  Mode 1:
 * when InArgs autoDetectHsv is set, and only then, detect* receive
 * trik_hsv_batch_auto_range_exact of the frame; targets and preview are the
 * same.  Returns the previous mode, or -1 (trik_hsv_last_error()) for a NULL
 * handle, another codec's handle or an unknown mode. */
int32_t trik_hsv_set_auto_detect(TRIK_VIDTRANSCODE_CV_Handle handle, int32_t mode);

/* The object sensor for N frames with HSV ranges PER FRAME, read from device
 * memory by the kernel: one camera, one calibration per frame of the batch.
 *   ranges_dev   [n_frames][n_ranges][6] uint16 (device): hueFrom, hueTo,
 *                satFrom, satTo, valFrom, valTo in InArgs units (hue 0..359,
 *                saturation and value 0..100);
 *   sums_dev     [n_frames][n_ranges] TrikHsvTargetSums (device), zeroed by
 *                the call;
 *   targets_dev  the same shape of TrikHsvTarget (device), or NULL.
 * Slot (f, t) holds exactly what trik_hsv_process_batch writes for frame f
 * alone with the one range that holds the same six numbers, sums and targets,
 * in both layouts and for every geometry that call takes (padded line_length,
 * odd frame_stride, a misaligned base: those read bytes instead of words).
 * The six numbers are scaled and packed as WSEQ:425-445 does, in int32: each
 * bound is clamped to 0..255 after the scaling, so a saturation or value above
 * 255 -- which an InArgs byte cannot hold -- behaves as 255.
 * No handle: no table depends on a range, H, S and V are computed per pixel
 * (DESIGN.md 4.10).  Stream-ordered, no host synchronisation; the host never
 * dereferences ranges_dev, the kernel reads it when it runs, so a producer
 * earlier on the stream (trik_hsv_ranges_of_detect, a copy) is seen.
 * n_ranges is 1..TRIK_HSV_MAX_RANGES.  n_frames == 0 returns 0 and touches
 * nothing; width or height 0 zeroes sums and targets.  Fails
 * (trik_hsv_last_error()) and enqueues nothing for a NULL batch, NULL ranges
 * or sums when n_frames > 0, an unknown layout, a geometry the other batched
 * calls refuse, or n_ranges out of bounds. */
int32_t trik_hsv_frame_ranges_batch(const TrikHsvFrameBatch* batch, const uint16_t* ranges_dev, int32_t n_ranges,
                                    TrikHsvTargetSums* sums_dev, TrikHsvTarget* targets_dev, void* hip_stream);

/* The closed loop on the device: detect_dev [n][6] uint16 (hue, hueTol, sat,
 * satTol, val, valTol, as trik_hsv_batch_auto_range and _auto_range_exact
 * write them) -> the from/to six-tuple of frame i at ranges_dev +
 * (i * n_ranges + t) * 6, by the rule of cv_bitmap_builder_reference.hpp:
 * 110-130 in int arithmetic: hue from/to = (hue -/+ tol) mod 360, saturation
 * and value from/to = centre -/+ tol clipped to 0..100.  For inputs that fit
 * TRIK_VIDTRANSCODE_CV_OV7670_InArgsAlg the result equals
 * trik_hsv_blob_range_of.  The other entries of ranges_dev are left as they
 * are.  Fails for a NULL buffer when n > 0, n < 0, n_ranges outside
 * 1..TRIK_HSV_MAX_RANGES or t outside 0..n_ranges-1. */
int32_t trik_hsv_ranges_of_detect(const uint16_t* detect_dev, int32_t n, uint16_t* ranges_dev, int32_t n_ranges,
                                  int32_t t, void* hip_stream);

/* The reference's RGB888/HSV image as an output: what convertImageYuyvToHsv
 * leaves in s_rgb888hsv (WSEQ:251-284, OSEQ:343-387, and the line, MxN and
 * edge copies), the first two stages of every sensor, for N frames, bit for
 * bit on every (Y, U, V) -- the image every other call computes and none hands
 * out.  Chroma as everywhere else: per YUYV word for packed frames; U from the
 * odd chroma byte and V from the even one for the ov7670 planes. */
#define TRIK_HSV_CONVERT_RGB888HSV  0  /* uint64 per pixel: ((uint64)0x00RRGGBB << 32) | 0x00VVSSHH,
                                          the s_rgb888hsv entry (_itoll(rgb, hsv), WSEQ:243-247), little-endian */
#define TRIK_HSV_CONVERT_HSV_PLANES 1  /* three uint8 planes per frame: H, S, V */
#define TRIK_HSV_CONVERT_RGB_PLANES 2  /* three uint8 planes per frame: R, G, B */

typedef struct TrikHsvConvertOut {
  void*   out;           /* device */
  int64_t frame_stride;  /* bytes from frame f to f + 1 */
  int64_t plane_stride;  /* bytes from plane p to p + 1 (ignored by form 0) */
  int32_t row_pitch;     /* bytes from row r to r + 1 */
  int32_t form;
} TrikHsvConvertOut;

/* Pixel (f, r, c) of form 0 is the 8 bytes at out + f*frame_stride +
 * r*row_pitch + 8*c; byte (f, p, r, c) of a planar form is at out +
 * f*frame_stride + p*plane_stride + r*row_pitch + c.  Only these bytes are
 * written: the bytes of a row past its pixels (pitch padding), between planes
 * and between frames are left as they are (the reference's buffer is dense
 * and static; the strides are this call's own surface).
 * Both layouts and every geometry the other batched calls take: width % 32
 * == 0, height % 4 == 0, padded line_length, odd frame_stride, a misaligned
 * base.  A misaligned out, or a stride or pitch that is no multiple of 16, is
 * no error: like misaligned frames it takes the slower kernel (a lane per
 * pixel instead of 16-byte loads and stores).
 * No handle: nothing depends on a range.  Stream-ordered, no host
 * synchronisation: frames written earlier on the stream are the ones
 * converted.  n_frames == 0 returns 0 and touches nothing; width or height 0
 * returns 0 and writes nothing.  Fails (trik_hsv_last_error()) and enqueues
 * nothing for a NULL batch or out; NULL frames or out->out when n_frames > 0;
 * an unknown layout or form; a geometry the other batched calls refuse;
 * row_pitch below the row's bytes (8*width for form 0, width for the planes);
 * plane_stride < height*row_pitch for a planar form; frame_stride below the
 * frame's extent (height*row_pitch for form 0, 2*plane_stride +
 * height*row_pitch for the planes; checked for a single frame too). */
int32_t trik_hsv_convert_batch(const TrikHsvFrameBatch* batch, const TrikHsvConvertOut* out, void* hip_stream);

/* The per-pixel detection mask as an output: the reference's detectHsvPixel
 * (WSEQ:171-179) on every pixel's s_rgb888hsv entry under range t of the
 * pixel's frame, bit for bit -- the "detected" image every sensor computes and
 * hands out only summed (sums, targets), reduced (4x4 metapixels) or drawn
 * (previews).  One plane per range. */
#define TRIK_HSV_MASK_BITS  0  /* n_ranges bit planes per frame; pixel c of row r is bit (c & 7)
                                  of byte c >> 3 of its row, least significant bit first
                                  (= bit c & 31 of little-endian uint32 c >> 5) */
#define TRIK_HSV_MASK_BYTES 1  /* n_ranges byte planes per frame; 0xFF detected, 0x00 not */

typedef struct TrikHsvMaskOut {
  void*   out;           /* device */
  int64_t frame_stride;  /* bytes from frame f to f + 1 */
  int64_t plane_stride;  /* bytes from range t's plane to range t + 1's */
  int32_t row_pitch;     /* bytes from row r to r + 1 */
  int32_t form;
} TrikHsvMaskOut;

/* Range t of frame f is the six-tuple at ranges_dev + f*ranges_frame_stride +
 * 6*t: uint16 in InArgs units (hueFrom, hueTo, satFrom, satTo, valFrom, valTo),
 * exactly the tuples of trik_hsv_frame_ranges_batch.  ranges_frame_stride
 * counts uint16 elements: 0 is one shared set of n_ranges tuples for every
 * frame; 6*n_ranges is the buffer trik_hsv_frame_ranges_batch and
 * trik_hsv_ranges_of_detect use, taken as it is; larger values skip the
 * elements between the sets; 1 .. 6*n_ranges-1 and negative values fail.
 * n_ranges is 1..TRIK_HSV_MAX_RANGES.  The host never dereferences ranges_dev,
 * the kernel reads it when it runs, so a producer earlier on the stream is
 * seen.  The tuples are scaled and packed as WSEQ:425-445 does, in int32 (the
 * packing of trik_hsv_frame_ranges_batch): a saturation or value above 255
 * behaves as 255.
 * Byte b of row r of plane t of frame f is at out + f*frame_stride +
 * t*plane_stride + r*row_pitch + b, with b < width/8 (bits) or b < width
 * (bytes).  Only these bytes are written, each exactly once per call, by plain
 * stores (no atomics, no read-modify-write): row padding and the bytes between
 * planes and between frames keep what they held, and the caller need not zero
 * anything.  The value is bit t of the mask trik_hsv_batch_masks gives for the
 * same ranges (any t up to 63 here).
 * Both layouts and every geometry and placement trik_hsv_frame_ranges_batch
 * takes: width % 32 == 0 (a bit row is whole 32-bit words), height % 4 == 0,
 * padded line_length, odd frame_stride, a misaligned base.  A misaligned out,
 * stride or pitch is no error: it takes the slower kernel (the fast one needs
 * 16-byte aligned frames, and out, row_pitch, plane_stride when n_ranges > 1
 * and frame_stride when n_frames > 1 as multiples of 4 for the bits, 8 for the
 * bytes).  Planes cannot interleave by rows: plane_stride >= height*row_pitch.
 * No handle, no table per range set.  Stream-ordered, no host synchronisation.
 * n_frames == 0 returns 0 and touches nothing; width or height 0 returns 0 and
 * writes nothing.  Fails (trik_hsv_last_error()) and enqueues nothing for a
 * NULL batch or out; NULL frames, ranges_dev or out->out when n_frames > 0; an
 * unknown layout or form; a geometry the other batched calls refuse; n_ranges
 * or ranges_frame_stride out of bounds; row_pitch below the row's bytes;
 * plane_stride < height*row_pitch; frame_stride < (n_ranges-1)*plane_stride +
 * height*row_pitch (checked for a single frame too). */
int32_t trik_hsv_mask_batch(const TrikHsvFrameBatch* batch, const uint16_t* ranges_dev, int32_t n_ranges,
                            int64_t ranges_frame_stride, const TrikHsvMaskOut* out, void* hip_stream);

/* The object sensor's preview for N frames with an HSV range PER FRAME, read
 * from device memory by the kernels: the operator's picture of what
 * trik_hsv_frame_ranges_batch detected.
 *   ranges_dev   frame f's range is the six-tuple at ranges_dev +
 *                (f * n_ranges + t) * 6: the buffer layout and units of
 *                trik_hsv_frame_ranges_batch, so a buffer written by
 *                trik_hsv_ranges_of_detect or used for the sums call is taken
 *                as it is; n_ranges is 1..TRIK_HSV_MAX_RANGES, t is
 *                0..n_ranges-1;
 *   sums_dev     the circle of preview f comes from sums_dev[f * sums_pitch]
 *                (its low words, as trik_hsv_batch_preview): with the sums
 *                call's buffer, sums_dev + t and sums_pitch = n_ranges.
 * Preview f is, byte for byte, what trik_hsv_batch_preview writes for frame f
 * alone with the range that holds the same six numbers and
 * sums_dev[f * sums_pitch]: every byte of out_height x out_line_length is
 * written, unwritten pixels and line padding as zero; the body goes through
 * the truncated scale maps, last writer wins, detected pixels are 0x00ffff;
 * then the eight guide lines, then the circle.  The six numbers are scaled and
 * packed as WSEQ:425-445 does, in int32 (a saturation or value above 255
 * behaves as 255).  Both layouts and every geometry and placement
 * trik_hsv_batch_preview takes: padded line_length, odd frame_stride,
 * misaligned frames and previews, any out_*.  Bytes between previews
 * (preview_stride > out_height * out_line_length) are not touched.
 * The handle rule is trik_hsv_batch_preview's; the handle lends its lock and
 * its scale maps only: no table is built (H, S and V are computed per sampled
 * pixel) and trik_hsv_last_hot_kernel's report is unchanged.
 * Stream-ordered, with no host synchronisation but the one a change of the
 * preview geometry costs any preview call; the host never dereferences
 * ranges_dev or sums_dev.
 * n_frames == 0 or no preview byte returns 0 and touches nothing; width or
 * height 0 gives the zero fill alone.  Fails (trik_hsv_last_error()) and
 * enqueues nothing for everything trik_hsv_batch_preview refuses, NULL
 * ranges_dev when n_frames > 0, and n_ranges or t out of bounds. */
int32_t trik_hsv_frame_ranges_preview(TRIK_VIDTRANSCODE_CV_Handle handle, const TrikHsvFrameBatch* batch,
                                      const uint16_t* ranges_dev, int32_t n_ranges, int32_t t,
                                      const TrikHsvTargetSums* sums_dev, int32_t sums_pitch,
                                      int32_t out_width, int32_t out_height, int32_t out_line_length,
                                      uint8_t* previews_dev, int64_t preview_stride, void* hip_stream);

/* The line sensor for N ov7670 frames: sums_dev[i] =
 * {points, sum_x, cross points} -- cross points in the sum_y slot -- for V in
 * [val_from, val_to] (InArgs percent units) in columns 5..W-5, cross points
 * over rows band_start..band_stop (the reference: H/2 .. H/2+80);
 * targets_dev[i] (may be NULL) = OutArgs of LSEQ:455-474. */
int32_t trik_hsv_line_batch(const TrikHsvFrameBatch* batch, int32_t val_from, int32_t val_to,
                            int32_t band_start, int32_t band_stop, TrikHsvTargetSums* sums_dev,
                            TrikHsvTarget* targets_dev, void* hip_stream);

/* The line sensors for N frames with a V range PER FRAME, read from device
 * memory by the kernel: one calibration per camera or lighting condition.
 *   ranges_dev   [n_frames][6] uint16 (device): the six-tuple layout of
 *                trik_hsv_frame_ranges_batch and trik_hsv_ranges_of_detect
 *                with n_ranges == 1, so one buffer serves all three calls.
 *                Entries 4 and 5 (valFrom, valTo, percent) are read; entries
 *                0..3 are ignored, as the reference ignores the hue and
 *                saturation InArgs (LSEQ:392-395, LSEQW:345-348).  Each bound
 *                is scaled on the device as LSEQ:397-398 does, in int32:
 *                clamp(v * 255 / 100, 0, 255) (trik_hsv_line_scale_val), so a
 *                value above 100 behaves as 255;
 *   sums_dev     [n_frames] TrikHsvTargetSums (device), zeroed by the call;
 *   targets_dev  [n_frames] TrikHsvTarget (device), or NULL.
 * TRIK_HSV_LAYOUT_OV7670, the ov7670 line sensor: slot f holds exactly what
 * trik_hsv_line_batch writes for frame f alone with (ranges[f][4],
 * ranges[f][5]) and the same band: {points, sum_x, cross points in the sum_y
 * slot}, window columns 5..W-5, band rows compared as uint32; targets of
 * LSEQ:455-474.
 * TRIK_HSV_LAYOUT_YUYV, the webcam line sensor (LSEQW:232-269, 401-417): every
 * column and row, slot f = {points, sum_x, sum_y = sum over rows of row x the
 * row's points}: the three numbers trik_hsv_frame_ranges_batch writes for
 * frame f with (0, 359, 0, 100, valFrom, valTo), and the webcam line codec's
 * process() leaves in its sums; targets with targetY 0.  band_start and
 * band_stop are ignored.
 * A frame whose scaled from > to detects nothing (sums 0, target 0); the
 * other frames are unaffected.  No handle; stream-ordered, no host
 * synchronisation; the host never dereferences ranges_dev, the kernel reads it
 * when it runs, so a producer earlier on the stream is seen.  n_frames == 0
 * returns 0 and touches nothing; width or height 0 zeroes sums and targets.
 * Fails (trik_hsv_last_error()) and enqueues nothing for a NULL batch, NULL
 * ranges or sums when n_frames > 0, an unknown layout, or a geometry the other
 * batched calls refuse.  Input the vector kernels cannot take (a base or
 * frame_stride not 8- / 16-byte aligned for ov7670 / YUYV, line_length no
 * multiple of that) is read byte by byte. */
int32_t trik_hsv_line_frame_ranges_batch(const TrikHsvFrameBatch* batch, const uint16_t* ranges_dev,
                                         int32_t band_start, int32_t band_stop,
                                         TrikHsvTargetSums* sums_dev, TrikHsvTarget* targets_dev,
                                         void* hip_stream);

/* The byte a line sensor compares V with for a percent bound (LSEQ:397-398):
 * clamp(percent * 255 / 100, 0, 255) in int32, |percent| < 2^23.  The one
 * definition trik_hsv_line_batch applies on the host and
 * trik_hsv_line_frame_ranges_batch's kernels on the device.  Host code, no
 * GPU call. */
int32_t trik_hsv_line_scale_val(int32_t percent);

/* The line sensor's preview for N frames (window columns, guide, band and
 * target lines, LSEQ:283-291, 433-467), from sums_dev of trik_hsv_line_batch. */
int32_t trik_hsv_line_preview(TRIK_VIDTRANSCODE_CV_Handle handle, const TrikHsvFrameBatch* batch,
                              int32_t val_from, int32_t val_to, const TrikHsvTargetSums* sums_dev,
                              int32_t out_width, int32_t out_height, int32_t out_line_length,
                              uint8_t* previews_dev, int64_t preview_stride, void* hip_stream);

/* The line sensors' previews for N frames with a V range PER FRAME, read from
 * device memory by the kernels: the operator's picture of what
 * trik_hsv_line_frame_ranges_batch detected.
 *   ranges_dev   [n_frames][6] uint16 (device), the buffer of
 *                trik_hsv_line_frame_ranges_batch taken as it is: entries 4 and
 *                5 (valFrom, valTo, percent) are read, entries 0..3 ignored.
 *                Each bound is scaled on the device as
 *                trik_hsv_line_scale_val does, so a value above 100 behaves as
 *                255.  A frame whose scaled from > to has no detected pixel;
 *                its colours and overlays are drawn as usual;
 *   sums_dev     [n_frames] TrikHsvTargetSums (device): frame f's target line
 *                comes from sums_dev[f], the low words of points and sum_x,
 *                drawn when points > 10 -- the numbers trik_hsv_line_preview
 *                reads.  The buffer trik_hsv_line_frame_ranges_batch wrote is
 *                taken as it is.
 * TRIK_HSV_LAYOUT_OV7670, the ov7670 line sensor: preview f is, byte for byte,
 * what trik_hsv_line_preview writes for frame f alone with (ranges[f][4],
 * ranges[f][5]) and sums_dev[f]: only source columns 5..W-5 write, detected
 * pixels are 0x00ffff, then the four magenta thin lines, the two red band
 * lines at the rows of H/2 and H/2+80 and the red three-column target line,
 * each through drawOutputPixelBound (LSEQ:283-291, 419-474).
 * TRIK_HSV_LAYOUT_YUYV, the webcam line sensor: preview f is, byte for byte,
 * what the webcam line codec's process() writes for that frame and range with
 * the same output geometry (LSEQW:232-269, 396-413): every column writes, the
 * thin lines and the target line, no band lines.
 * Every byte of out_height x out_line_length is written, unwritten pixels and
 * line padding as zero; bytes between previews (preview_stride > out_height *
 * out_line_length) are not touched.  Every geometry and placement
 * trik_hsv_batch_preview takes: padded line_length, odd frame_stride,
 * misaligned frames and previews, any out_*.
 * The handle rule is trik_hsv_batch_preview's and any handle serves either
 * layout; the handle lends its lock and its scale maps only (for ov7670 the
 * maps with the 5..W-5 column window): no table is built or looked up (V is
 * the maximum of the colour the preview computes anyway) and
 * trik_hsv_last_hot_kernel's report is unchanged.  Stream-ordered, with no
 * host synchronisation but the one a change of the preview geometry costs any
 * preview call; the host never dereferences ranges_dev or sums_dev.
 * n_frames == 0 or no preview byte returns 0 and touches nothing; width or
 * height 0 gives the zero fill alone.  Fails (trik_hsv_last_error()) and
 * enqueues nothing for everything trik_hsv_batch_preview refuses, an unknown
 * layout, NULL ranges_dev, sums_dev or previews_dev when there are frames, and
 * a ranges_dev that is not device-accessible memory of the handle's device. */
int32_t trik_hsv_line_frame_ranges_preview(TRIK_VIDTRANSCODE_CV_Handle handle, const TrikHsvFrameBatch* batch,
                                           const uint16_t* ranges_dev, const TrikHsvTargetSums* sums_dev,
                                           int32_t out_width, int32_t out_height, int32_t out_line_length,
                                           uint8_t* previews_dev, int64_t preview_stride, void* hip_stream);

/* The ov7670 multi-blob sensor for N ov7670 frames,
 * one HSV range given as the InArgs centre/tolerance (converted as
 * cv_bitmap_builder_reference.hpp:110-130):
 *   targets_dev  [N][8] TrikHsvTarget: OutArgs target[i] (x, y, size; 0 when
 *                not kept), OSEQ:563-590;
 *   top_dev      optional [N][8][3] int32: size, sum_x, sum_y of the 8
 *                largest clusters after the clusterer's postProcessing;
 *   meta_dev     optional [N][H/4][W/4] uint8: 1 for set metapixels (more than
 *                2 of 16 pixels detected);
 *   labels_dev   optional [N][H/4][W/4] uint16: the clusterer's label map;
 *   n_labels_dev optional [N] int32: labels including the background.
 * Scratch lives in the handle. */
int32_t trik_hsv_blob_batch(TRIK_VIDTRANSCODE_CV_Handle handle, const TrikHsvFrameBatch* batch,
                            const TRIK_VIDTRANSCODE_CV_OV7670_InArgsAlg* hsv, TrikHsvTarget* targets_dev,
                            int32_t* top_dev, uint8_t* meta_dev, uint16_t* labels_dev,
                            int32_t* n_labels_dev, void* hip_stream);

/* The multi-blob sensor for N frames and n_ranges HSV ranges per frame, from
 * one read of the frames per group of 4 ranges.  The ranges come in the
 * from/to form of trik_hsv_process_batch (autoDetectHsv is ignored; see
 * trik_hsv_blob_range_of for the centre/tolerance form); the batch may be
 * TRIK_HSV_LAYOUT_OV7670 or TRIK_HSV_LAYOUT_YUYV.  A slot is one (frame f,
 * range t) pair, s = f * n_ranges + t, and every output is laid out by slot:
 *   targets_dev  [N][T][8] TrikHsvTarget;
 *   top_dev      optional [N][T][8][3] int32;
 *   meta_dev     optional [N][T][H/4][W/4] uint8;
 *   labels_dev   optional [N][T][H/4][W/4] uint16;
 *   n_labels_dev optional [N][T] int32.
 * On ov7670 frames slot (f, t) holds exactly what trik_hsv_blob_batch writes
 * for frame f alone with range t; on YUYV frames (Y0 U Y1 V) what that call
 * writes for the ov7670 frame with the same (Y, U, V) at every pixel (there U
 * is the odd chroma byte and V the even one, OSEQ:369-373).  The reference
 * carries the bitmap builder and the clusterer under trik/webcam/object_sensor
 * as well, byte-identical to the ov7670 copies, but its webcam detector does
 * not include them: the YUYV form is the reference's algorithm on its other
 * input layout, not one of its builds.
 * The batch is walked in chunks of whole frames of at most
 * TRIK_HSV_BLOB_CHUNK_SLOTS slots (at least one frame), stream-ordered without
 * host synchronisation, so the handle's scratch is that of a single-range
 * call of TRIK_HSV_BLOB_CHUNK_SLOTS frames however large N * n_ranges is.
 * The bitmaps always come from the stripe arithmetic:
 * trik_hsv_set_hot_kernel does not affect this call, and
 * trik_hsv_last_hot_kernel reports TRIK_HSV_HOT_STRIPE after it.
 * Fails (trik_hsv_last_error()) and writes nothing for a NULL handle, batch,
 * ranges or (N > 0) targets, an unknown layout, n_ranges outside
 * 1..TRIK_HSV_MAX_RANGES, width % 32 or height % 4 not zero, width > 8192 or
 * more than 30,000 labels.  n_frames == 0 returns 0 and touches nothing;
 * width or height 0 zeroes targets, top and n_labels. */
#define TRIK_HSV_BLOB_CHUNK_SLOTS 4096
int32_t trik_hsv_blob_batch_ranges(TRIK_VIDTRANSCODE_CV_Handle handle, const TrikHsvFrameBatch* batch,
                                   const TRIK_VIDTRANSCODE_CV_InArgsAlg* ranges, int32_t n_ranges,
                                   TrikHsvTarget* targets_dev, int32_t* top_dev, uint8_t* meta_dev,
                                   uint16_t* labels_dev, int32_t* n_labels_dev, void* hip_stream);

/* The multi-blob sensor for N frames with HSV ranges PER FRAME, read from
 * device memory by the kernel: one camera, one calibration per frame.
 *   ranges_dev   [n_frames][n_ranges][6] uint16 (device), the layout and the
 *                units of trik_hsv_frame_ranges_batch (hueFrom, hueTo, satFrom,
 *                satTo, valFrom, valTo; hue 0..359, saturation and value
 *                0..100): a buffer written by trik_hsv_ranges_of_detect is
 *                taken as it is.
 * The outputs are those of trik_hsv_blob_batch_ranges, laid out by slot s =
 * f * n_ranges + t, and slot (f, t) holds, bit for bit, what that call writes
 * for frame f alone with the one range holding the same six numbers (targets,
 * top, meta, labels and n_labels), on TRIK_HSV_LAYOUT_OV7670 and
 * TRIK_HSV_LAYOUT_YUYV batches alike.  The six numbers are scaled and packed
 * as WSEQ:425-445 does, in int32: a saturation or value above 255 -- which an
 * InArgs byte cannot hold -- behaves as 255.
 * No table depends on a range: H, S and V are computed per pixel, once for
 * all n_ranges, so no table set is built or acquired.  The
 * handle lends its scratch only; trik_hsv_set_hot_kernel does not affect the
 * call and what trik_hsv_last_hot_kernel reports is left unchanged by it.
 * Stream-ordered, no host synchronisation; the host never dereferences
 * ranges_dev, the kernel reads it when it runs, so a producer earlier on the
 * stream is seen.  The batch goes in chunks of whole frames of at most
 * TRIK_HSV_BLOB_CHUNK_SLOTS slots, the ranges pointer advancing with each.
 * Fails (trik_hsv_last_error()) before any GPU call and writes nothing for
 * what trik_hsv_blob_batch_ranges refuses -- a NULL handle, batch or (N > 0)
 * targets, an unknown layout, n_ranges outside 1..TRIK_HSV_MAX_RANGES, width
 * % 32 or height % 4 not zero, width > 8192 or more than 30,000 labels -- and
 * for NULL ranges_dev when N > 0.  n_frames == 0 returns 0 and touches
 * nothing; width or height 0 zeroes targets, top and n_labels. */
int32_t trik_hsv_blob_frame_ranges_batch(TRIK_VIDTRANSCODE_CV_Handle handle, const TrikHsvFrameBatch* batch,
                                         const uint16_t* ranges_dev, int32_t n_ranges,
                                         TrikHsvTarget* targets_dev, int32_t* top_dev, uint8_t* meta_dev,
                                         uint16_t* labels_dev, int32_t* n_labels_dev, void* hip_stream);

/* The from/to range trik_hsv_blob_batch uses for a centre/tolerance range
 * (cv_bitmap_builder_reference.hpp:110-130: hue wraps in 0..359, saturation
 * and value clip to 0..100; setHsvRange is not read, autoDetectHsv of *out is
 * 0).  Host code, no GPU call.  Fails for a NULL argument. */
int32_t trik_hsv_blob_range_of(const TRIK_VIDTRANSCODE_CV_OV7670_InArgsAlg* hsv,
                               TRIK_VIDTRANSCODE_CV_InArgsAlg* out);

/* The multi-blob previews for N ov7670 frames from meta_dev and top_dev of
 * trik_hsv_blob_batch (OSEQ:387-420, 548-580). */
int32_t trik_hsv_blob_preview(TRIK_VIDTRANSCODE_CV_Handle handle, const TrikHsvFrameBatch* batch,
                              const uint8_t* meta_dev, const int32_t* top_dev, int32_t out_width,
                              int32_t out_height, int32_t out_line_length, uint8_t* previews_dev,
                              int64_t preview_stride, void* hip_stream);

/* The ov7670 MxN colour-grid sensor for N ov7670 frames:
 * rows_m x cols_n cells per frame (rows_m = InArgs widthM, cols_n = heightN;
 * 1 <= rows_m, 1 <= cols_n, rows_m * cols_n <= 100, else the call fails and
 * writes nothing):
 *   colors_dev  [N][rows_m * cols_n] int32: OutArgs outColor of each frame;
 *   bins_dev    optional [N][rows_m * cols_n] uint16: the winning bin,
 *               h << 4 | s << 2 | v with h = H >> 3, s = S >> 6, v = V >> 6.
 * Stream-ordered; scratch lives in the handle. */
int32_t trik_hsv_mxn_batch(TRIK_VIDTRANSCODE_CV_Handle handle, const TrikHsvFrameBatch* batch, int32_t rows_m,
                           int32_t cols_n, int32_t* colors_dev, uint16_t* bins_dev, void* hip_stream);

/* Its previews for N frames from colors_dev of trik_hsv_mxn_batch
 * (MSEQ:328-366, 609-618): zero fill, every source pixel, the cells' squares. */
int32_t trik_hsv_mxn_preview(TRIK_VIDTRANSCODE_CV_Handle handle, const TrikHsvFrameBatch* batch, int32_t rows_m,
                             int32_t cols_n, const int32_t* colors_dev, int32_t out_width, int32_t out_height,
                             int32_t out_line_length, uint8_t* previews_dev, int64_t preview_stride,
                             void* hip_stream);

/* The MxN sensor's colour of histogram bin (h_bin 0..31, s_bin 0..3, v_bin
 * 0..3): HSVtoRGB(8 h_bin, 64 s_bin, 64 v_bin) of MSEQ:480-517 as 0x00RRGGBB
 * (0 for a bin out of range).  Host code: a table built once, no GPU call. */
uint32_t trik_hsv_mxn_color(int32_t h_bin, int32_t s_bin, int32_t v_bin);

/* The ov7670 JPEG encoder for N ov7670 frames: frame i's
 * stream (see TRIK_VIDTRANSCODE_CV_create_jpeg) goes to out_dev + i *
 * out_stride.
 *   sizes_dev  [N] uint32: always the full length of each stream, like
 *              snprintf; a frame whose length exceeds out_capacity has
 *              nothing written to its slot;
 *   out_dev    may be NULL for a sizes-only call (else out_stride >=
 *              out_capacity when N > 1);
 *   coeffs_dev optional [N][blocks][components][64] int16: the quantised
 *              coefficients in zigzag order, blocks in raster order,
 *              components Y, U, V (Y alone in black and white) -- a
 *              verification output.
 * quality is clamped to 1..100.  The layout must be ov7670; line_length is
 * honoured (the reference uses width as the stride).  height % 8 != 0 and
 * sides above 65535 fail with trik_hsv_last_error() and write nothing; a
 * zero width or height gives sizes of 0.  Stream-ordered, no host
 * synchronisation; scratch lives in the handle and is bounded independently
 * of N (batches go through it in chunks of frames). */
int32_t trik_hsv_jpeg_batch(TRIK_VIDTRANSCODE_CV_Handle handle, const TrikHsvFrameBatch* batch, int32_t quality,
                            int32_t black_and_white, uint8_t* out_dev, int64_t out_stride, int64_t out_capacity,
                            uint32_t* sizes_dev, int16_t* coeffs_dev, void* hip_stream);

/* The encoder's header for a width x height frame: SOI, APP0 (JFIF 1.1), DQT
 * (the Annex K.1 tables scaled by quality, zigzag order), SOF0, DHT (the four
 * Annex K.3 tables), SOS (JENC:517-647).  Returns its length (607 in colour,
 * 324 in black and white) and writes it when out != NULL and capacity is
 * large enough; 0 for a side outside 0..65535.  Host code, no GPU call. */
int32_t trik_hsv_jpeg_header(int32_t quality, int32_t black_and_white, int32_t width, int32_t height, uint8_t* out,
                             int32_t capacity);

/* The ov7670 edge-line sensor for N ov7670 frames (see
 * TRIK_VIDTRANSCODE_CV_create_edge_line).  threshold is IMG_thr_gt2max_8's,
 * 0..255 (the codec uses 50; with 255 a pixel is detected only where
 * |H| + |V| >= 255).  line_length must equal width, both sides at most 2048;
 * otherwise, or with another layout, the call fails and writes nothing.
 *   sums_dev     [N]: {points, sum_x, 0} of ESEQ:189-205, zeroed by the call;
 *   targets_dev  optional [N]: OutArgs targetX / targetY / targetSize;
 *   edges_dev    optional [N][height][width] uint8: the thresholded map (the
 *                wrap columns and the never-written zero bytes included) -- a
 *                verification output, written by the generic kernel.
 * No handle: nothing is cached.  Stream-ordered. */
int32_t trik_hsv_edge_batch(const TrikHsvFrameBatch* batch, int32_t threshold, TrikHsvTargetSums* sums_dev,
                            TrikHsvTarget* targets_dev, uint8_t* edges_dev, void* hip_stream);

/* Its previews for N frames from sums_dev of trik_hsv_edge_batch with the
 * same threshold (ESEQ:226-249, 405): zero fill, every source pixel, the
 * target line of frames with points > 0.  uint16 RGB565 in native byte order. */
int32_t trik_hsv_edge_preview(TRIK_VIDTRANSCODE_CV_Handle handle, const TrikHsvFrameBatch* batch, int32_t threshold,
                              const TrikHsvTargetSums* sums_dev, int32_t out_width, int32_t out_height,
                              int32_t out_line_length, uint8_t* previews_dev, int64_t preview_stride,
                              void* hip_stream);

/* The edge-line sensor's OutArgs of one frame's sums (ESEQ:397-417) for a
 * width x height frame (each 1..2048).  Host code, no GPU call. */
int32_t trik_hsv_edge_targets(const TrikHsvTargetSums* sums, int32_t width, int32_t height, TrikHsvTarget* target);

/* Fill batch->frames (device, writable) with synthetic frames; frame i of the
 * batch is global frame first_frame + i.  kind 0 = uniform random bytes,
 * kind 1 = scene (gradients + 6 coloured discs).  Same bytes as the CPU
 * generator in oracle/trik_oracle.c for the same (seed, frame). */
int32_t trik_hsv_synth(const TrikHsvFrameBatch* batch, int32_t first_frame, int32_t kind,
                       uint64_t seed, void* hip_stream);

/* ---------------------------------------------------------------------- */
/* Layer 3: multi-GPU                                        */
/* ---------------------------------------------------------------------- */
/* Frames are independent units: a batch is sharded by frame index, each GPU
 * processes its shard resident in its own memory, and the one exchange is the
 * sum of the per-target batch totals (n_ranges x 3 int64) with one RCCL
 * all-reduce over xGMI.  The reference has no multi-device path (one DSP, one
 * frame per process call, WFXNS:174-264); these extend its batched surface.
 * RCCL (librccl.so.1) is loaded on the first group/comm call. */

/* Per-target batch totals on the device: totals_dev[r] = the sum over the
 * n_frames frames of sums_dev[f][r] (each field), stream-ordered. */
int32_t trik_hsv_batch_totals(int32_t n_frames, int32_t n_ranges, const TrikHsvTargetSums* sums_dev,
                              TrikHsvTargetSums* totals_dev, void* hip_stream);

/* One process driving several GPUs: per device an object-sensor handle
 * (TRIK_VIDTRANSCODE_CV_create defaults), a HIP stream and a host worker
 * thread, and an RCCL communicator over the devices (ncclCommInitAll). */
typedef struct TrikHsvGroup* TRIK_HSV_GroupHandle;
int32_t trik_hsv_group_create(int32_t n_devices, const int32_t* devices, TRIK_HSV_GroupHandle* out_group);
/* Device d (0 <= d < n_devices) processes batches[d] -- its frames, in the
 * memory of devices[d] -- as trik_hsv_process_batch does into sums_dev[d]
 * ([n_frames][n_ranges]) and targets_dev[d] (may be NULL), then the per-target
 * totals of its frames are summed over all devices with one ncclAllReduce
 * into totals_dev[d] ([n_ranges], on devices[d]), so every device holds the
 * totals of the whole batch.  Each device's worker thread enqueues its part on
 * the device's stream; the call returns once every part is enqueued (see
 * trik_hsv_group_sync).  A device with an empty shard (n_frames == 0) still
 * takes part in the all-reduce. */
int32_t trik_hsv_group_process(TRIK_HSV_GroupHandle group, const TrikHsvFrameBatch* batches,
                               const TRIK_VIDTRANSCODE_CV_InArgsAlg* ranges, int32_t n_ranges,
                               TrikHsvTargetSums* const* sums_dev, TrikHsvTarget* const* targets_dev,
                               TrikHsvTargetSums* const* totals_dev);
/* Waits for every device's enqueued work. */
int32_t trik_hsv_group_sync(TRIK_HSV_GroupHandle group);
/* The HIP stream device d's work runs on (for the caller's own ordering). */
void* trik_hsv_group_stream(TRIK_HSV_GroupHandle group, int32_t d);
int32_t trik_hsv_group_delete(TRIK_HSV_GroupHandle group);

/* One process per GPU (the layout of torch.distributed / bench.py): an RCCL
 * communicator over n_ranks processes, created on the calling thread's current
 * device from an id that rank 0 makes (trik_hsv_comm_id) and the caller
 * distributes to the other ranks by its own means. */
#define TRIK_HSV_COMM_ID_BYTES 128
typedef struct TrikHsvComm* TRIK_HSV_CommHandle;
int32_t trik_hsv_comm_id(uint8_t id[TRIK_HSV_COMM_ID_BYTES]);
int32_t trik_hsv_comm_create(int32_t n_ranks, int32_t rank, const uint8_t id[TRIK_HSV_COMM_ID_BYTES],
                             TRIK_HSV_CommHandle* out_comm);
/* In place, stream-ordered: totals_dev[n_ranges] summed over the ranks. */
int32_t trik_hsv_comm_all_reduce_totals(TRIK_HSV_CommHandle comm, TrikHsvTargetSums* totals_dev,
                                        int32_t n_ranges, void* hip_stream);
int32_t trik_hsv_comm_delete(TRIK_HSV_CommHandle comm);

#ifdef __cplusplus
}
#endif

#endif /* TRIK_HSV_H_ */
