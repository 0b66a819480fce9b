/* Host driver of the reference's ov7670 MxN colour-grid sensor:
 * trik/ov7670/mxn_sensor, BallDetector<YUV422P, RGB565X>::setup + run.
 * TEST INFRASTRUCTURE. */
#include "ref_driver.hpp"
#include "internal/cv_ball_detector.hpp"

typedef trik::cv::BallDetector<TRIK_VIDTRANSCODE_CV_VIDEO_FORMAT_YUV422P,
                               TRIK_VIDTRANSCODE_CV_VIDEO_FORMAT_RGB565X> Algo;

REF_API void* ref_create(int width, int height, int lineLength, int outWidth, int outHeight,
                         int outLineLength) {
  return refCreate<Algo>(width, height, lineLength, TRIK_VIDTRANSCODE_CV_VIDEO_FORMAT_YUV422P,
                         outWidth, outHeight, outLineLength, TRIK_VIDTRANSCODE_CV_VIDEO_FORMAT_RGB565X);
}

REF_API void ref_destroy(void* handle) { refDestroy<Algo>(handle); }

/* widthM (the number of cell rows) and heightN (the number of cell columns)
 * as InArgs names them; colors: widthM * heightN entries of outColor.
 * Returns 0, -1 when run() returns false, -2 for a grid the reference would
 * divide by zero on or that overflows outColor[100]. */
REF_API int ref_run(void* handle, const uint8_t* in, int64_t inSize, uint8_t* out, int64_t outSize,
                    int widthM, int heightN, int32_t* colors) {
  RefHandle<Algo>* h = static_cast<RefHandle<Algo>*>(handle);
  if (widthM < 1 || heightN < 1 || widthM * heightN > 100)
    return -2;
  TrikCvAlgInArgs ia;
  memset(&ia, 0, sizeof(ia));
  ia.widthM = widthM;
  ia.heightN = heightN;
  TrikCvAlgOutArgs oa;
  memset(&oa, 0xFF, sizeof(oa));
  const TrikCvImageBuffer inBuf = refBuffer(in, inSize);
  TrikCvImageBuffer outBuf = refBuffer(out, outSize);
  if (!h->algo.run(inBuf, outBuf, ia, oa))
    return -1;
  for (int i = 0; i < widthM * heightN; ++i)
    colors[i] = oa.outColor[i];
  return 0;
}
