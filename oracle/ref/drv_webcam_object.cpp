/* Host driver of the reference's webcam object sensor:
 * trik/webcam/object_sensor, BallDetector<YUV422, RGB565X>::setup + run, and
 * its two per-pixel functions for the exhaustive table.  TEST INFRASTRUCTURE. */
#include "ref_driver.hpp"
#include "internal/cv_ball_detector.hpp"

typedef trik::cv::BallDetector<TRIK_VIDTRANSCODE_CV_VIDEO_FORMAT_YUV422,
                               TRIK_VIDTRANSCODE_CV_VIDEO_FORMAT_RGB565X> Algo;

REF_API void* ref_create(int width, int height, int lineLength, int outWidth, int outHeight,
                         int outLineLength) {
  return refCreate<Algo>(width, height, lineLength, TRIK_VIDTRANSCODE_CV_VIDEO_FORMAT_YUV422,
                         outWidth, outHeight, outLineLength, TRIK_VIDTRANSCODE_CV_VIDEO_FORMAT_RGB565X);
}

REF_API void ref_destroy(void* handle) { refDestroy<Algo>(handle); }

/* range: hueFrom, hueTo, satFrom, satTo, valFrom, valTo.  res: targetX,
 * targetY, targetSize, then the six detect* fields (prefilled with 0xFFFF, so
 * an unwritten field shows).  Returns 0, or -1 when run() returns false. */
REF_API int ref_run(void* handle, const uint8_t* in, int64_t inSize, uint8_t* out, int64_t outSize,
                    const int32_t* range, int autoDetect, int32_t* res) {
  RefHandle<Algo>* h = static_cast<RefHandle<Algo>*>(handle);
  TrikCvAlgInArgs ia;
  memset(&ia, 0, sizeof(ia));
  ia.detectHueFrom = static_cast<XDAS_UInt16>(range[0]);
  ia.detectHueTo   = static_cast<XDAS_UInt16>(range[1]);
  ia.detectSatFrom = static_cast<XDAS_UInt8>(range[2]);
  ia.detectSatTo   = static_cast<XDAS_UInt8>(range[3]);
  ia.detectValFrom = static_cast<XDAS_UInt8>(range[4]);
  ia.detectValTo   = static_cast<XDAS_UInt8>(range[5]);
  ia.autoDetectHsv = autoDetect ? 1 : 0;
  TrikCvAlgOutArgs oa;
  memset(&oa, 0xFF, sizeof(oa));
  const TrikCvImageBuffer inBuf = refBuffer(in, inSize);
  TrikCvImageBuffer outBuf = refBuffer(out, outSize);
  if (!h->algo.run(inBuf, outBuf, ia, oa))
    return -1;
  res[0] = oa.targetX;
  res[1] = oa.targetY;
  res[2] = oa.targetSize;
  res[3] = oa.detectHue;
  res[4] = oa.detectHueTolerance;
  res[5] = oa.detectSat;
  res[6] = oa.detectSatTolerance;
  res[7] = oa.detectVal;
  res[8] = oa.detectValTolerance;
  return 0;
}

/* The per-pixel path on every (Y, U, V), through the detector's own
 * convert2xYuyvToRgb888 and convertRgb888ToHsv: first[Y | U << 8 | V << 16]
 * is (rgb << 32 | hsv) of the FIRST pixel of a YUYV word, second[...] that of
 * the SECOND pixel; the other pixel of each word carries Y ^ 0xA5, so every
 * luma passes through both halves of the word next to a different neighbour.
 * Needs one ref_create before it (the division tables live in fast RAM). */
REF_API int ref_pixel_tables(uint64_t* first, uint64_t* second) {
  if (Algo::s_mult43_div == NULL || Algo::s_mult255_div == NULL)
    return -1;
  for (uint32_t v = 0; v < 256; ++v)
    for (uint32_t u = 0; u < 256; ++u)
      for (uint32_t y0 = 0; y0 < 256; ++y0) {
        const uint32_t y1 = y0 ^ 0xA5u;
        const uint64_t rgb12 = Algo::convert2xYuyvToRgb888(y0 | (u << 8) | (y1 << 16) | (v << 24));
        const uint32_t p1 = _loll(rgb12), p2 = _hill(rgb12);
        first[y0 | (u << 8) | (v << 16)] = _itoll(p1, Algo::convertRgb888ToHsv(p1));
        second[y1 | (u << 8) | (v << 16)] = _itoll(p2, Algo::convertRgb888ToHsv(p2));
      }
  return 0;
}
