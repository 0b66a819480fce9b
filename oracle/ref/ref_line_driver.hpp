/* The body the two line-sensor drivers share; the including file defines
 * REF_LINE_FORMAT (the LineDetector specialisation's input format) and
 * REF_LINE_HAS_BAND (1 for the ov7670 sensor, whose run() counts cross points
 * in the row band the PREVIOUS run left).  TEST INFRASTRUCTURE. */
#include "ref_driver.hpp"
#include "internal/cv_line_detector.hpp"

typedef trik::cv::LineDetector<REF_LINE_FORMAT, TRIK_VIDTRANSCODE_CV_VIDEO_FORMAT_RGB565X> Algo;

REF_API void* ref_create(int width, int height, int lineLength, int outWidth, int outHeight,
                         int outLineLength) {
  return refCreate<Algo>(width, height, lineLength, REF_LINE_FORMAT, outWidth, outHeight, outLineLength,
                         TRIK_VIDTRANSCODE_CV_VIDEO_FORMAT_RGB565X);
}

REF_API void ref_destroy(void* handle) { refDestroy<Algo>(handle); }

/* band: hStart, hStop, in and out (the reference leaves them uninitialised
 * before its first run; the caller supplies that state).  autoDetectHsv stays
 * off: it is a simulated annealing seeded from the clock.  res: targetX,
 * targetY, targetSize; sums: N, sum of columns, then the cross points (ov7670)
 * or the sum of rows (webcam; the reference never resets that member, so the
 * driver zeroes it before the run).  Returns 0, or -1 when run() is false. */
REF_API int ref_run(void* handle, const uint8_t* in, int64_t inSize, uint8_t* out, int64_t outSize,
                    int valFrom, int valTo, int32_t* band, int32_t* res, int64_t* sums) {
  RefHandle<Algo>* h = static_cast<RefHandle<Algo>*>(handle);
  TrikCvAlgInArgs ia;
  memset(&ia, 0, sizeof(ia));
  ia.detectHueTo = 359;
  ia.detectSatTo = 100;
  ia.detectValFrom = static_cast<XDAS_UInt8>(valFrom);
  ia.detectValTo = static_cast<XDAS_UInt8>(valTo);
  TrikCvAlgOutArgs oa;
  memset(&oa, 0xFF, sizeof(oa));
#if REF_LINE_HAS_BAND
  h->algo.m_hStart = static_cast<uint32_t>(band[0]);
  h->algo.m_hStop = static_cast<uint32_t>(band[1]);
#else
  (void)band;
#endif
  h->algo.m_targetY = 0;
  const TrikCvImageBuffer inBuf = refBuffer(in, inSize);
  TrikCvImageBuffer outBuf = refBuffer(out, outSize);
  if (!h->algo.run(inBuf, outBuf, ia, oa))
    return -1;
  res[0] = oa.targetX;
  res[1] = oa.targetY;
  res[2] = oa.targetSize;
  sums[0] = h->algo.m_targetPoints;
  sums[1] = h->algo.m_targetX;
#if REF_LINE_HAS_BAND
  sums[2] = h->algo.m_crossPoints;
  band[0] = static_cast<int32_t>(h->algo.m_hStart);
  band[1] = static_cast<int32_t>(h->algo.m_hStop);
#else
  sums[2] = h->algo.m_targetY;
#endif
  return 0;
}
