/* Host driver of the reference's ov7670 object sensor (multi-blob):
 * trik/ov7670/object_sensor, BallDetector<YUV422P, RGB565X>::setup + run with
 * its BitmapBuilder and Clusterizer, and the per-pixel image for the
 * exhaustive table of the ov7670 unpacking.  TEST INFRASTRUCTURE. */
#include "ref_driver.hpp"
#include "internal/cv_ball_detector.hpp"

typedef trik::cv::BallDetector<TRIK_VIDTRANSCODE_CV_VIDEO_FORMAT_YUV422P,
                               TRIK_VIDTRANSCODE_CV_VIDEO_FORMAT_RGB565X> Algo;

/* run() reads clusters[0..7] whatever the label count (the reference reads
 * past the end of its vector).  The driver keeps that read inside the
 * vector's allocation and makes it see zeros: room for 16 entries, zeroed
 * before each run; a run with fewer than 8 labels never reallocates.
 * Zeroing storage between size() and capacity() is outside what std::vector
 * promises; it holds with libstdc++ because Clusterizer::run touches the
 * vector only through clear() and push_back (CLU:98-112, 177-185), neither
 * of which writes or releases storage past the elements it adds. */
static const size_t kClusterRoom = 16;

REF_API void* ref_create(int width, int height, int lineLength, int outWidth, int outHeight,
                         int outLineLength) {
  return refCreate<Algo>(width, height, lineLength, TRIK_VIDTRANSCODE_CV_VIDEO_FORMAT_YUV422P,
                         outWidth, outHeight, outLineLength, TRIK_VIDTRANSCODE_CV_VIDEO_FORMAT_RGB565X);
}

REF_API void ref_destroy(void* handle) { refDestroy<Algo>(handle); }

/* args: setHsvRange, hue, hueTol, sat, satTol, val, valTol, autoDetectHsv.
 * targets: 8 x (x, y, size).  top: clusters[0..7] after the sort, as (size,
 * sum x, sum y).  info: label count (with the background), the sticky packed
 * range (from, to, expect), the six detect* fields.  sorted (optional, room
 * for sortedRoom triples): every cluster after the sort, as (size, sum x,
 * sum y).  meta / labels (optional, (W/4) * (H/4)): set metapixels and the
 * label map.  Returns 0, or -1 when run() returns false. */
REF_API int ref_run(void* handle, const uint8_t* in, int64_t inSize, uint8_t* out, int64_t outSize,
                    const int32_t* args, int8_t* targets, int32_t* top, int64_t* info,
                    int32_t* sorted, int32_t sortedRoom, uint8_t* meta, uint16_t* labels) {
  RefHandle<Algo>* h = static_cast<RefHandle<Algo>*>(handle);
  TrikCvAlgInArgs ia;
  memset(&ia, 0, sizeof(ia));
  ia.setHsvRange = args[0] ? 1 : 0;
  ia.detectHue = static_cast<XDAS_UInt16>(args[1]);
  ia.detectHueTol = static_cast<XDAS_UInt16>(args[2]);
  ia.detectSat = static_cast<XDAS_UInt8>(args[3]);
  ia.detectSatTol = static_cast<XDAS_UInt8>(args[4]);
  ia.detectVal = static_cast<XDAS_UInt8>(args[5]);
  ia.detectValTol = static_cast<XDAS_UInt8>(args[6]);
  ia.autoDetectHsv = args[7] ? 1 : 0;
  TrikCvAlgOutArgs oa;
  memset(&oa, 0xFF, sizeof(oa));

  std::vector<trik::cv::Target>& clusters = h->algo.m_clusterizer.clusters;
  clusters.clear();
  clusters.reserve(kClusterRoom);
  memset(static_cast<void*>(clusters.data()), 0, clusters.capacity() * sizeof(trik::cv::Target));

  const TrikCvImageBuffer inBuf = refBuffer(in, inSize);
  TrikCvImageBuffer outBuf = refBuffer(out, outSize);
  if (!h->algo.run(inBuf, outBuf, ia, oa))
    return -1;
  for (int i = 0; i < 8; ++i) {
    targets[3 * i + 0] = oa.target[i].x;
    targets[3 * i + 1] = oa.target[i].y;
    targets[3 * i + 2] = static_cast<int8_t>(oa.target[i].size);
    const trik::cv::Target* c = clusters.data() + i;  /* inside the allocation, see kClusterRoom */
    top[3 * i + 0] = c->size;
    top[3 * i + 1] = c->x;
    top[3 * i + 2] = c->y;
  }
  info[0] = static_cast<int64_t>(h->algo.m_clusterizer.equalClusters.size());
  info[1] = _hill(h->algo.m_bitmapBuilder.m_detectRange);
  info[2] = _loll(h->algo.m_bitmapBuilder.m_detectRange);
  info[3] = h->algo.m_bitmapBuilder.m_detectExpected;
  info[4] = oa.detectHue;
  info[5] = oa.detectHueTolerance;
  info[6] = oa.detectSat;
  info[7] = oa.detectSatTolerance;
  info[8] = oa.detectVal;
  info[9] = oa.detectValTolerance;
  if (sorted != NULL)
    for (size_t i = 0; i < clusters.size() && static_cast<int32_t>(i) < sortedRoom; ++i) {
      sorted[3 * i + 0] = clusters[i].size;
      sorted[3 * i + 1] = clusters[i].x;
      sorted[3 * i + 2] = clusters[i].y;
    }
  const int n = (h->in.m_width / METAPIX_SIZE) * (h->in.m_height / METAPIX_SIZE);
  for (int i = 0; i < n; ++i) {
    if (meta != NULL)
      meta[i] = trik::pop(trik::cv::s_bitmap[i]) > METAPIX_SIZE / 2 ? 1 : 0;
    if (labels != NULL)
      labels[i] = trik::cv::s_clustermap[i];
  }
  return 0;
}

/* The ov7670 unpacking plus the per-pixel path on every (Y, U, V), through
 * the detector's own convertImageYuyvToHsv: 256 frames of 256 x 256 (one per
 * V; row = U, luma of column c = (c + rot) & 255, so rot = 0..3 puts every
 * luma in each of the four positions of a 4-pixel group).
 * out[Y | U << 8 | V << 16] = (rgb << 32 | hsv).  Returns 0. */
REF_API int ref_pixel_table(uint64_t* out, int rot) {
  void* handle = ref_create(256, 256, 256, 128, 128, 256);
  if (handle == NULL)
    return -1;
  RefHandle<Algo>* h = static_cast<RefHandle<Algo>*>(handle);
  std::vector<uint8_t> frame(2 * 256 * 256);
  TrikCvImageBuffer inBuf = refBuffer(frame.data(), static_cast<int64_t>(frame.size()));
  for (uint32_t u = 0; u < 256; ++u)
    for (uint32_t c = 0; c < 256; ++c)
      frame[u * 256 + c] = static_cast<uint8_t>((c + rot) & 255);
  for (uint32_t v = 0; v < 256; ++v) {
    for (uint32_t u = 0; u < 256; ++u)
      for (uint32_t c = 0; c < 256; c += 2) {
        frame[65536 + u * 256 + c] = static_cast<uint8_t>(v);      /* even chroma byte */
        frame[65536 + u * 256 + c + 1] = static_cast<uint8_t>(u);  /* odd chroma byte */
      }
    h->algo.convertImageYuyvToHsv(inBuf);
    for (uint32_t u = 0; u < 256; ++u)
      for (uint32_t c = 0; c < 256; ++c)
        out[((c + rot) & 255) | (u << 8) | (v << 16)] = trik::cv::s_rgb888hsv[u * 256 + c];
  }
  ref_destroy(handle);
  return 0;
}
