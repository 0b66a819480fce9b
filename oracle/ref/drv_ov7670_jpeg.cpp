/* Host driver of the reference's ov7670 JPEG encoder: trik/ov7670/jpeg_encoder,
 * JPGEncoderWrapper<YUV422P, RGB565X>::setup + run (JPGEncoder::init + encode).
 * TEST INFRASTRUCTURE. */
#include "ref_driver.hpp"
#include "internal/cv_jpeg_encoder_wrapper.hpp"

typedef trik::cv::JPGEncoderWrapper<TRIK_VIDTRANSCODE_CV_VIDEO_FORMAT_YUV422P,
                                    TRIK_VIDTRANSCODE_CV_VIDEO_FORMAT_RGB565X> Algo;

/* The encoder writes without a capacity.  Worst case: every one of the 64
 * coefficients of the 3 data units of a block costs a 16-bit code and 11
 * value bits (27 bits), every byte is 0xFF and gets a stuffed zero after it,
 * plus the headers (607 bytes in colour), the fill byte and EOI. */
static int64_t worstCase(int width, int height) {
  const int64_t blocks = static_cast<int64_t>((width + 7) / 8) * ((height + 7) / 8);
  return 2 * ((blocks * 27 * 64 * 3 + 7) / 8) + 1024;
}

struct JpegHandle {
  void* inner;
  std::vector<uint8_t> stream;
  int width, height;
};

/* The reference strides by width and takes the chroma plane at width * height:
 * lineLength is passed on to setup() but encode() does not read it.  Width and
 * height must be multiples of 8 (encode() reads whole 8 x 8 blocks). */
REF_API void* ref_create(int width, int height, int lineLength) {
  if (width % 8 != 0 || height % 8 != 0)
    return NULL;
  const int64_t room = worstCase(width, height);
  void* inner = refCreate<Algo>(width, height, lineLength, TRIK_VIDTRANSCODE_CV_VIDEO_FORMAT_YUV422P,
                                0, 1, static_cast<int>(room), TRIK_VIDTRANSCODE_CV_VIDEO_FORMAT_RGB565X);
  if (inner == NULL)
    return NULL;
  JpegHandle* h = new JpegHandle();
  h->inner = inner;
  h->stream.resize(static_cast<size_t>(room));
  h->width = width;
  h->height = height;
  return h;
}

REF_API void ref_destroy(void* handle) {
  JpegHandle* h = static_cast<JpegHandle*>(handle);
  refDestroy<Algo>(h->inner);
  delete h;
}

/* Returns the stream's length (OutArgs size), copied to out when it fits in
 * outRoom; -1 when run() returns false. */
REF_API int64_t ref_run(void* handle, const uint8_t* in, int64_t inSize, uint8_t* out, int64_t outRoom,
                        int quality, int blackAndWhite) {
  JpegHandle* h = static_cast<JpegHandle*>(handle);
  RefHandle<Algo>* a = static_cast<RefHandle<Algo>*>(h->inner);
  TrikCvAlgInArgs ia;
  memset(&ia, 0, sizeof(ia));
  ia.jpgImageQuality = static_cast<XDAS_UInt8>(quality);
  ia.ifBlackAndWhite = blackAndWhite ? 1 : 0;
  TrikCvAlgOutArgs oa;
  memset(&oa, 0, sizeof(oa));
  const TrikCvImageBuffer inBuf = refBuffer(in, inSize);
  TrikCvImageBuffer outBuf = refBuffer(h->stream.data(), static_cast<int64_t>(h->stream.size()));
  if (!a->algo.run(inBuf, outBuf, ia, oa))
    return -1;
  const int64_t n = oa.size;
  if (n <= outRoom && n <= static_cast<int64_t>(h->stream.size()))
    memcpy(out, h->stream.data(), static_cast<size_t>(n));
  return n;
}
