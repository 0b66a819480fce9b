/* Host driver of the reference's webcam line sensor: trik/webcam/line_sensor,
 * LineDetector<YUV422, RGB565X>::setup + run.  TEST INFRASTRUCTURE. */
#define REF_LINE_FORMAT TRIK_VIDTRANSCODE_CV_VIDEO_FORMAT_YUV422
#define REF_LINE_HAS_BAND 0
#include "ref_line_driver.hpp"
