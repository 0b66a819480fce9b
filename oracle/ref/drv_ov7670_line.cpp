/* Host driver of the reference's ov7670 line sensor: trik/ov7670/line_sensor,
 * LineDetector<YUV422P, RGB565X>::setup + run.  TEST INFRASTRUCTURE. */
#define REF_LINE_FORMAT TRIK_VIDTRANSCODE_CV_VIDEO_FORMAT_YUV422P
#define REF_LINE_HAS_BAND 1
#include "ref_line_driver.hpp"
