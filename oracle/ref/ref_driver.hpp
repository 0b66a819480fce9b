/*
 * ref_driver.hpp -- what the six drivers of the reference's host build share.
 * TEST INFRASTRUCTURE ONLY (oracle/ref/Makefile; loaded by tests/ref_lib.py).
 *
 * A driver is one translation unit per reference sensor: it includes that
 * sensor's algorithm headers from the reference checkout (found through -I,
 * never copied), instantiates the algorithm class, and exports create / run /
 * destroy with C linkage.  Every sensor defines the same class names in
 * trik::cv, hence one shared library per sensor.
 *
 * The standard headers come first: the reference leans on TI's transitive
 * includes, and one of its headers defines a `min` macro.  `private` is then
 * opened so that a driver can reach state the reference leaves uninitialised
 * (and the per-pixel functions); the reference's files stay untouched.
 */
#ifndef TRIK_REF_DRIVER_HPP_
#define TRIK_REF_DRIVER_HPP_

#include <algorithm>
#include <cassert>
#include <cmath>
#include <cstdlib>
#include <ctime>
#include <map>
#include <memory>
#include <new>
#include <set>
#include <vector>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#define private public
#define protected public

#include "internal/vidtranscode_cv.h"
#include "internal/cv_algorithm.hpp"

#define REF_API extern "C" __attribute__((visibility("default")))

/* The 4 KiB "fast RAM" of the codec (TrikCvFastRamSize).  The reference keeps
 * static pointers into the first instance's block, so it lives as long as the
 * library does. */
alignas(8) static int8_t g_refFastRam[0x1000];

template <class Algo>
struct RefHandle {
  Algo algo;
  TrikCvImageDesc in, out;
};

/* new Algo + setup(); NULL where setup() returns false.  The reference keeps
 * its scale maps and its per-pixel image in file statics, so one instance of a
 * sensor is live at a time: run an instance only until the next create. */
template <class Algo>
static void* refCreate(int width, int height, int lineLength, TrikCvImageFormat inFormat,
                       int outWidth, int outHeight, int outLineLength, TrikCvImageFormat outFormat) {
  RefHandle<Algo>* h = new RefHandle<Algo>();
  h->in.m_width = static_cast<TrikCvImageDimension>(width);
  h->in.m_height = static_cast<TrikCvImageDimension>(height);
  h->in.m_lineLength = lineLength;
  h->in.m_format = inFormat;
  h->out.m_width = static_cast<TrikCvImageDimension>(outWidth);
  h->out.m_height = static_cast<TrikCvImageDimension>(outHeight);
  h->out.m_lineLength = outLineLength;
  h->out.m_format = outFormat;
  if (width > 640 || height > 480 || width < 0 || height < 0  /* the reference's static images */
      || !h->algo.setup(h->in, h->out, g_refFastRam, sizeof(g_refFastRam))) {
    delete h;
    return NULL;
  }
  return h;
}

template <class Algo>
static void refDestroy(void* handle) {
  delete static_cast<RefHandle<Algo>*>(handle);
}

static inline TrikCvImageBuffer refBuffer(const void* ptr, int64_t size) {
  TrikCvImageBuffer b;
  b.m_ptr = reinterpret_cast<TrikCvImagePtr>(const_cast<void*>(ptr));
  b.m_size = static_cast<TrikCvImageSize>(size);
  return b;
}

#endif /* TRIK_REF_DRIVER_HPP_ */
