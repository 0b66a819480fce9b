// trik_hsv_tables.cpp -- host-side "range compiler": turns a group of InArgs
// HSV ranges into the LDS lookup tables the hot kernel uses.
//
// The reference tests a packed HSV word against packed bounds per pixel
// (detectHsvPixel, WSEQ:171-179): mask = cmpltu4(hsv, from) | cmpgtu4(hsv, to),
// det = (mask == expect).  The H, S and V lanes of that mask are independent,
// so det = hue_ok(H) && sat_ok(S) && val_ok(V) with
//   hue_ok(H) = ((H < from.H) || (H > to.H)) == expect.bit0
//   sat_ok(S) = !((S < from.S) || (S > to.S)),   val_ok likewise,
// which is exactly what the tables below enumerate.
#include <string.h>

#include "trik_hsv_internal.h"

namespace trik_hsv {

// (pack_range, WSEQ:425-445, is trik_hsv_internal.h's: the kernel that reads
// its ranges from device memory packs them with the same code)

static inline bool outside(uint32_t x, uint32_t lo, uint32_t hi) { return x < lo || x > hi; }

// Everything but the sat/val table: the LUTs and the per-value H, S, V tests
// (what the chroma-run builder and kernel read).
void compile_tables_head(const TRIK_VIDTRANSCODE_CV_InArgsAlg* ranges, int n, RangeTables* out) {
  memset(out->hue, 0, sizeof(out->hue));
  memset(out->smask, 0, sizeof(out->smask));
  memset(out->vmask, 0, sizeof(out->vmask));
  out->lut43[0] = 0;
  out->lut255[0] = 0;
  for (uint32_t i = 1; i < 256; ++i) {  // WSEQ:400-406
    out->lut43[i] = (uint16_t)((43u * 256u) / i);
    out->lut255[i] = (uint16_t)((255u * 256u) / i);
  }
  for (int t = 0; t < n; ++t) {
    const PackedRange p = pack_range(ranges[t]);
    const uint8_t bit = (uint8_t)(1u << t);
    const uint32_t fh = p.from & 0xFF, th = p.to & 0xFF;
    const uint32_t fs = (p.from >> 8) & 0xFF, ts = (p.to >> 8) & 0xFF;
    const uint32_t fv = (p.from >> 16) & 0xFF, tv = (p.to >> 16) & 0xFF;
    for (uint32_t h = 0; h < 256; ++h)
      if ((outside(h, fh, th) ? 1u : 0u) == (p.expect & 1u)) out->hue[h] |= bit;
    for (uint32_t x = 0; x < 256; ++x) {
      if (!outside(x, fs, ts)) out->smask[x] |= bit;
      if (!outside(x, fv, tv)) out->vmask[x] |= bit;
    }
  }
}

// The sat/val table sv[mx * 256 + mn] (compile_tables_head first: it reads
// lut255).  S = (LUT255[mx] * d) >> 8 with d = mx - mn does not fall as d
// grows, so the d with fs <= S <= ts form one interval [d_lo, d_hi]: solved
// per mx instead of testing every (mx, mn).
void compile_tables_sv(const TRIK_VIDTRANSCODE_CV_InArgsAlg* ranges, int n, RangeTables* out) {
  memset(out->sv, 0, sizeof(out->sv));
  const uint16_t* lut255 = out->lut255;
  for (int t = 0; t < n; ++t) {
    const PackedRange p = pack_range(ranges[t]);
    const uint8_t bit = (uint8_t)(1u << t);
    const uint32_t fs = (p.from >> 8) & 0xFF, ts = (p.to >> 8) & 0xFF;
    const uint32_t fv = (p.from >> 16) & 0xFF, tv = (p.to >> 16) & 0xFF;
    for (uint32_t mx = fv; mx <= tv && mx < 256; ++mx) {
      const uint32_t L = lut255[mx];
      uint32_t d_lo, d_hi;
      if (L == 0) {  // mx = 0: S = 0
        if (fs > 0) continue;
        d_lo = 0;
        d_hi = mx;
      } else {
        d_lo = (256u * fs + L - 1) / L;          // the least d with L d >= 256 fs
        d_hi = (256u * (ts + 1) - 1) / L;        // the largest d with L d < 256 (ts + 1)
        if (d_hi > mx) d_hi = mx;
      }
      uint8_t* row = out->sv + mx * 256;
      for (uint32_t d = d_lo; d <= d_hi; ++d) row[mx - d] |= bit;
    }
  }
}

void compile_tables(const TRIK_VIDTRANSCODE_CV_InArgsAlg* ranges, int n, RangeTables* out) {
  compile_tables_head(ranges, n, out);
  compile_tables_sv(ranges, n, out);
}

void compile_stripe_tables(const RangeTables& base, int n, StripeTables* out) {
  memset(out, 0, sizeof(*out));
  const uint8_t keep = (uint8_t)((1u << (n < 4 ? n : 4)) - 1u);
  for (int mx = 0; mx < 256; ++mx)
    for (int mn = 0; mn < 256; ++mn) out->sv[mx * kSvStride + mn] = base.sv[mx * 256 + mn] & keep;
  for (int i = 0; i < 256; ++i) {
    uint32_t spread = 0;
    for (int t = 0; t < n && t < 4; ++t) spread |= ((uint32_t)(base.hue[i] >> t) & 1u) << (8 * t);
    for (int c = 0; c < kHueCopies; ++c) out->hue[i * kHueCopies + c] = spread;
    for (int c = 0; c < kM43Copies; ++c) out->m43[i * kM43Copies + c] = base.lut43[i];
  }
}

int detect_mode(const RangeTables& t, int n) {
  const uint8_t all = (uint8_t)((1u << (n < 4 ? n : 4)) - 1u);
  if (n <= 0) return kDetectFull;
  for (int h = 0; h < 256; ++h)
    if ((t.hue[h] & all) != all) return kDetectFull;
  for (int x = 0; x < 256; ++x)
    if ((t.smask[x] & all) != all) return kDetectSV;
  return kDetectV;
}

void preview_maps(int width, int height, int out_w, int out_h, uint32_t* maps, int col_lo, int col_hi) {
  // WSEQ:371-387: shift = min(out/in) in double, maps truncate i * shift
  const double sw = width > 0 ? (double)out_w / width : 0.0;
  const double sh = height > 0 ? (double)out_h / height : 0.0;
  const double shift = sw < sh ? sw : sh;
  uint32_t* wi2wo = maps;
  uint32_t* hi2ho = wi2wo + width;
  int32_t* last_row = reinterpret_cast<int32_t*>(hi2ho + height);
  int32_t* last_col = last_row + out_h;
  for (int i = 0; i < width; ++i) wi2wo[i] = (uint32_t)(i * shift);
  for (int i = 0; i < height; ++i) hi2ho[i] = (uint32_t)(i * shift);
  for (int i = 0; i < out_h; ++i) last_row[i] = -1;
  for (int i = 0; i < out_w; ++i) last_col[i] = -1;
  // scan order: a later source row/column overwrites (proceedImageHsv)
  for (int i = 0; i < height; ++i)
    if (hi2ho[i] < (uint32_t)out_h) last_row[hi2ho[i]] = i;
  for (int i = 0; i < width; ++i)
    if (i >= col_lo && i <= col_hi && wi2wo[i] < (uint32_t)out_w) last_col[wi2wo[i]] = i;
}

// HSVtoRGB of the MxN sensor (MSEQ:480-517): h, s, v are float divisions
// widened to double, s is forced to 0 or 1, f, p, q, t are doubles, and the
// channels are truncated.  Contraction is off: fusing 1 - f * s into an FMA
// changes low bits, and with them a truncated channel.
static uint32_t mxn_hsv_to_rgb(int H, int S, int V) {
#pragma clang fp contract(off)
  double r = 0, g = 0, b = 0;
  const double h = (float)H / 255.0f;
  double s = (float)S / 255.0f;
  double v = (float)V / 255.0f;
  v = v < 0.2 ? 0 : v;
  s = s < 0.2 ? 0 : 1;
  const int i = (int)(h * 6);
  const double f = h * 6 - i;
  const double p = v * (1 - s);
  const double q = v * (1 - f * s);
  const double t = v * (1 - (1 - f) * s);
  switch (i % 6) {
    case 0: r = v; g = t; b = p; break;
    case 1: r = q; g = v; b = p; break;
    case 2: r = p; g = v; b = t; break;
    case 3: r = p; g = q; b = v; break;
    case 4: r = t; g = p; b = v; break;
    case 5: r = v; g = p; b = q; break;
  }
  const int ri = (int)(r * 255), gi = (int)(g * 255), bi = (int)(b * 255);
  return (uint32_t)((ri << 16) + (gi << 8) + bi);
}

const uint32_t* mxn_color_table() {
  struct Table {
    uint32_t c[kMxnColors];
    Table() {
      for (int i = 0; i < kMxnColors; ++i) c[i] = mxn_hsv_to_rgb(8 * (i >> 4), 64 * ((i >> 2) & 3), 64 * (i & 3));
    }
  };
  static const Table t;  // built once, on first use
  return t.c;
}

// ---------------------------------------------------------------------------
// The JPEG encoder's tables (JENC:244-315, 517-647): ITU-T T.81 Annex K.1
// quantisers and Annex K.3 Huffman tables, retyped from the standard.
// ---------------------------------------------------------------------------
namespace {

const uint8_t kJpegQLum[64] = {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,
                               14, 13, 16, 24, 40,  57,  69,  56,  14, 17, 22, 29, 51,  87,  80,  62,
                               18, 22, 37, 56, 68,  109, 103, 77,  24, 35, 55, 64, 81,  104, 113, 92,
                               49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
const uint8_t kJpegQChr[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99,
                               24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
                               99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
                               99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};
const uint8_t kJpegDcBits[2][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0},
                                    {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
const uint8_t kJpegAcBits[2][16] = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d},
                                    {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77}};
// HUFFVAL of the two AC tables: an irregular head, then runs r2..rA (or r1..rA)
const uint8_t kJpegAcLumHead[] = {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41,
                                  0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91,
                                  0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24,
                                  0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a};
const uint8_t kJpegAcLumRuns[][2] = {{0x25, 0x2a}, {0x34, 0x3a}, {0x43, 0x4a}, {0x53, 0x5a}, {0x63, 0x6a},
                                     {0x73, 0x7a}, {0x83, 0x8a}, {0x92, 0x9a}, {0xa2, 0xaa}, {0xb2, 0xba},
                                     {0xc2, 0xca}, {0xd2, 0xda}, {0xe1, 0xea}, {0xf1, 0xfa}};
const uint8_t kJpegAcChrHead[] = {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41,
                                  0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91,
                                  0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1,
                                  0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a};
const uint8_t kJpegAcChrRuns[][2] = {{0x26, 0x2a}, {0x35, 0x3a}, {0x43, 0x4a}, {0x53, 0x5a}, {0x63, 0x6a},
                                     {0x73, 0x7a}, {0x82, 0x8a}, {0x92, 0x9a}, {0xa2, 0xaa}, {0xb2, 0xba},
                                     {0xc2, 0xca}, {0xd2, 0xda}, {0xe2, 0xea}, {0xf2, 0xfa}};
// the eight AAN scale factors as the reference's decimal literals (JENC:207-210)
const double kJpegAasf[8] = {1.0, 1.387039845, 1.306562965, 1.175875602, 1.0, 0.785694958, 0.541196100, 0.275899379};

struct JpegStatic {
  JpegHuffman huff;
  uint8_t ac_vals[2][162];
  uint8_t zz[64];  // zz[natural index] = position in the zigzag scan
  JpegStatic() {
    memset(&huff, 0, sizeof huff);
    int n = 0;
    for (uint8_t v : kJpegAcLumHead) ac_vals[0][n++] = v;
    for (const auto& r : kJpegAcLumRuns)
      for (int v = r[0]; v <= r[1]; ++v) ac_vals[0][n++] = (uint8_t)v;
    n = 0;
    for (uint8_t v : kJpegAcChrHead) ac_vals[1][n++] = v;
    for (const auto& r : kJpegAcChrRuns)
      for (int v = r[0]; v <= r[1]; ++v) ac_vals[1][n++] = (uint8_t)v;
    for (int t = 0; t < 2; ++t) {  // computeHuffmanTbl, JENC:286-307
      int code = 0, pos = 0;
      for (int k = 1; k <= 16; ++k) {
        for (int j = 0; j < kJpegDcBits[t][k - 1]; ++j, ++pos, ++code) {
          huff.dc_code[t][pos] = (uint16_t)code;  // the DC symbols are 0..11 in order
          huff.dc_len[t][pos] = (uint8_t)k;
        }
        code *= 2;
      }
      code = 0; pos = 0;
      for (int k = 1; k <= 16; ++k) {
        for (int j = 0; j < kJpegAcBits[t][k - 1]; ++j, ++pos, ++code) {
          huff.ac_code[t][ac_vals[t][pos]] = (uint16_t)code;
          huff.ac_len[t][ac_vals[t][pos]] = (uint8_t)k;
        }
        code *= 2;
      }
    }
    int r = 0, c = 0;  // the zigzag walk of T.81 figure A.6
    for (int k = 0; k < 64; ++k) {
      zz[8 * r + c] = (uint8_t)k;
      if (((r + c) & 1) == 0) {
        if (c == 7) ++r; else if (r == 0) ++c; else { --r; ++c; }
      } else {
        if (r == 7) ++c; else if (c == 0) ++r; else { ++r; --c; }
      }
    }
  }
};
const JpegStatic& jpeg_static() {
  static const JpegStatic t;  // built once, on first use
  return t;
}

}  // namespace

const JpegHuffman* jpeg_huffman() { return &jpeg_static().huff; }

void jpeg_quant_tables(int quality, uint8_t* lum, uint8_t* chr) {  // JENC:244-267, 771-786
  const int q = quality <= 0 ? 1 : (quality > 100 ? 100 : quality);
  const int sf = q < 50 ? 5000 / q : 200 - q * 2;
  for (int i = 0; i < 64; ++i) {
    const int l = (kJpegQLum[i] * sf + 50) / 100, c = (kJpegQChr[i] * sf + 50) / 100;
    lum[i] = (uint8_t)(l < 1 ? 1 : (l > 255 ? 255 : l));
    chr[i] = (uint8_t)(c < 1 ? 1 : (c > 255 ? 255 : c));
  }
}

// fdtbl of JENC:268-278: each product rounded on its own, left to right
void jpeg_divisors(int quality, JpegDivisors& d) {
#pragma clang fp contract(off)
  uint8_t q[2][64];
  jpeg_quant_tables(quality, q[0], q[1]);
  for (int t = 0; t < 2; ++t)
    for (int row = 0; row < 8; ++row)
      for (int col = 0; col < 8; ++col) {
        const double a = (double)q[t][8 * row + col] * kJpegAasf[row];
        const double b = a * kJpegAasf[col];
        d.fd[t][8 * row + col] = 1.0 / (b * 8.0);
      }
}

// SOI, APP0, DQT, SOF0, DHT, SOS (JENC:517-647, 811-817)
void jpeg_header(int quality, bool bw, int width, int height, JpegHeader& hd) {
  const JpegStatic& st = jpeg_static();
  uint8_t q[2][64];
  jpeg_quant_tables(quality, q[0], q[1]);
  int n = 0;
  uint8_t* o = hd.bytes;
  auto byte = [&](int v) { o[n++] = (uint8_t)v; };
  auto word = [&](int v) { byte(v >> 8); byte(v); };
  word(0xFFD8);
  word(0xFFE0); word(16);
  for (char ch : {'J', 'F', 'I', 'F', '\0'}) byte(ch);
  byte(1); byte(1); byte(0); word(1); word(1); byte(0); byte(0);
  word(0xFFDB); word(bw ? 67 : 132);
  for (int t = 0; t < (bw ? 1 : 2); ++t) {  // the DQT carries the quantisers in zigzag order
    byte(t);
    uint8_t z[64];
    for (int i = 0; i < 64; ++i) z[st.zz[i]] = q[t][i];
    for (int i = 0; i < 64; ++i) byte(z[i]);
  }
  word(0xFFC0); word(bw ? 11 : 17); byte(8); word(height); word(width);
  byte(bw ? 1 : 3);
  byte(1); byte(0x11); byte(0);
  if (!bw) { byte(2); byte(0x11); byte(1); byte(3); byte(0x11); byte(1); }
  word(0xFFC4); word(bw ? 0xD2 : 0x01A2);
  for (int t = 0; t < (bw ? 1 : 2); ++t) {
    byte(t);
    for (int i = 0; i < 16; ++i) byte(kJpegDcBits[t][i]);
    for (int i = 0; i < 12; ++i) byte(i);
    byte(0x10 | t);
    for (int i = 0; i < 16; ++i) byte(kJpegAcBits[t][i]);
    for (int i = 0; i < 162; ++i) byte(st.ac_vals[t][i]);
  }
  word(0xFFDA);
  if (bw) { word(8); byte(1); byte(1); byte(0); }
  else { word(12); byte(3); byte(1); byte(0); byte(2); byte(0x11); byte(3); byte(0x11); }
  byte(0); byte(0x3F); byte(0);
  hd.size = n;
}

void auto_range_zone(int width, int height, int32_t& c_lo, int32_t& c_hi, int32_t& r_lo, int32_t& r_hi) {
  // HsvRangeDetector::initImg (cv_hsv_range_detector.hpp:88-108), zone scale 6
  // (WSEQ:32): uint16_t fields, so differences wrap modulo 2^16.
  const uint16_t h_height = (uint16_t)((uint32_t)height / 2);
  const uint16_t h_width = (uint16_t)((uint32_t)width / 2);
  const uint16_t step = (uint16_t)((uint32_t)height / 6);
  c_lo = (uint16_t)(h_width - step);
  c_hi = (uint16_t)(h_width + step);
  r_lo = (uint16_t)(h_height - step);
  r_hi = (uint16_t)(h_height + step);
}

std::string auto_exact_error(int kind, int layout, int64_t width, int64_t height) {
  if (kind != TRIK_HSV_AUTO_OV7670_OBJECT && kind != TRIK_HSV_AUTO_OV7670_LINE && kind != TRIK_HSV_AUTO_WEBCAM_LINE)
    return "auto range: unknown kind " + std::to_string(kind);
  if (layout != (kind == TRIK_HSV_AUTO_WEBCAM_LINE ? TRIK_HSV_LAYOUT_YUYV : TRIK_HSV_LAYOUT_OV7670))
    return kind == TRIK_HSV_AUTO_WEBCAM_LINE ? "auto range: the webcam line kind takes the YUYV layout (YUV422)"
                                             : "auto range: the ov7670 kinds take the ov7670 layout (YUV422P)";
  if (width > TRIK_HSV_AUTO_MAX_SIDE || height > TRIK_HSV_AUTO_MAX_SIDE)
    return "auto range: need width, height <= 2048";
  return "";
}

void auto_exact_zone(AutoExactArgs& a) {
  if (a.kind == TRIK_HSV_AUTO_OV7670_OBJECT) {  // ODET:156-175, plain int bounds, zone scale 6 (OSEQ)
    const int hh = a.height / 2, hw = a.width / 2, step = a.height / 6;
    a.pc_lo = hw - step; a.pc_hi = hw + step;
    a.pr_lo = hh - step; a.pr_hi = hh + step;
    a.nc_lo = hw - 2 * step; a.nc_hi = hw + 2 * step;
    a.nr_lo = hh - 2 * step; a.nr_hi = hh + 2 * step;
    return;
  }
  // LDET:165-187 with step 40 (LSEQ:430): uint16_t fields, so the bounds of a
  // narrow frame wrap modulo 2^16; the comparisons then promote them to int
  const uint16_t h_width = (uint16_t)(a.width / 2), step = 40;
  const uint16_t left_p = (uint16_t)(h_width - step), right_p = (uint16_t)(h_width + step);
  a.pc_lo = left_p;
  a.pc_hi = right_p;
  a.nc_lo = (uint16_t)(left_p - step);
  a.nc_hi = (uint16_t)(right_p + step);
  a.pr_lo = -1;  // every row
  a.pr_hi = a.height;
  a.nr_lo = INT32_MIN;  // no row test
  a.nr_hi = INT32_MAX;
}

}  // namespace trik_hsv
