"""The object sensors' RGB565X preview, restated plainly -- test code, not
product.

Two pieces of the reference as oracle/trik_oracle.c:trik_oracle_run restates
them (WSEQ:66-166, 371-387, 471-494): the truncated scale maps, and what is
drawn after the body -- eight magenta guide lines, then the yellow target
circle around the centre the sums give.  The body itself (proceedImageHsv's
per-pixel writes, WSEQ:316-354) comes from the oracle's 2^24-entry table and a
detection mask of the oracle's.

This module is the expectation wherever the caller's sums are not the frame's
own (tests/test_gpu_preview_shapes.py, part C) and wherever oracle.run per
frame would be too slow (part B).  tests/test_preview_cpu.py holds it to
oracle.run byte for byte.
"""
import numpy as np

LAYOUT_YUYV, LAYOUT_OV7670 = 0, 1
MAGENTA, YELLOW, DETECTED = 0xff00ff, 0xffff00, 0x00ffff


def maps(w, h, ow, oh):
    """(wi2wo, hi2ho), WSEQ:371-387: shift = min(ow / w, oh / h) in double, each
    entry the truncated product."""
    shift = min(ow / w, oh / h)
    return [int(i * shift) for i in range(w)], [int(i * shift) for i in range(h)]


def px565(rgb):
    """writeOutputPixel, WSEQ:66-70: 0x00RRGGBB -> B5 G6 R5, R in the low bits."""
    return ((rgb >> 19) & 0x001f) | ((rgb >> 5) & 0x07e0) | ((rgb << 8) & 0xf800)


class Canvas:
    """One preview (uint8 [oh, oll], changed in place) under the frame's maps."""

    def __init__(self, p, w, h, ow, oh):
        self.p, self.w, self.h = p, w, h
        self.wi2wo, self.hi2ho = maps(w, h, ow, oh)

    def draw_bound(self, col, row, rgb):
        """drawOutputPixelBound, WSEQ:72-89: the source point clamped to the
        frame, then mapped."""
        sc = min(max(col, 0), self.w - 1)
        sr = min(max(row, 0), self.h - 1)
        v = px565(rgb)
        self.p[self.hi2ho[sr], 2 * self.wi2wo[sc]] = v & 255
        self.p[self.hi2ho[sr], 2 * self.wi2wo[sc] + 1] = v >> 8

    def guides(self):
        """WSEQ:136-166, 471-485: four vertical, then four horizontal lines of
        2 x 100 points around the centre, step = h // 6."""
        step, hh, hw = self.h // 6, self.h // 2, self.w // 2
        for off in (-2, -1, 1, 2):
            for adj in range(100):
                self.draw_bound(hw + off * step, hh - adj, MAGENTA)
                self.draw_bound(hw + off * step, hh + adj, MAGENTA)
        for off in (-2, -1, 1, 2):
            for adj in range(100):
                self.draw_bound(hw - adj, hh + off * step, MAGENTA)
                self.draw_bound(hw + adj, hh + off * step, MAGENTA)

    def circle(self, cx, cy, radius, rgb=YELLOW):
        for col, row in circle_points(cx, cy, radius):
            self.draw_bound(col, row, rgb)


def circle_points(cx, cy, radius):
    """drawOutputCircle, WSEQ:91-134: the midpoint circle's source points in
    drawing order, before any clamp."""
    err, err_y, err_x, x, y = 1 - radius, 1, -2 * radius, radius, 0
    out = [(cx, cy + radius), (cx, cy - radius), (cx + radius, cy), (cx - radius, cy)]
    while y < x:
        if err >= 0:
            x -= 1
            err_x += 2
            err += err_x
        y += 1
        err_y += 2
        err += err_y
        out += [(cx + px, cy + py) for px, py in ((x, y), (x, -y), (-x, y), (-x, -y), (y, x), (y, -x), (-y, x), (-y, -x))]
    return out


def _i32(v):
    v &= 0xFFFFFFFF
    return v - (1 << 32) if v >= 1 << 31 else v


def centre_radius(sums):
    """WSEQ:486-490 on (points, sum_x, sum_y): None without points; else
    (cx, cy, radius), the centre by unsigned 32-bit division of the sums' low
    words (the quotient read as int32), the radius in IEEE float32."""
    n = int(sums[0]) & 0xFFFFFFFF
    if n == 0:
        return None
    cx = _i32((int(sums[1]) & 0xFFFFFFFF) // n)
    cy = _i32((int(sums[2]) & 0xFFFFFFFF) // n)
    radius = int(np.ceil(np.sqrt(np.float32(n) / np.float32(3.1415927))))
    return cx, cy, radius


def last_writers(w, h, ow, oh):
    """(last_row[oh], last_col[ow]): the source row / column that writes each
    output row / column last when the frame is walked in scan order, -1 where
    none does."""
    wi2wo, hi2ho = maps(w, h, ow, oh)
    last_row, last_col = [-1] * oh, [-1] * ow
    for i in range(h):
        if hi2ho[i] < oh:
            last_row[hi2ho[i]] = i
    for i in range(w):
        if wi2wo[i] < ow:
            last_col[wi2wo[i]] = i
    return last_row, last_col


def yuv_index(frame, w, h, ll, layout, rows, cols):
    """Y | U << 8 | V << 16 (the oracle table's index) of the source pixels
    rows x cols (int arrays) -> int64 [len(rows), len(cols)].  Packed YUYV
    (WSEQ:262-270), or the ov7670 planes (OSEQ:360-373: V the even chroma
    byte, U the odd one)."""
    fr = np.asarray(frame, np.uint8)
    r = np.asarray(rows, np.int64)[:, None]
    c = np.asarray(cols, np.int64)[None, :]
    if layout == LAYOUT_YUYV:
        img = fr[:h * ll].reshape(h, ll)
        Y, U, V = img[r, 2 * c], img[r, 4 * (c >> 1) + 1], img[r, 4 * (c >> 1) + 3]
    else:
        img, chroma = fr[:h * ll].reshape(h, ll), fr[h * ll:2 * h * ll].reshape(h, ll)
        Y, V, U = img[r, c], chroma[r, c & ~1], chroma[r, c | 1]
    return Y.astype(np.int64) | (U.astype(np.int64) << 8) | (V.astype(np.int64) << 16)


def body(table, mask, frame, w, h, ll, layout, ow, oh, oll):
    """The preview before any overlay, uint8 [oh, oll]: every source pixel
    written through the maps in scan order, the last writer wins (the maps do
    not fall, so output pixel (r', c') keeps source pixel (last_row[r'],
    last_col[c'])); a detected pixel is 0x00ffff, any other the table's RGB;
    the rest is zero.  `mask`: the detection of bit 0, either per pixel (uint8
    [h, w], oracle.frame's) or per triple (2^24 entries, indexed as the
    table)."""
    last_row, last_col = last_writers(w, h, ow, oh)
    orow = [i for i in range(oh) if last_row[i] >= 0]
    ocol = [i for i in range(ow) if last_col[i] >= 0]
    rows, cols = [last_row[i] for i in orow], [last_col[i] for i in ocol]
    idx = yuv_index(frame, w, h, ll, layout, rows, cols)
    mask = np.asarray(mask)
    if mask.ndim == 2:
        det = mask[np.asarray(rows)[:, None], np.asarray(cols)[None, :]] & 1
    else:
        det = mask[idx] & 1
    rgb = np.where(det != 0, np.uint64(DETECTED), table[idx] >> np.uint64(32)).astype(np.int64)
    v = px565(rgb)
    out = np.zeros((oh, oll), np.uint8)
    ro, co = np.asarray(orow, np.int64)[:, None], np.asarray(ocol, np.int64)[None, :]
    out[ro, 2 * co] = v & 255
    out[ro, 2 * co + 1] = v >> 8
    return out


def preview(body_px, w, h, ow, oh, oll, sums):
    """Body, then the guide lines, then the circle of `sums` (points, sum_x,
    sum_y): a new uint8 [oh, oll]."""
    p = np.array(body_px, np.uint8).reshape(oh, oll)
    cv = Canvas(p, w, h, ow, oh)
    cv.guides()
    t = centre_radius(sums)
    if t is not None:
        cv.circle(*t)
    return p


def colour_pixels(p, ow, rgb):
    """The output pixels (row, column) of preview p that hold colour rgb."""
    p = np.asarray(p)
    v = p[:, 0:2 * ow:2].astype(np.int64) | (p[:, 1:2 * ow:2].astype(np.int64) << 8)
    return set(map(tuple, np.argwhere(v == px565(rgb)).tolist()))
