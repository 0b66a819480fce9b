"""The two line sensors' RGB565X previews, restated plainly in numpy over the
oracle's per-pixel table (oracle.yuv_table: index Y | U<<8 | V<<16, the RGB in
the high half, the HSV word in the low half with its V byte in bits 16-23) --
test code, not product.

ov7670 line sensor (LSEQ = trik/ov7670/line_sensor/.../cv_line_detector_seqpass.hpp,
283-291 and 419-474): source columns 5..W-5 write through the truncated scale
maps (preview_ref.maps), the last writer wins; a pixel whose V lies in the
scaled range is 0x00ffff, any other its colour; then four magenta thin lines
(columns W/2 -+ 40, W/2 -+ 80 over every row), two red band lines (rows H/2 and
H/2 + 80 over every column) and, with more than 10 points, the red target line
(columns cx - 1 .. cx + 1 over every row), every point clamped to the frame and
then mapped (drawOutputPixelBound).  Webcam line sensor on packed YUYV (LSEQW,
232-269 and 396-413): every column writes; thin lines and target line, no band
lines.

The target line comes from caller-given sums (points, sum_x, anything): their
low words, cx the unsigned 32-bit quotient read as int32 (line_ref.center).
Every function takes a batch: frames uint8 [n, frame bytes], one (val_from,
val_to) pair and one sums row per frame.  tests/test_line_frame_ranges_preview_cpu.py
holds this module to oracle.line_run and oracle.wline_run byte for byte.
"""
import numpy as np

import line_ref
import preview_ref
from preview_ref import LAYOUT_OV7670, LAYOUT_YUYV

MAGENTA, RED, DETECTED = 0xff00ff, 0xff0000, 0x00ffff
STEP = 40


def window(w, layout):
    """The source columns that write, inclusive (LSEQ:288; LSEQW: all)."""
    return (5, w - 5) if layout == LAYOUT_OV7670 else (0, w - 1)


def last_writers(w, h, ow, oh, layout):
    """preview_ref.last_writers with the layout's column window: the source row
    / column that writes each output row / column last, -1 where none does."""
    wi2wo, hi2ho = preview_ref.maps(w, h, ow, oh) if w > 0 and h > 0 else ([], [])
    lo, hi = window(w, layout)
    last_row, last_col = [-1] * oh, [-1] * ow
    for i in range(h):
        if hi2ho[i] < oh:
            last_row[hi2ho[i]] = i
    for i in range(w):
        if lo <= i <= hi and wi2wo[i] < ow:
            last_col[wi2wo[i]] = i
    return last_row, last_col


def yuv_index(frames, w, h, ll, layout, rows, cols):
    """preview_ref.yuv_index over a batch: int64 [n, len(rows), len(cols)]."""
    fr = np.asarray(frames, np.uint8)
    n = fr.shape[0]
    r = np.asarray(rows, np.int64)[:, None]
    c = np.asarray(cols, np.int64)[None, :]
    if layout == LAYOUT_YUYV:
        img = fr[:, :h * ll].reshape(n, h, ll)
        Y, U, V = img[:, r, 2 * c], img[:, r, 4 * (c >> 1) + 1], img[:, r, 4 * (c >> 1) + 3]
    else:
        img, chroma = fr[:, :h * ll].reshape(n, h, ll), fr[:, h * ll:2 * h * ll].reshape(n, h, ll)
        Y, V, U = img[:, r, c], chroma[:, r, c & ~1], chroma[:, r, c | 1]
    return Y.astype(np.int64) | (U.astype(np.int64) << 8) | (V.astype(np.int64) << 16)


def sampled(table, frames, w, h, ll, layout, ow, oh):
    """What no range changes: (orow, ocol, colour, val) -- the written output
    rows and columns, and of the source pixel each (row, column) keeps its
    RGB565X colour and its V byte, int64 [n, len(orow), len(ocol)]."""
    last_row, last_col = last_writers(w, h, ow, oh, layout)
    orow = [i for i in range(oh) if last_row[i] >= 0]
    ocol = [i for i in range(ow) if last_col[i] >= 0]
    idx = yuv_index(frames, w, h, ll, layout, [last_row[i] for i in orow], [last_col[i] for i in ocol])
    word = table[idx]
    colour = preview_ref.px565((word >> np.uint64(32)).astype(np.int64))
    val = (word >> np.uint64(16)).astype(np.int64) & 255
    return orow, ocol, colour, val


def bodies(smp, ow, oh, oll, pairs):
    """uint8 [n, oh, oll]: the previews before any overlay, frame f under
    pairs[f] = (val_from, val_to) in percent (line_ref.scale_val); an empty
    scaled range detects nothing."""
    orow, ocol, colour, val = smp
    lo = np.array([line_ref.scale_val(p[0]) for p in pairs], np.int64)[:, None, None]
    hi = np.array([line_ref.scale_val(p[1]) for p in pairs], np.int64)[:, None, None]
    v = np.where((val >= lo) & (val <= hi), preview_ref.px565(DETECTED), colour)
    out = np.zeros((len(pairs), oh, oll), np.uint8)
    ro, co = np.asarray(orow, np.int64)[:, None], np.asarray(ocol, np.int64)[None, :]
    out[:, ro, 2 * co] = v & 255
    out[:, ro, 2 * co + 1] = v >> 8
    return out


def target_column(sums):
    """None unless the low word of points is above 10; else cx (line_ref.center)."""
    n = int(sums[0]) & line_ref.M32
    return line_ref.center(n, int(sums[1])) if n > 10 else None


def overlay(p, w, h, ow, oh, layout, sums):
    """Draws the thin, band and target lines into the previews p (uint8 [n, oh,
    oll], changed in place), the target line of preview f from sums[f].  Every
    point goes through clamp-then-map; a whole line's points are drawn at once
    (one colour per phase, and red is drawn after magenta)."""
    if w <= 0 or h <= 0:
        return p
    wi2wo, hi2ho = (np.asarray(m, np.int64) for m in preview_ref.maps(w, h, ow, oh))

    def draw(f, cols, rows, rgb):
        oc = wi2wo[np.clip(np.asarray(cols, np.int64), 0, w - 1)][None, :]
        orow = hi2ho[np.clip(np.asarray(rows, np.int64), 0, h - 1)][:, None]
        v = preview_ref.px565(rgb)
        p[f, orow, 2 * oc] = v & 255
        p[f, orow, 2 * oc + 1] = v >> 8

    hw, hh = w // 2, h // 2
    every = slice(None)
    draw(every, [hw - STEP, hw + STEP, hw - 2 * STEP, hw + 2 * STEP], range(h), MAGENTA)
    if layout == LAYOUT_OV7670:
        draw(every, range(w), [hh, hh + 2 * STEP], RED)
    for f in range(p.shape[0]):
        cx = target_column(sums[f])
        if cx is not None:
            draw(f, [cx - 1, cx, cx + 1], range(h), RED)
    return p


def previews(table, frames, w, h, ll, layout, ow, oh, oll, pairs, sums, smp=None):
    """uint8 [n, oh * oll]: preview f of frames[f] under pairs[f] with the
    target line of sums[f]; `smp`: sampled() of the same frames, kept by a
    caller that asks for several range sets."""
    n = len(pairs)
    if w <= 0 or h <= 0:
        return np.zeros((n, oh * oll), np.uint8)
    smp = sampled(table, np.asarray(frames).reshape(n, -1), w, h, ll, layout, ow, oh) if smp is None else smp
    return overlay(bodies(smp, ow, oh, oll, pairs), w, h, ow, oh, layout, sums).reshape(n, -1)
