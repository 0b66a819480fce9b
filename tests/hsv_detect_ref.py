"""HsvRangeDetector::detect (the webcam object sensor's autoDetectHsv,
cv_hsv_range_detector.hpp:79-198) restated in numpy over the oracle's
(Y, U, V) -> HSV table.  Test code, not product: the reference that
trik_hsv_batch_auto_range's kernels are compared with, frame by frame, where
oracle.run would be too slow or where a claim needs an altered zone.

  * The zone is strict and comes from uint16 arithmetic: step = h / 6,
    h/2 - step < row < h/2 + step, w/2 - step < col < w/2 + step.
  * Per channel the winner is, among the values at the maximum count, the one
    whose last occurrence in scan order comes earliest (the sequential strict
    '>' arg-max of the reference); an empty zone leaves the winners 0.
  * Output: (uint16)(H x (double)1.4f), 15, (uint16)(S x (double)0.39f), 30,
    the same for V, 30.

test_hsv_detect_cpu.py holds detect() to oracle.run(auto_detect=True) on a
sweep of geometries, and small_zone_winners() to detect()."""
import numpy as np

LAYOUT_YUYV, LAYOUT_OV7670 = 0, 1
K14 = np.float64(np.float32(1.4))
K39 = np.float64(np.float32(0.39))
# the scaled output of every channel value
HUE_OUT = (np.arange(256) * K14).astype(np.uint16).astype(np.int64)
SV_OUT = (np.arange(256) * K39).astype(np.uint16).astype(np.int64)


def zone(w, h):
    """(r0, r1, c0, c1): the zone's rows [r0, r1) and columns [c0, c1), clipped
    to the frame; empty when r0 >= r1 or c0 >= c1 (step = 0, or w/2 < step:
    the uint16 difference wraps)."""
    hw, hh, step = (w // 2) & 0xFFFF, (h // 2) & 0xFFFF, (h // 6) & 0xFFFF
    c_lo, c_hi = (hw - step) & 0xFFFF, (hw + step) & 0xFFFF
    r_lo, r_hi = (hh - step) & 0xFFFF, (hh + step) & 0xFFFF
    return r_lo + 1, min(r_hi, h), c_lo + 1, min(c_hi, w)


def pixel_yuv(frame, w, h, ll, layout):
    """Y, U, V [h, w] int64 of one frame's bytes."""
    fr = np.asarray(frame, np.uint8)
    if layout == LAYOUT_YUYV:
        px = fr[: h * ll].reshape(h, ll)[:, : 2 * w].reshape(h, w // 2, 4).astype(np.int64)
        Y = np.stack([px[..., 0], px[..., 2]], -1).reshape(h, w)
        U, V = np.repeat(px[..., 1], 2, axis=1), np.repeat(px[..., 3], 2, axis=1)
    else:
        Y = fr[: h * ll].reshape(h, ll)[:, :w].astype(np.int64)
        c = fr[h * ll: 2 * h * ll].reshape(h, ll)[:, :w].astype(np.int64)
        V, U = np.repeat(c[:, 0::2], 2, axis=1), np.repeat(c[:, 1::2], 2, axis=1)
    return Y, U, V


def pixel_hsv(table, frame, w, h, ll, layout):
    """[3, h, w] int64: H, S, V of every pixel, from the oracle's table."""
    Y, U, V = pixel_yuv(frame, w, h, ll, layout)
    e = table[Y | (U << 8) | (V << 16)] & 0xFFFFFFFF
    return np.stack([(e >> sh) & 0xFF for sh in (0, 8, 16)]).astype(np.int64)


def _cut(plane, zn, w, h):
    r0, r1, c0, c1 = zn
    r0, r1, c0, c1 = max(r0, 0), min(r1, h), max(c0, 0), min(c1, w)
    if r0 >= r1 or c0 >= c1:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    pos = (np.arange(r0, r1)[:, None] * w + np.arange(c0, c1)[None, :]).reshape(-1)
    return plane[r0:r1, c0:c1].reshape(-1), pos


def winner(vals, pos=None, last_vals=None, last_pos=None):
    """One channel's winner: `vals` in scan order (at scan positions `pos`).
    Returns (winner, tied values).  last_vals / last_pos: the pixels whose
    last occurrences decide a tie, where they are not the counted ones."""
    if vals.size == 0:
        return 0, np.zeros(0, np.int64)
    pos = np.arange(vals.size) if pos is None else pos
    if last_vals is None:
        last_vals, last_pos = vals, pos
    cnt = np.bincount(vals, minlength=256)
    tied = np.flatnonzero(cnt == cnt.max())
    last = np.full(256, -1, np.int64)
    np.maximum.at(last, last_vals, last_pos)
    return int(tied[np.argmin(last[tied])]), tied


def scale(wins):
    return [int(HUE_OUT[wins[0]]), 15, int(SV_OUT[wins[1]]), 30, int(SV_OUT[wins[2]]), 30]


def detect_hsv(hsv3, zn=None, last_zone=None, want_tied=False):
    """The six outputs of a [3, h, w] HSV image over zone `zn` (default: the
    detector's own).  With last_zone, counts come from `zn` and the last
    occurrences from `last_zone`: what a kernel would give that counted the
    right pixels and looked for the tied values' last occurrences in others."""
    _, h, w = hsv3.shape
    zn = zone(w, h) if zn is None else zn
    wins, tied = [], []
    for k in range(3):
        v, p = _cut(hsv3[k], zn, w, h)
        lv, lp = _cut(hsv3[k], last_zone, w, h) if last_zone is not None else (None, None)
        win, t = winner(v, p, lv, lp)
        wins.append(win)
        tied.append(t)
    return (scale(wins), tied) if want_tied else scale(wins)


def detect(table, frame, w, h, ll, layout, zn=None, last_zone=None):
    return detect_hsv(pixel_hsv(table, frame, w, h, ll, layout), zn, last_zone)


def alter(zn, what):
    """The zone widened (+) or narrowed (-) by one column or row on one side:
    what in 'L+', 'R+', 'T+', 'B+', 'L-', 'R-', 'T-', 'B-'."""
    r0, r1, c0, c1 = zn
    d = 1 if what[1] == "+" else -1
    return {"L": (r0, r1, c0 - d, c1), "R": (r0, r1, c0, c1 + d),
            "T": (r0 - d, r1, c0, c1), "B": (r0, r1 + d, c0, c1)}[what[0]]


def small_zone_winners(v):
    """winner() for many small zones at once: v is a torch integer tensor
    [N, P], P <= 32 zone pixels of one channel in scan order; returns [N].
    (Pixel i's count and last occurrence by comparing it with every pixel;
    the winner has the largest count and, among those, the earliest last
    occurrence.)"""
    import torch

    n, p = v.shape
    assert 0 < p <= 32
    eq = v[:, :, None] == v[:, None, :]
    cnt = eq.sum(2)
    idx = torch.arange(p, device=v.device)
    last = (eq * idx[None, None, :]).amax(2)
    key = cnt * 32 + (31 - last)
    return v.gather(1, key.argmax(1, keepdim=True))[:, 0]
