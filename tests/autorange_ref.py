"""A plain restatement of the three annealing range detectors' deterministic
parts, and of the exact search that replaces their annealing:
  ODET   trik/ov7670/object_sensor/include/internal/cv_hsv_range_detector.hpp
  LDET   trik/ov7670/line_sensor/include/internal/cv_hsv_range_detector.hpp
  LDETW  trik/webcam/line_sensor/include/internal/cv_hsv_range_detector.hpp
in numpy over the oracle's per-pixel table (oracle.yuv_table: index
Y | U<<8 | V<<16, the HSV word V<<16 | S<<8 | H in the low half).

The reference's own result cannot serve as an expectation: its detectors are
simulated annealings seeded by srand(time(NULL)), so ref_lib.BlobSensor.run(...,
auto_detect=True) and the line drivers return clock-seeded values.  This
restatement is the contract, as edge_ref.py is for the edge-line sensor:
  * histogram_loop() is the detectors' clustering loop as the sequential double
    loop it is (ODET:200-227, LDET:215-240); histogram() is the same in numpy --
    the running value of every cell at every event in raster order, not the
    kernel's per-row rule -- and tests/test_autorange_cpu.py holds the two
    together;
  * search() is a brute force over the stated domain with the stated tie rule;
  * range_of() is the output scaling in numpy.float32 (ODET:271-293,
    LDET:280-303, LDETW:280-303).
Test code, with no restriction on the geometry."""
import numpy as np

OBJECT, LINE, WLINE = 0, 1, 2  # TRIK_HSV_AUTO_OV7670_OBJECT, _OV7670_LINE, _WEBCAM_LINE
LAYOUT_YUYV, LAYOUT_OV7670 = 0, 1


def layout_of(kind):
    return LAYOUT_YUYV if kind == WLINE else LAYOUT_OV7670


def bins_of(kind):
    return 1024 if kind == OBJECT else 256


def k0_of(kind):
    return 2 if kind == OBJECT else 1


def frame_bytes(kind, height, line_length):
    return height * line_length * (2 if layout_of(kind) == LAYOUT_OV7670 else 1)


def cells(table, frame, width, height, line_length, kind):
    """int64 [height, width]: every pixel's histogram bin, (H >> 3) * 32 +
    (S >> 3) for the object kind, V for the line kinds."""
    fr = np.asarray(frame, np.uint8)
    if layout_of(kind) == LAYOUT_OV7670:  # luma plane, then chroma with V at even and U at odd bytes
        y = fr[:height * line_length].reshape(height, line_length)[:, :width].astype(np.int64)
        c = fr[height * line_length:2 * height * line_length].reshape(height, line_length)[:, :width]
        v = np.repeat(c[:, 0::2].astype(np.int64), 2, axis=1)
        u = np.repeat(c[:, 1::2].astype(np.int64), 2, axis=1)
    else:  # Y0 U Y1 V
        p = fr[:height * line_length].reshape(height, line_length)[:, :2 * width].astype(np.int64)
        y = p[:, 0::2]
        u = np.repeat(p[:, 1::4], 2, axis=1)
        v = np.repeat(p[:, 3::4], 2, axis=1)
    hsv = table[y | (u << 8) | (v << 16)].astype(np.int64)
    if kind == OBJECT:
        return (((hsv & 255) >> 3) << 5) | (((hsv >> 8) & 255) >> 3)
    return (hsv >> 16) & 255


def zones(kind, width, height):
    """(positive, negative) bool [height, width], by the detectors' own
    comparisons: plain ints for the object kind (ODET:156-175, 209, 222, the
    "wrong condition" as written), uint16 ROI fields promoted to int for the
    line kinds (LDET:165-187, 225-236, step 40)."""
    col = np.arange(width, dtype=np.int64)[None, :]
    row = np.arange(height, dtype=np.int64)[:, None]
    if kind == OBJECT:
        hh, hw, step = height // 2, width // 2, height // 6
        pos = (hw - step < col) & (col < hw + step) & (hh - step < row) & (row < hh + step)
        neg = (hw + 2 * step < col) | (col < hw - 2 * step) | (hh + 2 * step < row) | (row < hh - 2 * step)
    else:
        hw = (width // 2) & 0xFFFF
        left_p, right_p = (hw - 40) & 0xFFFF, (hw + 40) & 0xFFFF
        left_n, right_n = (left_p - 40) & 0xFFFF, (right_p + 40) & 0xFFFF
        pos = (left_p < col) & (right_p > col) & (row >= 0)
        neg = ((left_n > col) | (right_n < col)) & (row >= 0)
    return pos, neg & ~pos


def histogram_loop(cell, pos, neg, bins, trace=None):
    """The clustering loop, pixel by pixel: (final histogram int64 [bins],
    start cell, max_value).  trace, a list, receives (value, cell, row, col)
    of every positive event."""
    hist = [0] * bins
    start, max_value = 0, 0
    height, width = cell.shape
    cl, ps, ng = cell.tolist(), pos.tolist(), neg.tolist()
    for r in range(height):
        for c in range(width):
            k = cl[r][c]
            if ps[r][c]:
                hist[k] += 1
                if trace is not None:
                    trace.append((hist[k], k, r, c))
                if hist[k] > max_value:
                    max_value, start = hist[k], k
            elif ng[r][c]:
                hist[k] -= 2
    return np.array(hist, np.int64), start, max_value


def histogram(cell, pos, neg, bins):
    """histogram_loop in numpy: the events sorted by (cell, raster index), each
    cell's running value by a grouped cumulative sum, then the first positive
    event in raster order whose running value equals the largest one (> 0)."""
    c = cell.reshape(-1)
    delta = np.where(pos.reshape(-1), 1, np.where(neg.reshape(-1), -2, 0)).astype(np.int64)
    hist = np.bincount(c, weights=delta, minlength=bins).astype(np.int64)
    ev = np.flatnonzero(delta)
    order = ev[np.argsort(c[ev], kind="stable")]  # by cell, raster order within a cell
    d, k = delta[order], c[order]
    run = np.cumsum(d)
    first = np.r_[True, k[1:] != k[:-1]]
    base = np.maximum.accumulate(np.where(first, np.arange(len(k)), 0))
    run = run - (run[base] - d[base])  # the cumulative sum restarted at each cell's first event
    up = d > 0
    if not up.any() or run[up].max() <= 0:
        return hist, 0, 0
    g = int(run[up].max())
    hit = order[up & (run == g)].min()
    return hist, int(c[hit]), g


def weights(hist, kind):
    return np.where(hist != 0, hist, -k0_of(kind)).astype(np.int64)


def m_foo(hist, h1, h2, s1, s2):
    """ODET:109-153 as written."""
    res = 0
    hs = list(range(h1, h2 + 1)) if h1 <= h2 else list(range(h1, 32)) + list(range(0, h2 + 1))
    for h in hs:
        for s in range(s1, s2 + 1):
            v = int(hist[h * 32 + s])
            res += v if v != 0 else -2
    return res


def big_f(hist, v0, v1):
    """LDET:137-163 as written."""
    return sum(int(hist[v]) if hist[v] != 0 else -1 for v in range(v0, v1 + 1))


def search(hist, kind, start, all_best=False):
    """The exact maximum of the detector's objective over the annealing's
    domain with the tie rule: (L, h1, h2, s1, s2), or (L, v0, v1, 0, 0).
    Object kind: h1, h2 in 0..31, s1 in 0..s_start, s2 in s_start..31; ties by
    the fewest cells, the smallest h1, the smallest s1, the smallest h2.  Line
    kinds: 0 <= v0 <= v1 <= 255; ties by the shortest interval, the smallest
    v0.  all_best: every maximiser instead, as rows in tie-rule order."""
    w = weights(hist, kind)
    if kind == OBJECT:
        w = w.reshape(32, 32)
        s_max = start & 31
        hue = np.zeros((32, 32, 32), np.int64)  # [h1, h2, s]: the hues' weights summed one by one
        for h1 in range(32):
            for h2 in range(32):
                hs = list(range(h1, h2 + 1)) if h1 <= h2 else list(range(h1, 32)) + list(range(0, h2 + 1))
                hue[h1, h2] = w[hs].sum(axis=0)
        cs = np.concatenate([np.zeros((32, 32, 1), np.int64), np.cumsum(hue, axis=2)], axis=2)
        i = np.arange(32)
        big_l = cs[:, :, None, 1:] - cs[:, :, :32, None]  # [h1, h2, s1, s2]
        nh = np.where(i[:, None] <= i[None, :], i[None, :] - i[:, None] + 1, 32 - i[:, None] + i[None, :] + 1)
        h1g, h2g, s1g, s2g = np.meshgrid(i, i, i, i, indexing="ij")
        ok = (s1g <= s_max) & (s2g >= s_max)
        ncell = nh[:, :, None, None] * (s2g - s1g + 1)
        top = int(big_l[ok].max())
        at = ok & (big_l == top)
        rows = np.stack([ncell[at], h1g[at], s1g[at], h2g[at], s2g[at]], axis=1)
        rows = rows[np.lexsort((rows[:, 3], rows[:, 2], rows[:, 1], rows[:, 0]))]
        if all_best:
            return top, rows
        n, h1, s1, h2, s2 = (int(x) for x in rows[0])
        return (top, h1, h2, s1, s2)
    cs = np.concatenate([[0], np.cumsum(w)])
    i = np.arange(256)
    big_l = cs[None, 1:] - cs[:256, None]  # [v0, v1]
    ok = i[:, None] <= i[None, :]
    top = int(big_l[ok].max())
    v0, v1 = np.nonzero(ok & (big_l == top))
    rows = np.stack([v1 - v0, v0, v1], axis=1)
    rows = rows[np.lexsort((rows[:, 1], rows[:, 0]))]
    if all_best:
        return top, rows
    return (top, int(rows[0, 1]), int(rows[0, 2]), 0, 0)


def _trunc(x):
    return np.asarray(x).astype(np.int64)  # fp32 -> int: towards zero (all values here are >= 0)


def range_of(kind, h1, h2, s1=0, s2=0):
    """The six OutArgs values of a box (arrays broadcast): int64 [..., 6].
    One float32 product per bound, truncated to int -- and to uint8_t for the
    line kinds' C.v0 / C.v1, which these values always fit."""
    f32 = np.float32
    h1, h2, s1, s2 = (np.asarray(x, np.int64) for x in np.broadcast_arrays(h1, h2, s1, s2))
    if kind == OBJECT:
        a = _trunc((h1 << 3).astype(f32) * f32(1.4))
        b = _trunc((((h2 + 1) << 3) - 1).astype(f32) * f32(1.4))
        c = _trunc((s1 << 3).astype(f32) * f32(0.39))
        d = _trunc(((s2 + 1) << 3).astype(f32) * f32(0.39))
        hue = (b.astype(f32) - (f32(360.0) - a.astype(f32))) / f32(2)
        tol = (b.astype(f32) + (f32(360.0) - a.astype(f32))) / f32(2)
        wrapped_h = _trunc(np.where(hue >= 0, hue, hue + f32(360)))
        h = np.where(a <= b, (b + a) // 2, wrapped_h)
        ht = np.where(a <= b, (b - a) // 2, _trunc(tol))
        return np.stack([h, ht, (d + c) // 2, (d - c) // 2 + 2, np.full_like(h, 50), np.full_like(h, 50)], axis=-1)
    top = h2 + 1 if kind == LINE else (h2 + 1) - 1
    v0 = _trunc(h1.astype(f32) * f32(0.39)) & 255
    v1 = _trunc(top.astype(f32) * f32(0.39)) & 255
    z = np.zeros_like(v0)
    return np.stack([z, z, z, z, (v1 + v0) // 2, (v1 - v0) // 2], axis=-1)


def detect(table, frame, width, height, line_length, kind):
    """One frame through the whole restatement: dict of hist, start = [h or v,
    s or 0, max_value, 0], best = [L, h1, h2, s1, s2], out = the six values."""
    cell = cells(table, frame, width, height, line_length, kind)
    pos, neg = zones(kind, width, height)
    hist, start, g = histogram(cell, pos, neg, bins_of(kind))
    best = search(hist, kind, start)
    st = [start >> 5, start & 31, g, 0] if kind == OBJECT else [start, 0, g, 0]
    return {"hist": hist, "start": st, "best": list(best), "out": range_of(kind, *best[1:]).tolist(),
            "cell": cell, "pos": pos, "neg": neg}
