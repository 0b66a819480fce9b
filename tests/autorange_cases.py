"""Frames for the exact autoDetectHsv tests (tests/test_autorange_cpu.py,
tests/test_gpu_autorange.py): crafted ones that each aim at one property of
the detectors' histogram, start cell or search, and the geometries at which
the kernel's phases change.  Every coverage claim is asserted on the
restatement's own output (Case.check), so a case that stops reaching its
target fails loudly instead of passing for the wrong reason.

The kernel (trik_hsv_autorange.hip) has one shape; its phases are reached by:
  no band at all (every row folds)   line kinds at W = 32 and 64, object 32x4
  band rows with both side negatives  object 64x48, 96x20, 320x240; line 320
  band rows without side negatives    object 32x96; line kinds at W = 160
  rows before and after the band      every object case
Test code."""
import functools

import numpy as np

import autorange_ref as R

OBJECT, LINE, WLINE = R.OBJECT, R.LINE, R.WLINE


@functools.lru_cache(maxsize=None)
def _table():
    import oracle

    oracle.build()
    return oracle.yuv_table(closed=False)


@functools.lru_cache(maxsize=None)
def _object_palette():
    """cell -> (Y, U, V) of the first table entry (in a sparse walk) in it."""
    t = _table()
    idx = np.arange(0, 1 << 24, 5, dtype=np.int64)
    hsv = t[idx].astype(np.int64)
    cell = (((hsv & 255) >> 3) << 5) | (((hsv >> 8) & 255) >> 3)
    cells, first = np.unique(cell, return_index=True)
    return {int(c): (int(idx[f]) & 255, (int(idx[f]) >> 8) & 255, int(idx[f]) >> 16) for c, f in zip(cells, first)}


@functools.lru_cache(maxsize=None)
def _grey_y():
    """V byte -> a luma Y that gives it with U = V = 128 (grey: the V byte
    follows Y alone, so the line kinds' bins are set pixel by pixel)."""
    t = _table()
    y = np.arange(256, dtype=np.int64)
    v = (t[y | (128 << 8) | (128 << 16)].astype(np.int64) >> 16) & 255
    return {int(b): int(a) for a, b in reversed(list(zip(y, v)))}


def cell_of(h, s):
    return h * 32 + s


class Case:
    """n frames of one kind and geometry: `data` holds frame i at offset +
    i * stride (offset > 0: a base that is not 16-byte aligned)."""

    def __init__(self, name, kind, width, height, line_length, frames, stride=None, offset=0, check=None):
        self.name, self.kind, self.width, self.height, self.line_length = name, kind, width, height, line_length
        fb = R.frame_bytes(kind, height, line_length)
        self.n = len(frames)
        self.stride = fb if stride is None else stride
        assert self.stride >= fb
        self.offset = offset
        self.data = np.random.default_rng(len(name)).integers(0, 256, offset + self.stride * self.n, dtype=np.uint8)
        for i, f in enumerate(frames):
            assert f.size == fb
            self.data[offset + i * self.stride: offset + i * self.stride + fb] = f
        self._check = check
        self._want = None

    def frame(self, i):
        fb = R.frame_bytes(self.kind, self.height, self.line_length)
        return self.data[self.offset + i * self.stride: self.offset + i * self.stride + fb]

    def want(self):
        """The restatement's result per frame, computed once; asserts the
        case's coverage claim on it."""
        if self._want is None:
            self._want = [R.detect(_table(), self.frame(i), self.width, self.height, self.line_length, self.kind)
                          for i in range(self.n)]
            if self._check:
                self._check(self, self._want)
        return self._want

    def __repr__(self):
        return self.name


# ---------------------------------------------------------------------------
# painting
# ---------------------------------------------------------------------------
def _pack(kind, y, u, v, line_length, seed):
    """Planes y [H, W], u, v [H, W / 2] as one frame with random row padding."""
    h, w = y.shape
    fr = np.random.default_rng(seed).integers(0, 256, R.frame_bytes(kind, h, line_length), dtype=np.uint8)
    if R.layout_of(kind) == R.LAYOUT_OV7670:
        fr[:h * line_length].reshape(h, line_length)[:, :w] = y
        c = fr[h * line_length:].reshape(h, line_length)
        c[:, 0:w:2] = v
        c[:, 1:w:2] = u
    else:
        p = fr.reshape(h, line_length)
        p[:, 0:2 * w:2] = y
        p[:, 1:2 * w:4] = u
        p[:, 3:2 * w:4] = v
    return fr


def paint_object(width, height, line_length, pairs, background, seed=1):
    """An object-kind frame whose pixel pairs (row, pair column) -> cell are
    `pairs`, every other pair `background`."""
    pal = _object_palette()
    y = np.empty((height, width), np.uint8)
    u = np.empty((height, width // 2), np.uint8)
    v = np.empty((height, width // 2), np.uint8)
    by, bu, bv = pal[background]
    y[:], u[:], v[:] = by, bu, bv
    for (r, p), c in pairs.items():
        cy, cu, cv = pal[c]
        y[r, 2 * p:2 * p + 2], u[r, p], v[r, p] = cy, cu, cv
    return _pack(OBJECT, y, u, v, line_length, seed)


def paint_line(kind, width, height, line_length, values, seed=1):
    """A line-kind frame whose V byte per pixel is `values` [H, W] (grey chroma)."""
    gy = _grey_y()
    lut = np.array([gy.get(b, -1) for b in range(256)])
    y = lut[values]
    assert (y >= 0).all(), "a V byte no grey pixel has"
    half = np.full((height, width // 2), 128, np.uint8)
    return _pack(kind, y.astype(np.uint8), half, half, line_length, seed)


# ---------------------------------------------------------------------------
# the object kind at 64 x 48: step 8, positive columns 25..39 of rows 17..31
# (pairs 13..19 lie wholly inside), negative columns < 16 and > 48 (pairs 0..7
# and 25..31), negative rows < 8 and > 40
# ---------------------------------------------------------------------------
W0, H0 = 64, 48
BG = cell_of(16, 16)  # the background: thousands of negatives, never near zero
A, B = cell_of(20, 9), cell_of(5, 9)


def _row(r, first_pair, n_pairs, cell):
    return {(r, first_pair + i): cell for i in range(n_pairs)}


def _ties(case, i):
    """The positive events of frame i whose running value equals the final max_value."""
    w = case.want()[i]
    trace = []
    R.histogram_loop(w["cell"], w["pos"], w["neg"], R.bins_of(case.kind), trace)
    g = w["start"][2]
    return [t for t in trace if t[0] == g]


def _start_cell(w):
    return cell_of(w["start"][0], w["start"][1])


def _object_cases():
    out = []

    def add(name, pairs, check):
        out.append(Case(name, OBJECT, W0, H0, W0, [paint_object(W0, H0, W0, pairs, BG)], check=check))

    # A peaks at 8 in the band's first row and is worn down by right-hand
    # negatives afterwards; B ends highest with 6
    pairs = {**_row(17, 13, 4, A), **_row(18, 25, 7, A), **_row(20, 13, 3, B)}

    def eroded(case, want):
        w = want[0]
        assert _start_cell(w) == A and w["start"][2] == 8
        assert int(np.argmax(w["hist"])) == B and w["hist"][A] < 0
    add("eroded-early-peak", pairs, eroded)

    # A (the larger index) and B both reach 4 in row 17; A's last pixel comes first
    pairs = {**_row(17, 13, 2, A), **_row(17, 15, 2, B)}

    def same_row(case, want):
        t = _ties(case, 0)
        assert {x[1] for x in t} == {A, B} and {x[2] for x in t} == {17}
        assert _start_cell(want[0]) == A and A > B
    add("equal-G-one-row", pairs, same_row)

    # B reaches 4 in row 17, A in row 19 at earlier columns
    pairs = {**_row(19, 13, 2, A), **_row(17, 17, 2, B)}

    def two_rows(case, want):
        t = _ties(case, 0)
        assert {(x[1], x[2]) for x in t} == {(A, 19), (B, 17)}
        assert _start_cell(want[0]) == B
    add("equal-G-two-rows", pairs, two_rows)

    # A: 2 left negatives and 6 positives in row 17 (peak 2); B: 4 positives (peak 4)
    pairs = {**_row(17, 0, 1, A), **_row(17, 13, 3, A), **_row(17, 16, 2, B)}

    def same_row_neg(case, want):
        w = want[0]
        in_row = lambda c: int(((w["cell"][17] == c) & w["pos"][17]).sum())
        assert in_row(A) == 6 and in_row(B) == 4 and _start_cell(w) == B and w["start"][2] == 4
        assert w["hist"][A] == 2
    add("same-row-negatives", pairs, same_row_neg)

    # positive mass at hue bins 30, 31, 0, 1 of one saturation bin
    hues = [30, 31, 0, 1]
    pairs = {}
    for k, hb in enumerate(hues):
        pairs.update(_row(17 + k, 13, 4 - (k % 2), cell_of(hb, 9)))

    def wrap(case, want):
        l, h1, h2, s1, s2 = want[0]["best"]
        assert (h1, h2, s1, s2) == (30, 1, 9, 9) and l == 8 + 6 + 8 + 6
    add("hue-wrap", pairs, wrap)

    # the tie rule, level by level: every maximiser of L listed by the restatement
    def level(n, picked):
        def check(case, want):
            w = want[0]
            top, rows = R.search(w["hist"], OBJECT, _start_cell(w), all_best=True)
            assert len(rows) >= 2
            for k in range(n):  # the earlier levels leave more than one candidate ...
                rows = rows[rows[:, k] == rows[:, k].min()]
            assert len(set(rows[:, n].tolist())) >= 2  # ... and this one decides among them
            assert tuple(w["best"][1:]) == picked
        return check

    # {A} = 6 against {A, -4, +4}: the fewest cells
    pairs = {**_row(17, 13, 3, A), **_row(2, 3, 1, cell_of(21, 9)), **_row(18, 13, 2, cell_of(22, 9))}
    add("tie-cells", pairs, level(0, (20, 20, 9, 9)))
    # two lone cells of 6 in one saturation bin: the smallest h1
    pairs = {**_row(17, 13, 3, A), **_row(18, 13, 3, B)}
    add("tie-h1", pairs, level(1, (5, 5, 9, 9)))
    # (20, 9) = 6, (20, 8) = 2, (21, 9) = 2, (21, 8) = 0: two boxes of two cells from h1 = 20; the smallest s1
    pairs = {**_row(17, 13, 3, A), **_row(18, 13, 1, cell_of(20, 8)), **_row(19, 13, 1, cell_of(21, 9))}
    add("tie-s1", pairs, level(2, (20, 20, 8, 9)))
    # (20, 9) = 6, (20, 10) = 2, (21, 9) = 2: both boxes start at s1 = 9; the smallest h2
    pairs = {**_row(17, 13, 3, A), **_row(18, 13, 1, cell_of(20, 10)), **_row(19, 13, 1, cell_of(21, 9))}
    add("tie-h2", pairs, level(3, (20, 20, 9, 10)))

    # the start cell's saturation bin binds: a heavier box lies wholly above it
    pairs = {**_row(17, 13, 3, A), **_row(18, 13, 2, cell_of(20, 14)), **_row(19, 13, 2, cell_of(20, 15))}

    def s_bound(case, want):
        w = want[0]
        assert _start_cell(w) == A and w["best"][3] <= 9 <= w["best"][4]
        free = R.m_foo(w["hist"], 20, 20, 14, 15)
        assert free > w["best"][0]
    add("saturation-bound", pairs, s_bound)
    return out


# ---------------------------------------------------------------------------
# the line kinds
# ---------------------------------------------------------------------------
def _line_cases(kind):
    out = []
    gy = sorted(_grey_y())
    ll = lambda w: (2 if kind == WLINE else 1) * w
    rng = np.random.default_rng(7 + kind)

    def rand_values(w, h, lo=0, hi=None):
        pick = np.array(gy[lo:hi])
        return pick[rng.integers(0, len(pick), (h, w))]

    # the uint16 ROI wraps: every pixel is negative, the best interval is the first untouched bin
    for w in (32, 64):
        def all_neg(case, want):
            for x in want:
                assert x["pos"].sum() == 0 and x["neg"].all() and x["start"] == [0, 0, 0, 0]
                assert x["best"][0] == -1 and x["best"][1] == x["best"][2] == int(np.flatnonzero(x["hist"] == 0)[0])
        out.append(Case(f"roi-wrap-{w}", kind, w, 8, ll(w), [paint_line(kind, w, 8, ll(w), rand_values(w, 8, 0, 40))],
                        check=all_neg))

    # W = 160: the first width whose ROI does not wrap, and it has no negative column
    def first_plain(case, want):
        x = want[0]
        assert x["pos"].sum() == 79 * case.height and x["neg"].sum() == 0 and x["start"][2] > 0
    out.append(Case("roi-160", kind, 160, 8, ll(160), [paint_line(kind, 160, 8, ll(160), rand_values(160, 8))],
                    check=first_plain))

    # two masses three bins apart with nothing between: the interval pays -1 per empty bin to join them
    lo, hi = gy[60], gy[63]
    gap = [b for b in range(lo + 1, hi)]
    vals = np.full((8, 320), gy[5])
    vals[:, 121:199:2] = lo
    vals[:, 122:199:2] = hi

    def joined(case, want):
        x = want[0]
        assert len(gap) >= 1 and all(x["hist"][b] == 0 for b in gap)
        assert x["best"][1:3] == [lo, hi] and x["best"][0] == x["hist"][lo] + x["hist"][hi] - len(gap)
        assert x["hist"][gy[5]] < 0  # (and the side columns' negatives fell on another bin)
    out.append(Case("join-over-zeros", kind, 320, 8, ll(320), [paint_line(kind, 320, 8, ll(320), vals)], check=joined))

    # a value whose early peak is eroded by right-hand negatives of later rows
    vals = np.full((8, 320), gy[5])
    vals[0, 121:129] = gy[80]
    vals[1:, 250:320] = gy[80]
    vals[3, 121:127] = gy[90]

    def eroded(case, want):
        x = want[0]
        assert x["start"][0] == gy[80] and x["start"][2] == 8 and x["hist"][gy[80]] < 0
        assert x["best"][1:3] == [gy[90], gy[90]]
    out.append(Case("eroded-early-peak", kind, 320, 8, ll(320), [paint_line(kind, 320, 8, ll(320), vals)],
                    check=eroded))
    return out


# ---------------------------------------------------------------------------
# geometries and batches: synthetic scenes and uniform bytes
# ---------------------------------------------------------------------------
GEOMETRIES = [(32, 8, 0), (64, 48, 0), (96, 20, 32), (32, 96, 0), (320, 240, 0)]  # width, height, line padding


def _synth_cases(kind):
    import oracle

    out = []
    mul = 2 if kind == WLINE else 1
    for w, h, pad in GEOMETRIES:
        ll = mul * w + pad
        fb = R.frame_bytes(kind, h, ll)
        fr = oracle.synth(2, w, h, ll, R.layout_of(kind), 1, 0x51 + w, frame_stride=fb)
        un = oracle.synth(1, w, h, ll, R.layout_of(kind), 0, 0x52 + h, frame_stride=fb)
        frames = [fr[:fb], fr[fb:], un]
        check = None
        if kind == OBJECT and (w, h) == (32, 8):  # step = 1: one positive pixel
            def check(case, want):
                assert all(x["pos"].sum() == 1 for x in want)
        if kind == OBJECT and (w, h) == (32, 96):  # no negative column
            def check(case, want):
                assert not want[0]["neg"][48].any() and want[0]["neg"][0].all()
        out.append(Case(f"geometry-{w}x{h}", kind, w, h, ll, frames, stride=fb + 48, check=check))
    # a batch of 64 small frames, strided, and one of a single frame on an odd base
    w, h = 64, 48
    ll = mul * w
    fb = R.frame_bytes(kind, h, ll)
    fr = oracle.synth(64, w, h, ll, R.layout_of(kind), 1, 0x99, frame_stride=fb)
    out.append(Case("batch-64", kind, w, h, ll, [fr[i * fb:(i + 1) * fb] for i in range(64)], stride=fb + 16))
    out.append(Case("batch-1-odd-base", kind, w, h, ll, [fr[:fb]], offset=3))
    return out


def _empty_zone_case():
    # 32 x 4: step = 0, so the object detector's positive zone is empty
    import oracle

    fr = oracle.synth(1, 32, 4, 32, R.LAYOUT_OV7670, 1, 0x11)

    def empty(case, want):
        x = want[0]
        assert x["pos"].sum() == 0 and x["start"] == [0, 0, 0, 0] and x["neg"].sum() > 0
    return Case("empty-zone-32x4", OBJECT, 32, 4, 32, [fr], check=empty)


@functools.lru_cache(maxsize=None)
def cases(kind):
    out = _synth_cases(kind)
    if kind == OBJECT:
        out += _object_cases() + [_empty_zone_case()]
    else:
        out += _line_cases(kind)
    return out


def scene_batch(kind):
    """8 scene frames at 320 x 240: oracle.blob_scene for the object kind,
    oracle.line_scene for the ov7670 line kind, the synthetic scene for the
    webcam line kind (the oracle's scenes are ov7670 frames)."""
    import oracle

    w, h = 320, 240
    if kind == OBJECT:
        frames = [oracle.blob_scene(w, h, w, 40 + i) for i in range(8)]
    elif kind == LINE:
        frames = [oracle.line_scene(w, h, w, 40 + i, x0=100 + 15 * i) for i in range(8)]
    else:
        fb = R.frame_bytes(kind, h, 2 * w)
        fr = oracle.synth(8, w, h, 2 * w, R.LAYOUT_YUYV, 1, 0x40, frame_stride=fb)
        frames = [fr[i * fb:(i + 1) * fb] for i in range(8)]
    return Case(f"scenes-320x240-kind{kind}", kind, w, h, (2 if kind == WLINE else 1) * w, frames)
