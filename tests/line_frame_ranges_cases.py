"""The inputs of the line sensors' per-frame-range tests, shared by
tests/test_line_frame_ranges_cpu.py (which checks on the references' own
output that each input reaches what it is meant to reach) and
tests/test_gpu_line_frame_ranges.py (which compares
trik_hsv_line_frame_ranges_batch with them on the same inputs).

Expected values.  ov7670: tests/line_ref.py's sums and targets of frame f
under f's own (val_from, val_to) (held to oracle.line_run by
tests/test_line_cpu.py).  YUYV: oracle.frame(frame f, [(0, 359, 0, 100, vf,
vt)]) for the sums; line_ref.targets' x and size with y = 0 for the targets."""
import functools

import numpy as np

import frame_ranges_cases as FC
import line_cases
import line_ref

LAYOUT_YUYV, LAYOUT_OV7670 = 0, 1


# ---- the launchers' geometry, restated (csrc/trik_hsv_line.hip: line_geom) ----
def geom(layout, n_frames, w, h, ll, base=0, stride=None):
    """What launch_line picks for a batch whose first byte sits `base` bytes
    past a 16-byte boundary: None for the byte-load kernel, else a dict of
    line_geom's numbers.  A unit is 8 pixels of a row: 8 bytes of the ov7670
    luma plane, 16 bytes of packed YUYV; the rest is the same for both."""
    ub = 16 if layout == LAYOUT_YUYV else 8
    fb = h * ll * (2 if layout == LAYOUT_OV7670 else 1)
    stride = fb if stride is None else stride
    if w % 8 or ll % ub or base % ub or (n_frames > 1 and stride % ub):
        return None
    units = w // 8
    cu = min(units, 1024)
    chunks = (units + cu - 1) // cu
    rpi, best, r = 1, 2.0, 1
    while r * cu <= 1024:
        lanes = r * cu
        padded = (lanes + 63) // 64 * 64
        idle = (padded - lanes) / padded
        if idle < best - 1e-9:
            best, rpi = idle, r
        if padded == lanes:
            break
        r += 1
    block = (rpi * cu + 63) // 64 * 64
    base_wgs = n_frames * chunks
    max_segs = (h + rpi * 8 - 1) // (rpi * 8)
    segs = 1 if base_wgs >= 1024 else (2048 + base_wgs - 1) // base_wgs
    segs = max(1, min(segs, max(1, max_segs)))
    seg_rows = (h + segs - 1) // segs
    seg_rows = (seg_rows + rpi - 1) // rpi * rpi
    if seg_rows // rpi > 32767:  # the 16-bit per-column counters
        return None
    segs = (h + seg_rows - 1) // seg_rows
    if base_wgs * segs > 0x7FFFFFFF:
        return None
    return dict(units=units, cu=cu, chunks=chunks, rpi=rpi, block=block, idle=block - rpi * cu, segs=segs,
                seg_rows=seg_rows, iters=seg_rows // rpi)


# (w, h, frames) of the geometry tests, both layouts (line_length = the row's
# bytes), with what geom() must say of each (asserted by the CPU test).  The
# smallest frames the entry point takes (w % 32 == 0, h % 4 == 0) for each shape.
GEOMETRY = [
    ((8224, 40, 3), dict(chunks=2, segs=5, seg_rows=8, rpi=1, block=1024)),   # two column chunks x five row segments
    ((64, 100, 3), dict(chunks=1, segs=2, seg_rows=56, rpi=8)),              # two segments, the second of 44 rows
    ((64, 100, 1025), dict(chunks=1, segs=1, seg_rows=104, rpi=8)),          # >= 1024 frames: one segment
    ((544, 8, 2), dict(chunks=1, segs=1, rpi=15, block=1024, idle=4)),       # 1020 of 1024 lanes
    ((64, 36, 3), dict(segs=1, seg_rows=40, rpi=8, iters=5)),                # the last iteration holds rows 32..35 only
    ((32, 4, 3), dict(segs=1, rpi=16, seg_rows=16, iters=1)),                # the row offsets 4..15 start past the end
]


def row_bytes(w, layout):
    return 2 * w if layout == LAYOUT_YUYV else w


def frame_bytes(w, h, ll, layout):
    return h * ll * (2 if layout == LAYOUT_OV7670 else 1)


def yuyv_of(planes, w, h, ll=None):
    """The packed YUYV frame (line_length 2 w) with the (Y, U, V) of ov7670
    planes at every pixel: the inverse of frame_ranges_cases.ov7670_twin."""
    ll = w if ll is None else ll
    fr = np.asarray(planes, np.uint8)
    y = fr[:h * ll].reshape(h, ll)[:, :w]
    c = fr[h * ll:2 * h * ll].reshape(h, ll)[:, :w]
    out = np.empty((h, w // 2, 4), np.uint8)
    out[..., 0], out[..., 2] = y[:, 0::2], y[:, 1::2]
    out[..., 1], out[..., 3] = c[:, 1::2], c[:, 0::2]  # U = odd chroma byte, V = even
    return out.reshape(-1)


# ---- ranges -------------------------------------------------------------------
EMPTY = (60, 40)


def varied_pairs(n, seed=0):
    """n distinct (val_from, val_to) pairs, lo <= hi, spread over 0..100, with
    EMPTY at index n // 2 ("the middle")."""
    # the 5,151 pairs lo <= hi of 0..100, visited with a stride coprime to their number
    valid = [(lo, hi) for lo in range(101) for hi in range(lo, 101)]
    assert n <= len(valid)
    out = [valid[(1009 * (k + seed) + 17) % len(valid)] for k in range(n)]
    out[n // 2] = EMPTY
    return out


# 64 distinct ranges for the exhaustive frames
EXHAUSTIVE_PAIRS = ([(0, 100), (0, 0), (100, 100), EMPTY, (0, 1), (99, 100), (50, 50), (1, 99)]
                    + [(3 * k % 47, 48 + (5 * k) % 53) for k in range(56)])
# out-of-byte bounds among ordinary ones (ov7670: the reference is line_ref,
# which takes any integer); the ordinary neighbours must be unaffected
OUT_OF_BYTE = [(0, 70), (0, 65535), (50, 100), (65535, 65535), (0, 30), (101, 300), (20, 80), (300, 101), (0, 70)]

ALL_PAIRS = [(p, q) for p in range(101) for q in range(101)]


def six(pairs, fill=0):
    """[N, 6] uint16: entries 4 and 5 from the pairs, entries 0..3 = fill."""
    a = np.full((len(pairs), 6), fill, np.uint16)
    a[:, 4:] = np.asarray(pairs, np.int64).astype(np.uint16)
    return a


# ---- the level frames -----------------------------------------------------------
_cache = {}


def level_pairs(table):
    """128 pixel pairs (Y0, Y1, U, V) holding the V bytes 2 i and 2 i + 1: the
    two pixels of a pair share chroma, so each pair's chroma is searched in the
    oracle's table (grey alone skips levels, since 74/64 > 1), nearest grey
    first."""
    if "pairs" not in _cache:
        val = ((table >> np.uint64(16)) & np.uint64(255)).astype(np.uint8).reshape(65536, 256)  # [V<<8 | U][Y]
        present = np.zeros((65536, 256), bool)
        present[np.arange(65536)[:, None], val] = True
        c = np.arange(65536)
        order = np.argsort(np.abs((c >> 8) - 128) + np.abs((c & 255) - 128), kind="stable")
        out = []
        for i in range(128):
            both = present[order, 2 * i] & present[order, 2 * i + 1]
            assert both.any(), i
            ch = int(order[int(np.argmax(both))])
            out.append((int(np.argmax(val[ch] == 2 * i)), int(np.argmax(val[ch] == 2 * i + 1)), ch & 255, ch >> 8))
        _cache["pairs"] = out
    return _cache["pairs"]


def level_frame_yuyv(table):
    """32 x 8 packed YUYV: every V byte 0..255 exactly once."""
    px = np.array([(y0, u, y1, v) for y0, y1, u, v in level_pairs(table)], np.uint8)
    return px.reshape(-1)


def level_frame_ov7670(table):
    """64 x 8 planes: the 128 level pairs on columns 6..59 (27 pairs a row,
    inside the window 5..59), grey (Y 128) elsewhere."""
    w, h = 64, 8
    y = np.full((h, w), 128, np.uint8)
    c = np.full((h, w), 128, np.uint8)
    for i, (y0, y1, u, v) in enumerate(level_pairs(table)):
        r, q = divmod(i, 27)
        col = 6 + 2 * q
        y[r, col], y[r, col + 1] = y0, y1
        c[r, col], c[r, col + 1] = v, u
    return np.concatenate([y.reshape(-1), c.reshape(-1)])


def v_bytes(table, planes, w, h, ll=None):
    """[h, w] V byte of every pixel of ov7670 planes."""
    ll = w if ll is None else ll
    fr = np.asarray(planes, np.uint8)
    y = fr[:h * ll].reshape(h, ll)[:, :w].astype(np.int64)
    c = fr[h * ll:2 * h * ll].reshape(h, ll)[:, :w]
    v = np.repeat(c[:, 0::2].astype(np.int64), 2, axis=1)
    u = np.repeat(c[:, 1::2].astype(np.int64), 2, axis=1)
    return ((table[y | (u << 8) | (v << 16)] >> np.uint64(16)).astype(np.int64) & 255)


# ---- expected values ------------------------------------------------------------
def expected_ov7670(table, frames, w, h, ll, pairs, band=None):
    """(sums [N][3] Python ints, targets [N] (x, y, size)) of frames[f] under pairs[f]."""
    sums = [line_ref.sums(table, fr, w, h, ll, vf, vt, band) for fr, (vf, vt) in zip(frames, pairs)]
    return sums, [line_ref.targets(*s, w, h) for s in sums]


def wline_targets(sums3, w, h):
    """The webcam line sensor's OutArgs of {points, sum_x, sum_y}: targetY 0."""
    x, _, size = line_ref.targets(int(sums3[0]), int(sums3[1]), 0, w, h)
    return (x, 0, size)


def expected_yuyv(oracle_mod, frames, w, h, ll, pairs):
    """The same for packed YUYV frames: oracle.frame with hue and saturation open."""
    sums = []
    for fr, (vf, vt) in zip(frames, pairs):
        s, _ = oracle_mod.frame(fr, w, h, ll, LAYOUT_YUYV, [(0, 359, 0, 100, vf, vt)])
        sums.append([int(v) for v in s[0]])
    return sums, [wline_targets(s, w, h) for s in sums]


def expected_yuyv_wide(oracle_mod, frame, w, h, ll, pair):
    """One frame whose sums may pass 2^32: the reference's int32 accumulators
    wrap there and oracle.frame's sums with them, so the sums are those of
    oracle.frame's mask in 64 bits (what TrikHsvTargetSums holds)."""
    import gpu_util

    wrapped, mask = oracle_mod.frame(frame, w, h, ll, LAYOUT_YUYV, [(0, 359, 0, 100) + tuple(pair)], want_mask=True)
    want = gpu_util.sums_from_mask(mask, 1)[0]
    assert ((wrapped[0] - want) % 2**32 == 0).all()
    return [int(v) for v in want]


def pair_batch_expected_ov7670(table, band=None):
    """The 10,201 pairs on the 64 x 8 level frame (cached per band)."""
    key = ("pb_ov", band)
    if key not in _cache:
        fr = level_frame_ov7670(table)
        _cache[key] = expected_ov7670(table, [fr] * len(ALL_PAIRS), 64, 8, 64, ALL_PAIRS, band)
    return _cache[key]


def pair_batch_expected_yuyv(oracle_mod, table):
    """The 10,201 pairs on the 32 x 8 YUYV level frame: 64 ranges a call."""
    if "pb_yuyv" not in _cache:
        fr = level_frame_yuyv(table)
        sums = []
        for i in range(0, len(ALL_PAIRS), 64):
            s, _ = oracle_mod.frame(fr, 32, 8, 64, LAYOUT_YUYV, [(0, 359, 0, 100, p, q) for p, q in ALL_PAIRS[i:i + 64]])
            sums += [[int(v) for v in row] for row in s]
        _cache["pb_yuyv"] = (sums, [wline_targets(s, 32, 8) for s in sums])
    return _cache["pb_yuyv"]


# ---- the exhaustive frames ------------------------------------------------------
@functools.lru_cache(maxsize=None)
def exhaustive_frames_yuyv():
    """64 frames of 8192 x 32 packed YUYV (every (Y, U, V) once over the batch)."""
    buf = FC.exhaustive_yuyv()
    buf.setflags(write=False)
    return buf


@functools.lru_cache(maxsize=None)
def exhaustive_frames_ov7670():
    w, h = 8192, 32
    src = exhaustive_frames_yuyv().reshape(64, -1)
    buf = np.concatenate([FC.ov7670_twin(src[f], w, h) for f in range(64)])
    buf.setflags(write=False)
    return buf


# ---- noise batches of the geometry tests -----------------------------------------
@functools.lru_cache(maxsize=None)
def geometry_noise(w, h, n):
    """n ov7670 noise frames of line_cases (planted black and white pixels)."""
    buf = line_cases.noise(w, h, w, n, 7000 + 13 * w + h)
    buf.setflags(write=False)
    return buf


@functools.lru_cache(maxsize=None)
def geometry_noise_yuyv(w, h, n):
    src = geometry_noise(w, h, n).reshape(n, -1)
    buf = np.concatenate([yuyv_of(src[f], w, h) for f in range(n)])
    buf.setflags(write=False)
    return buf


# the generic (byte-load) cases: (frame_stride - frame bytes, line_length - row bytes, base offset), 3 frames
# of 64 x 8
GENERIC = [(0, 0, 1), (0, 0, 4), (3, 0, 0), (0, 4, 0)]


def generic_batch(layout, case, n=3, w=64, h=8):
    """(buffer, offset of frame 0, frame stride, line_length, frames): noise
    frames laid out as the case says, random bytes in every gap; the caller
    places the buffer on a 16-byte boundary."""
    spad, lpad, off = case
    ll = row_bytes(w, layout) + lpad
    fb = frame_bytes(w, h, ll, layout)
    stride = fb + spad
    buf = np.random.default_rng(31 * spad + 7 * lpad + off + layout).integers(0, 256, off + n * stride, dtype=np.uint8)
    ov = line_cases.noise(w, h, w, n, 900 + spad + lpad + off).reshape(n, -1)
    frames = []
    for f in range(n):
        dst = buf[off + f * stride:off + f * stride + fb]
        if layout == LAYOUT_OV7670:
            dst.reshape(2 * h, ll)[:, :w] = ov[f].reshape(2 * h, w)
        else:
            dst.reshape(h, ll)[:, :2 * w] = yuyv_of(ov[f], w, h).reshape(h, 2 * w)
        frames.append(dst)
    return buf, off, stride, ll, frames


# ---- one-hot batches (YUYV) -------------------------------------------------------
ONE_HOT_RANGE = (70, 100)  # takes Y 200 (V 212), not Y 20
ONE_HOT_WIDTHS = (32, 64)
ONE_HOT_ROWS = 36


def _dark_yuyv(w, h):
    fr = np.full((h, w // 2, 4), 128, np.uint8)
    fr[..., 0] = fr[..., 2] = 20
    return fr.reshape(h, 2 * w)


def one_hot_columns_yuyv(w):
    """w frames of w x 8: column c bright (Y 200) in frame c, the rest dark."""
    h = 8
    buf = np.tile(_dark_yuyv(w, h), (w, 1, 1))
    for c in range(w):
        buf[c, :, 2 * c] = 200
    return buf.reshape(-1)


def one_hot_rows_yuyv(h=ONE_HOT_ROWS):
    """h frames of 32 x h: row r bright in frame r."""
    w = 32
    buf = np.tile(_dark_yuyv(w, h), (h, 1, 1))
    for r in range(h):
        buf[r, r, 0::2] = 200
    return buf.reshape(-1)


def one_hot_columns_expected(w):
    return [[8, 8 * c, 28] for c in range(w)]


def one_hot_rows_expected(h=ONE_HOT_ROWS):
    return [[32, 496, 32 * r] for r in range(h)]
