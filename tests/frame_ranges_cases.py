"""The inputs of the per-frame-range tests, shared by
tests/test_frame_ranges_cpu.py (which checks on the oracle that each input
reaches what it is meant to reach) and tests/test_gpu_frame_ranges.py (which
compares trik_hsv_frame_ranges_batch with the oracle on the same inputs).
Expected values are oracle.frame(frame f, f's ranges), then oracle.targets."""
import functools

import numpy as np

LAYOUT_YUYV, LAYOUT_OV7670 = 0, 1

# the four ranges of the benchmark and the eight edge ranges of the parity
# tests (gpu_util.BENCH_RANGES, test_gpu_parity.EDGE_RANGES), restated
POOL = [
    (0, 30, 50, 100, 30, 100),
    (90, 150, 40, 100, 20, 100),
    (200, 260, 40, 100, 20, 100),
    (330, 20, 30, 100, 30, 100),   # hue wrap
    (0, 359, 0, 100, 0, 100),      # full
    (10, 10, 100, 100, 100, 100),  # single point
    (2, 1, 0, 100, 0, 100),        # wrap, From == To + 1 after scaling
    (359, 0, 20, 100, 20, 100),    # wrap through 0
    (400, 500, 200, 250, 0, 255),  # out-of-range args, clamped
    (0, 359, 0, 0, 0, 100),        # grey only
    (0, 359, 0, 100, 0, 10),       # dark only
    (120, 120, 0, 100, 0, 100),    # From == To
]
FULL, T3 = POOL[4], POOL[3]
SEED, FIRST_FRAME = 0x7A1C, 100


def frame_bytes(w, h, ll, layout):
    return h * ll * (2 if layout == LAYOUT_OV7670 else 1)


def row_bytes(w, layout):
    return 2 * w if layout == LAYOUT_YUYV else w


def rotated(n_frames, t=len(POOL)):
    """Frame f: the pool rotated by f, its first t ranges."""
    return [[POOL[(f + k) % len(POOL)] for k in range(t)] for f in range(n_frames)]


def drawn(n_frames, t, seed):
    """Frame f: t ranges drawn from the pool (a range may repeat within a frame)."""
    idx = np.random.default_rng(seed).integers(0, len(POOL), (n_frames, t))
    return [[POOL[i] for i in row] for row in idx]


def expected(oracle_mod, host, stride, n, w, h, ll, layout, ranges):
    """(sums int64 [n, T, 3], targets int8 [n, T, 3]: x, y and the size byte's
    bits) of n frames at host[f * stride:], frame f under ranges[f]."""
    fb = frame_bytes(w, h, ll, layout)
    T = len(ranges[0])
    sums = np.zeros((n, T, 3), np.int64)
    tg = np.zeros((n, T, 3), np.int64)
    for f in range(n):
        assert len(ranges[f]) == T
        s, _ = oracle_mod.frame(host[f * stride:f * stride + fb], w, h, ll, layout, ranges[f])
        sums[f] = s
        for t in range(T):
            tg[f, t] = oracle_mod.targets(s[t], w, h)
    return sums, tg.astype(np.uint8).view(np.int8)


def ov7670_twin(yuyv, w, h):
    """The ov7670 planes (line_length w) with the (Y, U, V) of a packed YUYV
    frame (line_length 2 w) at every pixel: V = even, U = odd chroma byte."""
    px = yuyv.reshape(h, w // 2, 4)
    ylum = np.stack([px[..., 0], px[..., 2]], -1).reshape(h, w)
    chroma = np.stack([px[..., 3], px[..., 1]], -1).reshape(h, w)
    return np.concatenate([ylum.reshape(-1), chroma.reshape(-1)])


def exhaustive_yuyv():
    """16,384 x 1,024 YUYV words holding every (Y, U, V) triple once
    (gpu_util.exhaustive_yuyv_frame's bytes): an 8192 x 2048 frame, or 64
    frames of 8192 x 32."""
    p = np.arange(1 << 23, dtype=np.uint32)
    k = p >> 16
    words = (2 * k) | ((p & 255) << 8) | ((2 * k + 1) << 16) | (((p >> 8) & 255) << 24)
    return words.astype("<u4").view(np.uint8)


# ---- per-frame variety: 37 frames of 160 x 120, T = 5 -----------------------
VARIETY = dict(n=37, w=160, h=120, t=5, seed=5)


def variety_ranges():
    v = VARIETY
    return drawn(v["n"], v["t"], v["seed"])


@functools.lru_cache(maxsize=None)
def variety_frames(oracle_mod, layout, kind):
    v = VARIETY
    host = oracle_mod.synth(v["n"], v["w"], v["h"], row_bytes(v["w"], layout), layout, kind, SEED,
                            first_frame=FIRST_FRAME)
    host.setflags(write=False)
    return host


@functools.lru_cache(maxsize=None)
def variety_expected(oracle_mod, layout, kind):
    v = VARIETY
    ll = row_bytes(v["w"], layout)
    return expected(oracle_mod, variety_frames(oracle_mod, layout, kind), frame_bytes(v["w"], v["h"], ll, layout),
                    v["n"], v["w"], v["h"], ll, layout, variety_ranges())


@functools.lru_cache(maxsize=None)
def variety_under_frame0(oracle_mod, layout, kind):
    """The same frames, every one under frame 0's set."""
    v = VARIETY
    ll = row_bytes(v["w"], layout)
    return expected(oracle_mod, variety_frames(oracle_mod, layout, kind), frame_bytes(v["w"], v["h"], ll, layout),
                    v["n"], v["w"], v["h"], ll, layout, [variety_ranges()[0]] * v["n"])


def check_variety(oracle_mod, layout, kind):
    """More than half the frames give other results than under frame 0's set
    (so a kernel that used one set for the batch would show); returns the
    number that do."""
    own, _ = variety_expected(oracle_mod, layout, kind)
    shared, _ = variety_under_frame0(oracle_mod, layout, kind)
    differ = int((own != shared).any(axis=(1, 2)).sum())
    assert differ > VARIETY["n"] // 2, differ
    return differ


# ---- the closed loop: 8 scene frames of 160 x 120 YUYV ----------------------
LOOP = dict(n=8, w=160, h=120)


@functools.lru_cache(maxsize=None)
def loop_frames(oracle_mod):
    v = LOOP
    host = oracle_mod.synth(v["n"], v["w"], v["h"], 2 * v["w"], LAYOUT_YUYV, 1, SEED, first_frame=FIRST_FRAME)
    host.setflags(write=False)
    return host


def blob_range_of(hsv):
    """BMB:110-130 on (hue, hueTol, sat, satTol, val, valTol), restated in
    Python for the CPU tests (the GPU test takes trik_hsv.blob_range_of)."""
    clip = lambda v: max(0, min(100, v))  # noqa: E731
    return ((hsv[0] - hsv[1]) % 360, (hsv[0] + hsv[1]) % 360, clip(hsv[2] - hsv[3]), clip(hsv[2] + hsv[3]),
            clip(hsv[4] - hsv[5]), clip(hsv[4] + hsv[5]))


@functools.lru_cache(maxsize=None)
def loop_detect(oracle_mod):
    """oracle.run(auto_detect=True)'s six detect* numbers of each loop frame."""
    v = LOOP
    fb = v["h"] * 2 * v["w"]
    host = loop_frames(oracle_mod)
    out = []
    for f in range(v["n"]):
        rc, oa, _ = oracle_mod.run(host[f * fb:(f + 1) * fb], v["w"], v["h"], 2 * v["w"], LAYOUT_YUYV, POOL[0],
                                   auto_detect=True, preview=False)
        assert rc == 0 and oa["detect_written"]
        out.append((oa["detect_hue"], oa["detect_hue_tol"], oa["detect_sat"], oa["detect_sat_tol"],
                    oa["detect_val"], oa["detect_val_tol"]))
    return out


def check_loop(ranges):
    """At least two distinct ranges and at least one wrapped hue (from > to)."""
    assert len(set(ranges)) >= 2, ranges
    assert any(r[0] > r[1] for r in ranges), ranges


# ---- shapes ---------------------------------------------------------------
# (layout, w, h, frames, T)
SMALL_MANY = [(LAYOUT_YUYV, 32, 4, 300, 5), (LAYOUT_OV7670, 96, 8, 64, 5), (LAYOUT_YUYV, 64, 8, 1, 5),
              (LAYOUT_OV7670, 64, 8, 1, 5)]
T_COUNTS = (1, 4, 5, 8, 9, 64)
WIDTHS = (32, 64, 96, 160, 320, 352, 640, 1280, 2080)
TALL = (32, 2052)
# (line_length - row bytes, frame_stride - frame bytes, base offset)
RAGGED = [(12, 0, 0), (3, 1, 1)]


def uniform_batch(layout, w, h, n, seed, pad=0, stride_pad=0, offset=0):
    """n frames of uniform random bytes (padding included): (buffer, offset
    of frame 0, frame stride, line_length)."""
    ll = row_bytes(w, layout) + pad
    stride = frame_bytes(w, h, ll, layout) + stride_pad
    buf = np.random.default_rng(seed).integers(0, 256, offset + n * stride, dtype=np.uint8)
    return buf, offset, stride, ll


def t_ranges(n_frames, t):
    """t ranges per frame for any t up to 64: the pool rotated by the frame,
    cycled, with the value bounds shifted by the cycle so that no two of a
    frame's ranges are equal."""
    out = []
    for f in range(n_frames):
        rs = []
        for k in range(t):
            hf, ht, sf, st, vf, vt = POOL[(f + k) % len(POOL)]
            c = k // len(POOL)
            rs.append((hf, ht, sf, st, vf + 3 * c, vt))
        out.append(rs)
    return out
