"""The inputs of the per-frame-range multi-blob tests, shared by
tests/test_blob_frame_ranges_cpu.py (which asserts on the oracle's output that
each input reaches what it is meant to reach) and
tests/test_gpu_blob_frame_ranges.py (which compares
trik_hsv_blob_frame_ranges_batch with the oracle on the same inputs).  Test
code, not product.

The expectation of slot (f, t) is blob_ranges_cases.expect on the ov7670 frame
f with the slot's six numbers -- oracle.blob_run(..., state=oracle.pack_range(
six)) -- with 255 in place of a saturation or value above 255; a packed-YUYV
batch holds the twins (blob_ranges_cases.to_yuyv) of the same frames."""
import functools

import numpy as np

import blob_ranges_cases as BR

OV, YUYV = 1, 0
CHUNK_SLOTS = 4096  # TRIK_HSV_BLOB_CHUNK_SLOTS (the CPU test holds it to the ABI's)
PALETTE = [BR.from_to(x) for x in BR.PALETTE_HSV]
ALL5 = [BR.from_to(x) for x in BR.ALL_HSV]


def clamped(six):
    """The six numbers as the call takes them: a saturation or value above 255 is 255."""
    return tuple(six[:2]) + tuple(min(int(v), 255) for v in six[2:])


_expect_cache = {}


def expect(oracle_mod, key, fr, w, h, ll, six):
    """The oracle's run of ov7670 frame `fr` (named `key`) under `six`, once."""
    k = (key, w, h, ll, tuple(six))
    if k not in _expect_cache:
        _expect_cache[k] = BR.expect(oracle_mod, fr, w, h, ll, clamped(six))
    return _expect_cache[k]


def expect_all(oracle_mod, case):
    """[f][t] -> the oracle's result, for a case dict (frames, keys, w, h, ll, ranges)."""
    return [[expect(oracle_mod, case["keys"][f], fr, case["w"], case["h"], case["ll"], six)
             for six in case["ranges"][f]] for f, fr in enumerate(case["frames"])]


def case(name, frames, w, h, ll, ranges):
    assert len(frames) == len(ranges) and len({len(r) for r in ranges}) == 1
    return dict(name=name, frames=frames, keys=[(name, f) for f in range(len(frames))], w=w, h=h, ll=ll,
                ranges=[[tuple(int(v) for v in six) for six in rs] for rs in ranges])


def host_batch(frames, stride=None, offset=0):
    """The frames in one buffer: frame f at offset + f * stride, 0xA5 between."""
    fb = len(frames[0])
    stride = fb if stride is None else stride
    host = np.full(offset + stride * len(frames), 0xA5, np.uint8)
    for i, fr in enumerate(frames):
        host[offset + i * stride: offset + i * stride + fb] = fr
    return host, stride


def widened(six, v):
    """Variant v < 3000 of a from/to range: the hue bounds and the saturation
    floor moved outwards by v's digits (radix 10, 10, 30), so that the variants
    of one range are pairwise distinct."""
    hf, ht, sf, st, vf, vt = six
    assert 0 <= v < 3000 and sf >= 30
    return ((hf - v % 10) % 360, (ht + (v // 10) % 10) % 360, sf - (v // 100) % 30, st, vf, vt)


def distinct_sets(n, t):
    """Frame f: t ranges, the palette (t = 5: with the wrapping range) rotated
    by f + f // 7 -- a rotation that no chunk length repeats -- and widened by
    f: no two frames hold the same set."""
    pool = ALL5 if t == 5 else PALETTE
    return [[widened(pool[(f + f // 7 + k) % len(pool)], f) for k in range(t)] for f in range(n)]


def cut_rows(tall, n, h, ll):
    """A tall ov7670 frame of n * h rows cut into n frames of h rows."""
    y, c = tall[: n * h * ll].reshape(n, h * ll), tall[n * h * ll:].reshape(n, h * ll)
    return [np.concatenate([y[f], c[f]]) for f in range(n)]


def random_mosaics(n, bh, bw, seed, t=4):
    """n frames cut from one tall mosaic of t random bitmaps (density 1/2)."""
    metas = np.stack([np.random.default_rng(seed + i).random((n * bh, bw)) < 0.5 for i in range(t)])
    return cut_rows(BR.mosaic(metas, seed=seed), n, 4 * bh, 4 * bw)


# ---- 1. the threshold at every count ----------------------------------------
@functools.lru_cache(maxsize=None)
def ladders():
    """The four ladder(t) frames (96 x 4) as one batch at T = 1, frame t under
    palette range t alone; and the counts k of metapixel c."""
    frames, counts = zip(*[BR.ladder(t) for t in range(4)])
    return case("ladders", list(frames), 96, 4, 96, [[PALETTE[t]] for t in range(4)]), counts


@functools.lru_cache(maxsize=None)
def lanes():
    """lane_ladder() under LANE_RANGES at T = 4: counts (k, 2, 3, 16)."""
    fr, k = BR.lane_ladder()
    return case("lanes", [fr], 96, 4, 96, [BR.LANE_RANGES]), k


# ---- 2. ranges are per frame -------------------------------------------------
@functools.lru_cache(maxsize=None)
def rotated():
    """8 mosaics (64 x 32) of four pattern_stack bitmaps, T = 4; frame f's four
    ranges are the palette rotated by f."""
    frames = [BR.mosaic(BR.pattern_stack(8, 16, 4, f), seed=20 + f) for f in range(8)]
    return case("rotated", frames, 64, 32, 64, [[PALETTE[(t + f) % 4] for t in range(4)] for f in range(8)])


def rotated_under_frame0(oracle_mod):
    """The same frames, every one under frame 0's set."""
    c = rotated()
    return [[expect(oracle_mod, c["keys"][f], fr, 64, 32, 64, six) for six in c["ranges"][0]]
            for f, fr in enumerate(c["frames"])]


def same_result(a, b):
    return all(np.array_equal(a[k], b[k]) for k in ("meta", "labels", "top", "targets")) and \
        a["n_labels"] == b["n_labels"]


# ---- 3. equal sets equal the shared call -------------------------------------
EQUAL_T = (1, 3, 4, 5, 8, 64)


@functools.lru_cache(maxsize=None)
def equal_frames():
    """64 x 32: two mosaics of clusterer patterns, a scene, uniform random bytes."""
    import oracle

    return [BR.mosaic(BR.pattern_stack(8, 16, 4, 0), seed=1), BR.mosaic(BR.pattern_stack(8, 16, 4, 5), seed=2),
            oracle.blob_scene(64, 32, 64, 3, noise=0.03),
            np.random.default_rng(4).integers(0, 256, 2 * 32 * 64, dtype=np.uint8)]


# ---- 4. geometry -------------------------------------------------------------
# name -> (w, h, n, T)
GEOMETRY = {"32x4": (32, 4, 2, 4), "96x12": (96, 12, 2, 4), "8192x4": (8192, 4, 1, 4), "32x2048": (32, 2048, 1, 4),
            "640x480": (640, 480, 2, 4), "3000x32x4": (32, 4, 3000, 1)}


@functools.lru_cache(maxsize=None)
def geometry(name):
    w, h, n, t = GEOMETRY[name]
    frames = random_mosaics(n, h // 4, w // 4, 300 + w + h)
    return case("geometry-" + name, frames, w, h, w, distinct_sets(n, t))


# ---- 5. chunks -----------------------------------------------------------------
CHUNKS = {4: 1030, 5: 825}  # T -> N, frames of 32 x 8


@functools.lru_cache(maxsize=None)
def chunked(t):
    n = CHUNKS[t]
    return case(f"chunks-T{t}", random_mosaics(n, 2, 8, 500 + t), 32, 8, 32, distinct_sets(n, t))


def chunk_split(n, t):
    """(frames per chunk, frames of the last chunk, chunks) as the call walks the batch."""
    per = max(1, CHUNK_SLOTS // t)
    return per, n - (n - 1) // per * per, (n + per - 1) // per


# ---- 6. load paths -------------------------------------------------------------
# name -> (line_length - row bytes, frame_stride - frame bytes, base offset)
LOADS = {"dwords": (12, 0, 0), "bytes": (3, 1, 1), "aligned16": (0, 0, 0)}
LOAD_W, LOAD_H, LOAD_N = 64, 8, 3


def load_geometry(name, layout):
    """(line_length, frame_stride, offset) of the batch of `layout`."""
    pad, spad, off = LOADS[name]
    ll = (2 * LOAD_W if layout == YUYV else LOAD_W) + pad
    return ll, LOAD_H * ll * (1 if layout == YUYV else 2) + spad, off


@functools.lru_cache(maxsize=None)
def load_case(name):
    """Uniform random ov7670 frames with the padded line length (the YUYV batch
    holds their twins at its own padded line length)."""
    ll = LOAD_W + LOADS[name][0]
    rng = np.random.default_rng(60 + ll)
    frames = [rng.integers(0, 256, 2 * LOAD_H * ll, dtype=np.uint8) for _ in range(LOAD_N)]
    return case("loads-" + name, frames, LOAD_W, LOAD_H, ll, [WIDE[f:f + 4] for f in range(LOAD_N)])


# wide ranges: on uniform random bytes each holds a good share of the pixels
WIDE = [(0, 120, 0, 100, 0, 100), (100, 260, 20, 100, 0, 100), (240, 30, 0, 100, 20, 100), (0, 359, 0, 60, 0, 100),
        (0, 359, 50, 100, 40, 100), (300, 100, 30, 100, 0, 100)]


# ---- 7. dense random bytes -----------------------------------------------------
DENSE = dict(w=1024, h=64, n=8, t=4, seed=77)


@functools.lru_cache(maxsize=None)
def dense(oracle_mod):
    """1024 x 64, N = 8, uniform random bytes, T = 4 per-frame ranges drawn (hue
    window, saturation floor) until the oracle's bitmap of the slot has between
    a quarter and three quarters of its metapixels set."""
    d = DENSE
    rng = np.random.default_rng(d["seed"])
    frames = [rng.integers(0, 256, 2 * d["h"] * d["w"], dtype=np.uint8) for _ in range(d["n"])]
    ranges = []
    for f, fr in enumerate(frames):
        rs = []
        while len(rs) < d["t"]:
            h0, span, s0 = int(rng.integers(0, 360)), int(rng.integers(20, 120)), int(rng.integers(0, 40))
            six = (h0, (h0 + span) % 360, s0, 100, 0, 100)
            share = BR.expect(oracle_mod, fr, d["w"], d["h"], d["w"], six)["meta"].mean()
            if 0.25 < share < 0.75 and six not in rs:
                rs.append(six)
        ranges.append(rs)
    return case("dense", frames, d["w"], d["h"], d["w"], ranges)


# ---- 8. edge ranges, one per frame ---------------------------------------------
EDGE = [(0, 359, 0, 100, 0, 100),      # full
        (10, 10, 100, 100, 100, 100),  # a point
        (330, 20, 30, 100, 30, 100),   # hue wrap
        (120, 120, 0, 100, 0, 100),    # From == To
        (2, 1, 0, 100, 0, 100),        # wrap, From == To + 1 after scaling
        (0, 359, 10, 400, 0, 100),     # a saturation of 400: clamps to 255
        (0, 359, 0, 100, 20, 400)]     # a value of 400: clamps to 255


@functools.lru_cache(maxsize=None)
def edges():
    rng = np.random.default_rng(88)
    frames = [rng.integers(0, 256, 2 * 32 * 64, dtype=np.uint8) for _ in EDGE]
    return case("edges", frames, 64, 32, 64, [[six] for six in EDGE])


# ---- 10. stream order ------------------------------------------------------------
def stream_sets():
    """Two sets over rotated()'s frames: its own, and the reversed batch order."""
    a = rotated()["ranges"]
    return a, [list(reversed(rs)) for rs in a[::-1]]


# ---- 11. the closed loop: 8 ov7670 scene frames of 160 x 120 --------------------
LOOP = dict(n=8, w=160, h=120)


@functools.lru_cache(maxsize=None)
def loop_frames():
    """Red discs on a grey floor; every other frame has a disc over the image
    centre (the auto detector's positive zone), the others only off-centre ones."""
    import oracle

    v = LOOP
    out = []
    for i in range(v["n"]):
        blobs = ((0.5, 0.5, 0.22), (0.8, 0.25, 0.1)) if i % 2 == 0 else ((0.2, 0.3, 0.15), (0.8, 0.7, 0.12))
        out.append(oracle.blob_scene(v["w"], v["h"], v["w"], 70 + i, blobs=blobs, noise=0.01 * (i % 3)))
    return out


def loop_expect(oracle_mod, detect):
    """Slot f: oracle.blob_run(frame f, hsv=detect[f]) (the sensor's own
    centre/tolerance conversion); detect as copied back from the device."""
    v = LOOP
    return [oracle_mod.blob_run(fr, v["w"], v["h"], v["w"], hsv=tuple(int(x) for x in detect[f]), preview=False)
            for f, fr in enumerate(loop_frames())]


def check_loop(detect, want):
    assert len({tuple(int(x) for x in d) for d in detect}) >= 2, detect
    assert any(r["targets"][:, 2].any() for r in want), "no kept target"


# ---- 12. scratch reuse -------------------------------------------------------------
def check_frame(res, f, t, ref, what, full=True):
    """Slot (f, t) of the call's dict (on the host) against one oracle result;
    `full`: bitmap and label map too."""
    assert ref["rc"] == 0
    if full:
        BR.check_slot(res, f, t, ref, what)
        return
    assert int(res["n_labels"][f, t]) == ref["n_labels"], what
    assert np.array_equal(np.asarray(res["top"][f, t]), ref["top"]), what
    assert np.array_equal(np.asarray(res["targets"][f, t, :, :3]), ref["targets"]), what
    assert not np.asarray(res["targets"][f, t, :, 3]).any(), what

