"""Frames, ranges and the comparison for the multi-range multi-blob tests
(trik_hsv_blob_batch_ranges; test code, not product).  Every claim made here
about a colour, a range or a builder is asserted on the oracle's output by
tests/test_oracle_blob_ranges.py, so none can quietly stop holding."""
import numpy as np

import blob_patterns

RED_HSV = (0, 20, 80, 20, 50, 50)  # oracle.RED_HSV

# (Y, U, V) of four colours and, in centre/tolerance form, four ranges that
# each hold exactly one of them (grey holds none)
COLOURS = [(80, 100, 215), (145, 54, 34), (41, 240, 110), (210, 16, 146)]  # red, green, blue, yellow
PALETTE_HSV = [RED_HSV, (120, 20, 80, 20, 80, 20), (240, 20, 80, 20, 80, 20), (60, 20, 80, 20, 80, 20)]
# hue 320..80 through 0: holds red and yellow -- overlapping and hue-wrapping
WRAP_HSV = (20, 60, 70, 30, 60, 40)
ALL_HSV = PALETTE_HSV + [WRAP_HSV]
# a luma with which a pixel of that colour's chroma lies in none of ALL_HSV
OFF_Y = [250, 250, 200, 10]


def from_to(hsv):
    """Centre/tolerance -> from/to (BMB:110-130), in Python: what
    trik_hsv.blob_range_of and oracle.blob_range are tested against each other with."""
    hue, ht, sat, st, val, vt = hsv
    clip = lambda v: max(0, min(100, v))  # noqa: E731
    return ((hue - ht) % 360, (hue + ht) % 360, clip(sat - st), clip(sat + st), clip(val - vt), clip(val + vt))


def ranges_for(t):
    """T from/to ranges: the palette, then the wrapping range, then the same
    again with the value floor raised step by step (distinct tables per range)."""
    out = []
    for i in range(t):
        h0, h1, s0, s1, v0, v1 = from_to(ALL_HSV[i % 5])
        out.append((h0, h1, s0, s1, min(v0 + 7 * (i // 5), v1), v1))
    return out


def to_yuyv(fr, w, h, ll, ll_yuyv, seed=0):
    """The packed-YUYV twin of an ov7670 frame: Y0 U Y1 V per pair with U the
    odd and V the even chroma byte (OSEQ:369-373); random padding bytes."""
    y = fr[: h * ll].reshape(h, ll)[:, :w]
    c = fr[h * ll: 2 * h * ll].reshape(h, ll)[:, :w]
    out = np.random.default_rng(seed).integers(0, 256, (h, ll_yuyv), dtype=np.uint8)
    out[:, 0:2 * w:2] = y
    out[:, 1:2 * w:4] = c[:, 1::2]
    out[:, 3:2 * w:4] = c[:, 0::2]
    return out.reshape(-1)


def _assemble(yv, vv, uu, ll, rng):
    """[bh, bw, 4, 4] luma and [bh, bw, 4, 2] V / U per pair -> an ov7670 frame."""
    bh, bw = yv.shape[:2]
    h, w = 4 * bh, 4 * bw
    fr = rng.integers(0, 256, 2 * h * ll, dtype=np.uint8)
    fr[: h * ll].reshape(h, ll)[:, :w] = yv.transpose(0, 2, 1, 3).reshape(h, w)
    c = fr[h * ll:].reshape(h, ll)
    c[:, 0:w:2] = vv.transpose(0, 2, 1, 3).reshape(h, w // 2)
    c[:, 1:w:2] = uu.transpose(0, 2, 1, 3).reshape(h, w // 2)
    return fr


def mosaic(metas, line_length=None, seed=0, counts=None):
    """An ov7670 frame from T <= 4 bitmaps [T][bh][bw]: each metapixel's 8
    chroma pairs go to colours so that palette range t has 3..16 pixels where
    metas[t] is set and 0..2 where it is not (counts [T][bh][bw], when given,
    sets the pixel numbers exactly: at most 2 * ceil(count / 2) summing to 16).
    A pixel is colour t iff its pair carries t's chroma and it has t's luma;
    the other pixel of such a pair gets OFF_Y[t]; the rest is grey."""
    rng = np.random.default_rng((seed, 0x6D6F73))  # (not the stream a caller drew the bitmaps from)
    metas = np.asarray(metas) != 0
    T, bh, bw = metas.shape
    ll = 4 * bw if line_length is None else line_length
    owner = np.full((bh, bw, 8), -1)
    pos = np.zeros((bh, bw), int)
    rows, cols = np.mgrid[0:bh, 0:bw]

    def give(t, where):
        owner[rows[where], cols[where], pos[where]] = t
        pos[where] += 1

    if counts is None:
        for t in range(T):  # a set colour: two pairs at least
            give(t, metas[t])
            give(t, metas[t])
        for t in range(T):  # an unset one: a pair at most
            give(t, ~metas[t] & (pos < 8) & (rng.random((bh, bw)) < 0.5))
        full = rng.random((bh, bw)) < 0.25  # a quarter of the metapixels: no grey, nearly every pixel on
        for _ in range(8):  # the rest: more pairs of set colours, or grey
            c = rng.integers(-1, T, (bh, bw))
            c = np.where(full & (c < 0), rng.integers(0, T, (bh, bw)), c)
            ok = (pos < 8) & (c >= 0) & np.take_along_axis(metas, np.maximum(c, 0)[None], 0)[0]
            for t in range(T):
                give(t, ok & (c == t))
            pos[(pos < 8) & ~ok] += 1
        npairs = np.stack([(owner == t).sum(2) for t in range(T)])
        k = np.where(metas, rng.integers(3, 17, (T, bh, bw)), rng.integers(0, 3, (T, bh, bw)))
        k = np.where(metas & full, np.maximum(3, 2 * npairs - rng.integers(0, 3, (T, bh, bw))), k)
        k = np.minimum(k, 2 * npairs)
    else:
        k = np.asarray(counts)
        for t in range(T):
            for j in range(8):
                give(t, 2 * j < k[t])
    owner = np.take_along_axis(owner, rng.random((bh, bw, 8)).argsort(2), 2)
    own_px = np.repeat(owner, 2, axis=2)  # pixel i of the 16 belongs to pair i // 2
    u = rng.random((bh, bw, 16))
    yv = rng.integers(100, 160, (bh, bw, 16))
    vv = np.full((bh, bw, 8), 128)
    uu = np.full((bh, bw, 8), 128)
    for t in range(T):
        mine = own_px == t
        rank = np.where(mine, u, 2.0).argsort(2).argsort(2)
        on = mine & (rank < k[t][:, :, None])
        yv = np.where(on, COLOURS[t][0], np.where(mine, OFF_Y[t], yv))
        uu = np.where(owner == t, COLOURS[t][1], uu)
        vv = np.where(owner == t, COLOURS[t][2], vv)
    return _assemble(yv.reshape(bh, bw, 4, 4), vv.reshape(bh, bw, 4, 2), uu.reshape(bh, bw, 4, 2), ll, rng)


def ladder(t, bw=24):
    """A 4-row frame whose metapixel c holds exactly c % 17 pixels of colour t
    (and the counts)."""
    k = (np.arange(bw) % 17)[None, None, :]
    metas = np.zeros((4, 1, bw), bool)
    counts = np.zeros((4, 1, bw), int)
    metas[t], counts[t] = k > 2, k
    return mosaic(metas, seed=t, counts=counts), k[0, 0]


# Byte lanes: four ranges whose counts in one metapixel are (k, 2, 3, 16) for
# k = 0..16.  All 16 pixels lie in the fourth; the first is a value band (V up
# to 80 %) each pixel enters or leaves by its luma alone; the second and third
# are nested value bands of the green hue.  Two pairs carry green chroma, with
# roles A, A (in both green bands), B (in the wider one) and C (in neither);
# six pairs are grey.  Luma by role: (inside the first range, outside it).
LANE_RANGES = [(0, 359, 0, 100, 0, 80), (100, 140, 60, 100, 70, 90), (100, 140, 60, 100, 60, 95),
               (0, 359, 0, 100, 0, 100)]
LANE_COUNTS = (2, 3, 16)
_ROLE_Y = {"A": (90, 112), "B": (68, 128), "C": (20, 160), "N": (100, 250)}


def lane_ladder(bw=24, seed=5):
    """(frame, k): metapixel c holds k = c % 17 pixels of LANE_RANGES[0] and
    LANE_COUNTS of the others, at random places."""
    rng = np.random.default_rng(seed)
    k = np.arange(bw) % 17
    yv = np.zeros((1, bw, 16), int)
    vv = np.full((1, bw, 8), 128)
    uu = np.full((1, bw, 8), 128)
    for c in range(bw):
        pairs = rng.permutation(8)
        roles = ["N"] * 16
        for role, px in zip("AABC", rng.permutation([2 * pairs[0], 2 * pairs[0] + 1, 2 * pairs[1], 2 * pairs[1] + 1])):
            roles[px] = role
        uu[0, c, pairs[:2]], vv[0, c, pairs[:2]] = COLOURS[1][1], COLOURS[1][2]
        inside = rng.permutation(16) < k[c]
        yv[0, c] = [_ROLE_Y[r][0 if i else 1] for r, i in zip(roles, inside)]
    return _assemble(yv.reshape(1, bw, 4, 4), vv.reshape(1, bw, 4, 2), uu.reshape(1, bw, 4, 2), 4 * bw, rng), k


def counts_of(mask, t):
    """Per-metapixel counts of bit t of an oracle.frame mask [H, W]."""
    h, w = mask.shape
    return ((mask >> t) & 1).reshape(h // 4, 4, w // 4, 4).sum((1, 3))


def pattern_stack(bh, bw, t, offset=0):
    """T bitmaps out of blob_patterns.patterns, a different one per range."""
    pats = list(blob_patterns.patterns(bh, bw).values())
    return np.stack([pats[(offset + 3 * i) % len(pats)] for i in range(t)])


def expect(oracle_mod, fr, w, h, ll, rng_from_to):
    """The full result of a slot: the oracle's run on the ov7670 frame with
    the packed range as the sticky state."""
    return oracle_mod.blob_run(fr, w, h, ll, hsv=None, state=oracle_mod.pack_range(rng_from_to), preview=False)


def check_slot(res, f, t, ref, what):
    """Slot (f, t) of Detector.blob_batch_ranges(..., meta=True, labels=True)
    against one oracle.blob_run result, as blob_patterns.check_frame."""
    blob_patterns.check_frame({key: val[f] for key, val in res.items()}, t, ref, what)
