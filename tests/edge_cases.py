"""The inputs of the edge-line sensor's arithmetic tests, shared by
tests/test_edge_cpu.py (which checks on tests/edge_ref.py that each input
reaches what it is meant to reach) and tests/test_gpu_edge.py (which compares
the GPU with tests/edge_ref.py on the same inputs).  Every coverage condition
is a function of the reference's own output."""
import numpy as np

import edge_ref

# the level frames of the threshold sweep: every even magnitude a threshold can
# separate, 256 (the first magnitude the 255 cap cuts) and the largest, 1020
SWEEP_LEVELS = tuple(range(0, 258, 2)) + (1020,)
# the level frames of the preview: every luma the thresholded map can hold at
# threshold 255 (the even values and, from 256, 255)
PREVIEW_LEVELS = tuple(range(0, 258, 2))
PREVIEW_GEOM = (2048, 68)
LADDER_GEOM = (320, 240)
H0_GEOM = (192, 8)
V0_GEOM = (64, 136)


def window(plane, width, height):
    """The counted part of a [height * width] plane: map rows 0 .. height-3,
    columns 16 .. width-16."""
    return np.asarray(plane).reshape(height, width)[:height - 2, 16:width - 15]


def last_row_frame(width, height):
    """A flat frame whose last input row is bright over its left half: the only
    windows that see it are those of map row height-3."""
    fr = np.full(2 * width * height, 128, np.uint8)
    y = fr[:width * height].reshape(height, width)
    y[:] = 100
    y[height - 1, :width // 2 + 5] = 255
    return fr


def check_last_row(frame, width, height):
    emap, (p, sx), _ = edge_ref.run(frame, width, height)
    assert p > 0 and (window(emap, width, height)[height - 3] == 255).sum() == p
    assert not (window(emap, width, height)[:height - 3] == 255).any()


def noise_ladder(seed=0x1ADDE5):
    """320 x 240, 16 bands of 15 rows of uniform noise around 128 whose
    amplitude grows from 1 to the full range."""
    w, h = LADDER_GEOM
    rng = np.random.default_rng(seed)
    fr = rng.integers(0, 256, 2 * w * h, dtype=np.uint8)
    y = fr[:w * h].reshape(h, w)
    amps = (1, 1, 2, 3, 4, 6, 8, 12, 16, 24, 32, 48, 64, 96, 128, 255)
    for b, amp in enumerate(amps):
        lo = 128 - (amp + 1) // 2
        y[15 * b:15 * b + 15] = lo + rng.integers(0, amp + 1, (15, w))
    return fr


def quadrant_magnitudes(frame, width, height):
    """{(sign H, sign V): the set of |H| + |V| inside the window}."""
    H, V = (window(p, width, height) for p in edge_ref.hv(frame, width, height))
    mag = np.abs(H) + np.abs(V)
    return {(sh, sv): set(mag[(np.sign(H) == sh) & (np.sign(V) == sv)].tolist())
            for sh in (-1, 0, 1) for sv in (-1, 0, 1)}


def covers(mags):
    """Every even magnitude 2 .. 254 and one past the 255 cap."""
    return bool(mags) and all(m in mags for m in range(2, 256, 2)) and max(mags) >= 256


def check_ladder(frame):
    q = quadrant_magnitudes(frame, *LADDER_GEOM)
    for sh in (-1, 1):
        for sv in (-1, 1):
            assert covers(q[sh, sv]), (sh, sv, sorted(set(range(2, 256, 2)) - q[sh, sv]))


def _chain(n):
    """T[0 .. n+2) around 255 with T[i+2] - T[i] = +-(i+1), the signs
    alternating along each of the two interleaved chains, so T stays within
    255 +- (n + 2) / 2."""
    T = [255, 255]
    for i in range(n):
        T.append(T[i] + (i + 1) * (1 if (i // 2) % 2 == 0 else -1))
    return np.array(T)


def h0_frame():
    """192 x 8 with period 2 along its rows (rows A, B, A, B, ...): H = 0
    everywhere, V = 2 ((A+B)[c+1] - (A+B)[c-1]) = +-2 (c - 15) on window
    column c: every even |V| from 2 to 322."""
    w, h = H0_GEOM
    S = np.full(w + 1, 255)
    S[15:] = _chain(w - 16)[:w + 1 - 15]  # S[c+1] - S[c-1] = +-(c - 15) for c >= 16
    S = S[:w]
    fr = np.full(2 * w * h, 128, np.uint8)
    y = fr[:w * h].reshape(h, w)
    y[0::2] = S // 2
    y[1::2] = S - S // 2
    return fr


def v0_frame():
    """64 x 136 with period 2 along its columns: V = 0 everywhere and
    H = 2 (T[r+2] - T[r]) = +-2 (r + 1) on map row r, T = the row's even +
    odd column value: every even |H| from 2 to 268."""
    w, h = V0_GEOM
    T = _chain(h - 2)
    fr = np.full(2 * w * h, 128, np.uint8)
    y = fr[:w * h].reshape(h, w)
    y[:, 0::2] = (T // 2)[:, None]
    y[:, 1::2] = (T - T // 2)[:, None]
    return fr


def check_axis(frame, width, height, axis):
    """axis "h0": H = 0 on every window pixel and |V| covers; "v0": the same
    with H and V exchanged."""
    H, V = (window(p, width, height) for p in edge_ref.hv(frame, width, height))
    zero, other = (H, V) if axis == "h0" else (V, H)
    assert not zero.any()
    assert covers(set(np.abs(other).reshape(-1).tolist()))
    assert (other > 0).any() and (other < 0).any()


def preview_chroma(width, height):
    """A chroma plane [height * width] that holds all 65536 (cb, cr) pairs on
    the pixel pairs of columns 2 .. width-3 of rows 0 .. height-3 (pair p:
    cb = p & 255, cr = p >> 8, in raster order, repeating)."""
    pairs = width // 2 - 2
    assert pairs * (height - 2) >= 65536
    p = np.arange(pairs * (height - 2)) % 65536
    c = np.full((height, width // 2, 2), 128, np.uint8)
    c[:height - 2, 1:width // 2 - 1, 0] = (p & 255).reshape(height - 2, pairs)
    c[:height - 2, 1:width // 2 - 1, 1] = (p >> 8).reshape(height - 2, pairs)
    return c.reshape(-1)


def preview_frame(level, chroma):
    w, h = PREVIEW_GEOM
    fr = edge_ref.level_frame(w, h, level)
    fr[w * h:] = chroma
    return fr


def preview_triples(frame, emap, seen):
    """Marks in seen[2^24] the (map value, cb, cr) of every pixel of columns
    2 .. width-3 of map rows 0 .. height-3."""
    w, h = PREVIEW_GEOM
    c = frame[w * h:].reshape(h, w // 2, 2).astype(np.int64)
    key = (emap.astype(np.int64) << 16) | np.repeat((c[:, :, 0] << 8) | c[:, :, 1], 2, axis=1)
    seen[key[:h - 2, 2:w - 2].reshape(-1)] = True
