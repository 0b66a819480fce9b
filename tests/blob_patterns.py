"""Structured metapixel bitmaps for the multi-blob clusterer tests, a vectorised
frame builder for them, and the comparison both GPU blob test files share
(test code, not product).

Each pattern exists for one property of Clusterizer::run (CLU:85-127) that
random bitmaps and discs do not produce on purpose; tests/test_oracle_blob.py
asserts those properties on the CPU, so a pattern cannot quietly lose its."""
import numpy as np


def patterns(bh, bw):
    """name -> uint8 [bh, bw], deterministic; every pattern is defined for any
    bh >= 1, bw >= 1 (a one-row bitmap has no bridges and no arms)."""
    z = lambda: np.zeros((bh, bw), np.uint8)  # noqa: E731
    rows, cols = np.arange(bh)[:, None], np.arange(bw)[None, :]
    p = {"full": np.ones((bh, bw), np.uint8), "empty": z()}
    m = z()
    m[0, 0] = m[0, -1] = m[-1, 0] = m[-1, -1] = 1
    p["corners"] = m
    m = z()
    m[0, :] = m[-1, :] = m[:, 0] = m[:, -1] = 1
    p["border"] = m
    # every set metapixel opens a label: the label capacity, blob_max_labels(bw, bh)
    m = z()
    m[0::2, 0::2] = 1
    p["iso_grid"] = m
    # runs across all 64 lanes, each row one label
    m = z()
    m[0::2, :] = 1
    p["hstripes"] = m
    # every run opens in row 0; (bw + 1) // 2 clusters of equal size bh - 1
    m = z()
    m[:, 0::2] = 1
    p["vstripes"] = m
    # all merges in the last row, left to right
    m = z()
    m[:, 0::2] = 1
    m[-1, :] = 1
    p["comb_up"] = m
    # joined from the first row: one label
    m = z()
    m[:, 0::2] = 1
    m[0, :] = 1
    p["comb_down"] = m
    # period-4 diagonals: the up-left (dn) and up-right (up) neighbour alone
    # carries the label, across lane boundaries, column 0 and column bw - 1
    p["diag_dn"] = ((cols - rows) % 4 == 0).astype(np.uint8)
    p["diag_up"] = ((cols + rows) % 4 == 0).astype(np.uint8)
    # V shapes of period 2 * bh: two labels open in row 0, the arms meet in the last row
    cc = cols % (2 * bh)
    p["vees"] = ((cc == rows) | (cc == 2 * (bh - 1) - rows)).astype(np.uint8)
    # alternate full rows linked at alternating ends (right first)
    m = z()
    m[0::2, :] = 1
    for i, r in enumerate(range(1, bh - 1, 2)):
        m[r, 0 if i % 2 else bw - 1] = 1
    p["serpentine"] = m
    # teeth of different lengths joined by the last row
    m = z()
    start = (np.arange(bw) // 2) % max(bh - 1, 1)
    m[:, :] = (rows >= start[None, :]) & (cols % 2 == 0)
    m[-1, :] = 1
    p["stair_comb"] = m
    # alternate columns; each odd column between two of them holds one bridge
    # metapixel, the bridge rows cycling 1 .. bh - 1 from the right (rtl: each
    # merge rewrites the eq entry that the one before it copied, so entries go
    # stale) or from the left (ltr: labels flatten as they go)
    odd = np.arange(1, bw - 1, 2)
    for name, order in (("bridges_rtl", odd[::-1]), ("bridges_ltr", odd)):
        m = z()
        m[:, 0::2] = 1
        if bh > 1:
            for k, c in enumerate(order):
                m[1 + k % (bh - 1), c] = 1
        p[name] = m
    p["rand45"] = rand(bh, bw, 0.45, 45)
    return p


def rand(bh, bw, density, seed):
    return (np.random.default_rng(seed).random((bh, bw)) < density).astype(np.uint8)


def frame(meta, line_length=None, seed=0):
    """oracle.blob_frame's construction without its loop per metapixel (another
    byte stream, the same contract): an ov7670 frame in which a set metapixel
    has 3..16 red pixels and an unset one 0..2, so that under oracle.RED_HSV
    exactly `meta` is set; random padding bytes."""
    rng = np.random.default_rng(seed)
    meta = np.asarray(meta) != 0
    bh, bw = meta.shape
    h, w = 4 * bh, 4 * bw
    ll = w if line_length is None else line_length
    fr = rng.integers(0, 256, 2 * h * ll, dtype=np.uint8)
    y = fr[: h * ll].reshape(h, ll)
    c = fr[h * ll:].reshape(h, ll)
    k = np.where(meta, rng.integers(3, 17, (bh, bw)), rng.integers(0, 3, (bh, bw)))
    rank = rng.random((bh, bw, 16)).argsort(axis=2).argsort(axis=2)  # a random order of each block's 16 pixels
    red = (rank < k[:, :, None]).reshape(bh, bw, 4, 4).transpose(0, 2, 1, 3).reshape(h, w)
    # a pixel is red iff its pair carries red chroma and its Y is the dark
    # value; the grey pixel of a red pair gets a bright Y outside RED_HSV
    pair = red[:, 0::2] | red[:, 1::2]
    grey_in_red_pair = ~red & np.repeat(pair, 2, axis=1)
    yv = np.where(red, 80, rng.integers(100, 160, (h, w))).astype(np.uint8)
    yv[grey_in_red_pair] = 250
    y[:, :w] = yv
    c[:, 0:w:2] = np.where(pair, 215, 128)
    c[:, 1:w:2] = np.where(pair, 100, 128)
    return fr


def check_frame(res, i, ref, what):
    """Frame i of Detector.blob_batch(..., meta=True, labels=True) against one
    oracle.blob_run result: bitmap, label map, label count, the 8 largest
    clusters, the 8 targets -- all bit-exact."""
    assert ref["rc"] == 0
    assert np.array_equal(np.asarray(res["meta"][i].cpu()), ref["meta"]), what
    assert np.array_equal(np.asarray(res["labels"][i].cpu()).view(np.uint16), ref["labels"]), what
    assert int(res["n_labels"][i]) == ref["n_labels"], what
    assert np.array_equal(np.asarray(res["top"][i].cpu()), ref["top"]), what
    assert np.array_equal(np.asarray(res["targets"][i, :, :3].cpu()), ref["targets"]), what
