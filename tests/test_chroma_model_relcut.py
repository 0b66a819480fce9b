"""CPU model of the chroma-run tables as the device stores them: run
descriptors relative to their block's cut (trik_hsv_chroma.hip:
chroma_desc_rel, select2), on top of tests/test_chroma_model.py's absolute
model (profiles, build).

The hot kernel takes the block's cut A from both Y of a word with one packed
subtract, t = (Y - A) mod 256, and compares t with b1' = max(b1 - A, 0) and
b2' = b2 - A: `t <= b2' ? (t < b1' ? M1 : M2) : 0`, window pixels b2' < t < b1'
flagged.  A pixel below the cut wraps to t >= 256 - A, above every b1' and b2'
of the block (<= 255 - A), so it gets 0 and no flag -- what the absolute
form's `Y >= A` compare did.  For the bench's 4-range set and its 1-range set,
over all 2^24 (Y, U, V):

* the relative fast mask equals the oracle's mask at every unflagged Y;
* the flagged set equals the absolute model's exactly (the exact-path word
  share stays what it was: 0.0288 of the words at 4 ranges, below 0.005 at 1);
* b2 >= A for every descriptor of a cut block but the exception code, which
  stays absolute, and no relative descriptor of a cut block equals that code.

The blocks with a cut of the 4-range set are also kept as a fixture
(tests/golden/relcut_blocks.json: block index and cut) for the GPU test
tests/test_gpu_chroma_relcut.py, which crafts its frames from them; this test
holds the fixture to the model.
"""
import json
import os

import numpy as np
import pytest

from test_chroma_model import BENCH, KEXC, build, profiles

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "relcut_blocks.json")


def relative(runs, M1, A):
    """chroma_desc_rel for every chroma: absolute descriptors `runs` under the
    block's first mask M1 and cut A (arrays per chroma)."""
    b1, b2 = runs & 255, runs >> 8
    rel = np.maximum(b1 - A, 0) | (np.maximum(b2 - A, 0) << 8)
    # b2 < A: nothing at or above the cut is set; expressible when M1 = 0 and
    # nothing is flagged there (b1 <= A) as "M1 on the whole of [A, 255]"
    under = b2 < A
    rel = np.where(under, np.where((M1 == 0) & (b1 <= A), (256 - A) | ((255 - A) << 8), KEXC), rel)
    return np.where((runs == KEXC) | (A == 0), runs, rel)


@pytest.fixture(scope="module")
def models(oracle_mod):
    out = {}
    for n in (4, 1):
        P = profiles(oracle_mod, BENCH[:n])
        out[n] = (P,) + tuple(build(P))
    return out


@pytest.mark.parametrize("n_ranges,lo,hi", [(4, 0.02875, 0.02885), (1, 0.0, 0.005)])
def test_relative_descriptors_exact_on_all_triples(models, n_ranges, lo, hi):
    P, runs, blocks, cut = models[n_ranges]
    Y = np.arange(256)[None, :]
    kk, AA = np.repeat(blocks, 16), np.repeat(cut, 16)
    M1, M2, A = (kk & 15)[:, None], (kk >> 4)[:, None], AA[:, None]
    # the absolute form (tests/test_chroma_model.py)
    b1, b2 = (runs & 255)[:, None], (runs >> 8)[:, None]
    x = (runs == KEXC)[:, None]
    flagged_abs = x | ((Y < b1) & (Y > b2))
    # every descriptor of a cut block but the exception code has b2 >= A
    # (this range set never meets chroma_desc_rel's b2 < A branch)
    assert ((runs >> 8) >= AA)[(runs != KEXC) & (AA > 0)].all()
    # the relative form
    rel = relative(runs, kk & 15, AA)
    assert not (rel[(AA > 0) & (runs != KEXC)] == KEXC).any()
    assert ((rel & 255) <= 255 - AA)[rel != KEXC].all() and ((rel >> 8) <= 255 - AA)[rel != KEXC].all()
    r1, r2 = (rel & 255)[:, None], (rel >> 8)[:, None]
    xr = (rel == KEXC)[:, None]
    t = (Y - A) & 255
    lt, le = t < r1, (t <= r2) & ~xr
    fast = np.where(le, np.where(lt, M1, M2), 0)
    flagged = xr | (lt & (t > r2))
    assert np.array_equal(flagged, flagged_abs)           # bit-identical exact-path set
    assert (fast[flagged] == 0).all()                     # the exact path adds these
    assert np.array_equal(np.where(flagged, P, fast), P)  # everything else is exact
    words = (1 - (1 - flagged.mean(1)) ** 2).mean()       # a word: two uniform Y of one chroma
    assert lo <= words < hi, words


def test_relative_edge_forms():
    """chroma_desc_rel's branches the bench sets do not all meet."""
    def one(d, M1, A):
        return int(relative(np.array([d]), np.array([M1]), np.array([A]))[0])
    assert one(0 | 200 << 8, 3, 50) == 0 | 150 << 8            # starts at A with M2: b1 = 0 stays 0
    assert one(40 | 200 << 8, 3, 50) == 0 | 150 << 8           # b1 < A clamps to 0
    assert one(255 | 254 << 8, 0, 50) == 205 | 204 << 8        # the all-zero forms shift like the rest
    assert one(0 | 255 << 8, 3, 50) == 0 | 205 << 8
    assert one(255 | 254 << 8, 0, 255) == 1 | 0 << 8           # the one descriptor with b2 < A
    assert one(KEXC, 3, 50) == KEXC and one(KEXC, 3, 0) == KEXC  # the exception code stays absolute
    assert one(255 | 100 << 8, 3, 0) == 255 | 100 << 8         # A = 0: unchanged
    # all A for the all-zero form under M1 = 0: zero on [A, 255], no flag, also below the cut
    for A in range(1, 256):
        d = one(255 | 254 << 8, 0, A)
        t = (np.arange(256) - A) & 255
        lt, le = t < (d & 255), t <= (d >> 8)
        assert not (lt & ~le).any() and (lt | ~le)[t <= 255 - A].all() and not le[t > 255 - A].any()


def test_cut_block_fixture_matches_the_model(models):
    _, _, _, cut = models[4]
    b = np.nonzero(cut > 0)[0]
    with open(FIXTURE) as f:
        fx = json.load(f)
    assert fx["ranges"] == [list(r) for r in BENCH]
    assert fx["blocks"] == b.tolist() and fx["cuts"] == cut[b].tolist()
