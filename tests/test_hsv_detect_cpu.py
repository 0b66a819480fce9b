"""The reference and the case lists of test_gpu_hsv_detect_shapes.py, checked
without a GPU: hsv_detect_ref's restatement of HsvRangeDetector::detect
against oracle.run, and every claim the GPU test's cases rest on (which
kernel form runs, which zone-edge classes are met, that a shifted zone, a
lost tie or an S or V one off would change the expected output), on the
reference's own output or through hsv_detect_cases.form()."""
import numpy as np
import pytest

import hsv_detect_cases as C
import hsv_detect_ref as R
from gpu_util import T0

YUYV, OV = C.LAYOUT_YUYV, C.LAYOUT_OV7670
LAYOUTS = [YUYV, OV]


def _oracle(oracle_mod, frame, w, h, ll, layout):
    rc, d, _ = oracle_mod.run(frame, w, h, ll, layout, T0, auto_detect=True, preview=False)
    assert rc == 0
    return [d["detect_hue"], d["detect_hue_tol"], d["detect_sat"], d["detect_sat_tol"], d["detect_val"],
            d["detect_val_tol"]]


@pytest.fixture(scope="module")
def table_t(table):
    import torch

    return torch.from_numpy((table & 0xFFFFFFFF).astype(np.int32))


def _hsv_of(table, y, u, v):
    e = int(table[y | (u << 8) | (v << 16)]) & 0xFFFFFFFF
    return e & 255, (e >> 8) & 255, (e >> 16) & 255


@pytest.mark.parametrize("layout", LAYOUTS)
def test_restatement_equals_oracle_run(oracle_mod, table, layout):
    """Widths 32 / 64 / 96, heights 4..216, minimal and padded lines: frames
    of four colours, three of them with equal counts in the zone (ties), and
    frames of random bytes."""
    rng = np.random.default_rng(0x7A1C + layout)
    ties = built = 0
    for w in C.SWEEP_WIDTHS:
        for h in C.SWEEP_HEIGHTS:
            for pad in (0, 16):
                ll = C.min_ll(w, layout) + pad
                Y = np.asarray(C.LUMA, np.uint8)[rng.integers(0, 4, (h, C.slots(ll, layout)))]
                r0, r1, c0, c1 = R.zone(w, h)
                if r0 < r1 and c0 < c1:  # three colours with equal counts in the zone, shuffled
                    n = (r1 - r0) * (c1 - c0)
                    built += n >= 3
                    seq = np.concatenate([np.repeat(np.arange(3), n // 3), np.full(n % 3, 3)])
                    Y[r0:r1, c0:c1] = np.asarray(C.LUMA, np.uint8)[rng.permutation(seq)].reshape(r1 - r0, c1 - c0)
                fr = C.luma_frame(Y, *C.UV, layout)
                got, tied = R.detect_hsv(R.pixel_hsv(table, fr, w, h, ll, layout), want_tied=True)
                ties += any(t.size > 1 for t in tied)
                assert got == _oracle(oracle_mod, fr, w, h, ll, layout), (w, h, ll)
                fr = rng.integers(0, 256, C.frame_bytes(w, h, ll, layout), dtype=np.uint8)
                assert R.detect(table, fr, w, h, ll, layout) == _oracle(oracle_mod, fr, w, h, ll, layout), (w, h, ll)
    assert ties == built > 200


def test_zone_is_the_detectors():
    assert R.zone(32, 12) == (5, 8, 15, 18) and R.zone(32, 20) == (8, 13, 14, 19)
    assert R.zone(64, 8) == (4, 5, 32, 33)
    r0, r1, c0, c1 = R.zone(32, 480)  # w/2 < step: the uint16 bounds wrap, nothing lies between them
    assert c0 > c1
    r0, r1, c0, c1 = R.zone(32, 4)  # step 0
    assert r0 >= r1 and c0 >= c1
    for h, n in zip(C.TIE_HEIGHTS, (81, 289, 1089)):
        r0, r1, c0, c1 = R.zone(C.TIE_WIDTH, h)
        assert (r1 - r0) * (c1 - c0) == n


def test_small_zone_winners_equals_winner():
    import torch

    rng = np.random.default_rng(5)
    for p, top in ((9, 3), (9, 256), (25, 4)):
        v = rng.integers(0, top, (500, p))
        got = R.small_zone_winners(torch.from_numpy(v)).numpy()
        assert got.tolist() == [R.winner(row)[0] for row in v]


# ---------------------------------------------------------------------------
# form()
# ---------------------------------------------------------------------------
def test_form_kernels():
    assert C.form(640, 480, 1280, YUYV, 6).kernel == "vec"
    assert C.form(640, 480, 1280, YUYV, 6, base_offset=4).kernel == "k1024"
    assert C.form(640, 480, 1280, YUYV, 33, base_offset=4).kernel == "k256"
    assert C.form(96, 72, 200, YUYV, 8).kernel == "k1024"
    # a frame stride that is no multiple of 16: only a single frame stays with the chunked kernel
    fb = C.frame_bytes(64, 32, 128, YUYV)
    assert C.form(64, 32, 128, YUYV, 4, frame_stride=fb + 8).kernel == "k1024"
    assert C.form(64, 32, 128, YUYV, 1, frame_stride=fb + 8).kernel == "vec"
    f = C.form(640, 480, 1280, YUYV, 1)  # the zone's 3,180 chunks (trik_hsv_operator.hip)
    assert f.total == 3180 and f == C.Form("vec", 30, 20, 1, 8, 3180)
    assert C.form(32, 4, 64, YUYV, 1).total == 0 and C.form(32, 480, 64, YUYV, 1).total == 0


# ---------------------------------------------------------------------------
# A. zone edges
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("layout,count", [(YUYV, 9), (OV, 17)])
def test_edge_geometries_reach_every_class(layout, count):
    want = C.reachable_edge_classes(layout)
    assert len(want) == count
    got = {C.edge_class(C.form(w, h, C.min_ll(w, layout) + pad, layout, 1))
           for w, h in C.edge_geometries(layout) for pad in (0, 16)}
    assert got == want
    assert len(C.edge_geometries(layout)) == count


@pytest.mark.parametrize("layout", LAYOUTS)
def test_edge_frames_flip_under_every_alteration(oracle_mod, table, layout):
    flips = 0
    geoms = C.edge_geometries(layout) + [(32, 12), (32, 20), (96, 100)]
    for w, h in geoms:
        zn = R.zone(w, h)
        for pad in (0, 16):
            ll = C.min_ll(w, layout) + pad
            for what in C.edge_alterations(w, h):
                fr = C.edge_frame(w, h, ll, layout, what)
                true = R.detect(table, fr, w, h, ll, layout)
                assert true == _oracle(oracle_mod, fr, w, h, ll, layout)
                assert true == R.scale(_hsv_of(table, C.LUMA[0], *C.UV)), "A wins the true zone"
                assert R.detect(table, fr, w, h, ll, layout, zn=R.alter(zn, what)) != true, (w, h, ll, what)
                flips += 1
            if len(C.edge_alterations(w, h)) == 6:
                # the one-pixel zone: no content right of or below it can win, a tie keeps the earlier pixel
                fr = C.edge_frame(w, h, ll, layout, "L+")
                for what in ("R+", "B+"):
                    assert R.detect(table, fr, w, h, ll, layout, zn=R.alter(zn, what)) == \
                        R.detect(table, fr, w, h, ll, layout)
    assert flips == 2 * (8 * len(geoms) - 2)


# ---------------------------------------------------------------------------
# B. ties
# ---------------------------------------------------------------------------
def test_tie_colours_differ_in_exactly_their_mask(table):
    for mask, (u, v, ya, yb, yc) in C.TIE_COLOURS.items():
        a, b, c = (_hsv_of(table, y, u, v) for y in (ya, yb, yc))
        assert sum((a[k] != b[k]) << k for k in range(3)) == mask
        assert sum((R.scale(a)[2 * k] != R.scale(b)[2 * k]) << k for k in range(3)) == mask
        assert all(c[k] != a[k] and c[k] != b[k] for k in range(3))
    four = [_hsv_of(table, y, *C.UV) for y in C.LUMA]
    assert four[:2] == [(7, 230, 211), (9, 142, 255)]
    assert all(len({f[k] for f in four}) == 4 for k in range(3))
    assert len({tuple(R.scale(f)[::2]) for f in four}) == 4


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("h", C.TIE_HEIGHTS)
def test_tie_frames_are_decisive(oracle_mod, table, h, layout):
    w, ll = C.TIE_WIDTH, C.min_ll(C.TIE_WIDTH, layout)
    zn = R.zone(w, h)
    n = (zn[1] - zn[0]) * (zn[3] - zn[2])
    frames = C.tie_frames(h, layout)
    not_smallest = {}
    ranks = [set(), set(), set()]
    for fr, (name, lumas, uv, seq, outside, mask) in zip(frames, C.tie_cases(h)):
        hsv3 = R.pixel_hsv(table, fr, w, h, ll, layout)
        got, tied = R.detect_hsv(hsv3, want_tied=True)
        assert got == _oracle(oracle_mod, fr, w, h, ll, layout), name
        k_way = 3 if name.startswith("three") else 2
        assert [t.size for t in tied] == [k_way if (mask >> k) & 1 else 1 for k in range(3)], name
        first = _hsv_of(table, lumas[_first_colour(seq, k_way)], *uv)
        assert got == R.scale(first), name
        for k in range(3):
            if (mask >> k) & 1:
                rank = int(np.searchsorted(tied[k], first[k]))
                if k_way == 3:
                    ranks[k].add(rank)
                else:
                    key = (mask, name.split("-")[2], k)
                    not_smallest[key] = not_smallest.get(key, False) or rank > 0
        # where the deciding last occurrences lie
        lasts = sorted(int(np.flatnonzero(seq == c)[-1]) for c in range(k_way))
        variant = name.split("-")[-1] if k_way == 2 else "waves"
        assert lasts == C.tie_positions(n, variant, k_way)
        for block in (256, 1024):
            passes = {p // block for p in lasts}
            waves = [(p % block) // 64 for p in lasts]
            if variant == "final":
                assert passes == {(n - 1) // block} and n % block != 0
            else:
                assert len(passes) == 1 and len(set(waves)) == min(k_way, -(-min(n, block) // 64))
        # the winner's colour also lies right of and below the zone: its last
        # occurrence taken over a widened zone would hand the tie to another value
        if outside == _first_colour(seq, k_way):
            for what in ("R+", "B+"):
                assert R.detect_hsv(hsv3, zn, last_zone=R.alter(zn, what)) != got, (name, what)
    assert len(not_smallest) == 2 * 12 and all(not_smallest.values())
    assert ranks == [{0, 1, 2}] * 3


def _first_colour(seq, k_way):
    """The tied colour whose last occurrence comes first."""
    return min(range(k_way), key=lambda c: int(np.flatnonzero(seq == c)[-1]))


# ---------------------------------------------------------------------------
# C. more than one load batch of chunks
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
def test_big_frame(oracle_mod, table, layout):
    w, h = C.BIG[layout]
    assert (w, h) == C.big_geometry(layout)
    ll = C.min_ll(w, layout)
    f = C.form(w, h, ll, layout, 1)
    assert f.kernel == "vec" and C.VEC_BATCH_CHUNKS < f.total < 2 * C.VEC_BATCH_CHUNKS
    assert C.form(w, h - 4, ll, layout, 1).total <= C.VEC_BATCH_CHUNKS
    fr = C.big_frame(layout)
    hsv3 = R.pixel_hsv(table, fr, w, h, ll, layout)
    got, tied = R.detect_hsv(hsv3, want_tied=True)
    assert got == _oracle(oracle_mod, fr, w, h, ll, layout)
    a, p = (_hsv_of(table, y, *C.UV) for y in C.LUMA[:2])
    assert [t.tolist() for t in tied] == [sorted((a[k], p[k])) for k in range(3)]
    assert got == R.scale(a) and a[1] > p[1], "A wins, and in S it is not the smallest tied value"
    r0, r1, c0, c1 = R.zone(w, h)
    zone_h = hsv3[0][r0:r1, c0:c1]
    rr, cc = np.meshgrid(np.arange(r0, r1), np.arange(c0, c1), indexing="ij")
    j = C.chunk_index(w, h, layout, rr, cc)
    last_a, last_p = (int(j[zone_h == c[0]].max()) for c in (a, p))
    assert last_a < C.VEC_BATCH_CHUNKS <= last_p
    for what in ("R+", "B+"):
        assert R.detect_hsv(hsv3, (r0, r1, c0, c1), last_zone=R.alter((r0, r1, c0, c1), what)) != got


# ---------------------------------------------------------------------------
# D, E. every (Y, U, V)
# ---------------------------------------------------------------------------
def _sample_triples():
    import torch

    rng = np.random.default_rng(11)
    corners = [y | (u << 8) | (v << 16) for y in (0, 255) for u in (0, 128, 255) for v in (0, 128, 255)]
    return torch.from_numpy(np.concatenate([np.asarray(corners, np.int64), rng.integers(0, 1 << 24, 300)]))


def test_other_luma_never_equal():
    assert all(C.other_luma(y) != y and 0 <= C.other_luma(y) < 256 for y in range(256))


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("geom", sorted(C.D_GEOMS))
def test_d_frames_winners_are_the_triple(oracle_mod, table, table_t, geom, layout):
    w, h, major = C.D_GEOMS[geom]
    r0, r1, c0, c1 = R.zone(w, h)
    cols = np.arange(c0, c1)
    assert 2 * int((cols % 2 == major).sum()) > cols.size
    tr = _sample_triples()
    frames = C.to_layout(C.d_words(tr, geom), layout).numpy()
    want = C.d_expected(tr, table_t).tolist()
    ll = C.min_ll(w, layout)
    assert frames.shape[1] == C.frame_bytes(w, h, ll, layout)
    for i, fr in enumerate(frames):
        assert R.detect(table, fr, w, h, ll, layout) == want[i], int(tr[i])
        if i < 40:
            assert _oracle(oracle_mod, fr, w, h, ll, layout) == want[i]


@pytest.mark.parametrize("ch", [1, 2])
def test_e_tables(table, ch):
    vals = ((table & 0xFFFFFFFF) >> (8 * ch)) & 255
    count = np.bincount(vals.astype(np.int64), minlength=256)
    assert table[np.isin(vals, np.flatnonzero(count == 1))].tolist() == C.E_SINGLE_TRIPLES and (count >= 2).all(), "a probe for every value"
    q1, q2, z, wf = C.e_tables(table, ch)
    v = np.arange(256)
    assert (q1 != q2).all() and (vals[q1] == v).all() and (vals[q2] == v).all()
    assert (vals[z] == (v + 128) & 255).all() and (vals[wf] == (v + 64) & 255).all()
    # X's value one off (the kernel's, not the table's) in both pixels of its
    # pair, in the first or in the second: the rival wins and the output differs
    xs = [i for i, k in enumerate(C.E_ZONE) if k == "x"]
    for x in range(256):
        zone = {"q": x, "x": x, "z": int(vals[z[x]]), "w": int(vals[wf[x]])}
        px = np.asarray([zone[k] for k in C.E_ZONE])
        assert R.winner(px)[0] == x
        for d in (-1, 1):
            for where in (xs, xs[:1], xs[1:]):
                if 0 <= x + d < 256:
                    off = px.copy()
                    off[where] = x + d
                    win = R.winner(off)[0]
                    assert win == zone["z"] and R.SV_OUT[win] != R.SV_OUT[x], (x, d, where)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("ch", [1, 2])
def test_e_frames(oracle_mod, table, table_t, ch, layout):
    import torch

    assert R.zone(32, 12) == (5, 8, 15, 18)
    tabs = torch.from_numpy(C.e_tables(table, ch))
    tr = torch.cat([_sample_triples(), tabs[0][::16], tabs[1][::16]])  # triples that are their value's own probe too
    t = C.e_triples(tr, tabs, table_t, ch)
    assert bool((t["q"] != tr).all())
    frames = C.to_layout(C.e_words(t), layout).numpy()
    want = C.e_expected(t, table_t).tolist()
    ll = C.min_ll(32, layout)
    for i, fr in enumerate(frames):
        assert R.detect(table, fr, 32, 12, ll, layout) == want[i], int(tr[i])
        x = _hsv_of(table, int(tr[i]) & 255, (int(tr[i]) >> 8) & 255, int(tr[i]) >> 16)
        assert want[i][2 * ch] == R.SV_OUT[x[ch]]
        if i < 40:
            assert _oracle(oracle_mod, fr, 32, 12, ll, layout) == want[i]
