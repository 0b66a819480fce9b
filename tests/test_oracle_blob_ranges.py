"""What tests/blob_ranges_cases.py claims, asserted on the oracle (no GPU):
the palette, the frame builders, the ov7670 / YUYV twin relation that defines
trik_hsv_blob_batch_ranges on YUYV frames, and the packed-state form of the
expectation.  Then the host-only half of the new C ABI: trik_hsv_blob_range_of
and the new exports."""
import ctypes as C

import numpy as np
import pytest

import blob_patterns
import blob_ranges_cases as cases


def _uniform(yuv, w=32, h=4):
    fr = np.empty(2 * h * w, np.uint8)
    fr[: h * w] = yuv[0]
    fr[h * w::2] = yuv[2]   # V: the even chroma byte
    fr[h * w + 1::2] = yuv[1]
    return fr


def _ranges():
    return [cases.from_to(h) for h in cases.ALL_HSV]


def test_helper_constants_are_the_oracles(oracle_mod):
    assert cases.RED_HSV == oracle_mod.RED_HSV
    assert cases.from_to(cases.RED_HSV) == (340, 20, 60, 100, 0, 100)
    for hsv in cases.ALL_HSV:
        assert oracle_mod.blob_range(hsv) == oracle_mod.pack_range(cases.from_to(hsv)), hsv


def test_palette_ranges_hold_their_colour_only(oracle_mod):
    rs = _ranges()
    for i, yuv in enumerate(cases.COLOURS):
        sums, mask = oracle_mod.frame(_uniform(yuv), 32, 4, 32, oracle_mod.LAYOUT_OV7670, rs, want_mask=True)
        want = (1 << i) | (16 if i in (0, 3) else 0)  # the wrapping range holds red and yellow
        assert (mask == want).all(), (i, np.unique(mask))
        # the other pixel of a coloured pair lies in no range
        _, off = oracle_mod.frame(_uniform((cases.OFF_Y[i],) + yuv[1:]), 32, 4, 32, oracle_mod.LAYOUT_OV7670, rs,
                                  want_mask=True)
        assert not off.any(), i
    for y in (100, 130, 159):  # the grey of the builders
        _, mask = oracle_mod.frame(_uniform((y, 128, 128)), 32, 4, 32, oracle_mod.LAYOUT_OV7670, rs, want_mask=True)
        assert not mask.any()


def test_packed_state_form_equals_centre_tolerance_form(oracle_mod):
    w, h, ll = 64, 32, 80
    fr = oracle_mod.blob_scene(w, h, ll, 3, noise=0.02)
    for hsv in cases.ALL_HSV:
        a = oracle_mod.blob_run(fr, w, h, ll, hsv=hsv, preview=False)
        b = cases.expect(oracle_mod, fr, w, h, ll, cases.from_to(hsv))
        for key in ("rc", "n_labels", "state"):
            assert a[key] == b[key], (hsv, key)
        for key in ("meta", "labels", "top", "targets"):
            assert np.array_equal(a[key], b[key]), (hsv, key)


@pytest.mark.parametrize("geom", [(32, 4, 32), (64, 32, 80), (352, 96, 352)])
@pytest.mark.parametrize("t", [1, 3, 4])
def test_mosaic_yields_the_intended_bitmaps(oracle_mod, geom, t):
    w, h, ll = geom
    rs = _ranges()
    for off in range(4):
        metas = cases.pattern_stack(h // 4, w // 4, t, off)
        fr = cases.mosaic(metas, ll, seed=off)
        _, mask = oracle_mod.frame(fr, w, h, ll, oracle_mod.LAYOUT_OV7670, rs, want_mask=True)
        for i in range(t):
            cnt = cases.counts_of(mask, i)
            assert np.array_equal(cnt > 2, metas[i] != 0), (geom, t, off, i)
            assert cnt[metas[i] != 0].min(initial=3) >= 3 and cnt[metas[i] == 0].max(initial=0) <= 2
            ref = cases.expect(oracle_mod, fr, w, h, ll, rs[i])
            assert np.array_equal(ref["meta"], metas[i]), (geom, t, off, i)
        for i in range(t, 4):
            assert not cases.counts_of(mask, i).any()
        if t == 4:  # the wrapping range: red or yellow
            assert np.array_equal(cases.counts_of(mask, 4), cases.counts_of(mask, 0) + cases.counts_of(mask, 3))


def test_mosaic_reaches_every_count(oracle_mod):
    seen = set()
    for seed in range(6):
        metas = blob_patterns.rand(8, 16, 0.5, seed)[None]
        _, mask = oracle_mod.frame(cases.mosaic(metas, seed=seed), 64, 32, 64, oracle_mod.LAYOUT_OV7670, _ranges()[:1],
                                   want_mask=True)
        seen |= set(cases.counts_of(mask, 0).reshape(-1).tolist())
    assert seen == set(range(17))


@pytest.mark.parametrize("t", range(4))
def test_count_ladder(oracle_mod, t):
    """Exactly k pixels of a colour in a metapixel, k = 0..16: set iff k > 2."""
    fr, k = cases.ladder(t)
    rs = _ranges()
    _, mask = oracle_mod.frame(fr, 96, 4, 96, oracle_mod.LAYOUT_OV7670, rs, want_mask=True)
    assert set(k.tolist()) == set(range(17))
    assert np.array_equal(cases.counts_of(mask, t)[0], k)
    for other in set(range(4)) - {t}:
        assert not cases.counts_of(mask, other).any()
    ref = cases.expect(oracle_mod, fr, 96, 4, 96, rs[t])
    assert np.array_equal(ref["meta"][0], k > 2)


def test_lane_ladder_counts(oracle_mod):
    fr, k = cases.lane_ladder()
    _, mask = oracle_mod.frame(fr, 96, 4, 96, oracle_mod.LAYOUT_OV7670, cases.LANE_RANGES, want_mask=True)
    assert set(k.tolist()) == set(range(17))
    assert np.array_equal(cases.counts_of(mask, 0)[0], k)
    for i, want in enumerate(cases.LANE_COUNTS):
        assert (cases.counts_of(mask, i + 1) == want).all(), i


@pytest.mark.parametrize("ll_extra", [0, 16])
def test_yuyv_twin_has_the_same_masks(oracle_mod, ll_extra):
    """The contract of the YUYV form: the same (Y, U, V) per pixel, so the
    same per-pixel masks, whose 4x4 counts tested > 2 are blob_run's bitmap."""
    w, h, ll = 64, 32, 80
    rs = _ranges()
    frames = [oracle_mod.blob_scene(w, h, ll, 7, noise=0.05), cases.mosaic(cases.pattern_stack(8, 16, 4), ll, seed=1),
              np.random.default_rng(2).integers(0, 256, 2 * h * ll, dtype=np.uint8)]
    for fr in frames:
        tw = cases.to_yuyv(fr, w, h, ll, 2 * w + ll_extra, seed=9)
        sa, ma = oracle_mod.frame(fr, w, h, ll, oracle_mod.LAYOUT_OV7670, rs, want_mask=True)
        sb, mb = oracle_mod.frame(tw, w, h, 2 * w + ll_extra, oracle_mod.LAYOUT_YUYV, rs, want_mask=True)
        assert np.array_equal(ma, mb) and np.array_equal(sa, sb)
        for i, r in enumerate(rs):
            assert np.array_equal(cases.counts_of(mb, i) > 2, cases.expect(oracle_mod, fr, w, h, ll, r)["meta"]), i
    # the twin's bytes: Y0 U Y1 V with U the odd and V the even chroma byte
    fr = np.arange(2 * 4 * 32, dtype=np.uint8)
    tw = cases.to_yuyv(fr, 32, 4, 32, 64).reshape(4, 64)
    assert tw[1, :8].tolist() == [32, 128 + 33, 33, 128 + 32, 34, 128 + 35, 35, 128 + 34]


def test_blob_range_of_equals_the_oracle(oracle_mod):
    import trik_hsv

    tols = (0, 1, 20, 179, 180, 359)
    for hue in range(360):
        for tol in tols:
            hsv = (hue, tol, 80, 20, 50, 50)
            r = trik_hsv.blob_range_of(hsv)
            assert r == cases.from_to(hsv), hsv
            assert oracle_mod.pack_range(r) == oracle_mod.blob_range(hsv), hsv
    for sat, st, val, vt in ((0, 0, 100, 0), (0, 30, 100, 30), (100, 100, 0, 100), (10, 20, 90, 20), (50, 50, 50, 50),
                             (99, 1, 1, 1), (99, 2, 1, 2), (255, 10, 255, 10), (100, 255, 0, 255)):
        hsv = (120, 20, sat, st, val, vt)
        r = trik_hsv.blob_range_of(hsv)
        assert oracle_mod.pack_range(r) == oracle_mod.blob_range(hsv), hsv
        assert all(0 <= v <= 100 for v in r[2:])


def test_blob_range_of_refuses_null():
    from trik_hsv import _abi

    lib = _abi.load()
    alg, out = _abi.OV7670InArgsAlg(1, 0, 20, 80, 20, 50, 50, 0), _abi.InArgsAlg()
    assert lib.trik_hsv_blob_range_of(None, C.byref(out)) != 0 and "NULL" in _abi.last_error()
    assert lib.trik_hsv_blob_range_of(C.byref(alg), None) != 0
    assert lib.trik_hsv_blob_range_of(C.byref(alg), C.byref(out)) == 0
    assert (out.detectHueFrom, out.detectHueTo, out.autoDetectHsv) == (340, 20, 0)


def test_blob_ranges_symbols_are_exported():
    import trik_hsv
    from trik_hsv import _abi

    lib = _abi.load()
    for name in ("trik_hsv_blob_batch_ranges", "trik_hsv_blob_range_of"):
        assert getattr(lib, name) and name in _abi.PROTOTYPES
    assert trik_hsv.BLOB_CHUNK_SLOTS == 4096
    assert callable(trik_hsv.Detector.blob_batch_ranges)
