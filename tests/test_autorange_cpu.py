"""The exact autoDetectHsv without a GPU: the restatement held to its own
sequential loop on every case, the library's host-side output scaling held to
the float32 restatement on every box, and the arguments the new calls refuse
(all refused before any GPU call)."""
import ctypes as C

import numpy as np
import pytest

import autorange_cases as AC
import autorange_ref as R

KINDS = [R.OBJECT, R.LINE, R.WLINE]


@pytest.fixture(scope="module")
def lib():
    import trik_hsv

    return trik_hsv


@pytest.mark.parametrize("kind", KINDS)
def test_vectorised_histogram_is_the_sequential_loop(kind):
    for case in AC.cases(kind):
        for i, w in enumerate(case.want()):
            hist, start, g = R.histogram_loop(w["cell"], w["pos"], w["neg"], R.bins_of(kind))
            st = [start >> 5, start & 31, g, 0] if kind == R.OBJECT else [start, 0, g, 0]
            assert np.array_equal(hist, w["hist"]) and st == w["start"], (case.name, i)


@pytest.mark.parametrize("kind", KINDS)
def test_best_box_is_the_objective_as_written(kind):
    """The search's L against m_foo / F summed cell by cell, and no single
    step of the annealing's moves from the best box improves it."""
    for case in AC.cases(kind):
        w = case.want()[0]
        l, a, b, c, d = w["best"]
        if kind == R.OBJECT:
            assert l == R.m_foo(w["hist"], a, b, c, d), case.name
            s_max = w["start"][1]
            assert c <= s_max <= d
            for h1, h2 in ((a - 1, b), (a + 1, b), (a, b - 1), (a, b + 1)):
                assert R.m_foo(w["hist"], h1 % 32, h2 % 32, c, d) <= l, case.name
        else:
            assert l == R.big_f(w["hist"], a, b), case.name
            for v0, v1 in ((a - 1, b), (a + 1, b), (a, b - 1), (a, b + 1)):
                if 0 <= v0 <= v1 <= 255:
                    assert R.big_f(w["hist"], v0, v1) <= l, case.name


def _of(lib, kind, h1, h2, s1, s2):
    out = (C.c_uint16 * 6)()
    rc = lib._lib.trik_hsv_auto_range_of(kind, h1, h2, s1, s2, out)
    return rc, list(out)


def test_auto_range_of_every_object_box(lib):
    i = np.arange(32)
    h1, h2, s1, s2 = (x.reshape(-1) for x in np.meshgrid(i, i, i, i, indexing="ij"))
    keep = s1 <= s2
    h1, h2, s1, s2 = h1[keep], h2[keep], s1[keep], s2[keep]
    assert len(h1) == 32 * 32 * 528
    want = R.range_of(R.OBJECT, h1, h2, s1, s2)
    fn = lib._lib.trik_hsv_auto_range_of
    out = (C.c_uint16 * 6)()
    got = np.empty((len(h1), 6), np.int64)
    for k, (a, b, c, d) in enumerate(zip(h1.tolist(), h2.tolist(), s1.tolist(), s2.tolist())):
        assert fn(0, a, b, c, d, out) == 0
        got[k] = out[:]
    bad = np.flatnonzero((got != want).any(axis=1))
    assert len(bad) == 0, (h1[bad[0]], h2[bad[0]], s1[bad[0]], s2[bad[0]], got[bad[0]], want[bad[0]])
    assert (h1 > h2).any() and (want[:, 0] < 360).all()


@pytest.mark.parametrize("kind", [R.LINE, R.WLINE])
def test_auto_range_of_every_interval(lib, kind):
    v0, v1 = np.nonzero(np.arange(256)[:, None] <= np.arange(256)[None, :])
    assert len(v0) == 256 * 257 // 2
    want = R.range_of(kind, v0, v1)
    for a, b, w in zip(v0.tolist(), v1.tolist(), want.tolist()):
        rc, got = _of(lib, kind, a, b, 7, 3)  # s1, s2 are ignored
        assert rc == 0 and got == w, (a, b, got, w)
    # the two copies differ: the ov7670 one scales v1 + 1, the webcam one v1
    assert R.range_of(R.LINE, 0, 102).tolist() == [0, 0, 0, 0, 20, 20]   # 103 * 0.39f -> 40
    assert R.range_of(R.WLINE, 0, 102).tolist() == [0, 0, 0, 0, 19, 19]  # 102 * 0.39f -> 39


def test_auto_range_of_refuses(lib):
    for args in ((0, -1, 0, 0, 0), (0, 0, 32, 0, 0), (0, 0, 0, 5, 4), (0, 0, 0, 0, 32), (0, 0, 0, -1, 3),
                 (1, 5, 4, 0, 0), (1, -1, 4, 0, 0), (2, 0, 256, 0, 0), (3, 0, 0, 0, 0), (-1, 0, 0, 0, 0)):
        rc, out = _of(lib, *args)
        assert rc != 0 and out == [0] * 6 and lib._abi.last_error(), args
    assert lib._lib.trik_hsv_auto_range_of(0, 0, 0, 0, 0, None) != 0
    with pytest.raises(lib.TrikHsvError):
        lib.auto_range_of(0, 40, 0, 0, 0)
    assert lib.auto_range_of(R.LINE, 10, 255) == tuple(R.range_of(R.LINE, 10, 255).tolist())


def _batch(lib, kind, w, h, ll=None, n=0, layout=None):
    ll = ((2 if kind == R.WLINE else 1) * w) if ll is None else ll
    return lib._abi.FrameBatch(None, 0, n, w, h, ll, R.layout_of(kind) if layout is None else layout)


@pytest.mark.parametrize("call", ["trik_hsv_auto_scores", "trik_hsv_batch_auto_range_exact"])
def test_batch_calls_refuse(lib, call):
    fn = getattr(lib._lib, call)
    ok = _batch(lib, R.OBJECT, 64, 48)
    assert fn(C.byref(ok), R.OBJECT, None, None, None) == 0  # an empty batch launches nothing
    bad = [(_batch(lib, R.OBJECT, 64, 48), 3),                         # unknown kinds
           (_batch(lib, R.OBJECT, 64, 48), -1),
           (_batch(lib, R.OBJECT, 64, 48, layout=0, ll=128), R.OBJECT),  # a layout that is not the kind's
           (_batch(lib, R.LINE, 64, 48, layout=0, ll=128), R.LINE),
           (_batch(lib, R.WLINE, 64, 48, layout=1), R.WLINE),
           (_batch(lib, R.OBJECT, 48, 48), R.OBJECT),                    # geometries SETPARAMS refuses
           (_batch(lib, R.LINE, 64, 50), R.LINE),
           (_batch(lib, R.LINE, 64, 48, ll=32), R.LINE),
           (_batch(lib, R.OBJECT, 2080, 48), R.OBJECT),                  # above the 2048 cap
           (_batch(lib, R.WLINE, 64, 2052), R.WLINE),
           (_batch(lib, R.OBJECT, 64, 48, n=-1), R.OBJECT)]
    for b, kind in bad:
        assert fn(C.byref(b), kind, None, None, None) != 0 and lib._abi.last_error(), (b.width, b.height, kind)
    assert fn(None, R.OBJECT, None, None, None) != 0
    # frames to read but no buffer to write
    one = lib._abi.FrameBatch(1 << 20, 0, 1, 64, 48, 64, 1)
    assert fn(C.byref(one), R.OBJECT, None, None, None) != 0


def test_set_auto_detect_refuses(lib):
    assert lib._lib.trik_hsv_set_auto_detect(None, 1) == -1 and lib._abi.last_error()
