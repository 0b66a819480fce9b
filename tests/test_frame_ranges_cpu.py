"""CPU-only checks of the per-frame-range call: every argument the C ABI
refuses is refused before any GPU call (there is no GPU here, and no pointer
is dereferenced on the host), the ctypes mirror has the prototypes, and the
inputs of tests/test_gpu_frame_ranges.py (tests/frame_ranges_cases.py) reach
what they are meant to reach, stated on the oracle's output."""
import ctypes as C

import numpy as np
import pytest

import frame_ranges_cases as FC

FAKE = 0x10000  # a non-NULL address nothing reads


@pytest.fixture(scope="module")
def abi():
    from trik_hsv import _abi

    return _abi


def _batch(abi, n=2, w=64, h=8, ll=128, layout=0, stride=None, frames=FAKE):
    return abi.FrameBatch(frames, h * ll * (2 if layout == 1 else 1) if stride is None else stride, n, w, h, ll,
                          layout)


def _refused(abi, rc):
    assert rc != 0
    msg = abi.last_error()
    assert msg, "a refused call leaves a message"
    return msg


def test_prototypes_present(abi):
    args, res = abi.PROTOTYPES["trik_hsv_frame_ranges_batch"]
    assert len(args) == 6 and res is C.c_int32
    args, res = abi.PROTOTYPES["trik_hsv_ranges_of_detect"]
    assert len(args) == 6 and res is C.c_int32
    lib = abi.load()
    assert hasattr(lib, "trik_hsv_frame_ranges_batch") and hasattr(lib, "trik_hsv_ranges_of_detect")
    import trik_hsv

    assert callable(trik_hsv.frame_ranges_batch) and callable(trik_hsv.ranges_of_detect)


def test_frame_ranges_batch_refuses(abi):
    call = abi.load().trik_hsv_frame_ranges_batch
    ok = _batch(abi)
    assert "NULL" in _refused(abi, call(None, FAKE, 1, FAKE, FAKE, None))
    assert "ranges" in _refused(abi, call(C.byref(ok), None, 1, FAKE, FAKE, None))
    assert "sums" in _refused(abi, call(C.byref(ok), FAKE, 1, None, FAKE, None))
    assert "layout" in _refused(abi, call(C.byref(_batch(abi, layout=2)), FAKE, 1, FAKE, None, None))
    for bad in (_batch(abi, w=33), _batch(abi, h=6), _batch(abi, w=-32), _batch(abi, ll=127),
                _batch(abi, layout=1, ll=63), _batch(abi, stride=8 * 128 - 1), _batch(abi, n=-1),
                _batch(abi, w=32768, ll=65536), _batch(abi, frames=None)):
        _refused(abi, call(C.byref(bad), FAKE, 1, FAKE, None, None))
    for t in (0, -1, abi.MAX_RANGES + 1):
        assert "n_ranges" in _refused(abi, call(C.byref(ok), FAKE, t, FAKE, None, None))


def test_frame_ranges_batch_empty_batch_touches_nothing(abi):
    """n_frames == 0 returns 0 with every buffer NULL: nothing is enqueued."""
    call = abi.load().trik_hsv_frame_ranges_batch
    assert call(C.byref(_batch(abi, n=0, frames=None)), None, 1, None, None, None) == 0
    assert call(C.byref(_batch(abi, n=0, frames=None)), None, abi.MAX_RANGES, None, None, None) == 0


def test_ranges_of_detect_refuses(abi):
    call = abi.load().trik_hsv_ranges_of_detect
    assert "NULL" in _refused(abi, call(None, 1, FAKE, 1, 0, None))
    assert "NULL" in _refused(abi, call(FAKE, 1, None, 1, 0, None))
    _refused(abi, call(FAKE, -1, FAKE, 1, 0, None))
    for t in (0, -3, 65):
        assert "n_ranges" in _refused(abi, call(FAKE, 1, FAKE, t, 0, None))
    for t in (-1, 4, 64):
        _refused(abi, call(FAKE, 1, FAKE, 4, t, None))
    assert call(None, 0, None, 1, 0, None) == 0  # n == 0: nothing to do


def test_pool_is_the_parity_tests_pool():
    import gpu_util

    assert FC.POOL[:4] == gpu_util.BENCH_RANGES and len(FC.POOL) == 12 and len(set(FC.POOL)) == 12
    assert FC.FULL == (0, 359, 0, 100, 0, 100) and FC.T3[0] > FC.T3[1]


def test_variety_cases(oracle_mod):
    """37 frames of 160 x 120, T = 5 drawn with default_rng(5): the figures of
    the YUYV batch, on the oracle."""
    v = FC.VARIETY
    ranges = FC.variety_ranges()
    assert (v["n"], v["w"], v["h"], v["t"]) == (37, 160, 120, 5)
    assert len({tuple(r) for r in ranges}) == 37
    figures = {}
    for kind in (1, 0):
        own, _ = FC.variety_expected(oracle_mod, FC.LAYOUT_YUYV, kind)
        assert FC.check_variety(oracle_mod, FC.LAYOUT_YUYV, kind) == 36
        figures[kind] = (int((own[:, :, 0] > 0).sum()), int((own[:, :, 0] == v["w"] * v["h"]).sum()))
    assert figures[1] == (160, 31) and figures[0] == (177, 31)  # of 185 slots: scenes, uniform bytes
    for kind in (1, 0):  # the ov7670 batches hold the same property
        assert FC.check_variety(oracle_mod, FC.LAYOUT_OV7670, kind) > v["n"] // 2


def test_expected_is_the_oracle_batch(oracle_mod):
    """expected() with one shared set is oracle.batch()."""
    v = FC.VARIETY
    ll = 2 * v["w"]
    host = FC.variety_frames(oracle_mod, FC.LAYOUT_YUYV, 1)
    rs = FC.variety_ranges()[3]
    got_s, got_t = FC.expected(oracle_mod, host, v["h"] * ll, 6, v["w"], v["h"], ll, FC.LAYOUT_YUYV, [rs] * 6)
    want_s, want_t = oracle_mod.batch(host, v["h"] * ll, 6, v["w"], v["h"], ll, FC.LAYOUT_YUYV, rs)
    assert np.array_equal(got_s, want_s) and np.array_equal(got_t, want_t)


def test_ov7670_twin(oracle_mod):
    """The twin of a YUYV frame gives the same sums under every pool range."""
    w, h = 64, 8
    yuyv = np.random.default_rng(3).integers(0, 256, h * 2 * w, dtype=np.uint8)
    a, _ = oracle_mod.frame(yuyv, w, h, 2 * w, FC.LAYOUT_YUYV, FC.POOL)
    b, _ = oracle_mod.frame(FC.ov7670_twin(yuyv, w, h), w, h, w, FC.LAYOUT_OV7670, FC.POOL)
    assert np.array_equal(a, b) and (a[:, 0] > 0).sum() >= 8


def test_exhaustive_bytes():
    import gpu_util

    frame, w, h, ll = gpu_util.exhaustive_yuyv_frame()
    assert (w, h, ll) == (8192, 2048, 16384) and np.array_equal(FC.exhaustive_yuyv(), frame)
    # one frame, the full range: sum_x and sum_y pass 2^32 (a 32-bit partial sum across rows would wrap)
    assert w * h * (w - 1) // 2 > 2**32 and w * h * (h - 1) // 2 > 2**32


def test_closed_loop_cases(oracle_mod):
    """The 8 scene frames' detected ranges: hues 0, 179 and 118, at least two
    distinct ranges, at least one wrapped hue."""
    det = FC.loop_detect(oracle_mod)
    assert {d[0] for d in det} >= {0, 118, 179}
    assert all(d[2] <= 255 and d[3] <= 255 and d[4] <= 255 and d[5] <= 255 for d in det)  # fit the InArgs bytes
    FC.check_loop([FC.blob_range_of(d) for d in det])


def test_t_ranges_are_distinct_per_frame():
    for t in FC.T_COUNTS:
        for rs in FC.t_ranges(8, t):
            assert len(rs) == t and len(set(rs)) == t
            assert all(0 <= r[4] <= 255 and r[2] <= 255 and r[3] <= 255 for r in rs)


def test_ragged_cases_take_their_paths():
    """line_length + 12 keeps dword loads (not 16-byte ones); + 3 with an odd
    frame stride and a base offset of 1 leaves only bytes."""
    for layout in (FC.LAYOUT_YUYV, FC.LAYOUT_OV7670):
        for pad, spad, off in FC.RAGGED:
            _, offset, stride, ll = FC.uniform_batch(layout, 64, 8, 3, 1, pad, spad, off)
            if off:
                assert offset % 2 == 1 and stride % 2 == 1 and ll % 2 == 1
            else:
                assert ll % 4 == 0 and ll % 16 != 0 and stride % 4 == 0
