"""CPU-only checks of the line sensors' per-frame-range call
(trik_hsv_line_frame_ranges_batch): what the C ABI refuses is refused before
any GPU call, the shared scale_val equals the test reference's for every
uint16, and the inputs of tests/test_gpu_line_frame_ranges.py
(tests/line_frame_ranges_cases.py) reach what they are meant to reach, stated
on the references' own output (tests/line_ref.py, the oracle)."""
import ctypes as C

import numpy as np
import pytest

import frame_ranges_cases as FC
import line_frame_ranges_cases as LC
import line_ref

FAKE = 0x10000  # a non-NULL address nothing reads


@pytest.fixture(scope="module")
def abi():
    from trik_hsv import _abi

    return _abi


def _batch(abi, n=2, w=64, h=8, ll=None, layout=1, stride=None, frames=FAKE):
    ll = LC.row_bytes(w, layout) if ll is None else ll
    return abi.FrameBatch(frames, LC.frame_bytes(w, h, ll, layout) if stride is None else stride, n, w, h, ll, layout)


def _refused(abi, rc):
    assert rc != 0
    msg = abi.last_error()
    assert msg, "a refused call leaves a message"
    return msg


def test_prototype_and_wrapper_present(abi):
    args, res = abi.PROTOTYPES["trik_hsv_line_frame_ranges_batch"]
    assert len(args) == 7 and res is C.c_int32
    assert hasattr(abi.load(), "trik_hsv_line_frame_ranges_batch")
    import trik_hsv

    assert callable(trik_hsv.line_frame_ranges_batch)


@pytest.mark.parametrize("layout", [LC.LAYOUT_YUYV, LC.LAYOUT_OV7670])
def test_call_refuses(abi, layout):
    """Each failure of the call conventions, one at a time; nothing is enqueued
    (there is no GPU here and no pointer is dereferenced)."""
    call = abi.load().trik_hsv_line_frame_ranges_batch
    ok = _batch(abi, layout=layout)
    assert "NULL" in _refused(abi, call(None, FAKE, 4, 84, FAKE, FAKE, None))
    assert "ranges" in _refused(abi, call(C.byref(ok), None, 4, 84, FAKE, FAKE, None))
    assert "sums" in _refused(abi, call(C.byref(ok), FAKE, 4, 84, None, FAKE, None))
    assert "layout" in _refused(abi, call(C.byref(_batch(abi, layout=2, ll=128)), FAKE, 4, 84, FAKE, None, None))
    row = LC.row_bytes(64, layout)
    for bad in (_batch(abi, w=33, ll=128, layout=layout), _batch(abi, h=6, layout=layout),
                _batch(abi, w=-32, ll=128, layout=layout), _batch(abi, ll=row - 1, layout=layout),
                _batch(abi, stride=LC.frame_bytes(64, 8, row, layout) - 1, layout=layout),
                _batch(abi, n=-1, layout=layout), _batch(abi, w=32768, ll=65536, layout=layout),
                _batch(abi, frames=None, layout=layout)):
        _refused(abi, call(C.byref(bad), FAKE, 4, 84, FAKE, None, None))


def test_empty_batch_touches_nothing(abi):
    """n_frames == 0 returns 0 with every buffer NULL: nothing is enqueued."""
    call = abi.load().trik_hsv_line_frame_ranges_batch
    for layout in (LC.LAYOUT_YUYV, LC.LAYOUT_OV7670):
        assert call(C.byref(_batch(abi, n=0, frames=None, layout=layout)), None, 4, 84, None, None, None) == 0


def test_scale_val_every_uint16(abi):
    """The one scale_val of the library (host call and kernels) = line_ref's,
    for all 65,536 values a ranges entry can hold, 101..65535 included."""
    f = abi.load().trik_hsv_line_scale_val
    got = [f(v) for v in range(65536)]
    assert got == [line_ref.scale_val(v) for v in range(65536)]
    assert got[100] == 255 and got[101] == 255 and got[99] == 252 and got[65535] == 255 and got[0] == 0
    assert f(-5) == 0


def test_level_frames_hold_every_level(table):
    """All 256 V bytes: inside the ov7670 frame's window, and exactly once each
    in the YUYV frame."""
    ov = LC.level_frame_ov7670(table)
    assert ov.size == 2 * 64 * 8
    v = LC.v_bytes(table, ov, 64, 8)
    assert set(v[:, 5:60].reshape(-1).tolist()) == set(range(256))
    yuyv = LC.level_frame_yuyv(table)
    assert yuyv.size == 8 * 64
    vy = LC.v_bytes(table, FC.ov7670_twin(yuyv, 32, 8), 32, 8)
    assert sorted(vy.reshape(-1).tolist()) == list(range(256))
    # some pair needs chroma other than grey
    assert any((u, vv) != (128, 128) for _, _, u, vv in LC.level_pairs(table))


def _pair_grid(sums):
    return np.array([s[0] for s in sums]).reshape(101, 101)


def _check_pair_batch(n):
    """n[p, q] = points under (p, q): some count changes when p moves by one,
    some when q does; every pair with scaled from > to is empty, and only
    those need be (the frame holds every level)."""
    assert (n[1:, :] != n[:-1, :]).any() and (n[:, 1:] != n[:, :-1]).any()
    sv = np.array([line_ref.scale_val(v) for v in range(101)])
    empty = sv[:, None] > sv[None, :]
    assert empty.any() and (n[empty] == 0).all() and (n[~empty] > 0).all()
    # each step of p or q that moves the scaled bound moves a count
    assert all((n[p + 1, :] != n[p, :]).any() for p in range(100) if sv[p + 1] != sv[p])
    assert all((n[:, q + 1] != n[:, q]).any() for q in range(100) if sv[q + 1] != sv[q])


def test_pair_batch_ov7670(table):
    sums, targets = LC.pair_batch_expected_ov7670(table)
    assert len(sums) == 10201
    _check_pair_batch(_pair_grid(sums))
    assert any(t != (0, 0, 0) for t in targets) and any(s[2] > 0 for s in sums)
    one_row, _ = LC.pair_batch_expected_ov7670(table, (2, 2))
    assert one_row != sums and any(s[2] > 0 for s in one_row)


def test_pair_batch_yuyv(oracle_mod, table):
    sums, targets = LC.pair_batch_expected_yuyv(oracle_mod, table)
    assert len(sums) == 10201
    n = _pair_grid(sums)
    _check_pair_batch(n)
    assert n[0, 100] == 256 and sums[100][1:] == [sum(range(32)) * 8, sum(range(8)) * 32]
    assert any(t != (0, 0, 0) for t in targets) and all(t[1] == 0 for t in targets)


def test_yuyv_reference_is_the_webcam_line_sensor(oracle_mod):
    """oracle.frame with hue and saturation open gives the three sums the
    webcam line sensor's run leaves (oracle.wline_run), and wline_targets its
    OutArgs."""
    w, h = 64, 36
    for seed, (vf, vt) in enumerate([(0, 30), (50, 100), (80, 20), (0, 100)]):
        fr = oracle_mod.wline_scene(w, h, 2 * w, seed)
        (s,), _ = LC.expected_yuyv(oracle_mod, [fr], w, h, 2 * w, [(vf, vt)])
        rc, oa, _, ws = oracle_mod.wline_run(fr, w, h, 2 * w, vf, vt, out_width=32, out_height=18, preview=False)
        assert rc == 0 and [int(v) for v in ws] == s
        assert LC.wline_targets(s, w, h) == (oa["target_x"], oa["target_y"], oa["target_size"])


def test_ranges_lists():
    assert len(LC.EXHAUSTIVE_PAIRS) == 64 == len(set(LC.EXHAUSTIVE_PAIRS))
    assert {(0, 100), (0, 0), (100, 100), LC.EMPTY} <= set(LC.EXHAUSTIVE_PAIRS)
    assert line_ref.scale_val(LC.EMPTY[0]) > line_ref.scale_val(LC.EMPTY[1])
    for n in (2, 3, 24, 32, 1025):
        ps = LC.varied_pairs(n)
        assert len(ps) == n == len(set(ps)) and ps[n // 2] == LC.EMPTY
        assert all(lo <= hi for i, (lo, hi) in enumerate(ps) if i != n // 2)
    six = LC.six(LC.OUT_OF_BYTE, fill=0xABCD)
    assert six.dtype == np.uint16 and six[1].tolist() == [0xABCD] * 4 + [0, 65535] and six[7].tolist()[4:] == [300, 101]
    sv = line_ref.scale_val
    assert sv(101) == 255 and sv(300) == 255 and sv(65535) == 255  # (300, 101) is (255, 255), not empty


@pytest.mark.parametrize("layout", [LC.LAYOUT_OV7670, LC.LAYOUT_YUYV])
def test_geometry_cases_select_what_they_claim(layout):
    for (w, h, n), want in LC.GEOMETRY:
        g = LC.geom(layout, n, w, h, LC.row_bytes(w, layout))
        assert g is not None, (w, h, n)
        assert {k: g[k] for k in want} == want, (w, h, n, g)
    # one segment from 1024 frames on, two below
    assert LC.geom(layout, 1023, 64, 100, LC.row_bytes(64, layout))["segs"] == 2
    assert LC.geom(layout, 1024, 64, 100, LC.row_bytes(64, layout))["segs"] == 1
    # the partial last iteration and the late row offsets
    g = LC.geom(layout, 3, 64, 36, LC.row_bytes(64, layout))
    assert g["iters"] * g["rpi"] > 36 > (g["iters"] - 1) * g["rpi"]
    assert LC.geom(layout, 3, 32, 4, LC.row_bytes(32, layout))["rpi"] > 4
    # the counters: the tallest frame the entry point takes stays within 16 bits
    assert LC.geom(layout, 1, 32, 32764, LC.row_bytes(32, layout))["iters"] <= 32767


def test_generic_cases_take_the_byte_kernel():
    for layout in (LC.LAYOUT_OV7670, LC.LAYOUT_YUYV):
        for case in LC.GENERIC:
            buf, off, stride, ll, frames = LC.generic_batch(layout, case)
            assert LC.geom(layout, 3, 64, 8, ll, base=off, stride=stride) is None, (layout, case)
            assert len(frames) == 3 and len({f.tobytes() for f in frames}) == 3
        assert LC.geom(layout, 3, 64, 8, LC.row_bytes(64, layout)) is not None
    # YUYV: 8-byte alignment is not enough for the 16-byte unit
    assert LC.geom(LC.LAYOUT_YUYV, 1, 64, 8, 128, base=8) is None
    assert LC.geom(LC.LAYOUT_OV7670, 1, 64, 8, 64, base=8) is not None


def test_yuyv_of_inverts_the_twin():
    w, h = 64, 8
    yuyv = np.random.default_rng(5).integers(0, 256, h * 2 * w, dtype=np.uint8)
    assert np.array_equal(LC.yuyv_of(FC.ov7670_twin(yuyv, w, h), w, h), yuyv)


def test_geometry_noise_reaches_detections_and_misses(oracle_mod, table):
    """Every frame of the small geometry batches, under its own range: some
    pixels detected and some not (but for the empty range), in both layouts,
    which agree outside the window's effect."""
    for (w, h, n), _ in LC.GEOMETRY:
        if n > 3:
            continue
        pairs = LC.varied_pairs(n)
        fb = 2 * w * h
        ov = [LC.geometry_noise(w, h, n)[f * fb:(f + 1) * fb] for f in range(n)]
        yu = [LC.geometry_noise_yuyv(w, h, n)[f * fb:(f + 1) * fb] for f in range(n)]
        so, _ = LC.expected_ov7670(table, ov, w, h, w, pairs)
        sy, _ = LC.expected_yuyv(oracle_mod, yu, w, h, 2 * w, pairs)
        for f in range(n):
            if f == n // 2:
                assert so[f] == [0, 0, 0] and sy[f] == [0, 0, 0]
            else:
                assert 0 < so[f][0] < h * (w - 9) and so[f][0] <= sy[f][0] < h * w, (w, h, f)


def test_one_hot_batches(oracle_mod):
    for w in LC.ONE_HOT_WIDTHS:
        buf = LC.one_hot_columns_yuyv(w).reshape(w, -1)
        got, _ = LC.expected_yuyv(oracle_mod, list(buf), w, 8, 2 * w, [LC.ONE_HOT_RANGE] * w)
        assert got == LC.one_hot_columns_expected(w)
    h = LC.ONE_HOT_ROWS
    buf = LC.one_hot_rows_yuyv().reshape(h, -1)
    got, _ = LC.expected_yuyv(oracle_mod, list(buf), 32, h, 64, [LC.ONE_HOT_RANGE] * h)
    assert got == LC.one_hot_rows_expected()


def test_exhaustive_sums_pass_2_32(oracle_mod):
    """The 64 frames as one 8192 x 2048 frame under (0, 100): every pixel
    detected, sum_x and sum_y past 2^32."""
    w, h = 8192, 2048
    s = LC.expected_yuyv_wide(oracle_mod, LC.exhaustive_frames_yuyv(), w, h, 2 * w, (0, 100))
    assert s ==[w * h, w * h * (w - 1) // 2, w * h * (h - 1) // 2] and s[1] > 2**32 and s[2] > 2**32
    assert LC.exhaustive_frames_ov7670().size == 2 * w * h
