"""trik_hsv_line_frame_ranges_batch on the GPU: the two line sensors with a V
range per frame, read on the device.  ov7670 against tests/line_ref.py per
frame with that frame's range, packed YUYV against oracle.frame with hue and
saturation open; every comparison exact.  The inputs are those of
tests/line_frame_ranges_cases.py, whose claims tests/
test_line_frame_ranges_cpu.py asserts on the references' own output."""
import ctypes as C

import numpy as np
import pytest

import frame_ranges_cases as FC
import line_frame_ranges_cases as LC
import line_ref

pytestmark = pytest.mark.gpu
YUYV, OV7670 = LC.LAYOUT_YUYV, LC.LAYOUT_OV7670


@pytest.fixture(scope="module")
def hsv():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import trik_hsv

    return trik_hsv


def _dev(a):
    import torch

    return torch.from_numpy(np.array(a)).cuda()  # (a copy: the cached inputs are read-only)


def _ranges(pairs, fill=0):
    import torch

    return torch.from_numpy(LC.six(pairs, fill).view(np.int16)).cuda()


def _tg(t):
    return [(x, y, s & 0xFF) for x, y, s, _ in t.cpu().tolist()]


def _split(buf, n, stride, fb, off=0):
    return [buf[off + f * stride:off + f * stride + fb] for f in range(n)]


def _run(hsv, dev, w, h, ll, layout, pairs, **kw):
    sums, tg = hsv.line_frame_ranges_batch(dev, w, h, ll, layout, _ranges(pairs), n_frames=len(pairs), **kw)
    return sums.cpu().tolist(), _tg(tg)


def _expected(oracle_mod, table, layout, frames, w, h, ll, pairs, band=None):
    if layout == OV7670:
        return LC.expected_ov7670(table, frames, w, h, ll, pairs, band)
    return LC.expected_yuyv(oracle_mod, frames, w, h, ll, pairs)


# ---- the pair batch ---------------------------------------------------------------
@pytest.mark.parametrize("band", [None, (2, 2)], ids=["default_band", "one_row_band"])
def test_ov7670_pair_batch(hsv, table, band):
    """10,201 frames of the level frame, frame (p, q) under (p, q), one call."""
    fr = LC.level_frame_ov7670(table)
    dev = _dev(np.tile(fr, len(LC.ALL_PAIRS)))
    got = _run(hsv, dev, 64, 8, 64, OV7670, LC.ALL_PAIRS, band=band)
    want = LC.pair_batch_expected_ov7670(table, band)
    assert got[0] == want[0] and got[1] == want[1]


def test_yuyv_pair_batch(hsv, oracle_mod, table):
    fr = LC.level_frame_yuyv(table)
    dev = _dev(np.tile(fr, len(LC.ALL_PAIRS)))
    got = _run(hsv, dev, 32, 8, 64, YUYV, LC.ALL_PAIRS)
    want = LC.pair_batch_expected_yuyv(oracle_mod, table)
    assert got[0] == want[0] and got[1] == want[1]


def test_ov7670_out_of_byte_values(hsv, table):
    """(0, 65535), (65535, 65535), (101, 300), (300, 101) among ordinary
    ranges: scaled in int32 and clamped, the neighbours unaffected."""
    pairs = LC.OUT_OF_BYTE
    fr = LC.level_frame_ov7670(table)
    got = _run(hsv, _dev(np.tile(fr, len(pairs))), 64, 8, 64, OV7670, pairs)
    want = LC.expected_ov7670(table, [fr] * len(pairs), 64, 8, 64, pairs)
    assert got[0] == want[0] and got[1] == want[1]
    assert want[0][0] == want[0][8] and want[0][3] == want[0][5] == want[0][7] and want[0][3][0] > 0


# ---- every (Y, U, V) ----------------------------------------------------------------
@pytest.mark.parametrize("layout", [OV7670, YUYV], ids=["ov7670", "yuyv"])
def test_exhaustive_64_frames(hsv, oracle_mod, table, layout):
    """64 frames of 8192 x 32 holding every (Y, U, V) once, frame f under the
    f-th of 64 distinct ranges."""
    w, h, n = 8192, 32, 64
    buf = LC.exhaustive_frames_ov7670() if layout == OV7670 else LC.exhaustive_frames_yuyv()
    ll = LC.row_bytes(w, layout)
    fb = LC.frame_bytes(w, h, ll, layout)
    got = _run(hsv, _dev(buf), w, h, ll, layout, LC.EXHAUSTIVE_PAIRS)
    want = _expected(oracle_mod, table, layout, _split(buf, n, fb, fb), w, h, ll, LC.EXHAUSTIVE_PAIRS)
    assert got[0] == want[0] and got[1] == want[1]


def test_yuyv_one_frame_sums_pass_2_32(hsv, oracle_mod):
    """The same bytes as one 8192 x 2048 frame under (0, 100): sum_x and sum_y
    arrive whole in the 64-bit sums."""
    w, h = 8192, 2048
    buf = LC.exhaustive_frames_yuyv()
    want = LC.expected_yuyv_wide(oracle_mod, buf, w, h, 2 * w, (0, 100))
    assert want[1] > 2**32 and want[2] > 2**32
    got = _run(hsv, _dev(buf), w, h, 2 * w, YUYV, [(0, 100)])
    assert got[0] == [want] and got[1] == [LC.wline_targets(want, w, h)]


# ---- the workgroup -> frame -> range derivation under every (chunks, segs) ----------
@pytest.mark.parametrize("layout", [OV7670, YUYV], ids=["ov7670", "yuyv"])
@pytest.mark.parametrize("shape", [s for s, _ in LC.GEOMETRY], ids=lambda s: "%dx%dx%d" % s)
def test_geometry_with_per_frame_ranges(hsv, oracle_mod, table, layout, shape):
    w, h, n = shape
    pairs = LC.varied_pairs(n)
    buf = LC.geometry_noise(w, h, n) if layout == OV7670 else LC.geometry_noise_yuyv(w, h, n)
    ll = LC.row_bytes(w, layout)
    fb = LC.frame_bytes(w, h, ll, layout)
    got = _run(hsv, _dev(buf), w, h, ll, layout, pairs)
    want = _expected(oracle_mod, table, layout, _split(buf, n, fb, fb), w, h, ll, pairs)
    assert got[0] == want[0] and got[1] == want[1]
    assert got[0][n // 2] == [0, 0, 0] and got[0][n // 2 - 1][0] > 0 and got[0][n // 2 + 1 if n > 2 else 0][0] > 0


# ---- against the existing calls -----------------------------------------------------
def test_ov7670_equals_line_batch_frame_by_frame(hsv):
    """24 frames of 64 x 36 under three bands (one with a negative start): each
    slot = trik_hsv_line_batch on that frame alone with its pair."""
    import torch

    w, h, n = 64, 36, 24
    buf = LC.geometry_noise(w, h, n)
    dev = _dev(buf)
    fb = 2 * w * h
    pairs = LC.varied_pairs(n, seed=5)
    for band in (None, (3, 17), (-5, 40)):
        sums, tg = hsv.line_frame_ranges_batch(dev, w, h, w, OV7670, _ranges(pairs), band=band)
        one = [hsv.line_batch(dev[f * fb:(f + 1) * fb], w, h, w, *pairs[f], band=band) for f in range(n)]
        assert torch.equal(sums, torch.cat([s for s, _ in one])) and torch.equal(tg, torch.cat([t for _, t in one]))
        assert int((sums[:, 0] > 0).sum()) == n - 1


def test_yuyv_agrees_with_existing_paths(hsv, oracle_mod):
    """32 frames of 64 x 36: the sums trik_hsv_frame_ranges_batch gives with
    (0, 359, 0, 100, vf, vt); garbage in entries 0..3 changes nothing; on 4
    frames, the OutArgs of WebcamLineSensor.process."""
    import torch

    w, h, n = 64, 36, 32
    buf = np.concatenate([oracle_mod.wline_scene(w, h, 2 * w, 40 + f, x0=8 + f) for f in range(n)])
    dev = _dev(buf)
    pairs = [(0, 30 + f) for f in range(n)]
    pairs[n // 2] = LC.EMPTY
    sums, tg = hsv.line_frame_ranges_batch(dev, w, h, 2 * w, YUYV, _ranges(pairs))
    full = np.zeros((n, 1, 6), np.int16)
    full[:, 0] = [(0, 359, 0, 100, vf, vt) for vf, vt in pairs]
    ref_sums, _ = hsv.frame_ranges_batch(dev, w, h, 2 * w, YUYV, _dev(full))
    assert torch.equal(sums, ref_sums[:, 0]) and int((sums[:, 0] > 10).sum()) >= 4
    for fill in (0xFFFF, 0x1234):
        s2, t2 = hsv.line_frame_ranges_batch(dev, w, h, 2 * w, YUYV, _ranges(pairs, fill))
        assert torch.equal(s2, sums) and torch.equal(t2, tg)
    sensor = hsv.WebcamLineSensor(hsv._default_params(1, hsv.FORMAT_YUV422, 640, 480))
    try:
        assert sensor.set_params(w, h, 2 * w, out_width=32, out_height=18, out_line_length=64) == 0
        for f in (0, 1, n // 2, n - 1):
            rc, oa = sensor.process(buf[f * h * 2 * w:(f + 1) * h * 2 * w], (0, 359, 0, 100) + pairs[f],
                                    out_buffer=np.zeros(18 * 64, np.uint8))
            assert rc == 0, hsv._abi.last_error()
            assert (oa.alg.targetX, oa.alg.targetY, oa.alg.targetSize) == _tg(tg)[f] and oa.alg.targetY == 0
    finally:
        sensor.close()


# ---- the byte-load kernels ----------------------------------------------------------
@pytest.mark.parametrize("layout", [OV7670, YUYV], ids=["ov7670", "yuyv"])
@pytest.mark.parametrize("case", LC.GENERIC, ids=lambda c: "stride%d_ll%d_off%d" % c)
def test_generic_kernel(hsv, oracle_mod, table, layout, case):
    """A base 1 and 4 bytes past a 16-byte boundary, an odd frame stride, a
    line_length of the row + 4: per-frame ranges on 64 x 8."""
    w, h, n = 64, 8, 3
    buf, off, stride, ll, frames = LC.generic_batch(layout, case)
    dev = _dev(buf)
    assert dev.data_ptr() % 16 == 0
    pairs = LC.varied_pairs(n, seed=2)
    got = _run(hsv, dev[off:], w, h, ll, layout, pairs, frame_stride=stride)
    want = _expected(oracle_mod, table, layout, frames, w, h, ll, pairs)
    assert got[0] == want[0] and got[1] == want[1] and want[0][0][0] > 0 and want[0][1] == [0, 0, 0]


# ---- one-hot batches (YUYV) -----------------------------------------------------------
@pytest.mark.parametrize("width", LC.ONE_HOT_WIDTHS)
def test_yuyv_one_hot_columns(hsv, width):
    """Frame c has column c bright: every column, the first and last five
    included."""
    dev = _dev(LC.one_hot_columns_yuyv(width))
    got = _run(hsv, dev, width, 8, 2 * width, YUYV, [LC.ONE_HOT_RANGE] * width)
    assert got[0] == LC.one_hot_columns_expected(width)


def test_yuyv_one_hot_rows(hsv):
    """Frame r has row r bright: the row term of sum_y at every offset relative
    to the rows per iteration and the unroll."""
    h = LC.ONE_HOT_ROWS
    got = _run(hsv, _dev(LC.one_hot_rows_yuyv()), 32, h, 64, YUYV, [LC.ONE_HOT_RANGE] * h)
    assert got[0] == LC.one_hot_rows_expected()


# ---- both layouts: stream order, the closed loop, refusals ---------------------------
@pytest.mark.parametrize("layout", [OV7670, YUYV], ids=["ov7670", "yuyv"])
def test_stream_order(hsv, oracle_mod, table, layout):
    """Call, rewrite ranges_dev on the stream, call again: each call sees its
    own ranges, with no host synchronisation between them."""
    import torch

    w, h, n = 64, 36, 3
    buf = LC.geometry_noise(w, h, n) if layout == OV7670 else LC.geometry_noise_yuyv(w, h, n)
    ll = LC.row_bytes(w, layout)
    fb = LC.frame_bytes(w, h, ll, layout)
    first, second = LC.varied_pairs(n, seed=3), LC.varied_pairs(n, seed=9)
    dev, rng, nxt = _dev(buf), _ranges(first), _ranges(second)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        a = hsv.line_frame_ranges_batch(dev, w, h, ll, layout, rng, stream=s)
        rng.copy_(nxt, non_blocking=True)
        b = hsv.line_frame_ranges_batch(dev, w, h, ll, layout, rng, stream=s)
    s.synchronize()
    frames = _split(buf, n, fb, fb)
    for (sums, tg), pairs in ((a, first), (b, second)):
        want = _expected(oracle_mod, table, layout, frames, w, h, ll, pairs)
        assert sums.cpu().tolist() == want[0] and _tg(tg) == want[1]
    assert a[0].cpu().tolist() != b[0].cpu().tolist()


@pytest.mark.parametrize("layout", [OV7670, YUYV], ids=["ov7670", "yuyv"])
def test_closed_loop(hsv, oracle_mod, table, layout):
    """batch_auto_range_exact -> ranges_of_detect(n_ranges = 1) -> the call, on
    8 scene frames of 320 x 240, against the same with the middle step's
    result read back and fed to the reference frame by frame."""
    w, h, n = 320, 240, 8
    ll = LC.row_bytes(w, layout)
    scene = oracle_mod.line_scene if layout == OV7670 else oracle_mod.wline_scene
    kind = hsv.AUTO_OV7670_LINE if layout == OV7670 else hsv.AUTO_WEBCAM_LINE
    frames = [scene(w, h, ll, 70 + f, x0=60 + 25 * f, slope=0.1 * (f - 3)) for f in range(n)]
    dev = _dev(np.concatenate(frames))
    detect, _ = hsv.batch_auto_range_exact(dev, w, h, ll, kind)
    ranges = hsv.ranges_of_detect(detect, n_ranges=1)
    sums, tg = hsv.line_frame_ranges_batch(dev, w, h, ll, layout, ranges)
    back = ranges.cpu().numpy().view(np.uint16).reshape(n, 6)
    pairs = [(int(r[4]), int(r[5])) for r in back]
    want = _expected(oracle_mod, table, layout, frames, w, h, ll, pairs)
    assert sums.cpu().tolist() == want[0] and _tg(tg) == want[1], pairs


def test_refusals_and_empties(hsv):
    """Each failure of the call conventions enqueues nothing; n_frames == 0
    touches nothing; width or height 0 zeroes sums and targets."""
    import torch

    lib, abi = hsv._lib, hsv._abi
    call = lib.trik_hsv_line_frame_ranges_batch
    for layout in (OV7670, YUYV):
        w, h = 64, 8
        ll = LC.row_bytes(w, layout)
        fb = LC.frame_bytes(w, h, ll, layout)
        dev = torch.zeros(2 * fb, dtype=torch.uint8, device="cuda")
        rng = _ranges([(0, 100), (0, 100)])
        sums = torch.full((2, 3), 0x55, dtype=torch.int64, device="cuda")
        tg = torch.full((2, 4), 0x55, dtype=torch.int8, device="cuda")
        p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
        b = lambda **kw: abi.FrameBatch(**{**dict(frames=dev.data_ptr(), frame_stride=fb, n_frames=2, width=w,  # noqa: E731
                                                  height=h, line_length=ll, layout=layout), **kw})
        bad = [(None, p(rng), p(sums)), (b(), None, p(sums)), (b(), p(rng), None), (b(layout=2), p(rng), p(sums)),
               (b(width=33), p(rng), p(sums)), (b(line_length=ll - 1), p(rng), p(sums)),
               (b(frame_stride=fb - 1), p(rng), p(sums))]
        for batch, r, s in bad:
            assert call(C.byref(batch) if batch is not None else None, r, 4, 84, s, p(tg), None) != 0
            assert abi.last_error()
        assert call(C.byref(b(n_frames=0)), p(rng), 4, 84, p(sums), p(tg), None) == 0
        torch.cuda.synchronize()
        assert bool((sums == 0x55).all()) and bool((tg == 0x55).all())  # the sentinels stay
        for kw in (dict(width=0, line_length=0, frame_stride=0), dict(height=0, frame_stride=0)):
            sums.fill_(0x55)
            tg.fill_(0x55)
            assert call(C.byref(b(**kw)), p(rng), 4, 84, p(sums), p(tg), None) == 0
            torch.cuda.synchronize()
            assert not bool(sums.any()) and not bool(tg.any())
