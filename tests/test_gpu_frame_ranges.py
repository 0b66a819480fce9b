"""trik_hsv_frame_ranges_batch and trik_hsv_ranges_of_detect on the GPU against
the oracle: slot (f, t) is oracle.frame(frame f, range t of f's set), then
oracle.targets, bit for bit, on the cases of tests/frame_ranges_cases.py.  Each
coverage claim is asserted on the oracle's output before the GPU is compared."""
import numpy as np
import pytest

import frame_ranges_cases as FC

pytestmark = pytest.mark.gpu

YUYV, OV7670 = FC.LAYOUT_YUYV, FC.LAYOUT_OV7670


@pytest.fixture(scope="module")
def hsv():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import trik_hsv

    return trik_hsv


def _dev(buf, offset=0):
    """The buffer on a 256-byte boundary (torch's allocator), frame 0 at `offset`."""
    import torch

    t = torch.from_numpy(np.array(buf)).cuda()  # (a copy: the cached cases are read-only)
    assert t.data_ptr() % 16 == 0
    return t[offset:]


def _ranges_dev(ranges):
    import torch

    return torch.tensor(ranges, dtype=torch.int32).to(torch.int16).cuda()


def _check(hsv, oracle_mod, host, layout, w, h, ll, n, ranges, stride=None, offset=0, what=""):
    """Runs the call on host[offset:] and compares with the oracle."""
    stride = FC.frame_bytes(w, h, ll, layout) if stride is None else stride
    want_s, want_t = FC.expected(oracle_mod, host[offset:], stride, n, w, h, ll, layout, ranges)
    sums, tg = hsv.frame_ranges_batch(_dev(host, offset), w, h, ll, layout, _ranges_dev(ranges), n_frames=n,
                                      frame_stride=stride)
    got_s, got_t = sums.cpu().numpy(), tg.cpu().numpy()
    bad = np.argwhere((got_s != want_s).any(axis=2))
    assert len(bad) == 0, (what, "slots differ", bad[:4].tolist(), got_s[tuple(bad[0])], want_s[tuple(bad[0])])
    assert np.array_equal(got_t[:, :, :3], want_t) and not got_t[:, :, 3].any(), (what, "targets")
    return want_s


# ---- 1. all 2^24 triples ----------------------------------------------------
@pytest.mark.parametrize("layout", [YUYV, OV7670])
def test_exhaustive_64_frames(hsv, oracle_mod, layout):
    """Every (Y, U, V) as 64 frames of 8192 x 32, T = 12, frame f under the
    pool rotated by f: every triple meets every range."""
    w, h, n = 8192, 32, 64
    host = FC.exhaustive_yuyv()
    ll = 2 * w
    if layout == OV7670:
        host = np.concatenate([FC.ov7670_twin(host[f * h * ll:(f + 1) * h * ll], w, h) for f in range(n)])
        ll = w
    ranges = FC.rotated(n)
    assert all(sorted(r) == sorted(FC.POOL) for r in ranges) and ranges[1][0] == FC.POOL[1]
    want = _check(hsv, oracle_mod, host, layout, w, h, ll, n, ranges)
    assert (want[:, :, 0] > 0).any(axis=0).all()  # every range detects somewhere


def test_exhaustive_one_frame_sums_pass_32_bits(hsv, oracle_mod):
    """The same bytes as one 8192 x 2048 frame under the full range and T3:
    sum_x and sum_y of the full range exceed 2^32.  The reference's int32
    accumulators wrap there and oracle.frame's sums with them, so the sums
    wanted are those of oracle.frame's mask in 64 bits (what TrikHsvTargetSums
    holds), and the targets those of trik_hsv_process_batch on the frame (the
    call's contract; T3's sum_x passes 2^32 as well)."""
    import gpu_util

    w, h = 8192, 2048
    host = FC.exhaustive_yuyv()
    ranges = [FC.FULL, FC.T3]
    wrapped, mask = oracle_mod.frame(host, w, h, 2 * w, YUYV, ranges, want_mask=True)
    want = gpu_util.sums_from_mask(mask, 2)
    assert want[0].tolist() == [w * h, w * h * (w - 1) // 2, w * h * (h - 1) // 2]
    assert want[0, 1] > 2**32 and want[0, 2] > 2**32 and 0 < want[1, 0] < w * h
    assert wrapped[:, 0].tolist() == want[:, 0].tolist() and (wrapped[:, 1] != want[:, 1]).all()
    assert ((wrapped - want) % 2**32 == 0).all()
    frames = _dev(host)
    sums, tg = hsv.frame_ranges_batch(frames, w, h, 2 * w, YUYV, _ranges_dev([ranges]))
    assert sums[0].cpu().numpy().tolist() == want.tolist()
    det = hsv.Detector()
    try:
        s1, t1 = det.process_batch(frames, w, h, 2 * w, YUYV, ranges)
    finally:
        det.close()
    assert (sums == s1).all().item() and (tg == t1).all().item()


# ---- 2. per-frame variety ---------------------------------------------------
@pytest.mark.parametrize("kind", [1, 0], ids=["scenes", "uniform"])
@pytest.mark.parametrize("layout", [YUYV, OV7670])
def test_per_frame_variety(hsv, oracle_mod, layout, kind):
    v = FC.VARIETY
    assert FC.check_variety(oracle_mod, layout, kind) > v["n"] // 2
    want_s, want_t = FC.variety_expected(oracle_mod, layout, kind)
    host = FC.variety_frames(oracle_mod, layout, kind)
    sums, tg = hsv.frame_ranges_batch(_dev(host), v["w"], v["h"], FC.row_bytes(v["w"], layout), layout,
                                      _ranges_dev(FC.variety_ranges()))
    assert np.array_equal(sums.cpu().numpy(), want_s)
    assert np.array_equal(tg.cpu().numpy()[:, :, :3], want_t)


# ---- 3. small and many ------------------------------------------------------
@pytest.mark.parametrize("case", FC.SMALL_MANY, ids=lambda c: f"{'yuyv ov7670'.split()[c[0]]}-{c[1]}x{c[2]}x{c[3]}")
def test_small_and_many(hsv, oracle_mod, case):
    layout, w, h, n, t = case
    host, _, stride, ll = FC.uniform_batch(layout, w, h, n, 11 * w + n)
    want = _check(hsv, oracle_mod, host, layout, w, h, ll, n, FC.drawn(n, t, w + n), stride)
    assert (want[:, :, 0] > 0).any()


@pytest.mark.parametrize("t", FC.T_COUNTS)
def test_range_counts(hsv, oracle_mod, t):
    """T on both sides of the 4-range groups, up to TRIK_HSV_MAX_RANGES."""
    w, h, n = 64, 8, 8
    host, _, stride, ll = FC.uniform_batch(YUYV, w, h, n, 64 + t)
    want = _check(hsv, oracle_mod, host, YUYV, w, h, ll, n, FC.t_ranges(n, t), stride)
    assert len({tuple(s) for s in want[0].tolist()}) > min(t, 12) // 2  # a frame's slots are not copies


# ---- 4. widths --------------------------------------------------------------
@pytest.mark.parametrize("layout", [YUYV, OV7670])
def test_widths(hsv, oracle_mod, layout):
    for w in FC.WIDTHS:
        host, _, stride, ll = FC.uniform_batch(layout, w, 8, 3, 7 * w)
        want = _check(hsv, oracle_mod, host, layout, w, 8, ll, 3, FC.drawn(3, 5, w), stride, what=w)
        assert (want[:, :, 0] > 0).any()


@pytest.mark.parametrize("layout", [YUYV, OV7670])
def test_tall_narrow(hsv, oracle_mod, layout):
    w, h = FC.TALL
    host, _, stride, ll = FC.uniform_batch(layout, w, h, 1, 2052)
    _check(hsv, oracle_mod, host, layout, w, h, ll, 1, FC.drawn(1, 5, 2052), stride)


# ---- 5. ragged --------------------------------------------------------------
@pytest.mark.parametrize("ragged", FC.RAGGED, ids=["ll+12", "ll+3-odd-stride-base+1"])
@pytest.mark.parametrize("layout", [YUYV, OV7670])
def test_ragged(hsv, oracle_mod, layout, ragged):
    pad, spad, off = ragged
    for w, h, n in ((64, 8, 5), (160, 12, 3)):
        host, offset, stride, ll = FC.uniform_batch(layout, w, h, n, 5 * w + pad, pad, spad, off)
        if off:
            assert stride % 2 == 1 and _dev(host, offset).data_ptr() % 2 == 1  # the byte path
        _check(hsv, oracle_mod, host, layout, w, h, ll, n, FC.drawn(n, 5, w + pad), stride, offset, what=(w, pad))


# ---- 6. stream order --------------------------------------------------------
def test_ranges_are_read_in_stream_order(hsv, oracle_mod):
    """Set A, a call, set B copied over it from pinned memory without waiting,
    a second call: each output matches its own set."""
    import torch

    v = FC.VARIETY
    w, h, n, ll = v["w"], v["h"], v["n"], 2 * v["w"]
    host = FC.variety_frames(oracle_mod, YUYV, 1)
    set_a = FC.variety_ranges()
    set_b = [list(reversed(r)) for r in set_a[::-1]]
    want_a, _ = FC.variety_expected(oracle_mod, YUYV, 1)
    want_b, _ = FC.expected(oracle_mod, host, h * ll, n, w, h, ll, YUYV, set_b)
    assert (want_a != want_b).any(axis=(1, 2)).sum() > n // 2
    frames = _dev(host)
    pinned_b = torch.tensor(set_b, dtype=torch.int32).to(torch.int16).pin_memory()
    ranges = _ranges_dev(set_a)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        out1, _ = hsv.frame_ranges_batch(frames, w, h, ll, YUYV, ranges, stream=s)
        ranges.copy_(pinned_b, non_blocking=True)
        out2, _ = hsv.frame_ranges_batch(frames, w, h, ll, YUYV, ranges, stream=s)
    s.synchronize()
    assert np.array_equal(out1.cpu().numpy(), want_a)
    assert np.array_equal(out2.cpu().numpy(), want_b)


# ---- 7. the closed loop on the device ---------------------------------------
def test_closed_loop_on_the_device(hsv, oracle_mod):
    """batch_auto_range -> ranges_of_detect -> frame_ranges_batch with no host
    step between, against oracle.run(auto_detect) -> blob_range_of ->
    oracle.frame."""
    v = FC.LOOP
    w, h, n, ll = v["w"], v["h"], v["n"], 2 * v["w"]
    host = FC.loop_frames(oracle_mod)
    detect = FC.loop_detect(oracle_mod)
    ranges = [hsv.blob_range_of(d) for d in detect]
    assert ranges == [FC.blob_range_of(d) for d in detect]
    FC.check_loop(ranges)
    want_s, want_t = FC.expected(oracle_mod, host, h * ll, n, w, h, ll, YUYV, [[r] for r in ranges])
    assert (want_s[:, 0, 0] > 0).any()
    frames = _dev(host)
    det_dev = hsv.batch_auto_range(frames, w, h, ll, YUYV)
    rng_dev = hsv.ranges_of_detect(det_dev)
    sums, tg = hsv.frame_ranges_batch(frames, w, h, ll, YUYV, rng_dev)
    assert (det_dev.cpu().numpy().astype(np.int64) & 0xFFFF).tolist() == [list(d) for d in detect]
    assert rng_dev.cpu().numpy()[:, 0].tolist() == [list(r) for r in ranges]
    assert np.array_equal(sums.cpu().numpy(), want_s)
    assert np.array_equal(tg.cpu().numpy()[:, :, :3], want_t)


def test_ranges_of_detect_slots_and_wide_inputs(hsv):
    """Entry t of T is written, the others are left; hue wraps mod 360 and
    saturation / value clip for inputs no InArgs byte holds."""
    import torch

    det = [(0, 20, 80, 20, 50, 50), (350, 30, 10, 30, 95, 10), (179, 0, 0, 0, 100, 0), (10, 400, 300, 20, 50, 300),
           (65535, 65535, 65535, 0, 0, 65535)]
    d = torch.tensor(det, dtype=torch.int32).to(torch.int16).cuda()
    out = torch.full((len(det), 3, 6), 7, dtype=torch.int16, device="cuda")
    assert hsv.ranges_of_detect(d, ranges=out, t=1) is out
    got = out.cpu().numpy().astype(np.int64) & 0xFFFF
    assert (got[:, 0] == 7).all() and (got[:, 2] == 7).all()
    assert got[:, 1].tolist() == [list(FC.blob_range_of(x)) for x in det]
    assert got[:3, 1].tolist() == [list(hsv.blob_range_of(x)) for x in det[:3]]


def test_sat_and_val_above_255_behave_as_255(hsv, oracle_mod):
    v = FC.LOOP
    w, h, ll = v["w"], v["h"], 2 * v["w"]
    host = FC.loop_frames(oracle_mod)[:2 * h * ll]
    wide = [[(0, 359, 10, 300, 20, 300), (330, 20, 30, 65535, 30, 256)]] * 2
    as255 = [[(0, 359, 10, 255, 20, 255), (330, 20, 30, 255, 30, 255)]] * 2
    want_s, want_t = FC.expected(oracle_mod, host, h * ll, 2, w, h, ll, YUYV, as255)
    assert (want_s[:, :, 0] > 0).all()
    sums, tg = hsv.frame_ranges_batch(_dev(host), w, h, ll, YUYV, _ranges_dev(wide))
    assert np.array_equal(sums.cpu().numpy(), want_s) and np.array_equal(tg.cpu().numpy()[:, :, :3], want_t)


# ---- 8. against the existing kernels ----------------------------------------
def test_equals_process_batch_per_frame(hsv, oracle_mod):
    """8 VGA frames, T = 4: slot (f, .) is Detector.process_batch on frame f
    alone with f's set."""
    w, h, n, ll = 640, 480, 8, 1280
    fb = h * ll
    frames = _dev(oracle_mod.synth(n, w, h, ll, YUYV, 1, FC.SEED, first_frame=FC.FIRST_FRAME))
    ranges = FC.drawn(n, 4, 8)
    assert len({tuple(r) for r in ranges}) > 1
    sums, tg = hsv.frame_ranges_batch(frames, w, h, ll, YUYV, ranges)  # a host sequence: uploaded on the stream
    det = hsv.Detector()
    try:
        for f in range(n):
            s1, t1 = det.process_batch(frames[f * fb:(f + 1) * fb], w, h, ll, YUYV, ranges[f])
            assert (sums[f] == s1[0]).all().item() and (tg[f] == t1[0]).all().item(), f
    finally:
        det.close()
    assert (sums[:, :, 0] > 0).any().item()


def test_empty_geometry(hsv):
    """Width or height 0: zero sums and targets; n_frames 0: empty outputs."""
    import torch

    frames = torch.zeros(64, dtype=torch.uint8, device="cuda")
    rng = torch.zeros((3, 2, 6), dtype=torch.int16, device="cuda")
    sums, tg = hsv.frame_ranges_batch(frames, 640, 0, 1280, YUYV, rng, n_frames=3, frame_stride=0)
    assert sums.abs().sum().item() == 0 and tg.abs().sum().item() == 0
    sums, tg = hsv.frame_ranges_batch(frames, 64, 8, 128, YUYV, rng[:0], n_frames=0)
    assert sums.shape == (0, 2, 3) and tg.shape == (0, 2, 4)
