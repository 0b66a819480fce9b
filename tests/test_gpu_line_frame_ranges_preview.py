"""trik_hsv_line_frame_ranges_preview (fr_preview_rows2_kernel and
fr_preview_gather_kernel of
trik-media-sensors-dsp_amd/csrc/trik_hsv_frame_ranges_preview.hip under its
ValTest, then line_overlay_kernel behind the gather) on the GPU, byte for byte,
both layouts:

a. the range follows the frame: small frames, one task each, a V range per
   frame, an empty one and one above 100 among them;
b. grid passes: every wave takes three tasks and some a fourth;
c. every (Y, U, V) under 64 V ranges, in both kernels;
d. the target line from the caller's sums, at every edge;
e. equality with single-frame trik_hsv_line_preview calls (ov7670) and with
   WebcamLineSensor.process (YUYV);
f. placement: each refusal of the 2:1 kernel alone, byte loads and stores, gaps
   between previews;
g. ranges and sums are read in stream order;
h. the closed loop on the device, for both line kinds;
i. no table is built; refusals and empty cases.

Inputs, the launcher's restated decision and the expectation are
tests/line_frame_ranges_preview_cases.py's and tests/line_preview_ref.py's;
tests/test_line_frame_ranges_preview_cpu.py asserts what each input reaches and
holds the reference to the oracle.  Each test asserts the restated decision for
the device's own CU count before it runs.
"""
import ctypes as C

import numpy as np
import pytest

import autorange_ref
import frame_ranges_cases as FC
import line_frame_ranges_preview_cases as LP
import line_preview_ref as LR
import preview_cases as pc
from preview_ref import LAYOUT_OV7670, LAYOUT_YUYV

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
LAYOUT_IDS = ["yuyv", "ov7670"]


@pytest.fixture(scope="module")
def hsv():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import trik_hsv

    return trik_hsv


@pytest.fixture(scope="module")
def det(hsv):
    d = hsv.Detector()
    yield d
    d.close()


def _cus():
    import torch

    return torch.cuda.get_device_properties(0).multi_processor_count


def _ranges_dev(pairs):
    """int16 [n, 6] on the device: the pairs in entries 4 and 5."""
    import torch

    return torch.from_numpy(LP.six(pairs).view(np.int16)).cuda()


def _sums_dev(sums):
    import torch

    return torch.from_numpy(np.ascontiguousarray(np.asarray(sums, np.int64).reshape(-1, 3))).cuda()


def _place(c, host):
    """The case's frames on the device at its offset from a 16-byte boundary."""
    import torch

    span = (c.n - 1) * c.frame_stride + c.fb
    raw = torch.full((span + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
    assert raw.data_ptr() % 16 == 0
    frames = raw[c.frames_offset:c.frames_offset + span]
    frames.copy_(torch.from_numpy(np.ascontiguousarray(host[:span])))
    return frames


def _call(hsv, det, c, frames, ranges, sums):
    """The call through the C ABI on `frames` (a device tensor that starts at
    the first frame); the previews at the case's offset and stride inside a
    sentinel-filled buffer, so an unwritten preview byte shows and so does a
    write outside the previews.  Returns uint8 [n, pb]."""
    import torch

    assert frames.data_ptr() % 16 == c.frames_offset
    pspan = (c.n - 1) * c.preview_stride + c.pb
    raw_p = torch.full((pspan + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
    assert raw_p.data_ptr() % 16 == 0
    b = hsv._abi.FrameBatch(frames.data_ptr(), c.frame_stride, c.n, c.w, c.h, c.ll, c.layout)
    rc = hsv._lib.trik_hsv_line_frame_ranges_preview(
        det._h, C.byref(b), C.c_void_p(ranges.data_ptr()), C.c_void_p(sums.data_ptr()), c.ow, c.oh, c.oll,
        C.c_void_p(raw_p.data_ptr() + c.previews_offset), c.preview_stride,
        C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, hsv._abi.last_error()
    out = raw_p.cpu().numpy()
    keep = np.ones(out.size, bool)
    for f in range(c.n):
        keep[c.previews_offset + f * c.preview_stride:c.previews_offset + f * c.preview_stride + c.pb] = False
    assert (out[keep] == SENTINEL).all(), (c, "bytes outside the previews were written")
    if c.preview_stride == c.pb:
        return out[c.previews_offset:c.previews_offset + c.n * c.pb].reshape(c.n, c.pb)
    return np.stack([out[c.previews_offset + f * c.preview_stride:][:c.pb] for f in range(c.n)])


def _same(got, want, what):
    got, want = np.asarray(got).reshape(len(want), -1), np.asarray(want)
    bad = np.flatnonzero((got != want).any(axis=1))
    if bad.size:
        f = int(bad[0])
        at = np.flatnonzero(got[f] != want[f])
        raise AssertionError("%s: %d of %d previews differ, first %d at bytes %s: got %s, want %s" % (
            what, bad.size, len(want), f, at[:6].tolist(), got[f][at[:6]].tolist(), want[f][at[:6]].tolist()))


def _kernel(c, want):
    f = LP.forms_of(c, _cus())
    assert f["kernel"] == want, (c, f)
    return f


def _own_sums(hsv, c, frames, rd):
    """trik_hsv_line_frame_ranges_batch's sums buffer, taken as it is."""
    sums, _ = hsv.line_frame_ranges_batch(frames, c.w, c.h, c.ll, c.layout, rd, n_frames=c.n, frame_stride=c.frame_stride)
    return sums


# ------------------------------------------ a. the range follows the frame

@pytest.mark.parametrize("c", LP.follow_cases(), ids=repr)
def test_range_follows_the_frame(hsv, det, oracle_mod, table, c):
    f = _kernel(c, "gather" if "gather" in c.name else "rows2")
    assert f["idle"] > 0 and f["tasks"] == c.n
    host = LP.noise_frames(c, 11)
    frames = _place(c, host)
    smp = LR.sampled(table, LP.frames2d(host, c), c.w, c.h, c.ll, c.layout, c.ow, c.oh)
    for shift in (0, 1):  # the same frames, every range moved on by one frame
        pairs = LP.follow_pairs(c.n, shift)
        sums = LP.own_sums(oracle_mod, table, host, c, pairs)
        want = LP.expected(table, host, c, pairs, sums, smp)
        got = _call(hsv, det, c, frames, _ranges_dev(pairs), _sums_dev(sums))
        _same(got, want, (c, f, shift))
        assert (sums[:, 0] > 10).any() and (sums[:, 0] == 0).any()


# ---------------------------------------------------------- b. grid passes

GRID_NAMES = [c.name for c in LP.grid_cases(1)]


@pytest.mark.parametrize("name", GRID_NAMES)
def test_grid_passes(hsv, det, table, name):
    """The sums are the frames' own, written on the device by
    trik_hsv_line_frame_ranges_batch from the same range buffer."""
    c = next(c for c in LP.grid_cases(_cus()) if c.name == name)
    f = _kernel(c, "gather" if "gather" in name else "rows2")
    assert f["grid"] == LP.BLOCKS_PER_CU * _cus() and f["min_tasks"] >= 3 and f["partial"], (c, f)
    host = LP.noise_frames(c, 3)
    frames = _place(c, host)
    pairs = LP.follow_pairs(c.n)
    rd = _ranges_dev(pairs)
    sums = _own_sums(hsv, c, frames, rd)
    got = _call(hsv, det, c, frames, rd, sums)
    sums = sums.cpu().numpy()
    _same(got, LP.expected(table, host, c, pairs, sums), (name, f))
    assert int((sums[:, 0] > 10).sum()) > c.n // 4  # target lines are drawn


# ---------------------------------------------------- c. every (Y, U, V)

@pytest.mark.parametrize("c", LP.exhaustive_cases(), ids=repr)
def test_every_triple(hsv, det, table, c):
    """Sixteen frames that hold every (Y, U, V) at a sampled pixel, four passes
    of sixteen V ranges; no points in the sums, so no target line.  (The ov7670
    window keeps source columns 0..4 and W-4..W-1 out of the preview; the YUYV
    cases hold every triple.)"""
    import torch

    _kernel(c, "gather" if "gather" in c.name else "rows2")
    host = LP.exhaustive_host(c)
    assert host.size == c.n * c.fb
    dev = torch.from_numpy(host).cuda()
    smp = LR.sampled(table, LP.frames2d(host, c), c.w, c.h, c.ll, c.layout, c.ow, c.oh)
    if c.layout == LAYOUT_YUYV:
        assert smp[3].size == 1 << 24
    sums = np.zeros((c.n, 3), np.int64)
    sums[:, 1:] = 12345  # (the sums of x and y must not matter without points)
    sd = _sums_dev(sums)
    for p in range(LP.PASSES):
        pairs = LP.exhaustive_pairs(p)
        want = LP.expected(table, host, c, pairs, sums, smp)
        got = _call(hsv, det, c, dev, _ranges_dev(pairs), sd)
        _same(got, want, (c, "pass %d" % p))


# ------------------------------- d. the target line from the caller's sums

@pytest.mark.parametrize("c", LP.target_cases(), ids=repr)
def test_target_line_from_the_callers_sums(hsv, det, table, c):
    """One picture, a sums row per preview: cx at both edges and beside them,
    10 and 11 points, high words set, a quotient past the frame.  Once through
    the C ABI, once through the method."""
    _kernel(c, "rows2" if 2 * c.ow == c.w else "gather")
    cases = LP.target_sums(c.w)
    one = pc.Case("one", c.w, c.h, c.layout, c.ow, c.oh, 1)
    host = np.tile(LP.noise_frames(one, 5), c.n)
    pairs = LP.follow_pairs(c.n)
    sums = [s for _, s in cases]
    want = LP.expected(table, host, c, pairs, sums)
    frames, rd, sd = _place(c, host), _ranges_dev(pairs), _sums_dev(sums)
    got = _call(hsv, det, c, frames, rd, sd)
    for i, (name, s) in enumerate(cases):
        assert np.array_equal(got[i], want[i]), (c, name, s, np.flatnonzero(got[i] != want[i])[:6].tolist())
    pv = det.line_frame_ranges_preview(frames, c.w, c.h, c.ll, c.layout, rd, sd, out_width=c.ow, out_height=c.oh)
    assert tuple(pv.shape) == (c.n, c.oh, c.oll) and np.array_equal(pv.cpu().numpy().reshape(c.n, -1), want)
    # into the caller's tensor at the caller's stride: the bytes between the previews stay
    import torch

    stride = c.pb + 16
    mine = torch.full((c.n * stride,), SENTINEL, dtype=torch.uint8, device="cuda")
    assert det.line_frame_ranges_preview(frames, c.w, c.h, c.ll, c.layout, rd, sd, out_width=c.ow, out_height=c.oh,
                                         previews=mine, preview_stride=stride) is mine
    back = mine.cpu().numpy().reshape(c.n, stride)
    assert np.array_equal(back[:, :c.pb], want) and (back[:, c.pb:] == SENTINEL).all()


# ---------------------------------------- e. against the existing calls

@pytest.mark.parametrize("c", LP.equal_cases(), ids=repr)
def test_equals_the_existing_calls(hsv, det, oracle_mod, table, c):
    import torch

    host = LP.scene_frames(oracle_mod, c)
    pairs = LP.EQUAL_PAIRS[:c.n]
    frames, rd = _place(c, host), _ranges_dev(pairs)
    sums = _own_sums(hsv, c, frames, rd)
    got = _call(hsv, det, c, frames, rd, sums)
    assert int((sums[:, 0] > 10).sum()) >= 2
    if c.layout == LAYOUT_OV7670:  # frame f alone through trik_hsv_line_preview with the same two numbers
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        for f, (vf, vt) in enumerate(pairs):
            one = torch.full((c.pb,), SENTINEL, dtype=torch.uint8, device="cuda")
            b = hsv._abi.FrameBatch(frames.data_ptr() + f * c.frame_stride, c.fb, 1, c.w, c.h, c.ll, c.layout)
            rc = hsv._lib.trik_hsv_line_preview(det._h, C.byref(b), vf, vt, C.c_void_p(sums[f].data_ptr()), c.ow, c.oh,
                                                c.oll, C.c_void_p(one.data_ptr()), c.pb, stream)
            assert rc == 0, hsv._abi.last_error()
            assert np.array_equal(got[f], one.cpu().numpy()), (c, f)
    else:  # the webcam line codec's own preview of that frame and range
        s = hsv.WebcamLineSensor(hsv._default_params(1, hsv.FORMAT_YUV422, max(640, c.w), max(480, c.h, c.oh)))
        try:
            assert s.set_params(c.w, c.h, c.ll, out_width=c.ow, out_height=c.oh, out_line_length=c.oll) == 0
            for f, (vf, vt) in enumerate(pairs):
                out = np.full(c.pb, 0xCD, np.uint8)
                rc, _ = s.process(np.array(LP.frames2d(host, c)[f]), (0, 359, 0, 100, vf, vt), out_buffer=out)
                assert rc == 0, hsv._abi.last_error()
                assert np.array_equal(got[f], out), (c, f)
        finally:
            s.close()
    _same(got, LP.expected(table, host, c, pairs, sums.cpu().numpy()), c)


# -------------------------------------------------------------- f. placement

@pytest.mark.parametrize("c", LP.placement_cases(), ids=repr)
def test_placement(hsv, det, oracle_mod, table, c):
    f = LP.forms_of(c, _cus())
    cond = c.name.split("_", 2)[2]
    if c.name.startswith("refuse"):
        assert f["kernel"] == ("rows2" if cond == "twin" else "gather") and (cond == "twin" or f["refused"][0] == cond), f
    elif c.name.startswith("bytes"):
        assert f["kernel"] == "gather" and f["loads"] == "byte", f
    else:
        assert f["kernel"] == ("rows2" if cond == "gap" else "gather") and (cond != "gap" or c.preview_stride > c.pb), f
    host = LP.noise_frames(c, 7)
    pairs = LP.follow_pairs(c.n, shift=2)
    sums = LP.own_sums(oracle_mod, table, host, c, pairs)
    want = LP.expected(table, host, c, pairs, sums)
    got = _call(hsv, det, c, _place(c, host), _ranges_dev(pairs), _sums_dev(sums))
    _same(got, want, (c, f))
    if c.oll > 2 * c.ow:
        assert not got.reshape(c.n, c.oh, c.oll)[:, :, 2 * c.ow:].any()


# ----------------------------------------------------------- g. stream order

@pytest.mark.parametrize("layout", LP.LAYOUTS, ids=LAYOUT_IDS)
def test_ranges_and_sums_are_read_in_stream_order(hsv, det, oracle_mod, table, layout):
    """Ranges and sums A, a call, ranges and sums B copied over them on the
    same stream without waiting, a second call: each call's previews are those
    of its own ranges and sums."""
    import torch

    c = pc.Case("stream", 96, 64, layout, 48, 32, 7)
    host = LP.noise_frames(c, 13)
    set_a, set_b = LP.follow_pairs(c.n), LP.follow_pairs(c.n, shift=3)
    sums_a = LP.own_sums(oracle_mod, table, host, c, set_a)
    sums_b = LP.own_sums(oracle_mod, table, host, c, set_b)
    smp = LR.sampled(table, LP.frames2d(host, c), c.w, c.h, c.ll, c.layout, c.ow, c.oh)
    want_a, want_b = LP.expected(table, host, c, set_a, sums_a, smp), LP.expected(table, host, c, set_b, sums_b, smp)
    assert (want_a != want_b).any(axis=1).all()
    frames = _place(c, host)
    ranges, sums = _ranges_dev(set_a), _sums_dev(sums_a)
    next_ranges, next_sums = _ranges_dev(set_b), _sums_dev(sums_b)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        out1 = det.line_frame_ranges_preview(frames, c.w, c.h, c.ll, layout, ranges, sums, stream=s)
        ranges.copy_(next_ranges, non_blocking=True)
        sums.copy_(next_sums, non_blocking=True)
        out2 = det.line_frame_ranges_preview(frames, c.w, c.h, c.ll, layout, ranges, sums, stream=s)
    s.synchronize()
    _same(out1.cpu().numpy(), want_a, "first call")
    _same(out2.cpu().numpy(), want_b, "second call")


# ---------------------------------------------- h. the closed loop on the device

@pytest.mark.parametrize("layout", LP.LAYOUTS, ids=LAYOUT_IDS)
def test_closed_loop_on_the_device(hsv, det, oracle_mod, table, layout):
    """batch_auto_range_exact -> ranges_of_detect -> line_frame_ranges_batch ->
    the preview with no host step between; the expectation is built on the host
    alone: autorange_ref's detect values, their from / to form, line_ref's or
    oracle.frame's sums, line_preview_ref's previews."""
    c = pc.Case("loop", 320, 240, layout, 160, 120, 4)
    kind = autorange_ref.LINE if layout == LAYOUT_OV7670 else autorange_ref.WLINE
    host = LP.scene_frames(oracle_mod, c)
    detect = [autorange_ref.detect(table, fr, c.w, c.h, c.ll, kind)["out"] for fr in LP.frames2d(host, c)]
    pairs = [tuple(FC.blob_range_of(d)[4:6]) for d in detect]
    assert len(set(pairs)) >= 2, pairs
    sums_want = LP.own_sums(oracle_mod, table, host, c, pairs)
    want = LP.expected(table, host, c, pairs, sums_want)
    frames = _place(c, host)
    kind_dev = hsv.AUTO_OV7670_LINE if layout == LAYOUT_OV7670 else hsv.AUTO_WEBCAM_LINE
    assert kind_dev == kind
    det_dev, _ = hsv.batch_auto_range_exact(frames, c.w, c.h, c.ll, kind_dev)
    rng_dev = hsv.ranges_of_detect(det_dev, n_ranges=1)
    sums, _ = hsv.line_frame_ranges_batch(frames, c.w, c.h, c.ll, layout, rng_dev)
    pv = det.line_frame_ranges_preview(frames, c.w, c.h, c.ll, layout, rng_dev, sums)
    # the host reads only now
    back = rng_dev.cpu().numpy().view(np.uint16).reshape(c.n, 6)
    assert [(int(r[4]), int(r[5])) for r in back] == pairs
    assert sums.cpu().numpy().tolist() == sums_want.tolist()
    _same(pv.cpu().numpy(), want, "closed loop")
    assert int((sums[:, 0] > 10).sum()) > 0


# ------------------------------------------ i. no table, refusals, empties

def _raw(hsv, det, b, ranges, sums, ow, oh, oll, previews, stride):
    import torch

    p = lambda x: (x if isinstance(x, C.c_void_p) else C.c_void_p(x.data_ptr())) if x is not None else None  # noqa: E731
    rc = hsv._lib.trik_hsv_line_frame_ranges_preview(det._h, C.byref(b), p(ranges), p(sums), ow, oh, oll, p(previews),
                                                     stride, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc, hsv._abi.last_error()


@pytest.mark.parametrize("layout", LP.LAYOUTS, ids=LAYOUT_IDS)
def test_no_table_refusals_and_empty_cases(hsv, oracle_mod, layout):
    import torch

    w, h, ow, oh, oll, n = 64, 8, 32, 4, 64, 3
    ll = pc.line_length(w, layout)
    fb, pb = pc.frame_bytes(w, h, ll, layout), oh * oll
    c = pc.Case("raw", w, h, layout, ow, oh, n)
    frames = torch.from_numpy(LP.noise_frames(c, 17)).cuda()
    ranges = _ranges_dev(LP.follow_pairs(n))
    sums = torch.zeros((n, 3), dtype=torch.int64, device="cuda")
    det = hsv.Detector()
    try:
        yuyv = torch.from_numpy(oracle_mod.synth(n, w, h, 2 * w, LAYOUT_YUYV, 1, 5)).cuda()
        det.process_batch(yuyv, w, h, 2 * w, LAYOUT_YUYV, [FC.POOL[0]])
        hot = det.last_hot_kernel()

        def batch(n_frames=n, width=w, height=h, line_length=ll, lay=layout):
            return hsv._abi.FrameBatch(frames.data_ptr(), fb, n_frames, width, height, line_length, lay)

        def previews():
            return torch.full((n * pb,), SENTINEL, dtype=torch.uint8, device="cuda")

        host_ranges = np.zeros((n, 6), np.uint16)  # pageable host memory: refused by its kind, never read
        for what, kw in (("ranges is NULL", dict(ranges=None)), ("sums is NULL", dict(sums=None)),
                         ("previews is NULL", dict(previews=None)), ("unknown layout", dict(b=batch(lay=2))),
                         ("ranges is", dict(ranges=C.c_void_p(host_ranges.ctypes.data)))):
            pv = previews()
            args = dict(b=batch(), ranges=ranges, sums=sums, previews=pv)
            args.update(kw)
            rc, err = _raw(hsv, det, args["b"], args["ranges"], args["sums"], ow, oh, oll, args["previews"], pb)
            assert rc != 0 and err.startswith(what), (kw, rc, err)
            assert bool((pv == SENTINEL).all()), (kw, "a refused call wrote the previews")
        # no frames, no preview rows, no output at all: 0, nothing touched (NULL buffers are fine without frames)
        for b, r, s, dims in ((batch(n_frames=0), None, None, (ow, oh, oll)), (batch(), ranges, sums, (ow, 0, oll)),
                              (batch(), ranges, sums, (0, 0, 0)), (batch(), ranges, sums, (0, oh, 0))):
            pv = previews()
            rc, err = _raw(hsv, det, b, r, s, dims[0], dims[1], dims[2], pv, pb)
            assert rc == 0 and bool((pv == SENTINEL).all()), (dims, err)
        # frames without pixels: the zero fill alone
        for b in (batch(width=0, line_length=0), batch(height=0)):
            pv = previews()
            rc, err = _raw(hsv, det, b, ranges, sums, ow, oh, oll, pv, pb)
            assert rc == 0 and bool((pv == 0).all()), err
        # a full call on this handle leaves the hot-kernel report as it was: no table set was acquired
        # (every byte is written: two calls over different fills leave the same bytes)
        pv, other = previews(), torch.full((n * pb,), SENTINEL ^ 0xFF, dtype=torch.uint8, device="cuda")
        for buf in (pv, other):
            rc, err = _raw(hsv, det, batch(), ranges, sums, ow, oh, oll, buf, pb)
            assert rc == 0, err
        assert torch.equal(pv, other)
        assert det.last_hot_kernel() == hot
    finally:
        det.close()
