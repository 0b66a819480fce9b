"""trik_hsv_frame_ranges_preview (fr_preview_rows2_kernel and
fr_preview_gather_kernel of
trik-media-sensors-dsp_amd/csrc/trik_hsv_frame_ranges_preview.hip under its
HsvTest, then overlay_kernel) on the GPU, byte for byte:

a. the range follows the frame: small frames, one task each, a range per frame;
b. grid passes: every wave takes three tasks and some a fourth, of other frames
   under other ranges;
c. every (Y, U, V) under sixteen ranges, in both kernels and both layouts, then
   again with the ranges rotated by one frame;
d. the slot: entry t of T ranges and the sums at the caller's pointer and pitch;
e. equality with N single-frame trik_hsv_batch_preview calls, line padding and
   gaps between previews included;
f. placement: each refusal of the 2:1 kernel alone, byte loads and stores,
   maps read from memory;
g. the ranges are read in stream order;
h. the closed loop on the device;
i. bounds and empty cases.

Inputs, the launcher's restated decision and the expectation are
tests/frame_ranges_preview_cases.py's; tests/test_frame_ranges_preview_cpu.py
asserts what each input reaches.  Each test asserts the restated decision for
the device's own CU count before it runs.
"""
import ctypes as C

import numpy as np
import pytest

import frame_ranges_cases as FC
import frame_ranges_preview_cases as PC
import preview_cases as pc
import preview_ref
from preview_ref import LAYOUT_OV7670, LAYOUT_YUYV

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5


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


def _ranges_dev(ranges):
    """[n][6] or [n][T][6] host ranges -> int16 [n, T, 6] on the device."""
    import torch

    t = torch.tensor(ranges, dtype=torch.int32).to(torch.int16)
    return (t[:, None, :] if t.dim() == 2 else t).contiguous().cuda()


def _sums_dev(sums):
    import torch

    return torch.from_numpy(np.ascontiguousarray(np.asarray(sums, np.int64))).cuda()


def _place(c, host):
    """The case's frames on the device at its offset from a 16-byte boundary."""
    import torch

    span = (c.n - 1) * c.frame_stride + c.fb
    raw = torch.full((span + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
    assert raw.data_ptr() % 16 == 0
    frames = raw[c.frames_offset:c.frames_offset + span]
    frames.copy_(torch.from_numpy(np.ascontiguousarray(host[:span])))
    return frames


def _call(hsv, det, c, frames, ranges, sums, *, t=0, sums_offset=0, sums_pitch=1, expect_rc0=True):
    """trik_hsv_frame_ranges_preview through the C ABI on `frames` (a device
    tensor that starts at the first frame), ranges int16 [n, T, 6], the sums at
    sums + sums_offset entries; the previews at the case's offset and stride
    inside a sentinel-filled buffer, so an unwritten preview byte shows and so
    does a write outside the previews.  Returns uint8 [n, pb]."""
    import torch

    assert frames.data_ptr() % 16 == c.frames_offset
    pspan = (c.n - 1) * c.preview_stride + c.pb
    raw_p = torch.full((pspan + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
    assert raw_p.data_ptr() % 16 == 0
    b = hsv._abi.FrameBatch(frames.data_ptr(), c.frame_stride, c.n, c.w, c.h, c.ll, c.layout)
    rc = hsv._lib.trik_hsv_frame_ranges_preview(
        det._h, C.byref(b), C.c_void_p(ranges.data_ptr()), ranges.shape[1], t,
        C.c_void_p(sums.data_ptr() + 24 * sums_offset), sums_pitch, c.ow, c.oh, c.oll,
        C.c_void_p(raw_p.data_ptr() + c.previews_offset), c.preview_stride,
        C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, hsv._abi.last_error()
    out = raw_p.cpu().numpy()
    keep = np.ones(out.size, bool)
    for f in range(c.n):
        keep[c.previews_offset + f * c.preview_stride:c.previews_offset + f * c.preview_stride + c.pb] = False
    assert (out[keep] == SENTINEL).all(), (c, "bytes outside the previews were written")
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
    p = PC.plan_of(c, _cus())
    assert p["kernel"] == want, (c, p)
    return p


# ------------------------------------------ a. the range follows the frame

@pytest.mark.parametrize("c", PC.follow_cases(), ids=repr)
def test_range_follows_the_frame(hsv, det, oracle_mod, table, c):
    p = _kernel(c, "gather" if "gather" in c.name else "rows2")
    assert p["idle"] > 0 and p["tasks"] == c.n * p["segs"]
    host = PC.follow_frames(table, c)
    ranges = PC.follow_ranges(c.n)
    sums = PC.own_sums(oracle_mod, host, c, ranges)
    assert (sums[:, 0] > 0).all()
    want = PC.expected(oracle_mod, table, host, c, ranges, sums)
    got = _call(hsv, det, c, _place(c, host), _ranges_dev(ranges), _sums_dev(sums))
    _same(got, want, (c, p))


# ---------------------------------------------------------- b. grid passes

GRID_NAMES = [c.name for c in PC.grid_cases(1)]


def _synth(hsv, c):
    """c.n different frames on the device: uniform bytes and scenes alternate."""
    import torch

    dev = torch.empty(c.n * c.fb, dtype=torch.uint8, device="cuda")
    hsv.synth(dev, c.w, c.h, c.ll, c.layout, 0, PC.SEED, first_frame=0, n_frames=(c.n + 1) // 2, frame_stride=2 * c.fb)
    hsv.synth(dev[c.fb:], c.w, c.h, c.ll, c.layout, 1, PC.SEED, first_frame=1, n_frames=c.n // 2, frame_stride=2 * c.fb)
    return dev, dev.cpu().numpy()


@pytest.mark.parametrize("name", GRID_NAMES)
def test_grid_passes(hsv, det, oracle_mod, name):
    """The sums are the frames' own (trik_hsv_frame_ranges_batch on the same
    range buffer), so preview f is oracle.run(frame f, range f)'s."""
    c = next(c for c in PC.grid_cases(_cus()) if c.name == name)
    p = _kernel(c, "gather" if "gather" in name else "rows2")
    assert p["grid"] == PC.BLOCKS_PER_CU * _cus() and p["min_tasks"] >= 3 and p["partial"], (c, p)
    dev, host = _synth(hsv, c)
    ranges = PC.pool_ranges(c.n)
    rd = _ranges_dev(ranges)
    sums, _ = hsv.frame_ranges_batch(dev, c.w, c.h, c.ll, c.layout, rd)
    got = _call(hsv, det, c, dev, rd, sums)
    _same(got, PC.oracle_previews(oracle_mod, host, c, ranges), (name, p))
    assert int((sums[:, 0, 0] > 0).sum()) > c.n // 4  # circles are drawn


# ---------------------------------------------------- c. every (Y, U, V)

@pytest.mark.parametrize("c", PC.exhaustive_cases(), ids=repr)
def test_every_triple(hsv, det, oracle_mod, table, c):
    """Sixteen frames that hold every (Y, U, V) at a sampled pixel, a range
    each; no points in the sums, so no circle."""
    import torch

    kind = "gather" if "gather" in c.name else "rows2"
    _kernel(c, kind)
    host = PC.exhaustive_batch(c.layout) if kind == "gather" else pc.sampled_batch(c.layout)
    assert host.size == c.n * c.fb
    dev = torch.from_numpy(host).cuda()
    sums = np.zeros((c.n, 3), np.int64)
    sums[:, 1:] = 12345  # (the sums of x and y must not matter without points)
    for shift in (0, 1):
        ranges = PC.sixteen_ranges(shift)
        want = PC.expected(oracle_mod, table, host, c, ranges, sums)
        got = _call(hsv, det, c, dev, _ranges_dev(ranges), _sums_dev(sums))
        _same(got, want, (c, "ranges rotated by %d" % shift))


# ------------------------------------------------------------- d. the slot

@pytest.mark.parametrize("c", pc.circle_cases(), ids=repr)
@pytest.mark.parametrize("layout", [LAYOUT_YUYV, LAYOUT_OV7670], ids=["yuyv", "ov7670"])
def test_the_slot(hsv, det, oracle_mod, table, layout, c):
    """T = 3, t = 1: entries 0 and 2 hold ranges and sums of other pictures;
    the circle comes from the caller's sums, at every edge.  Once through the
    C ABI with the sums pointer moved to the slot, once through the method."""
    c = pc.Case(c.name, c.w, c.h, layout, c.ow, c.oh, c.n)
    cases = pc.circle_sums(c.w, c.h)
    fr = pc.corner_block(table, pc.T0, c.w, c.h, c.ll, layout, "centre")
    host = np.tile(fr, c.n)
    ranges = [[PC.SLOT_OTHERS[0], pc.T0, PC.SLOT_OTHERS[1]]] * c.n
    sums = np.empty((c.n, PC.SLOT_T, 3), np.int64)
    sums[:] = PC.OTHER_SUMS
    sums[:, PC.SLOT_t] = [list(s) for _, s in cases]
    want = PC.expected(oracle_mod, table, host, c, [pc.T0] * c.n, sums[:, PC.SLOT_t])
    assert not np.array_equal(want[0], want[-1])
    frames, rd, sd = _place(c, host), _ranges_dev(ranges), _sums_dev(sums)
    got = _call(hsv, det, c, frames, rd, sd, t=PC.SLOT_t, sums_offset=PC.SLOT_t, sums_pitch=PC.SLOT_T)
    for i, (name, s) in enumerate(cases):
        assert np.array_equal(got[i], want[i]), (c, name, s, np.flatnonzero(got[i] != want[i])[:6].tolist())
    pv = det.frame_ranges_preview(frames, c.w, c.h, c.ll, layout, rd, sd, t=PC.SLOT_t, out_width=c.ow, out_height=c.oh)
    assert tuple(pv.shape) == (c.n, c.oh, c.oll) and np.array_equal(pv.cpu().numpy().reshape(c.n, -1), want)


# ---------------------------------------- e. against the shared-range call

@pytest.mark.parametrize("c", PC.equal_cases(), ids=repr)
def test_equals_the_shared_range_call(hsv, det, oracle_mod, table, c):
    import torch

    _kernel(c, "rows2" if "rows2" in c.name else "gather")
    host = PC.scene_frames(oracle_mod, c)
    ranges = PC.pool_ranges(c.n)
    frames, rd = _place(c, host), _ranges_dev(ranges)
    sums, _ = hsv.frame_ranges_batch(frames, c.w, c.h, c.ll, c.layout, rd)
    got = _call(hsv, det, c, frames, rd, sums)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for f in range(c.n):  # frame f alone through trik_hsv_batch_preview with the same six numbers
        one = torch.full((c.pb,), SENTINEL, dtype=torch.uint8, device="cuda")
        b = hsv._abi.FrameBatch(frames.data_ptr() + f * c.frame_stride, c.fb, 1, c.w, c.h, c.ll, c.layout)
        arr, _ = hsv._ranges([ranges[f]])
        rc = hsv._lib.trik_hsv_batch_preview(det._h, C.byref(b), arr, C.c_void_p(sums[f].data_ptr()), 1, c.ow, c.oh,
                                             c.oll, C.c_void_p(one.data_ptr()), c.pb, stream)
        assert rc == 0, hsv._abi.last_error()
        assert np.array_equal(got[f], one.cpu().numpy()), (c, f)
    _same(got, PC.expected(oracle_mod, table, host, c, ranges, sums[:, 0].cpu().numpy()), c)
    if c.oll > 2 * c.ow:
        assert not got.reshape(c.n, c.oh, c.oll)[:, :, 2 * c.ow:].any()


# -------------------------------------------------------------- f. placement

@pytest.mark.parametrize("c", PC.placement_cases(), ids=repr)
def test_placement(hsv, det, oracle_mod, table, c):
    p = PC.plan_of(c, _cus())
    if c.name.startswith("refuse"):
        cond = c.name.split("_", 2)[2]
        assert p["kernel"] == ("rows2" if cond == "twin" else "gather") and (cond == "twin" or p["refused"][0] == cond), p
    elif c.name.startswith("bytes"):
        assert p["kernel"] == "gather" and p["loads"] == "byte", p
    else:
        assert p["kernel"] == "gather" and not p["maps_lds"], p
    host = PC.scene_frames(oracle_mod, c)
    ranges = PC.pool_ranges(c.n, shift=1)
    sums = PC.own_sums(oracle_mod, host, c, ranges)
    want = PC.expected(oracle_mod, table, host, c, ranges, sums)
    got = _call(hsv, det, c, _place(c, host), _ranges_dev(ranges), _sums_dev(sums))
    _same(got, want, (c, p))


# ----------------------------------------------------------- g. stream order

def test_ranges_are_read_in_stream_order(hsv, det, oracle_mod, table):
    """Ranges A, a call, ranges B copied over them from pinned memory without
    waiting, a second call: each call's previews are those of its ranges."""
    import torch

    c = PC.equal_cases()[0]
    c = pc.Case("stream", c.w, c.h, c.layout, c.ow, c.oh, c.n)
    host = PC.scene_frames(oracle_mod, c)
    set_a, set_b = PC.pool_ranges(c.n), PC.pool_ranges(c.n, shift=5)
    sums = np.zeros((c.n, 3), np.int64)
    want_a = PC.expected(oracle_mod, table, host, c, set_a, sums)
    want_b = PC.expected(oracle_mod, table, host, c, set_b, sums)
    assert (want_a != want_b).any(axis=1).sum() > c.n // 2
    frames, sd = _place(c, host), _sums_dev(sums)
    pinned_b = torch.tensor(set_b, dtype=torch.int32).to(torch.int16)[:, None, :].contiguous().pin_memory()
    ranges = _ranges_dev(set_a)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        out1 = det.frame_ranges_preview(frames, c.w, c.h, c.ll, c.layout, ranges, sd, stream=s)
        ranges.copy_(pinned_b, non_blocking=True)
        out2 = det.frame_ranges_preview(frames, c.w, c.h, c.ll, c.layout, ranges, sd, stream=s)
    s.synchronize()
    _same(out1.cpu().numpy(), want_a, "first call")
    _same(out2.cpu().numpy(), want_b, "second call")


# ---------------------------------------------- h. the closed loop on the device

def test_closed_loop_on_the_device(hsv, det, oracle_mod):
    """batch_auto_range -> ranges_of_detect -> frame_ranges_batch ->
    frame_ranges_preview with no host step between, against oracle.run(frame
    f, range f)'s preview."""
    import torch

    c = PC.loop_case()
    host = FC.loop_frames(oracle_mod)
    ranges = PC.loop_ranges(oracle_mod)
    FC.check_loop(ranges)
    want = PC.oracle_previews(oracle_mod, host, c, ranges)
    frames = torch.from_numpy(np.array(host)).cuda()
    det_dev = hsv.batch_auto_range(frames, c.w, c.h, c.ll, c.layout)
    rng_dev = hsv.ranges_of_detect(det_dev)
    sums, _ = hsv.frame_ranges_batch(frames, c.w, c.h, c.ll, c.layout, rng_dev)
    pv = det.frame_ranges_preview(frames, c.w, c.h, c.ll, c.layout, rng_dev, sums)
    # the host reads only now
    assert rng_dev.cpu().numpy()[:, 0].tolist() == [list(r) for r in ranges]
    _same(pv.cpu().numpy(), want, "closed loop")
    assert int((sums[:, 0, 0] > 0).sum()) > 0


# ------------------------------------------------------ i. bounds and empties

def test_sat_and_val_above_255_behave_as_255(hsv, det, oracle_mod, table):
    c = pc.Case("wide", 96, 64, LAYOUT_YUYV, 48, 32, 4)
    host = PC.scene_frames(oracle_mod, c)
    wide = [(0, 359, 10, 300, 20, 300), (330, 20, 30, 65535, 30, 256)] * 2
    as255 = [(0, 359, 10, 255, 20, 255), (330, 20, 30, 255, 30, 255)] * 2
    sums = PC.own_sums(oracle_mod, host, c, as255)
    assert (sums[:, 0] > 0).all()
    want = PC.expected(oracle_mod, table, host, c, as255, sums)
    got = _call(hsv, det, c, _place(c, host), _ranges_dev(wide), _sums_dev(sums))
    _same(got, want, "bounds above 255")


def _raw(hsv, det, b, ranges, n_ranges, t, sums, ow, oh, oll, previews, stride):
    import torch

    p = lambda x: C.c_void_p(x.data_ptr()) if x is not None else None  # noqa: E731
    rc = hsv._lib.trik_hsv_frame_ranges_preview(det._h, C.byref(b), p(ranges), n_ranges, t, p(sums), 1, ow, oh, oll,
                                                p(previews), stride,
                                                C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc, hsv._abi.last_error()


def test_refusals_and_empty_cases(hsv, oracle_mod):
    import torch

    w, h, ow, oh, oll, n = 64, 8, 32, 4, 64, 3
    pb = oh * oll
    frames = torch.from_numpy(oracle_mod.synth(n, w, h, 2 * w, LAYOUT_YUYV, 1, PC.SEED)).cuda()
    ranges = _ranges_dev([[PC.POOL[0], PC.POOL[1]]] * n)
    sums = torch.zeros((n, 3), dtype=torch.int64, device="cuda")
    det = hsv.Detector()
    try:
        det.process_batch(frames, w, h, 2 * w, LAYOUT_YUYV, [PC.POOL[0]])
        hot = det.last_hot_kernel()

        def batch(n_frames=n, width=w, height=h, ll=2 * w):
            return hsv._abi.FrameBatch(frames.data_ptr(), h * 2 * w, n_frames, width, height, ll, LAYOUT_YUYV)

        def previews():
            return torch.full((n * pb,), SENTINEL, dtype=torch.uint8, device="cuda")

        for what, kw in (("ranges is NULL", dict(ranges=None)), ("n_ranges must be 1..64", dict(n_ranges=0)),
                         ("n_ranges must be 1..64", dict(n_ranges=65)),
                         ("frame_ranges_preview: t must be 0..n_ranges-1", dict(t=-1)),
                         ("frame_ranges_preview: t must be 0..n_ranges-1", dict(t=2)),
                         ("sums is NULL", dict(sums=None))):
            pv = previews()
            args = dict(ranges=ranges, n_ranges=2, t=0, sums=sums)
            args.update(kw)
            rc, err = _raw(hsv, det, batch(), args["ranges"], args["n_ranges"], args["t"], args["sums"], ow, oh, oll, pv, pb)
            assert rc != 0 and err == what, (kw, rc, err)
            assert bool((pv == SENTINEL).all()), (kw, "a refused call wrote the previews")
        # no frames, no preview rows: 0, nothing touched (NULL ranges are fine without frames)
        for b, r, rows in ((batch(n_frames=0), None, oh), (batch(), ranges, 0)):
            pv = previews()
            rc, err = _raw(hsv, det, b, r, 2, 0, sums, ow, rows, oll, pv, pb)
            assert rc == 0 and bool((pv == SENTINEL).all()), err
        # frames without pixels: the zero fill alone, as trik_hsv_batch_preview's
        for b in (batch(width=0, ll=0), batch(height=0)):
            pv = previews()
            rc, err = _raw(hsv, det, b, ranges, 2, 1, sums, ow, oh, oll, pv, pb)
            assert rc == 0 and bool((pv == 0).all()), err
            shared = previews()
            arr, _ = hsv._ranges([PC.POOL[1]])
            assert hsv._lib.trik_hsv_batch_preview(det._h, C.byref(b), arr, C.c_void_p(sums.data_ptr()), 1, ow, oh, oll,
                                                   C.c_void_p(shared.data_ptr()), pb,
                                                   C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
            assert torch.equal(pv, shared)
        # a full call on this handle leaves the hot-kernel report as it was
        pv = previews()
        rc, err = _raw(hsv, det, batch(), ranges, 2, 1, sums, ow, oh, oll, pv, pb)
        assert rc == 0 and not bool((pv == SENTINEL).any()), err
        assert det.last_hot_kernel() == hot
    finally:
        det.close()
