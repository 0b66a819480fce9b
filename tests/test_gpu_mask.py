"""trik_hsv_mask_batch on the GPU against tests/mask_ref.py, byte for byte: the
output buffer starts as a sentinel pattern and the whole buffer is compared, so
every mask byte is the reference's detectHsvPixel and every byte the call may
not write (pitch padding, between planes and frames, before `out` and after
the last frame) still holds the sentinel.  The cases are tests/mask_cases.py's;
tests/test_mask_cpu.py asserts what they cover."""
import ctypes as C

import numpy as np
import pytest

import mask_cases as MC
import mask_ref as MR

pytestmark = pytest.mark.gpu

YUYV, OV7670 = MC.LAYOUT_YUYV, MC.LAYOUT_OV7670
LAYOUTS = [YUYV, OV7670]


@pytest.fixture(scope="module")
def hsv():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import trik_hsv

    return trik_hsv


def _dev(buf):
    import torch

    t = torch.from_numpy(np.array(buf)).cuda()  # (a copy: cached cases are read-only)
    assert t.data_ptr() % 16 == 0
    return t


def _call(hsv, frames, i, ranges_dev, t, ranges_stride, out, off, frame_stride, plane_stride, row_pitch, form,
          stream=None):
    """The C ABI itself: frame 0 at frames[i.off], `out` at out[off]."""
    import torch

    b = hsv._abi.FrameBatch(frames.data_ptr() + i.off, MC.in_stride(i), i.n, i.w, i.h, MC.in_ll(i), i.layout)
    o = hsv._abi.MaskOut(out.data_ptr() + off, frame_stride, plane_stride, row_pitch, form)
    s = torch.cuda.current_stream() if stream is None else stream
    return hsv._lib.trik_hsv_mask_batch(C.byref(b), C.c_void_p(ranges_dev.data_ptr()), t, ranges_stride, C.byref(o),
                                        C.c_void_p(s.cuda_stream))


def _diff(got, want, what):
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (what, f"{bad.size} bytes differ, first at {bad[:6].tolist()} of {want.size}",
                           got[bad[:6]].tolist(), want[bad[:6]].tolist())


def _check(hsv, oracle_mod, table, buf, i, ranges, o, ranges_stride=None, kernel=None):
    """Runs case (i, ranges, o) on input buffer buf and compares the whole output
    buffer; ranges_stride None: 6 T.  Returns the reference planes."""
    t = len(ranges[0])
    if kernel is not None:
        assert MC.form(i, o, t) == kernel
    want, off, frame_stride, plane_stride, row_pitch, det = MC.expected(oracle_mod, table, buf, i, ranges, o)
    out = _dev(MC.sentinel(want.size))
    stride = 6 * t if ranges_stride is None else ranges_stride
    rng = _dev(MC.ranges_buffer(ranges, stride))
    rc = _call(hsv, _dev(buf), i, rng, t, stride, out, off, frame_stride, plane_stride, row_pitch, o.form)
    assert rc == 0, hsv._abi.last_error()
    _diff(out.cpu().numpy(), want, MC.case_id(i, o))
    return det


# ---- 1. all 2^24 (Y, U, V) ------------------------------------------------------
_exh_planes = []


def _exhaustive_planes(oracle_mod, table):
    """bool [64, 16, 32, 8192] of the exhaustive frames, computed once: the two
    layouts hold the same (Y, U, V) at every pixel (tests/test_mask_cpu.py),
    and the base offset and the pitches of a case do not change the pixels."""
    if not _exh_planes:
        i = MC.In(YUYV, MC.EXH["w"], MC.EXH["h"], MC.EXH["n"])
        det = MR.planes(oracle_mod, table, MC.exhaustive_frames(YUYV), MC.in_stride(i), i.n, i.w, i.h, MC.in_ll(i), YUYV,
                        MC.exhaustive_ranges())
        det.setflags(write=False)
        _exh_planes.append(det)
    return _exh_planes[0]


@pytest.mark.parametrize("case", MC.EXHAUSTIVE,
                         ids=lambda c: f"{MC.LAYOUT_NAMES[c[0]]}-{MC.FORM_NAMES[c[1]]}-in{c[2]}-rowpad{c[3]}")
def test_exhaustive(hsv, oracle_mod, table, case):
    """Every (Y, U, V) as 64 frames of 8192 x 32 under 16 ranges, frame f under
    their rotation by f: all 2^24 triples under every range."""
    import torch

    i, o = MC.exhaustive_case(*case)
    assert MC.form(i, o, 16) == ("vec" if case[2] == 0 and case[3] == 0 else "generic")
    det = _exhaustive_planes(oracle_mod, table)
    assert det.shape == (64, 16, 32, 8192)
    off, frame_stride, plane_stride, row_pitch, size = MC.out_geometry(o, i.w, i.h, i.n, 16)
    want = MC.sentinel(size)
    out = torch.from_numpy(want).cuda()  # (the device's copy of the sentinel, before the mask is laid over it)
    MR.lay_out(det, o.form, want, off, frame_stride, plane_stride, row_pitch)
    frames = torch.cat([torch.zeros(i.off, dtype=torch.uint8),
                        torch.from_numpy(MC.exhaustive_frames(i.layout).copy())]).cuda()
    rng = _dev(MC.ranges_buffer(MC.exhaustive_ranges()))
    assert frames.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0
    rc = _call(hsv, frames, i, rng, 16, 96, out, off, frame_stride, plane_stride, row_pitch, o.form)
    assert rc == 0, hsv._abi.last_error()
    assert torch.equal(out, torch.from_numpy(want).cuda())


# ---- 2. smallest geometries -------------------------------------------------------
def _small_cases():
    for layout in LAYOUTS:
        for k, i in enumerate(MC.small_inputs(layout)):
            for f in MC.FORMS:
                yield pytest.param(i, MC.Out(f), 100 + k, id=MC.case_id(i, MC.Out(f)))


@pytest.mark.parametrize("i,o,seed", list(_small_cases()))
def test_small_geometries(hsv, oracle_mod, table, i, o, seed):
    _check(hsv, oracle_mod, table, MC.uniform_input(i, seed), i, MC.small_ranges(i), o)


# ---- 3. T, and the three ways to pass the ranges ------------------------------------------
@pytest.mark.parametrize("t", MC.T_VALUES)
@pytest.mark.parametrize("f", MC.FORMS, ids=lambda f: MC.FORM_NAMES[f])
@pytest.mark.parametrize("layout", LAYOUTS, ids=lambda v: MC.LAYOUT_NAMES[v])
def test_range_counts_and_strides(hsv, oracle_mod, table, layout, f, t):
    i = MC.T_IN[layout]
    buf = MC.uniform_input(i, 40 + layout)
    ranges = MC.t_sets(i.n, t)
    # a set per frame, at 6 T; then with padding tuples between the sets (an odd stride too)
    _check(hsv, oracle_mod, table, buf, i, ranges, MC.Out(f), kernel="vec")
    _check(hsv, oracle_mod, table, buf, i, ranges, MC.Out(f), ranges_stride=6 * t + 12)
    _check(hsv, oracle_mod, table, buf, i, ranges, MC.Out(f, row_pad=1), ranges_stride=6 * t + 7, kernel="generic")
    # stride 0: the per-frame call given N copies of the set
    shared = [ranges[2]] * i.n
    want, off, frame_stride, plane_stride, row_pitch, _ = MC.expected(oracle_mod, table, buf, i, shared, MC.Out(f))
    frames = _dev(buf)
    outs = []
    for rng, stride in ((MC.ranges_buffer(shared), 6 * t), (MC.ranges_buffer(shared[:1]), 0)):
        out = _dev(MC.sentinel(want.size))
        assert _call(hsv, frames, i, _dev(rng), t, stride, out, off, frame_stride, plane_stride, row_pitch, f) == 0
        outs.append(out.cpu().numpy())
    _diff(outs[0], want, "N copies")
    _diff(outs[1], want, "stride 0")


# ---- 4. range edges ---------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS, ids=lambda v: MC.LAYOUT_NAMES[v])
def test_range_edges_one_hot(hsv, oracle_mod, table, layout):
    """Each edge range alone (T = 1), then all of them as one set."""
    i = MC.In(layout, 96, 8, 2)
    buf = MC.uniform_input(i, 61 + layout)
    for f in MC.FORMS:
        for r in MC.EDGE_RANGES:
            det = _check(hsv, oracle_mod, table, buf, i, [[r]] * 2, MC.Out(f))
            MC.check_planes(det, [[r]] * 2, r)
        _check(hsv, oracle_mod, table, buf, i, [MC.EDGE_RANGES, MC.EDGE_RANGES[::-1]], MC.Out(f))


# ---- 5. output placement ----------------------------------------------------------------------
def _pitch_cases():
    for layout in LAYOUTS:
        for f in MC.FORMS:
            for o in MC.pitch_outs(f):
                yield pytest.param(MC.PITCH_IN[layout], o, id=MC.case_id(MC.PITCH_IN[layout], o))


@pytest.mark.parametrize("i,o", list(_pitch_cases()))
def test_output_placement_leaves_the_padding(hsv, oracle_mod, table, i, o):
    _check(hsv, oracle_mod, table, MC.uniform_input(i, 7 + i.layout), i, MC.small_ranges(i), o)


def test_planes_interleaved_by_rows_are_refused(hsv):
    """plane_stride = a row's bytes with row_pitch = T rows would interleave the
    planes row by row: plane_stride < height * row_pitch, which the call
    refuses (the header says so); nothing is written."""
    import torch

    w, h, t = 64, 8, 3
    frames = torch.zeros(h * 2 * w, dtype=torch.uint8, device="cuda")
    rng = _dev(MC.ranges_buffer([[MC.FULL] * t]))
    for f in MC.FORMS:
        rb = MC.row_bytes(f, w)
        size = t * h * rb
        out = _dev(MC.sentinel(size))
        b = hsv._abi.FrameBatch(frames.data_ptr(), h * 2 * w, 1, w, h, 2 * w, YUYV)
        o = hsv._abi.MaskOut(out.data_ptr(), size, rb, t * rb, f)
        s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        assert hsv._lib.trik_hsv_mask_batch(C.byref(b), C.c_void_p(rng.data_ptr()), t, 0, C.byref(o), s) != 0
        assert "plane_stride" in hsv._abi.last_error()
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), MC.sentinel(size))


# ---- 6. one-hot columns -----------------------------------------------------------------------
@pytest.mark.parametrize("width", MC.COLUMN_WIDTHS)
@pytest.mark.parametrize("f", MC.FORMS, ids=lambda f: MC.FORM_NAMES[f])
@pytest.mark.parametrize("layout", LAYOUTS, ids=lambda v: MC.LAYOUT_NAMES[v])
def test_one_hot_columns(hsv, oracle_mod, table, layout, f, width):
    """Frame c has column c detected alone: the lane-to-bit formula a column at
    a time, through the vector kernel and (row_pitch + 1) the generic one."""
    i = MC.In(layout, width, MC.COLUMN_H, width)
    buf = MC.one_hot_columns(width, layout)
    ranges = [[MC.COLUMN_RANGE]] * width
    for o, kernel in ((MC.Out(f), "vec"), (MC.Out(f, row_pad=1), "generic")):
        det = _check(hsv, oracle_mod, table, buf, i, ranges, o, kernel=kernel)
        assert np.array_equal(det, MC.one_hot_planes(width))


# ---- 7. consistency with the sums call ----------------------------------------------------------
@pytest.mark.parametrize("f", MC.FORMS, ids=lambda f: MC.FORM_NAMES[f])
@pytest.mark.parametrize("layout", LAYOUTS, ids=lambda v: MC.LAYOUT_NAMES[v])
def test_mask_agrees_with_the_sums_call(hsv, layout, f):
    """On the same device buffers: popcount of plane (f, t) = points, the sums
    of the set bits' columns and rows = sum_x and sum_y of
    trik_hsv_frame_ranges_batch."""
    import torch

    i = MC.In(layout, 160, 120, 6)
    t = 5
    frames = _dev(MC.uniform_input(i, 90 + layout))
    rng = torch.from_numpy(MC.ranges_buffer(MC.drawn(i.n, t, 3))).cuda().reshape(i.n, t, 6)
    sums, _ = hsv.frame_ranges_batch(frames, i.w, i.h, MC.in_ll(i), layout, rng)
    mask = hsv.mask_batch(frames, i.w, i.h, MC.in_ll(i), layout, rng, f)
    m = mask.cpu().numpy()
    assert m.shape == (i.n, t, i.h, MC.row_bytes(f, i.w)) and m.dtype == np.uint8
    if f == MC.BITS:
        det = np.unpackbits(m, axis=-1, bitorder="little").astype(bool)
    else:
        assert np.isin(m, (0, 255)).all()
        det = m == 255
    got = np.stack([det.sum(axis=(2, 3)), (det * np.arange(i.w)).sum(axis=(2, 3)),
                    (det * np.arange(i.h)[:, None]).sum(axis=(2, 3))], axis=-1)
    want = sums.cpu().numpy()
    assert np.array_equal(got, want)
    assert (want[:, :, 0] > 0).any() and (want[:, :, 0] < i.w * i.h).any()


# ---- 8. stream order and the closed loop ----------------------------------------------------------
def test_ranges_rewritten_on_the_stream(hsv, oracle_mod, table):
    """On a non-default stream; the ranges a copy earlier on that stream wrote
    are the ones the second call uses (the host never reads them)."""
    import torch

    i = MC.In(YUYV, 640, 480, 4)
    buf = MC.uniform_input(i, 77)
    ra, rb = MC.t_sets(i.n, 4), MC.t_sets(i.n + 1, 4)[1:]
    ll, stride = MC.in_ll(i), MC.in_stride(i)
    want_a = MR.dense(MR.planes(oracle_mod, table, buf, stride, i.n, i.w, i.h, ll, YUYV, ra), MR.BITS)
    want_b = MR.dense(MR.planes(oracle_mod, table, buf, stride, i.n, i.w, i.h, ll, YUYV, rb), MR.BITS)
    assert (want_a != want_b).any(axis=(1, 2, 3)).all()
    frames = _dev(buf)
    ranges = torch.from_numpy(MC.ranges_buffer(ra)).cuda().reshape(i.n, 4, 6)
    pinned_b = torch.from_numpy(MC.ranges_buffer(rb)).reshape(i.n, 4, 6).pin_memory()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    assert s.cuda_stream != torch.cuda.current_stream().cuda_stream
    with torch.cuda.stream(s):
        out1 = hsv.mask_batch(frames, i.w, i.h, ll, YUYV, ranges, stream=s)
        ranges.copy_(pinned_b, non_blocking=True)
        out2 = hsv.mask_batch(frames, i.w, i.h, ll, YUYV, ranges, stream=s)
    s.synchronize()
    assert np.array_equal(out1.cpu().numpy(), want_a)
    assert np.array_equal(out2.cpu().numpy(), want_b)


@pytest.mark.parametrize("f", MC.FORMS, ids=lambda f: MC.FORM_NAMES[f])
def test_closed_loop_on_the_device(hsv, oracle_mod, table, f):
    """batch_auto_range_exact -> ranges_of_detect -> mask_batch on one stream
    with no host step between (the loop frames as ov7670 planes, the exact
    search's layout), against the reference under the ranges read back."""
    import torch

    v = MC.LOOP
    w, h, n = v["w"], v["h"], v["n"]
    host = MC.loop_frames(oracle_mod)
    fb = h * 2 * w
    planes = np.concatenate([MC.ov7670_twin(host[k * fb:(k + 1) * fb], w, h) for k in range(n)])
    dev = _dev(planes)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        det_dev, _ = hsv.batch_auto_range_exact(dev, w, h, w, hsv.AUTO_OV7670_OBJECT, stream=s)
        rng_dev = hsv.ranges_of_detect(det_dev, stream=s)
        mask = hsv.mask_batch(dev, w, h, w, OV7670, rng_dev, f, stream=s)
    s.synchronize()
    ranges = [[tuple(int(x) for x in r[0])] for r in (rng_dev.cpu().numpy().astype(np.int64) & 0xFFFF)]
    assert len({r[0] for r in ranges}) >= 2, ranges
    want = MR.planes(oracle_mod, table, planes, fb, n, w, h, w, OV7670, ranges)
    assert want.any() and not want.all()
    assert np.array_equal(mask.cpu().numpy(), MR.dense(want, f))


# ---- the Python surface --------------------------------------------------------------------------
def test_python_shared_set_and_strided_views(hsv, oracle_mod, table):
    import torch

    i = MC.In(YUYV, 64, 8, 3)
    buf = MC.uniform_input(i, 33)
    ranges = MC.small_ranges(i)
    ll = MC.in_ll(i)
    det = MR.planes(oracle_mod, table, buf, MC.in_stride(i), i.n, i.w, i.h, ll, YUYV, ranges)
    frames = _dev(buf)
    assert hsv.MASK_BITS == MC.BITS and hsv.MASK_BYTES == MC.BYTES
    # a host sequence, per frame and shared
    got = hsv.mask_batch(frames, i.w, i.h, ll, YUYV, ranges)
    assert got.dtype == torch.uint8 and got.is_contiguous() and np.array_equal(got.cpu().numpy(), MR.dense(det, MR.BITS))
    shared = hsv.mask_batch(frames, i.w, i.h, ll, YUYV, ranges[1], hsv.MASK_BYTES)
    want = MR.planes(oracle_mod, table, buf, MC.in_stride(i), i.n, i.w, i.h, ll, YUYV, [ranges[1]] * i.n)
    assert np.array_equal(shared.cpu().numpy(), MR.dense(want, MR.BYTES))
    # ranges as a view with a larger first stride; `out` as a view of a larger tensor
    wide = torch.full((i.n, 7, 6), 0, dtype=torch.int16, device="cuda")
    wide[:] = torch.tensor(MC.PAD_RANGE, dtype=torch.int16)
    wide[:, :5] = torch.from_numpy(MC.ranges_buffer(ranges)).reshape(i.n, 5, 6)
    big = torch.full((4, 6, 10, 70), 0xA5, dtype=torch.uint8, device="cuda")
    view = big[:3, 1:, 2:, 3:67]
    before = big.clone()
    assert hsv.mask_batch(frames, i.w, i.h, ll, YUYV, wide[:, :5], hsv.MASK_BYTES, out=view) is view
    assert np.array_equal(view.cpu().numpy(), MR.dense(det, MR.BYTES))
    inside = torch.zeros_like(big, dtype=torch.bool)
    inside[:3, 1:, 2:, 3:67] = True
    assert torch.equal(big[~inside], before[~inside])
    with pytest.raises(ValueError):
        hsv.mask_batch(frames, i.w, i.h, ll, YUYV, wide[:, :5], hsv.MASK_BITS, out=view)
    with pytest.raises(ValueError):
        hsv.mask_batch(frames, i.w, i.h, ll, YUYV, wide[:2, :5])


# ---- 9. refusals and degenerate calls ---------------------------------------------------------------
def test_refusals_leave_the_output_untouched(hsv):
    """Each refusal of the header, one at a time, with real buffers: non-zero,
    a message, and the sentinel-filled output as it was."""
    import torch

    abi = hsv._abi
    w, h, n, t = 64, 8, 2, 3
    frames = torch.zeros(n * h * 2 * w, dtype=torch.uint8, device="cuda")
    size = n * t * h * w  # room for both forms
    out = _dev(MC.sentinel(size))
    rng = _dev(MC.ranges_buffer([[MC.FULL] * t] * n))
    F, O, R = frames.data_ptr(), out.data_ptr(), rng.data_ptr()

    def batch(n=n, w=w, h=h, ll=2 * w, layout=YUYV, stride=None, frames=F):
        return abi.FrameBatch(frames, h * ll * (2 if layout == OV7670 else 1) if stride is None else stride, n, w, h, ll,
                              layout)

    def dst(form=0, out=O, row=None, plane=None, frame=None, t=t):
        row = MC.row_bytes(form, w) if row is None else row
        plane = h * row if plane is None else plane
        frame = (t - 1) * plane + h * row if frame is None else frame
        return abi.MaskOut(out, frame, plane, row, form)

    ok = (R, t, 6 * t)
    cases = [(None, ok, dst()), (batch(), ok, None), (batch(frames=None), ok, dst()), (batch(), ok, dst(out=None)),
             (batch(), (None, t, 6 * t), dst()),
             (batch(layout=2), ok, dst()), (batch(), ok, dst(form=2)), (batch(), ok, dst(form=-1)),
             (batch(w=33), ok, dst()), (batch(h=6), ok, dst()), (batch(w=-32), ok, dst()), (batch(ll=2 * w - 1), ok, dst()),
             (batch(layout=OV7670, ll=w - 1), ok, dst()), (batch(stride=h * 2 * w - 1), ok, dst()), (batch(n=-1), ok, dst()),
             (batch(w=32768, ll=65536), ok, dst()),
             (batch(), (R, 0, 0), dst(t=1)), (batch(), (R, -1, 0), dst(t=1)), (batch(), (R, 65, 0), dst(t=65)),
             (batch(), (R, t, 1), dst()), (batch(), (R, t, 6 * t - 1), dst()), (batch(), (R, t, -6 * t), dst()),
             (batch(), (R, t, -1), dst())]
    for f in MC.FORMS:
        rb = MC.row_bytes(f, w)
        cases += [(batch(), ok, dst(f, row=rb - 1, plane=h * rb, frame=t * h * rb)),
                  (batch(), ok, dst(f, plane=h * rb - 1, frame=t * h * rb)),
                  (batch(), ok, dst(f, plane=rb, row=t * rb, frame=t * h * rb)),
                  (batch(), ok, dst(f, frame=t * h * rb - 1)),
                  (batch(n=1), ok, dst(f, frame=t * h * rb - 1)),
                  (batch(), ok, dst(f, plane=h * rb + 16, frame=t * h * rb + 31))]
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    call = hsv._lib.trik_hsv_mask_batch
    for k, (b, (r, nr, rs), o) in enumerate(cases):
        rc = call(C.byref(b) if b is not None else None, C.c_void_p(r), nr, rs, C.byref(o) if o is not None else None, s)
        assert rc != 0 and abi.last_error(), k
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), MC.sentinel(size))
    # and the same buffers are fine: the call they refuse runs once the argument is mended
    assert call(C.byref(batch()), C.c_void_p(R), t, 6 * t, C.byref(dst()), s) == 0
    assert call(C.byref(batch()), C.c_void_p(R), t, 0, C.byref(dst(1)), s) == 0
    assert not np.array_equal(out.cpu().numpy(), MC.sentinel(size))


def test_degenerate_calls_write_nothing(hsv):
    import torch

    abi = hsv._abi
    size = 4096
    out = _dev(MC.sentinel(size))
    frames = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    rng = _dev(MC.ranges_buffer([[MC.FULL]]))
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for f in MC.FORMS:
        for b, r, o in ((abi.FrameBatch(frames.data_ptr(), 1024, 0, 64, 8, 128, YUYV), rng.data_ptr(),
                         abi.MaskOut(out.data_ptr(), 8 * 64, 8 * 64, 64, f)),
                        (abi.FrameBatch(None, 1024, 0, 64, 8, 128, YUYV), None, abi.MaskOut(None, 8 * 64, 8 * 64, 64, f)),
                        (abi.FrameBatch(frames.data_ptr(), 0, 2, 0, 8, 0, YUYV), rng.data_ptr(),
                         abi.MaskOut(out.data_ptr(), 0, 0, 0, f)),
                        (abi.FrameBatch(frames.data_ptr(), 0, 2, 64, 0, 128, OV7670), rng.data_ptr(),
                         abi.MaskOut(out.data_ptr(), 0, 0, 64, f))):
            assert hsv._lib.trik_hsv_mask_batch(C.byref(b), C.c_void_p(r), 1, 0, C.byref(o), s) == 0, abi.last_error()
        for n, w, h in ((0, 64, 8), (2, 0, 8), (2, 64, 0)):
            got = hsv.mask_batch(frames, w, h, 128, YUYV, rng.reshape(1, 6), f, n_frames=n)
            assert got.numel() == 0 and tuple(got.shape) == (n, 1, h, MC.row_bytes(f, w))
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), MC.sentinel(size))
