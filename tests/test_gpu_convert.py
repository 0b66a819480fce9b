"""trik_hsv_convert_batch on the GPU against tests/convert_ref.py, byte for
byte: the output buffer starts as a sentinel pattern and the whole buffer is
compared, so every pixel byte equals oracle.yuv_table's entry and every byte
the call may not write (pitch padding, between planes and frames, before `out`
and after the last frame) still holds the sentinel.  The cases are
tests/convert_cases.py's; tests/test_convert_cpu.py asserts what they cover."""
import ctypes as C

import numpy as np
import pytest

import convert_cases as CC
import convert_ref as CR
import gpu_util

pytestmark = pytest.mark.gpu

YUYV, OV7670 = CC.LAYOUT_YUYV, CC.LAYOUT_OV7670


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


def _call(hsv, frames, i, out, off, frame_stride, plane_stride, row_pitch, form, stream=None):
    """The C ABI itself: frame 0 at frames[i.off], `out` at out[off]."""
    import torch

    b = hsv._abi.FrameBatch(frames.data_ptr() + i.off, CC.in_stride(i), i.n, i.w, i.h, CC.in_ll(i), i.layout)
    o = hsv._abi.ConvertOut(out.data_ptr() + off, frame_stride, plane_stride, row_pitch, form)
    s = torch.cuda.current_stream() if stream is None else stream
    return hsv._lib.trik_hsv_convert_batch(C.byref(b), C.byref(o), C.c_void_p(s.cuda_stream))


def _check(hsv, table, buf, i, o):
    """Runs case (i, o) on input buffer buf and compares the whole output buffer."""
    want, off, frame_stride, plane_stride, row_pitch = CC.expected(table, buf, i, o)
    out = _dev(CC.sentinel(want.size))
    rc = _call(hsv, _dev(buf), i, out, off, frame_stride, plane_stride, row_pitch, o.form)
    assert rc == 0, hsv._abi.last_error()
    got = out.cpu().numpy()
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (CC.case_id(i, o), f"{bad.size} bytes differ, first at {bad[:6].tolist()} of {want.size}",
                           got[bad[:6]].tolist(), want[bad[:6]].tolist())


# ---- 1. all 2^24 (Y, U, V) ------------------------------------------------------
_exh_entries = {}


def _exhaustive_entries(table, layout):
    """uint64 [64, 32, 8192] of the exhaustive frames, computed once per layout
    (the base offset and the pitches of a case do not change the pixels)."""
    if layout not in _exh_entries:
        w, h, n = CC.EXH["w"], CC.EXH["h"], CC.EXH["n"]
        ll = CC.row_bytes(w, layout)
        ent = CR.entries(table, CC.exhaustive_frames(layout), CC.frame_bytes(w, h, ll, layout), n, w, h, ll, layout)
        ent.setflags(write=False)
        _exh_entries[layout] = ent
    return _exh_entries[layout]


@pytest.mark.parametrize("case", CC.EXHAUSTIVE,
                         ids=lambda c: f"{CC.LAYOUT_NAMES[c[0]]}-{CC.FORM_NAMES[c[1]]}-in{c[2]}-rowpad{c[3]}")
def test_exhaustive(hsv, table, case):
    """Every (Y, U, V) as 64 frames of 8192 x 32: all 2^24 entries compared."""
    import torch

    i, o = CC.exhaustive_case(*case)
    assert CC.form(i, o) == ("vec" if case[2] == 0 and case[3] == 0 else "generic")
    ent = _exhaustive_entries(table, i.layout)
    assert ent.size == 1 << 24
    off, frame_stride, plane_stride, row_pitch, size = CC.out_geometry(o, i.w, i.h, i.n)
    want = CC.sentinel(size)
    out = torch.from_numpy(want).cuda()  # (the device's copy of the sentinel, before the pixels are laid over it)
    CR.lay_out(ent, o.form, want, off, frame_stride, plane_stride, row_pitch)
    frames = torch.cat([torch.zeros(i.off, dtype=torch.uint8), torch.from_numpy(CC.exhaustive_frames(i.layout).copy())]).cuda()
    assert frames.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0
    assert _call(hsv, frames, i, out, off, frame_stride, plane_stride, row_pitch, o.form) == 0, hsv._abi.last_error()
    assert torch.equal(out.cpu(), torch.from_numpy(want))


# ---- 2. smallest geometries -------------------------------------------------------
def _small_cases():
    for layout in (YUYV, OV7670):
        for k, i in enumerate(CC.small_inputs(layout)):
            for f in CC.FORMS:
                yield pytest.param(i, CC.Out(f), 100 + k, id=CC.case_id(i, CC.Out(f)))


@pytest.mark.parametrize("i,o,seed", list(_small_cases()))
def test_small_geometries(hsv, table, i, o, seed):
    _check(hsv, table, CC.uniform_input(i, seed), i, o)


# ---- 3. output layout -------------------------------------------------------------
def _pitch_cases():
    for layout in (YUYV, OV7670):
        for f in CC.FORMS:
            for o in CC.pitch_outs(f):
                yield pytest.param(CC.PITCH_IN[layout], o, id=CC.case_id(CC.PITCH_IN[layout], o))


@pytest.mark.parametrize("i,o", list(_pitch_cases()))
def test_output_layout_leaves_the_padding(hsv, table, i, o):
    _check(hsv, table, CC.uniform_input(i, 7 + i.layout), i, o)


# ---- 4. Python surface --------------------------------------------------------------
@pytest.mark.parametrize("layout", [YUYV, OV7670])
def test_python_dense_defaults(hsv, table, layout):
    import torch

    i = CC.In(layout, 96, 8, 3)
    buf = CC.uniform_input(i, 21)
    ent = CR.entries(table, buf, CC.in_stride(i), i.n, i.w, i.h, CC.in_ll(i), layout)
    frames = _dev(buf)
    assert hsv.CONVERT_RGB888HSV == CC.RGB888HSV and hsv.CONVERT_HSV_PLANES == CC.HSV_PLANES
    default = hsv.convert_batch(frames, i.w, i.h, CC.in_ll(i), layout)
    assert default.dtype == torch.uint8 and tuple(default.shape) == (3, 3, 8, 96) and default.is_contiguous()
    assert np.array_equal(default.cpu().numpy(), CR.dense(ent, CC.HSV_PLANES))
    for f in CC.FORMS:
        got = hsv.convert_batch(frames, i.w, i.h, CC.in_ll(i), layout, f)
        want = CR.dense(ent, f)
        assert got.dtype == (torch.int64 if f == CC.RGB888HSV else torch.uint8) and got.is_contiguous()
        assert got.shape == want.shape and np.array_equal(got.cpu().numpy(), want)
    # n_frames and frame_stride: the first two frames, then frames 0 and 2
    two = hsv.convert_batch(frames, i.w, i.h, CC.in_ll(i), layout, CC.RGB888HSV, n_frames=2)
    assert np.array_equal(two.cpu().numpy(), CR.dense(ent[:2], CC.RGB888HSV))
    skip = hsv.convert_batch(frames, i.w, i.h, CC.in_ll(i), layout, CC.RGB_PLANES, n_frames=2,
                             frame_stride=2 * CC.in_stride(i))
    assert np.array_equal(skip.cpu().numpy(), CR.dense(ent[::2], CC.RGB_PLANES))


@pytest.mark.parametrize("f", CC.FORMS, ids=lambda f: CC.FORM_NAMES[f])
def test_python_out_as_a_strided_view(hsv, table, f):
    """`out` as a view of a larger tensor: its strides are taken as they are and
    the elements of the larger tensor outside the view keep their values."""
    import torch

    i = CC.In(YUYV, 64, 8, 2)
    buf = CC.uniform_input(i, 33)
    ent = CR.entries(table, buf, CC.in_stride(i), i.n, i.w, i.h, CC.in_ll(i), YUYV)
    want = CR.dense(ent, f)
    if f == CC.RGB888HSV:
        big = torch.full((3, 10, 72), -7, dtype=torch.int64, device="cuda")
        view = big[1:, 1:9, 4:68]
    else:
        big = torch.full((3, 4, 11, 70), 0xA5, dtype=torch.uint8, device="cuda")
        view = big[:2, 1:, 2:10, 3:67]
    before = big.clone()
    assert not view.is_contiguous()
    ret = hsv.convert_batch(_dev(buf), i.w, i.h, CC.in_ll(i), YUYV, f, out=view)
    assert ret is view and np.array_equal(view.cpu().numpy(), want)
    inside = torch.zeros_like(big, dtype=torch.bool)
    (inside[1:, 1:9, 4:68] if f == CC.RGB888HSV else inside[:2, 1:, 2:10, 3:67])[...] = True
    assert torch.equal(big[~inside], before[~inside])
    with pytest.raises(ValueError):
        hsv.convert_batch(_dev(buf), i.w, i.h, CC.in_ll(i), YUYV, f, out=view[..., :32])
    with pytest.raises(ValueError):
        hsv.convert_batch(_dev(buf), i.w, i.h, CC.in_ll(i), YUYV, f, out=view.to(torch.int32))


def test_python_stream_and_stream_order(hsv, table):
    """On a non-default stream; frames rewritten by a copy earlier on that
    stream are the ones converted (the host never reads them)."""
    import torch

    i = CC.In(OV7670, 640, 480, 4)
    old, new = CC.uniform_input(i, 1), CC.uniform_input(i, 2)
    ent = CR.entries(table, new, CC.in_stride(i), i.n, i.w, i.h, CC.in_ll(i), OV7670)
    assert (ent != CR.entries(table, old, CC.in_stride(i), i.n, i.w, i.h, CC.in_ll(i), OV7670)).any(axis=(1, 2)).all()
    frames = _dev(old)
    pinned = torch.from_numpy(new).pin_memory()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    assert s.cuda_stream != torch.cuda.current_stream().cuda_stream
    with torch.cuda.stream(s):
        frames.copy_(pinned, non_blocking=True)
    got = hsv.convert_batch(frames, i.w, i.h, CC.in_ll(i), OV7670, CC.RGB888HSV, stream=s)
    s.synchronize()
    assert np.array_equal(got.cpu().numpy(), CR.dense(ent, CC.RGB888HSV))


# ---- 5. consistency with the rest of the library ------------------------------------
@pytest.mark.parametrize("layout", [YUYV, OV7670])
def test_thresholded_planes_are_the_detectors_masks(hsv, oracle_mod, layout):
    """One 320 x 240 scene frame: HSV_PLANES thresholded on the host with
    oracle.pack_range and trik_oracle_detect gives Detector.batch_masks' mask
    for four ranges, one of them hue-wrapped."""
    w, h = 320, 240
    ll = CC.row_bytes(w, layout)
    ranges = gpu_util.BENCH_RANGES
    assert len(ranges) == 4 and sum(r[0] > r[1] for r in ranges) == 1
    frame = oracle_mod.synth(1, w, h, ll, layout, 1, 0x7A1C, first_frame=100)
    dev = _dev(frame)
    p = hsv.convert_batch(dev, w, h, ll, layout, CC.HSV_PLANES)[0].cpu().numpy().astype(np.uint32)
    packed = p[0] | (p[1] << 8) | (p[2] << 16)
    values, inverse = np.unique(packed, return_inverse=True)
    detect = oracle_mod.lib().trik_oracle_detect
    want = np.zeros(values.size, np.uint8)
    for t, r in enumerate(ranges):
        lo, hi, expect = oracle_mod.pack_range(r)
        want |= np.array([detect(int(v), lo, hi, expect) != 0 for v in values], np.uint8) << t
    want = want[inverse.reshape(-1)].reshape(h, w)
    det = hsv.Detector()
    try:
        masks, _ = det.batch_masks(dev, w, h, ll, layout, ranges)
    finally:
        det.close()
    assert np.array_equal(masks[0].cpu().numpy(), want)
    assert all(((want >> t) & 1).any() for t in range(4)) and not want.all()


# ---- 6. refusals and degenerate calls -----------------------------------------------
def test_refusals_leave_the_output_untouched(hsv):
    """Each refusal of the header, one at a time, with real buffers: non-zero,
    a message, and the sentinel-filled output as it was."""
    import torch

    abi = hsv._abi
    w, h, n = 64, 8, 2
    frames = torch.zeros(n * h * 2 * w, dtype=torch.uint8, device="cuda")
    size = n * 3 * h * 8 * w  # room for every form
    out = _dev(CC.sentinel(size))
    F, O = frames.data_ptr(), out.data_ptr()

    def batch(n=n, w=w, h=h, ll=2 * w, layout=YUYV, stride=None, frames=F):
        return abi.FrameBatch(frames, h * ll * (2 if layout == OV7670 else 1) if stride is None else stride, n, w, h, ll,
                              layout)

    def dst(form=0, out=O, row=None, plane=None, frame=None):
        row = (8 * w if form == 0 else w) if row is None else row
        plane = (0 if form == 0 else h * row) if plane is None else plane
        frame = (2 * plane + h * row) if frame is None else frame
        return abi.ConvertOut(out, frame, plane, row, form)

    cases = [(None, dst()), (batch(), None), (batch(frames=None), dst()), (batch(), dst(out=None)),
             (batch(layout=2), dst()), (batch(), dst(form=3)), (batch(), dst(form=-1)),
             (batch(w=33), dst()), (batch(h=6), dst()), (batch(w=-32), dst()), (batch(ll=2 * w - 1), dst()),
             (batch(layout=OV7670, ll=w - 1), dst()), (batch(stride=h * 2 * w - 1), dst()), (batch(n=-1), dst()),
             (batch(w=32768, ll=65536), dst())]
    for f in CC.FORMS:
        rb = 8 * w if f == 0 else w
        cases += [(batch(), dst(f, row=rb - 1, plane=h * rb, frame=3 * h * rb)),
                  (batch(), dst(f, frame=(1 if f == 0 else 3) * h * rb - 1)),
                  (batch(n=1), dst(f, frame=(1 if f == 0 else 3) * h * rb - 1))]
        if f:
            cases += [(batch(), dst(f, plane=h * rb - 1, frame=3 * h * rb)),
                      (batch(), dst(f, plane=h * rb + 16, frame=3 * h * rb + 31))]
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for k, (b, o) in enumerate(cases):
        rc = hsv._lib.trik_hsv_convert_batch(C.byref(b) if b is not None else None,
                                             C.byref(o) if o is not None else None, s)
        assert rc != 0 and abi.last_error(), k
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), CC.sentinel(size))
    # and the same buffers are fine: the call they refuse runs once the argument is mended
    assert hsv._lib.trik_hsv_convert_batch(C.byref(batch()), C.byref(dst()), s) == 0
    assert not np.array_equal(out.cpu().numpy(), CC.sentinel(size))


def test_degenerate_calls_write_nothing(hsv):
    import torch

    abi = hsv._abi
    size = 4096
    out = _dev(CC.sentinel(size))
    frames = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for f in CC.FORMS:
        for b, o in ((abi.FrameBatch(frames.data_ptr(), 1024, 0, 64, 8, 128, YUYV),
                      abi.ConvertOut(out.data_ptr(), 3 * 8 * 512, 8 * 512, 512, f)),
                     (abi.FrameBatch(None, 1024, 0, 64, 8, 128, YUYV), abi.ConvertOut(None, 3 * 8 * 512, 8 * 512, 512, f)),
                     (abi.FrameBatch(frames.data_ptr(), 0, 2, 0, 8, 0, YUYV), abi.ConvertOut(out.data_ptr(), 0, 0, 0, f)),
                     (abi.FrameBatch(frames.data_ptr(), 0, 2, 64, 0, 128, OV7670),
                      abi.ConvertOut(out.data_ptr(), 0, 0, 512, f))):
            assert hsv._lib.trik_hsv_convert_batch(C.byref(b), C.byref(o), s) == 0, abi.last_error()
        for n, w, h in ((0, 64, 8), (2, 0, 8), (2, 64, 0)):
            got = hsv.convert_batch(frames, w, h, 128, YUYV, f, n_frames=n)
            assert got.numel() == 0 and tuple(got.shape) == ((n, h, w) if f == 0 else (n, 3, h, w))
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), CC.sentinel(size))
