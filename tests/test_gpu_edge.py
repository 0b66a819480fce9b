"""The ov7670 edge-line sensor on the GPU against tests/edge_ref.py (TI's
documented natural-C semantics of the three IMGLIB calls plus ESEQ =
trik/ov7670/edge_line_sensor/include/internal/cv_ball_detector_seqpass.hpp):
sums, targets, the thresholded map and the preview bytes, bit-exact, through
edge_batch / Detector.edge_preview (trik_hsv_edge_batch / trik_hsv_edge_preview),
EdgeLineSensor.process (TRIK_VIDTRANSCODE_CV_create_edge_line) and the exported
XDAIS function table."""
import ctypes as C

import numpy as np
import pytest

import edge_ref
from gpu_util import LAYOUT_OV7670

pytestmark = pytest.mark.gpu


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


_REF = {}


def ref_run(key, frame, w, h, thr=50):
    """edge_ref.run, computed once per (frame, threshold) and shared."""
    k = (key, w, h, thr)
    if k not in _REF:
        _REF[k] = edge_ref.run(frame, w, h, thr)
    return _REF[k]


def binary_frame(w, h, seed):
    rng = np.random.default_rng(seed)
    fr = rng.integers(0, 256, 2 * w * h, dtype=np.uint8)
    fr[:w * h] = rng.integers(0, 2, w * h, dtype=np.uint8) * 255
    return fr


def steps_frame(w, h):
    """Rows 0, 0, 255, 255, ...: |H| = 1020 on every live row, so every window
    pixel is detected and, from 384 columns, every row's column sum wraps."""
    fr = np.full(2 * w * h, 128, np.uint8)
    fr[:w * h].reshape(h, w)[(np.arange(h) % 4) >= 2] = 255
    fr[:w * h].reshape(h, w)[(np.arange(h) % 4) < 2] = 0
    return fr


def make_frames(oracle_mod, w, h):
    """Uniform bytes, a scene, random {0, 255} luma, single-pixel frames (one
    inside the window, one whose edges straddle its left end), the steps."""
    return [("uniform", oracle_mod.synth(1, w, h, w, LAYOUT_OV7670, 0, 0x51DE)),
            ("scene", oracle_mod.synth(1, w, h, w, LAYOUT_OV7670, 1, 0x7A1C, first_frame=3)),
            ("binary", binary_frame(w, h, 11 * w + h)),
            ("pixel", edge_ref.single_pixel(w, h, 1, w // 2)),
            ("pixel16", edge_ref.single_pixel(w, h, h - 2, 16)),
            ("steps", steps_frame(w, h))]


def upload(frames):
    import torch

    return torch.from_numpy(np.concatenate([fr for _, fr in frames])).cuda()


# 32x4: a one-column window and two live rows; 352x8: the widest frame whose
# row sums cannot wrap; 384x4 and 640x8: the wrap frames; 320x240: the TRIK frame.
# The fast kernel's other shapes: 160x8 (a row takes 32 lanes), 64x52 (row
# segments of 17, 17 and 16 rows), 1024x4 (16 columns per lane), 1056x4 and
# 2048x4 (32 columns per lane; the cap)
GEOMS = [(32, 4), (64, 8), (96, 12), (352, 8), (384, 4), (640, 8), (320, 240), (160, 8), (64, 52), (1024, 4),
         (1056, 4), (2048, 4)]


@pytest.mark.parametrize("geom", GEOMS)
def test_edge_batch_vs_reference(hsv, oracle_mod, geom):
    w, h = geom
    frames = make_frames(oracle_mod, w, h)
    refs = [ref_run(name, fr, w, h) for name, fr in frames]
    assert refs[5][1][0] == (h - 2) * (w - 31)  # the steps: every window pixel of every live row
    for i in (0, 5):  # from 384 columns the per-row uint16 wrap decides the uniform and the steps frames' sums
        assert (edge_ref.sums(refs[i][0], wrap=False)[1] != refs[i][1][1]) == (w >= 384), (geom, i)
    assert refs[2][1][0] > 0 and refs[3][1][0] > 0
    dev = upload(frames)
    sums, targets = hsv.edge_batch(dev, w, h, w)  # the fast kernel
    sums_m, targets_m, emap = hsv.edge_batch(dev, w, h, w, edges=True)  # the generic kernel, with the map
    sums, targets, sums_m, targets_m, emap = (t.cpu().numpy() for t in (sums, targets, sums_m, targets_m, emap))
    for i, (name, _) in enumerate(frames):
        want_map, (p, sx), tg = refs[i]
        assert sums[i].tolist() == [p, sx, 0], (geom, name, "fast")
        assert sums_m[i].tolist() == [p, sx, 0], (geom, name, "generic")
        assert targets[i, :3].tolist() == [tg[0], tg[1], tg[2] - 256 * (tg[2] > 127)], (geom, name)
        assert np.array_equal(targets_m[i], targets[i])
        assert np.array_equal(emap[i], want_map), (geom, name)
        # the wrap columns, the two bytes and the two rows the Sobel loop never writes
        assert np.array_equal(emap[i][:, 0], want_map[:, 0]) and np.array_equal(emap[i][:, -1], want_map[:, -1])
        flat = emap[i].reshape(-1)
        assert flat[0] == 0 and flat[w * (h - 2) - 1] == 0 and not emap[i][h - 2:].any()
    # the wrap columns carry values (they mix two rows): the comparison above is not of zeros
    assert refs[0][0][:h - 2, 0].any() and refs[0][0][:h - 2, -1].any()


def test_edge_thresholds(hsv):
    """49, 50, 51, 52 and 255 on one frame: low-amplitude noise (magnitudes
    around 50) left, {0, 255} right.  O is even: 50 and 51 select the same
    pixels, 49 more, 52 fewer; 255 detects only where |H| + |V| >= 255."""
    w, h = 96, 12
    rng = np.random.default_rng(3)
    fr = rng.integers(0, 256, 2 * w * h, dtype=np.uint8)
    y = fr[:w * h].reshape(h, w)
    y[:, :48] = 100 + rng.integers(0, 30, (h, 48))
    y[:, 48:] = rng.integers(0, 2, (h, 48)) * 255
    dev = upload([("t", fr)])
    got = {}
    for thr in (49, 50, 51, 52, 255):
        want_map, (p, sx), tg = ref_run("thr", fr, w, h, thr)
        sums, targets = hsv.edge_batch(dev, w, h, w, thr)
        sums_m, _, emap = hsv.edge_batch(dev, w, h, w, thr, edges=True)
        assert sums[0].tolist() == [p, sx, 0] and sums_m[0].tolist() == [p, sx, 0], thr
        assert np.array_equal(emap[0].cpu().numpy(), want_map), thr
        got[thr] = p
    o = edge_ref.sobel(fr, w, h).reshape(h, w)[:, 16:w - 15]
    assert got[255] == int((o >= 255).sum()) > 0
    assert got[49] > got[50] == got[51] > got[52] > got[255]


@pytest.mark.parametrize("geom", [(64, 8), (384, 4), (320, 240)])
def test_edge_window_edges(hsv, geom):
    """A lone bright pixel at input column x marks map columns x-1 .. x+1:
    edges up to column 15 and from column W-15 are not counted, those at
    columns 16 and W-16 are."""
    w, h = geom
    cases = [(14, 0, 0), (15, 3, 3 * 16), (w - 14, 0, 0), (w - 15, 3, 3 * (w - 16))]
    if h == 4:  # two live rows: the pixel (input row 1) marks map rows 0 and 1, not three rows
        cases = [(x, n * 2 // 3, sx * 2 // 3) for x, n, sx in cases]
    frames = [(f"x{x}", edge_ref.single_pixel(w, h, 1 if h == 4 else 3, x)) for x, _, _ in cases]
    sums, _ = hsv.edge_batch(upload(frames), w, h, w)
    sums_m, _, _ = hsv.edge_batch(upload(frames), w, h, w, edges=True)
    for i, (x, n, sx) in enumerate(cases):
        assert ref_run(("edge", x), frames[i][1], w, h)[1] == (n, sx), (geom, x)
        assert sums[i].tolist() == [n, sx, 0] and sums_m[i].tolist() == [n, sx, 0], (geom, x)


@pytest.mark.parametrize("geom", [(64, 8), (640, 8)])
def test_edge_frames_are_isolated(hsv, oracle_mod, geom):
    """Three different frames, frame_stride larger than a frame with 0xFF
    between them: map row H-3 takes nothing from the next frame, rows H-2 and
    H-1 are 0, and every frame's results are its own."""
    import torch

    w, h = geom
    fb, stride = 2 * w * h, 2 * w * h + 64
    frames = make_frames(oracle_mod, w, h)[:3]
    host = np.full(3 * stride, 0xFF, np.uint8)
    for i, (_, fr) in enumerate(frames):
        host[i * stride:i * stride + fb] = fr
    dev = torch.from_numpy(host).cuda()
    sums, targets = hsv.edge_batch(dev, w, h, w, n_frames=3, frame_stride=stride)
    sums_m, _, emap = hsv.edge_batch(dev, w, h, w, n_frames=3, frame_stride=stride, edges=True)
    for i, (name, fr) in enumerate(frames):
        want_map, (p, sx), tg = ref_run(name, fr, w, h)
        assert sums[i].tolist() == [p, sx, 0] and sums_m[i].tolist() == [p, sx, 0], (geom, name)
        got = emap[i].cpu().numpy()
        assert np.array_equal(got, want_map) and not got[h - 2:].any(), (geom, name)


@pytest.mark.parametrize("geom", [(96, 12), (640, 8)])
def test_edge_misaligned_frames(hsv, oracle_mod, geom):
    """Frames at an odd address and an odd stride: the generic kernel, equal results."""
    import torch

    w, h = geom
    fb, stride = 2 * w * h, 2 * w * h + 3
    frames = make_frames(oracle_mod, w, h)[:3]
    host = np.zeros(1 + 3 * stride, np.uint8)
    for i, (_, fr) in enumerate(frames):
        host[1 + i * stride:1 + i * stride + fb] = fr
    dev = torch.from_numpy(host).cuda()
    sums, targets = hsv.edge_batch(dev[1:], w, h, w, n_frames=3, frame_stride=stride)
    for i, (name, fr) in enumerate(frames):
        _, (p, sx), tg = ref_run(name, fr, w, h)
        assert sums[i].tolist() == [p, sx, 0], (geom, name)
        assert [int(v) & 255 for v in targets[i, :3].tolist()] == [v & 255 for v in tg], (geom, name)


# (w, h, ow, oh, oll): 1:1; the TRIK default 2:1; a portrait output (shift
# 0.75); 2x up (the gaps stay zero); H = 8 (the line's rows clamp to the frame);
# a padded output line
PREVIEWS = [(64, 8, 64, 8, 128), (320, 240, 320, 240, 640), (320, 240, 160, 120, 320), (320, 240, 240, 320, 480),
            (64, 8, 128, 16, 256), (96, 12, 48, 6, 100)]


@pytest.mark.parametrize("geom", PREVIEWS)
def test_edge_preview_vs_reference(hsv, det, oracle_mod, geom):
    w, h, ow, oh, oll = geom
    flat = np.full(2 * w * h, 90, np.uint8)  # no edge: points = 0, no line
    frames = make_frames(oracle_mod, w, h)[:4] + [("flat", flat)]
    dev = upload(frames)
    sums, _ = hsv.edge_batch(dev, w, h, w)
    pv = det.edge_preview(dev, w, h, w, sums, out_width=ow, out_height=oh, out_line_length=oll).cpu().numpy()
    assert pv.shape == (len(frames), oh, oll)
    for i, (name, fr) in enumerate(frames):
        emap, (p, sx), _ = ref_run(name, fr, w, h)
        assert p == 0 if name == "flat" else p > 0 or name != "binary"
        want = edge_ref.preview(fr, w, h, emap, p, sx, ow, oh, oll)
        assert np.array_equal(pv[i], want), (geom, name)
        px = pv[i][:, :2 * ow].copy().view("<u2")
        if name == "flat":
            assert not (px == edge_ref.LINE_PIXEL).any()
        elif h == 8:  # rows 4 +- 99 clamp to 0 .. 7: the line spans every mapped output row
            col = edge_ref.scale_maps(w, h, ow, oh)[0][min(sx // p, w - 1)]
            rows = sorted(set(edge_ref.scale_maps(w, h, ow, oh)[1]))
            assert (px[rows, col] == edge_ref.LINE_PIXEL).all()
    if (ow, oh) == (2 * w, 2 * h):  # odd output rows and columns are never written
        assert not pv[:, 1::2].any() and not pv[:, :, 2::4].any() and not pv[:, :, 3::4].any()


def sensor(hsv, w, h, ow, oh, oll, streams=1):
    s = hsv.EdgeLineSensor(hsv._default_params(streams, fmt_in=hsv.FORMAT_YUV422P))
    assert s.set_params(w, h, w, out_width=ow, out_height=oh, out_line_length=oll) == 0, hsv._abi.last_error()
    return s


@pytest.mark.parametrize("geom", [(32, 4, 16, 2, 32), (64, 8, 64, 8, 128), (384, 4, 192, 2, 384),
                                  (320, 240, 320, 240, 640), (320, 240, 240, 320, 480)])
def test_edge_sensor_process(hsv, det, oracle_mod, geom):
    w, h, ow, oh, oll = geom
    s = sensor(hsv, w, h, ow, oh, oll)
    try:
        for name, fr in make_frames(oracle_mod, w, h)[:3]:
            out = np.full(oh * oll + 32, 0xAB, np.uint8)
            rc, oa = s.process(fr, out_buffer=out, hsv_range=(1, 2, 3, 4, 5, 6), auto_detect=True, input_id=7)
            assert rc == hsv.IVIDTRANSCODE_EOK, hsv._abi.last_error()
            emap, (p, sx), tg = ref_run(name, fr, w, h)
            assert (oa.alg.targetX, oa.alg.targetY, oa.alg.targetSize) == tg, (geom, name)
            assert oa.base.encodedBuf[0].bufSize == oh * oll and oa.base.bitsConsumed == fr.size * 8
            assert oa.base.outputID[0] == 7 and oa.base.outBufsInUseFlag == 0
            want = edge_ref.preview(fr, w, h, emap, p, sx, ow, oh, oll)
            assert np.array_equal(out[:oh * oll].reshape(oh, oll), want), (geom, name)
            assert not out[oh * oll:].any()  # the glue's zero fill of the whole buffer
            # process() = edge_batch + edge_preview
            import torch

            dev = torch.from_numpy(fr).cuda()
            sums, targets = hsv.edge_batch(dev, w, h, w)
            assert targets[0, :2].tolist() == [oa.alg.targetX, oa.alg.targetY]
            pv = det.edge_preview(dev, w, h, w, sums, out_width=ow, out_height=oh, out_line_length=oll)
            assert np.array_equal(pv[0].cpu().numpy(), out[:oh * oll].reshape(oh, oll))
    finally:
        s.close()


def test_edge_sensor_validation(hsv, det, oracle_mod):
    import torch

    w, h = 64, 8
    fr = oracle_mod.synth(1, w, h, w, LAYOUT_OV7670, 1, 2)
    s = sensor(hsv, w, h, 32, 4, 64)
    try:
        # SETPARAMS: a padded input line, a width that is no multiple of 32, a height that is no multiple of 4
        for bad in ((64, 8, 96), (48, 8, 48), (64, 6, 64), (4096, 8, 4096)):
            assert s.set_params(*bad, out_width=32, out_height=4, out_line_length=64) != 0, bad
            rc, oa = s.process(fr, out_buffer=np.zeros(4 * 64, np.uint8))
            assert rc == hsv.IVIDTRANSCODE_EFAIL, bad  # no algorithm until a valid SETPARAMS
        assert s.set_params(w, h, w, out_width=32, out_height=4, out_line_length=64) == 0
        # an input shorter than both planes, an output smaller than the preview
        rc, oa = s.process(fr[:w * h], out_buffer=np.zeros(4 * 64, np.uint8))
        assert rc == hsv.IVIDTRANSCODE_EFAIL and oa.base.extendedError & (1 << hsv._abi.XDM_CORRUPTEDDATA_BIT)
        rc, oa = s.process(fr, out_buffer=np.zeros(4 * 64 - 1, np.uint8))
        assert rc == hsv.IVIDTRANSCODE_EFAIL
        # the packed-YUYV input format is not this codec's
        with pytest.raises(hsv.TrikHsvError):
            hsv.EdgeLineSensor(hsv._default_params(1, fmt_in=hsv.FORMAT_YUV422))
        # still working after the failures
        rc, oa = s.process(fr, out_buffer=np.zeros(4 * 64, np.uint8))
        assert rc == 0 and (oa.alg.targetX, oa.alg.targetY, oa.alg.targetSize) == edge_ref.run(fr, w, h)[2]
    finally:
        s.close()
    # the batched calls: a padded line, the packed layout, a threshold out of range
    dev = torch.from_numpy(np.zeros(2 * 8 * 96, np.uint8)).cuda()
    with pytest.raises(hsv.TrikHsvError):
        hsv.edge_batch(dev, 64, 8, 96)
    with pytest.raises(hsv.TrikHsvError):
        hsv.edge_batch(dev, 64, 8, 64, 256)
    sums, _ = hsv.edge_batch(dev, 64, 8, 64)
    with pytest.raises(hsv.TrikHsvError):
        det.edge_preview(dev, 64, 8, 96, sums)
    with pytest.raises(hsv.TrikHsvError):  # the host-side OutArgs: a frame without columns
        hsv.edge_targets(1, 1, 0, 240)
    yuyv = hsv._abi.FrameBatch(dev.data_ptr(), 2 * 8 * 64, 1, 32, 8, 64, 0)
    assert hsv._lib.trik_hsv_edge_batch(C.byref(yuyv), 50, C.c_void_p(sums.data_ptr()), None, None, None) != 0


def test_edge_sensor_zero_output_streams(hsv, oracle_mod):
    w, h = 96, 12
    fr = oracle_mod.synth(1, w, h, w, LAYOUT_OV7670, 1, 4)
    s = sensor(hsv, w, h, 48, 6, 96, streams=0)
    try:
        out = np.full(6 * 96, 0xAB, np.uint8)
        rc, oa = s.process(fr, out_buffer=out)
        assert rc == 0 and (oa.alg.targetX, oa.alg.targetY, oa.alg.targetSize) == edge_ref.run(fr, w, h)[2]
        assert (out == 0xAB).all()  # no output stream: the buffer is left alone
    finally:
        s.close()


class MemRec(C.Structure):
    _fields_ = [("size", C.c_uint32), ("alignment", C.c_int32), ("space", C.c_int32), ("attrs", C.c_int32),
                ("base", C.c_void_p)]


class IalgFxns(C.Structure):
    _fields_ = [("implementationId", C.c_void_p), ("algActivate", C.c_void_p),
                ("algAlloc", C.CFUNCTYPE(C.c_int32, C.c_void_p, C.c_void_p, C.POINTER(MemRec))),
                ("algControl", C.c_void_p), ("algDeactivate", C.c_void_p),
                ("algFree", C.CFUNCTYPE(C.c_int32, C.c_void_p, C.POINTER(MemRec))),
                ("algInit", C.CFUNCTYPE(C.c_int32, C.c_void_p, C.POINTER(MemRec), C.c_void_p, C.c_void_p)),
                ("algMoved", C.c_void_p), ("algNumAlloc", C.c_void_p)]


class TranscodeFxns(C.Structure):
    _fields_ = [("ialg", IalgFxns),
                ("process", C.CFUNCTYPE(C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p)),
                ("control", C.CFUNCTYPE(C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p))]


def test_edge_through_the_function_table(hsv, oracle_mod):
    """A framework-style caller: algAlloc, its own record, algInit, control and
    process through TRIK_VIDTRANSCODE_CV_EDGE_LINE_FXNS, algFree.  The detect*
    OutArgs keep the caller's values."""
    w, h, ow, oh, oll = 96, 12, 48, 6, 100
    fr = binary_frame(w, h, 6)
    fx = TranscodeFxns.in_dll(hsv._lib, "TRIK_VIDTRANSCODE_CV_EDGE_LINE_FXNS")
    recs = (MemRec * 16)()
    assert fx.ialg.algAlloc(None, None, recs) == 1
    raw = C.create_string_buffer(recs[0].size + 256)
    base = (C.addressof(raw) + 255) & ~255
    recs[0].base = base
    C.c_void_p.from_address(base).value = C.addressof(fx)  # IALG_Obj.fxns, as the framework stores it
    assert fx.ialg.algInit(base, recs, None, None) == hsv.IALG_EOK, hsv._abi.last_error()
    try:
        dyn = hsv.dynamic_params(w, h, w, out_width=ow, out_height=oh, out_line_length=oll)
        st = hsv._abi.Status()
        assert fx.control(base, hsv.XDM_SETPARAMS, C.addressof(dyn), C.addressof(st)) == 0
        out = np.full(oh * oll, 0xAB, np.uint8)
        ib = hsv._abi.BufDesc1()
        ib.numBufs = 1
        ib.descs[0].buf = fr.ctypes.data
        ib.descs[0].bufSize = fr.size
        ob = hsv._abi.BufDesc()
        ob_arr, sz_arr = (C.c_void_p * 1)(out.ctypes.data), (C.c_int32 * 1)(out.nbytes)
        ob.bufs, ob.numBufs, ob.bufSizes = ob_arr, 1, sz_arr
        ia = hsv._abi.InArgs()
        ia.base.size, ia.base.numBytes = C.sizeof(hsv._abi.InArgs), fr.size
        oa = hsv._abi.OutArgs()
        oa.base.size = C.sizeof(hsv._abi.OutArgs)
        oa.alg = hsv._abi.OutArgsAlg(99, 99, 99, 11, 12, 13, 14, 15, 16)
        rc = fx.process(base, C.addressof(ib), C.addressof(ob), C.addressof(ia), C.addressof(oa))
        assert rc == hsv.IVIDTRANSCODE_EOK, hsv._abi.last_error()
        emap, (p, sx), tg = edge_ref.run(fr, w, h)
        assert p > 0 and (oa.alg.targetX, oa.alg.targetY, oa.alg.targetSize) == tg
        assert [oa.alg.detectHue, oa.alg.detectHueTolerance, oa.alg.detectSat, oa.alg.detectSatTolerance,
                oa.alg.detectVal, oa.alg.detectValTolerance] == [11, 12, 13, 14, 15, 16]
        assert np.array_equal(out.reshape(oh, oll), edge_ref.preview(fr, w, h, emap, p, sx, ow, oh, oll))
    finally:
        assert fx.ialg.algFree(base, recs) == 1
