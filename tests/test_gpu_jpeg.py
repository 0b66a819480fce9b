"""The ov7670 JPEG encoder on the GPU against tests/jpeg_ref.py (the reference's
sequential encoder, JENC = trik/ov7670/jpeg_encoder/include/internal/
jpeg_encoder_reference.hpp): quantised coefficients, stream lengths and stream
bytes, all exact, through Detector.jpeg_batch (trik_hsv_jpeg_batch),
JpegSensor.process (TRIK_VIDTRANSCODE_CV_create_jpeg) and the exported XDAIS
function table.  The inputs are tests/jpeg_cases.py's; tests/test_jpeg_cpu.py
checks that they reach every path of the coder."""
import ctypes as C

import numpy as np
import pytest

import jpeg_cases
from jpeg_cases import LAYOUT_OV7670

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A


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


def run_batch(det, frames, geom, q, bw, *, capacity, stride=None, frame_stride=None, coeffs=True):
    """One jpeg_batch call over the frames (host arrays) into a sentinel-filled
    buffer: (streams [N, stride] uint8, sizes [N], coeffs) as numpy."""
    import torch

    w, h, ll = geom
    fb = 2 * h * ll
    fs = fb if frame_stride is None else frame_stride
    host = np.zeros(fs * len(frames), np.uint8)
    for i, fr in enumerate(frames):
        host[i * fs: i * fs + fb] = fr
    stride = capacity if stride is None else stride
    out = torch.full((len(frames), stride), SENTINEL, dtype=torch.uint8, device="cuda")
    res = det.jpeg_batch(torch.from_numpy(host).cuda(), w, h, ll, q, bw, capacity=capacity, out_stride=stride,
                         n_frames=len(frames), frame_stride=fs, coeffs=coeffs, out=out)
    torch.cuda.synchronize()
    return (out.cpu().numpy(), res[1].cpu().numpy(), res[2].cpu().numpy() if coeffs else None)


def check_against_ref(oracle_mod, det, geom, names, q, bw, **kw):
    frames = jpeg_cases.frames_of(oracle_mod, geom)
    refs = [jpeg_cases.ref(oracle_mod, geom, n, q, bw) for n in names]
    cap = max(len(r[0]) for r in refs) + 37
    streams, sizes, coeffs = run_batch(det, [frames[n] for n in names], geom, q, bw, capacity=cap, **kw)
    for i, (n, (want, want_c, _)) in enumerate(zip(names, refs)):
        tag = (geom, n, q, bw)
        assert np.array_equal(coeffs[i], want_c), tag  # transform, truncations, rounding
        assert int(sizes[i]) == len(want), tag
        assert streams[i, : len(want)].tobytes() == want, tag
        assert (streams[i, len(want):] == SENTINEL).all(), tag  # nothing past the stream


@pytest.mark.parametrize("geom", jpeg_cases.SMALL)
@pytest.mark.parametrize("bw", [False, True])
def test_small_geometries_vs_reference(det, oracle_mod, geom, bw):
    names = sorted(jpeg_cases.frames_of(oracle_mod, geom))
    for q in jpeg_cases.QUALITIES_SMALL:
        check_against_ref(oracle_mod, det, geom, names, q, bw)


@pytest.mark.parametrize("q", jpeg_cases.QUALITIES_MID)
@pytest.mark.parametrize("bw", [False, True])
def test_320x240_vs_reference(det, oracle_mod, q, bw):
    check_against_ref(oracle_mod, det, jpeg_cases.MID, list(jpeg_cases.MID_NAMES), q, bw)


@pytest.mark.parametrize("case", jpeg_cases.VGA_CASES)
def test_640x480_vs_reference(det, oracle_mod, case):
    name, q, bw = case
    check_against_ref(oracle_mod, det, jpeg_cases.VGA, [name], q, bw)


def test_random_blocks_coefficients_quality_100(det, oracle_mod):
    """About 20,000 data units of uniform random bytes at quality 100, where
    every coefficient survives quantisation: the guard against a fused
    multiply-add or a wrong rounding anywhere in the transform."""
    import jpeg_ref

    w, h, ll = 640, 96, 640
    n = 3  # 3 frames x 960 blocks x 3 components = 8640 data units, and the 14400 of the VGA case
    host = oracle_mod.synth(n, w, h, ll, LAYOUT_OV7670, 0, 0xC0EF)
    fb = 2 * h * ll
    _, _, coeffs = run_batch(det, [host[i * fb: (i + 1) * fb] for i in range(n)], (w, h, ll), 100, False,
                             capacity=0)
    for i in range(n):
        want = jpeg_ref.coefficients(host[i * fb: (i + 1) * fb], w, h, ll, 100, False)
        assert np.array_equal(coeffs[i], want), i


@pytest.mark.parametrize("pad", [64, 1])
def test_batch_of_seven_equals_single_frames(det, oracle_mod, pad):
    """Seven different frames in one call, frame_stride and out_stride larger
    than needed (pad 1: no 4-byte alignment, the byte-load path): each equals
    its single-frame result -- no frame leaks into another."""
    geom = (64, 64, 64)
    frames = jpeg_cases.frames_of(oracle_mod, geom)
    names = sorted(frames)
    assert len(names) == 7
    for q, bw in ((75, False), (100, True)):
        refs = [jpeg_cases.ref(oracle_mod, geom, n, q, bw) for n in names]
        cap = max(len(r[0]) for r in refs)
        streams, sizes, coeffs = run_batch(det, [frames[n] for n in names], geom, q, bw, capacity=cap,
                                           stride=cap + 123, frame_stride=2 * 64 * 64 + pad)
        for i, (want, want_c, _) in enumerate(refs):
            assert int(sizes[i]) == len(want) and streams[i, : len(want)].tobytes() == want, (names[i], q, bw)
            assert (streams[i, len(want):] == SENTINEL).all() and np.array_equal(coeffs[i], want_c)


def test_capacity_and_sizes_only(hsv, det, oracle_mod):
    """capacity = size - 1: the slot keeps its sentinel, sizes is the full
    length (like snprintf); capacity = size: written; out NULL: the same sizes."""
    import torch

    geom = (64, 16, 64)
    frames = jpeg_cases.frames_of(oracle_mod, geom)
    names = ["uniform", "flat"]
    refs = [jpeg_cases.ref(oracle_mod, geom, n, 50, False)[0] for n in names]
    big, small = len(refs[0]), len(refs[1])
    assert small < big
    streams, sizes, _ = run_batch(det, [frames[n] for n in names], geom, 50, False, capacity=big - 1, stride=big + 8,
                                  coeffs=False)
    assert sizes.tolist() == [big, small]
    assert (streams[0] == SENTINEL).all()  # one byte short: nothing written
    assert streams[1, :small].tobytes() == refs[1] and (streams[1, small:] == SENTINEL).all()
    streams, sizes, _ = run_batch(det, [frames[n] for n in names], geom, 50, False, capacity=big, stride=big + 8,
                                  coeffs=False)
    assert sizes.tolist() == [big, small] and streams[0, :big].tobytes() == refs[0]
    assert (streams[0, big:] == SENTINEL).all()
    dev = torch.from_numpy(np.concatenate([frames[n] for n in names])).cuda()
    none, sizes = det.jpeg_batch(dev, 64, 16, 64, 50, False, sizes_only=True)
    assert none is None and sizes.cpu().tolist() == [big, small]


def test_batch_divergences(hsv, det, oracle_mod):
    """A height that is no multiple of 8 fails the batched call with nothing
    written; so does the packed layout."""
    import torch

    w, h, ll = 32, 12, 32
    dev = torch.from_numpy(oracle_mod.synth(1, w, h, ll, LAYOUT_OV7670, 0, 9)).cuda()
    out = torch.full((4096,), SENTINEL, dtype=torch.uint8, device="cuda")
    sizes = torch.full((1,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    b = hsv._batch(dev, w, h, ll, LAYOUT_OV7670)
    hsv._lib.trik_hsv_last_error()
    rc = hsv._lib.trik_hsv_jpeg_batch(det._h, C.byref(b), 50, 0, C.c_void_p(out.data_ptr()), 4096, 4096,
                                      C.c_void_p(sizes.data_ptr()), None, None)
    assert rc != 0 and b"height % 8" in hsv._lib.trik_hsv_last_error()
    with pytest.raises(hsv.TrikHsvError):
        det.jpeg_batch(dev, w, h, ll, 50)
    yuyv = hsv._batch(dev, 32, 8, 64, hsv.LAYOUT_YUYV)
    assert hsv._lib.trik_hsv_jpeg_batch(det._h, C.byref(yuyv), 50, 0, C.c_void_p(out.data_ptr()), 4096, 4096,
                                        C.c_void_p(sizes.data_ptr()), None, None) != 0
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == SENTINEL).all() and sizes.cpu().tolist() == [0x5A5A5A5A]


def sensor(hsv, w, h, ll, streams=1):
    """A JPEG codec instance; the declared output image is 16 x 2 (64 bytes), so
    that the stream's length alone decides whether a buffer is large enough."""
    s = hsv.JpegSensor(hsv._default_params(streams, fmt_in=hsv.FORMAT_YUV422P))
    assert s.set_params(w, h, ll, out_width=16, out_height=2, out_line_length=32) == 0
    return s


def sentinel_out_args(hsv):
    oa = hsv._abi.JpegOutArgs()
    oa.base.size = C.sizeof(hsv._abi.JpegOutArgs)
    oa.alg.size = 0x5A5A5A5A
    return oa


@pytest.mark.parametrize("geom", [(32, 8, 32), (96, 24, 128), (64, 64, 64)])
def test_jpeg_sensor_process(hsv, det, oracle_mod, geom):
    """JpegSensor.process: the bytes and OutArgs.size of the batched call."""
    w, h, ll = geom
    frames = jpeg_cases.frames_of(oracle_mod, geom)
    s = sensor(hsv, w, h, ll)
    try:
        for name, q, bw in (("uniform", 100, False), ("scene", 50, False), ("checker", 255, True),
                            ("flat", 0, True)):
            want = jpeg_cases.ref(oracle_mod, geom, name, q, bw)[0]
            streams, sizes, _ = run_batch(det, [frames[name]], geom, q, bw, capacity=len(want), coeffs=False)
            assert int(sizes[0]) == len(want) and streams[0].tobytes() == want
            out = np.full(len(want) + 40, 0xAB, np.uint8)
            rc, oa, data = s.process(frames[name], q, bw, out_buffer=out, input_id=7, out_args=sentinel_out_args(hsv))
            assert rc == hsv.IVIDTRANSCODE_EOK, hsv._abi.last_error()
            assert oa.alg.size == len(want) and data == want, (geom, name, q, bw)
            assert not out[len(want):].any()  # the glue's zero fill of the whole buffer
            assert oa.base.encodedBuf[0].bufSize == 64 and oa.base.bitsConsumed == frames[name].size * 8
            assert oa.base.outputID[0] == 7 and oa.base.outBufsInUseFlag == 0
    finally:
        s.close()


def test_jpeg_sensor_divergences_and_validation(hsv, oracle_mod):
    geom = (64, 16, 64)
    w, h, ll = geom
    fr = jpeg_cases.frames_of(oracle_mod, geom)["uniform"]
    want = jpeg_cases.ref(oracle_mod, geom, "uniform", 50, False)[0]
    s = sensor(hsv, w, h, ll)
    try:
        # an output buffer one byte short: EFAIL, none of the stream written, size untouched
        out = np.full(len(want) - 1, 0xAB, np.uint8)
        rc, oa, data = s.process(fr, 50, False, out_buffer=out, out_args=sentinel_out_args(hsv))
        assert rc == hsv.IVIDTRANSCODE_EFAIL and data is None
        assert oa.base.extendedError & (1 << hsv._abi.XDM_CORRUPTEDDATA_BIT)
        assert oa.alg.size == 0x5A5A5A5A and not out.any()  # (the shell's zero fill, no stream byte)
        # exactly large enough
        out = np.full(len(want), 0xAB, np.uint8)
        rc, oa, data = s.process(fr, 50, False, out_buffer=out)
        assert rc == 0 and data == want and oa.alg.size == len(want)
        # smaller than the declared output image (the wrapper's second check, JWRAP:57-58)
        rc, oa, _ = s.process(fr, 50, False, out_buffer=np.zeros(63, np.uint8), out_args=sentinel_out_args(hsv))
        assert rc == hsv.IVIDTRANSCODE_EFAIL and oa.alg.size == 0x5A5A5A5A
        # an input shorter than both planes (the first check, on both planes here)
        rc, oa, _ = s.process(fr[: h * ll], 50, False, out_buffer=np.zeros(4096, np.uint8))
        assert rc == hsv.IVIDTRANSCODE_EFAIL and oa.base.extendedError & (1 << hsv._abi.XDM_CORRUPTEDDATA_BIT)
        # wrong size fields: EUNSUPPORTED + XDM_UNSUPPORTEDPARAM, as the other codecs (WFXNS:192-197)
        out = np.full(4096, 0xAB, np.uint8)
        frb, ib, ob, keep = s._bufs(fr, out, None)
        for in_size, out_size in ((C.sizeof(hsv._abi.InArgs), C.sizeof(hsv._abi.JpegOutArgs)),
                                  (C.sizeof(hsv._abi.JpegInArgs), C.sizeof(hsv._abi.OutArgs))):
            ia = hsv._abi.JpegInArgs()
            ia.base.size, ia.base.numBytes = in_size, frb.size
            ia.alg = hsv._abi.JpegInArgsAlg(50, 0)
            oa = sentinel_out_args(hsv)
            oa.base.size = out_size
            rc = hsv._lib.TRIK_VIDTRANSCODE_CV_process(s._h, C.byref(ib), C.byref(ob), C.byref(ia), C.byref(oa))
            assert rc == hsv.IVIDTRANSCODE_EUNSUPPORTED
            assert oa.base.extendedError & (1 << hsv._abi.XDM_UNSUPPORTEDPARAM_BIT)
            assert oa.alg.size == 0x5A5A5A5A and (out == 0xAB).all()
        # a height that is no multiple of 8: setup takes it (height % 4), the run fails, nothing written
        assert s.set_params(32, 12, 32, out_width=16, out_height=2, out_line_length=32) == 0
        out = np.full(4096, 0xAB, np.uint8)
        rc, oa, data = s.process(oracle_mod.synth(1, 32, 12, 32, LAYOUT_OV7670, 0, 9), 50, False, out_buffer=out,
                                 out_args=sentinel_out_args(hsv))
        assert rc == hsv.IVIDTRANSCODE_EFAIL and data is None and oa.alg.size == 0x5A5A5A5A and not out.any()
        assert b"height % 8" in hsv._abi.last_error().encode()
        # a zero-sized image: nothing is encoded, size is left untouched (JWRAP:67)
        assert s.set_params(0, 0, 0, out_width=16, out_height=2, out_line_length=32) == 0
        rc, oa, _ = s.process(np.zeros(4, np.uint8), 50, False, out_buffer=np.zeros(64, np.uint8), num_bytes=0,
                              out_args=sentinel_out_args(hsv))
        assert rc == 0 and oa.alg.size == 0x5A5A5A5A
        # the packed-YUYV input format is not this codec's
        with pytest.raises(hsv.TrikHsvError):
            hsv.JpegSensor(hsv._default_params(1, fmt_in=hsv.FORMAT_YUV422))
        # still working after the failures
        assert s.set_params(w, h, ll, out_width=16, out_height=2, out_line_length=32) == 0
        rc, oa, data = s.process(fr, 50, False, out_buffer=np.zeros(len(want) + 5, np.uint8))
        assert rc == 0 and data == want
    finally:
        s.close()


def test_jpeg_sensor_zero_output_streams(hsv, oracle_mod):
    """numOutputStreams == 0: the size alone, the buffer left alone."""
    geom = (96, 24, 128)
    fr = jpeg_cases.frames_of(oracle_mod, geom)["scene"]
    want = jpeg_cases.ref(oracle_mod, geom, "scene", 75, False)[0]
    s = sensor(hsv, *geom, streams=0)
    try:
        out = np.full(4096, 0xAB, np.uint8)
        rc, oa, _ = s.process(fr, 75, False, out_buffer=out)
        assert rc == 0 and oa.alg.size == len(want)
        assert (out == 0xAB).all()
        rc, oa, data = s.process(fr, 75, False)
        assert rc == 0 and oa.alg.size == len(want) and data is None
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


def test_jpeg_through_the_function_table(hsv, oracle_mod):
    """A framework-style caller: algAlloc, its own record, algInit, control and
    process through TRIK_VIDTRANSCODE_CV_JPEG_FXNS, algFree."""
    geom = (96, 24, 128)
    w, h, ll = geom
    fr = jpeg_cases.frames_of(oracle_mod, geom)["uniform"]
    want = jpeg_cases.ref(oracle_mod, geom, "uniform", 10, False)[0]
    fx = TranscodeFxns.in_dll(hsv._lib, "TRIK_VIDTRANSCODE_CV_JPEG_FXNS")
    recs = (MemRec * 16)()
    assert fx.ialg.algAlloc(None, None, recs) == 1
    raw = C.create_string_buffer(recs[0].size + 256)
    base = (C.addressof(raw) + 255) & ~255
    recs[0].base = base
    C.c_void_p.from_address(base).value = C.addressof(fx)  # IALG_Obj.fxns, as the framework stores it
    assert fx.ialg.algInit(base, recs, None, None) == hsv.IALG_EOK, hsv._abi.last_error()
    try:
        dyn = hsv.dynamic_params(w, h, ll, out_width=16, out_height=2, out_line_length=32)
        st = hsv._abi.Status()
        assert fx.control(base, hsv.XDM_SETPARAMS, C.addressof(dyn), C.addressof(st)) == 0
        out = np.full(len(want) + 9, 0xAB, np.uint8)
        ib = hsv._abi.BufDesc1()
        ib.numBufs = 1
        ib.descs[0].buf = fr.ctypes.data
        ib.descs[0].bufSize = fr.size
        ob = hsv._abi.BufDesc()
        ob_arr, sz_arr = (C.c_void_p * 1)(out.ctypes.data), (C.c_int32 * 1)(out.nbytes)
        ob.bufs, ob.numBufs, ob.bufSizes = ob_arr, 1, sz_arr
        ia = hsv._abi.JpegInArgs()
        ia.base.size, ia.base.numBytes = C.sizeof(hsv._abi.JpegInArgs), fr.size
        ia.alg = hsv._abi.JpegInArgsAlg(10, 0)
        oa = sentinel_out_args(hsv)
        rc = fx.process(base, C.addressof(ib), C.addressof(ob), C.addressof(ia), C.addressof(oa))
        assert rc == hsv.IVIDTRANSCODE_EOK, hsv._abi.last_error()
        assert oa.alg.size == len(want) and out[: len(want)].tobytes() == want and not out[len(want):].any()
    finally:
        assert fx.ialg.algFree(base, recs) == 1


def test_jpeg_stream_order(det, oracle_mod):
    """On a non-default stream with the upload before it and no sync in between."""
    import torch

    geom = (64, 16, 64)
    fr = jpeg_cases.frames_of(oracle_mod, geom)["scene"]
    want = jpeg_cases.ref(oracle_mod, geom, "scene", 50, False)[0]
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        dev = torch.from_numpy(fr).cuda()
        streams, sizes = det.jpeg_batch(dev, 64, 16, 64, 50, False, stream=s)
    s.synchronize()
    assert int(sizes[0]) == len(want) and streams[0, : len(want)].cpu().numpy().tobytes() == want
