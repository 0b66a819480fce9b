"""The ov7670 MxN colour-grid sensor on the GPU against tests/mxn_ref.py (the
reference's sequential strictly-greater loop, MSEQ = trik/ov7670/mxn_sensor/
include/internal/cv_ball_detector_seqpass.hpp): cell colours, winning bins and
preview bytes, bit-exact, through Detector.mxn_batch / mxn_preview
(trik_hsv_mxn_batch / trik_hsv_mxn_preview), MxnSensor.process
(TRIK_VIDTRANSCODE_CV_create_mxn) and the exported XDAIS function table."""
import ctypes as C

import numpy as np
import pytest

import mxn_ref
from gpu_util import LAYOUT_OV7670

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A5A5A


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


@pytest.fixture(scope="module")
def yuv_of_bin(table):
    return yuv_of_bin_map(table)


def yuv_of_bin_map(table):
    """bin -> (Y, U, V) of the first table entry in that bin (reachable bins only)."""
    hsvw = (table & np.uint64(0xFFFFFFFF)).astype(np.int64)
    bins = (((hsvw & 255) >> 3) << 4) | ((((hsvw >> 8) & 255) >> 6) << 2) | (((hsvw >> 16) & 255) >> 6)
    b, idx = np.unique(bins, return_index=True)
    return {int(k): (int(i) & 255, (int(i) >> 8) & 255, int(i) >> 16) for k, i in zip(b, idx)}


_REF = {}


def ref_run(table, key, frame, w, h, ll, m, n):
    """mxn_ref.run, computed once per (frame, grid) and shared."""
    k = (key, w, h, ll, m, n)
    if k not in _REF:
        _REF[k] = mxn_ref.run(table, frame, w, h, ll, m, n)
    return _REF[k]


def single_colour(w, h, ll, y, u, v):
    fr = np.zeros(2 * h * ll, np.uint8)
    fr[:h * ll] = y
    c = fr[h * ll:].reshape(h, ll)
    c[:, 0::2] = v
    c[:, 1::2] = u
    return fr


def make_frames(oracle_mod, w, h, ll):
    """Uniform bytes, a scene frame and a single-colour frame of one geometry."""
    return [("uniform", oracle_mod.synth(1, w, h, ll, LAYOUT_OV7670, 0, 0x51DE)),
            ("scene", oracle_mod.synth(1, w, h, ll, LAYOUT_OV7670, 1, 0x7A1C, first_frame=3)),
            ("single", single_colour(w, h, ll, 150, 90, 200))]


# (w, h, ll, m, n): one cell; 2 x 2; 32 x 6 cells with 2 leftover rows; the
# TRIK default (106-column step, 2 leftover columns); steps of 64 x 48,
# 6 columns, 4 rows; empty cells (row step 0); a padded input line
GEOMS = [
    (64, 8, 64, 1, 1),
    (64, 8, 64, 2, 2),
    (96, 20, 96, 3, 3),
    (320, 240, 320, 3, 3),
    (640, 480, 640, 10, 10),
    (640, 480, 640, 1, 100),
    (640, 480, 640, 100, 1),
    (32, 4, 32, 5, 1),
    (320, 240, 352, 3, 3),
]


@pytest.mark.parametrize("geom", GEOMS)
def test_mxn_batch_vs_reference(hsv, det, oracle_mod, table, geom):
    import torch

    w, h, ll, m, n = geom
    frames = make_frames(oracle_mod, w, h, ll)
    refs = [ref_run(table, name, fr, w, h, ll, m, n) for name, fr in frames]
    if (m, n) == (1, 100):  # the tie rule decides real cells here, not only crafted ones
        assert any(refs[0][2]), "the uniform-byte frame has no tied cell at 1 x 100"
    if h // m == 0:
        assert all(c == 0 for r in refs for c in r[0])  # empty cells: bin (0, 0, 0), colour 0
    dev = torch.from_numpy(np.concatenate([fr for _, fr in frames])).cuda()
    colors, bins = det.mxn_batch(dev, w, h, ll, m, n, bins=True)
    colors, bins = colors.cpu().numpy(), bins.cpu().numpy()
    assert colors.shape == (3, m * n) and bins.shape == (3, m * n)
    for i, (name, _) in enumerate(frames):
        assert bins[i].tolist() == refs[i][1], (geom, name)
        assert colors[i].tolist() == refs[i][0], (geom, name)
    only = det.mxn_batch(dev, w, h, ll, m, n)  # without the optional bins
    assert np.array_equal(only.cpu().numpy(), colors)


def test_mxn_batch_unaligned_frames(hsv, det, oracle_mod, table):
    """Frames at an odd address and an odd stride: the byte-load path."""
    import torch

    w, h, ll, m, n = 96, 20, 96, 3, 3
    fb, stride = 2 * h * ll, 2 * h * ll + 3
    frames = make_frames(oracle_mod, w, h, ll)
    host = np.zeros(1 + 3 * stride, np.uint8)
    for i, (_, fr) in enumerate(frames):
        host[1 + i * stride:1 + i * stride + fb] = fr
    dev = torch.from_numpy(host).cuda()
    colors, bins = det.mxn_batch(dev[1:], w, h, ll, m, n, n_frames=3, frame_stride=stride, bins=True)
    for i, (name, fr) in enumerate(frames):
        want = ref_run(table, name, fr, w, h, ll, m, n)
        assert bins[i].cpu().tolist() == want[1] and colors[i].cpu().tolist() == want[0], name


def test_mxn_every_yuv_triple(hsv, det, table):
    """All 2^24 (Y, U, V) triples through the kernel's per-pixel arithmetic:
    32 x 4 frames at 3 x 32 have 96 one-pixel cells (steps 1 and 1), so a
    cell's winner is its pixel's bin (the sequential loop over one pixel).
    Pair p has U = p & 255, V = (p >> 8) & 255, Y = 2k, 2k + 1 (k = p >> 16);
    a frame holds 48 pairs in rows 0..2 (row 3 belongs to no cell)."""
    import torch

    # 174,763 frames x 96 cells is just over the blocks one launch holds (2^32 / 256 threads): launch_mxn
    # splits this batch in two, the suite's only run of its frame loop.  Keep that when resizing.
    nf = -(-(1 << 23) // 48)
    assert nf * 96 > 0xFFFFFFFF // 256
    p = np.arange(nf * 48, dtype=np.int64) % (1 << 23)
    u, v, k = p & 255, (p >> 8) & 255, p >> 16
    y = np.stack([2 * k, 2 * k + 1], -1).reshape(nf, 3, 32)
    uu, vv = np.repeat(u, 2).reshape(nf, 3, 32), np.repeat(v, 2).reshape(nf, 3, 32)
    host = np.zeros((nf, 2, 4, 32), np.uint8)
    host[:, 0, :3] = y
    host[:, 1, :3, 0::2] = vv[:, :, 0::2]
    host[:, 1, :3, 1::2] = uu[:, :, 1::2]
    hsvw = (table[y | (uu << 8) | (vv << 16)] & np.uint64(0xFFFFFFFF)).astype(np.int64)
    want = (((hsvw & 255) >> 3) << 4) | ((((hsvw >> 8) & 255) >> 6) << 2) | (((hsvw >> 16) & 255) >> 6)
    want = want.reshape(nf, 96)
    color_of = np.array([mxn_ref.bin_color(b) for b in range(mxn_ref.N_BINS)], np.int64)
    colors, bins = det.mxn_batch(torch.from_numpy(host.reshape(-1)).cuda(), 32, 4, 32, 3, 32, bins=True)
    bins = bins.cpu().numpy().astype(np.int64)
    bad = np.argwhere(bins != want)
    assert bad.size == 0, (len(bad), bad[:4].tolist())
    assert np.array_equal(colors.cpu().numpy().astype(np.int64), color_of[want])


def crafted(yuv_of_bin, w, h, ll, m, n, cell_seqs):
    """A frame whose cell k holds, pair by pair in the cell's raster order, the
    bins of cell_seqs[k] (same-Y pixel pairs, so every count is even)."""
    fr = np.zeros(2 * h * ll, np.uint8)
    ypl = fr[:h * ll].reshape(h, ll)
    cpl = fr[h * ll:].reshape(h, ll)
    for k, r0, c0, rs, cs in mxn_ref.cells(w, h, m, n):
        assert cs % 2 == 0 and c0 % 2 == 0 and len(cell_seqs[k]) == rs * cs // 2
        for p, b in enumerate(cell_seqs[k]):
            y, u, v = yuv_of_bin[b]
            r, c = r0 + (2 * p) // cs, c0 + (2 * p) % cs
            ypl[r, c:c + 2] = y
            cpl[r, c] = v
            cpl[r, c + 1] = u
    return fr


def crafted_tie_frames(yuv_of_bin):
    """[(frame, (m, n), winning bins)] at 64 x 8: cells holding two or three
    bins with equal final counts (shared with tests/test_reference_cpu.py)."""
    reach = sorted(yuv_of_bin)
    lo, mid, hi, fill = reach[1], reach[len(reach) // 2], reach[-2], reach[-1]
    assert lo < mid < hi
    # 64 x 8 at 2 x 2: cells of 32 x 4 = 64 pairs
    a = [lo] * 10 + [hi] * 32 + [lo] * 22                 # (a) the higher index finishes first
    b = [hi] * 10 + [lo] * 32 + [hi] * 22                 # (b) the lower index finishes first
    c = [lo] * 5 + [hi] * 20 + [mid] * 10 + [lo] * 15 + [mid] * 10 + [fill] * 4  # (c) second to appear
    d = [mid] * 7 + [lo] * 20 + [hi] * 10 + [mid] * 13 + [hi] * 10 + [fill] * 4  # (c) with the lowest index
    fr4 = crafted(yuv_of_bin, 64, 8, 64, 2, 2, [a, b, c, d])
    want4 = [hi, lo, hi, lo]
    # 64 x 8 at 1 x 1: one cell of 256 pairs, three bins at 80 pairs
    one = [hi] * 40 + [mid] * 80 + [lo] * 50 + [hi] * 40 + [lo] * 30 + [fill] * 16
    fr1 = crafted(yuv_of_bin, 64, 8, 64, 1, 1, [one])
    return [(fr4, (2, 2), want4), (fr1, (1, 1), [mid])]


def test_mxn_crafted_ties(hsv, det, table, yuv_of_bin):
    """Cells holding two or three bins with equal final counts: the winner is
    the bin that reaches the count first, whatever its index."""
    import torch

    for fr, (m, n), want in crafted_tie_frames(yuv_of_bin):
        ref_colors, ref_bins, ties = mxn_ref.run(table, fr, 64, 8, 64, m, n)
        assert all(ties), "a crafted cell lost its tie"
        assert ref_bins == want
        colors, bins = det.mxn_batch(torch.from_numpy(fr).cuda(), 64, 8, 64, m, n, bins=True)
        assert bins[0].cpu().tolist() == want
        assert colors[0].cpu().tolist() == ref_colors


def test_mxn_batch_many_frames(hsv, det, oracle_mod, table):
    """More frames than two per CU, every one different, at a padded stride."""
    import torch

    w, h, ll, m, n = 96, 20, 96, 3, 3
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    nf = 2 * cus + 3
    fb, stride = 2 * h * ll, 2 * h * ll + 64
    half = nf // 2
    host = np.concatenate([oracle_mod.synth(half, w, h, ll, LAYOUT_OV7670, 1, 0xBEEF, frame_stride=stride),
                           oracle_mod.synth(nf - half, w, h, ll, LAYOUT_OV7670, 0, 0xF00D, first_frame=half,
                                            frame_stride=stride)])
    dev = torch.from_numpy(host).cuda()
    colors, bins = det.mxn_batch(dev, w, h, ll, m, n, n_frames=nf, frame_stride=stride, bins=True)
    colors, bins = colors.cpu().numpy(), bins.cpu().numpy()
    for i in range(nf):
        want = mxn_ref.run(table, host[i * stride:i * stride + fb], w, h, ll, m, n)
        assert bins[i].tolist() == want[1] and colors[i].tolist() == want[0], i


# (w, h, ll, m, n, ow, oh, oll): the 2:1 default; the portrait output with
# non-uniform maps; a padded odd output line; squares that overlap (steps 2
# and 9 under 20) and clamp at the right and bottom edges
PREVIEWS = [
    (640, 480, 640, 3, 3, 320, 240, 640),
    (640, 480, 640, 10, 10, 320, 240, 640),
    (320, 240, 320, 3, 3, 240, 320, 480),
    (320, 240, 352, 3, 3, 160, 120, 331),
    (96, 20, 96, 10, 10, 48, 10, 100),
    (96, 20, 96, 10, 10, 96, 20, 192),
]


@pytest.mark.parametrize("geom", PREVIEWS)
def test_mxn_preview_vs_reference(hsv, det, oracle_mod, table, geom):
    import torch

    w, h, ll, m, n, ow, oh, oll = geom
    frames = make_frames(oracle_mod, w, h, ll)[:2]
    dev = torch.from_numpy(np.concatenate([fr for _, fr in frames])).cuda()
    colors = det.mxn_batch(dev, w, h, ll, m, n)
    pv = det.mxn_preview(dev, w, h, ll, m, n, colors, out_width=ow, out_height=oh, out_line_length=oll)
    pv = pv.cpu().numpy()
    for i, (name, fr) in enumerate(frames):
        ref_colors = ref_run(table, name, fr, w, h, ll, m, n)[0]
        assert colors[i].cpu().tolist() == ref_colors
        want = mxn_ref.preview(table, fr, w, h, ll, m, n, ref_colors, ow, oh, oll)
        assert np.array_equal(pv[i], want), (geom, name)
        assert not pv[i][:, 2 * ow:].any()  # the line padding stays 0


def test_mxn_stream_order(hsv, det, oracle_mod, table):
    """mxn_batch then mxn_preview on a non-default stream, no sync in between."""
    import torch

    w, h, ll, m, n = 320, 240, 320, 3, 3
    name, fr = make_frames(oracle_mod, w, h, ll)[1]
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        dev = torch.from_numpy(fr).cuda()
        colors = det.mxn_batch(dev, w, h, ll, m, n, stream=s)
        pv = det.mxn_preview(dev, w, h, ll, m, n, colors, stream=s)
    s.synchronize()
    ref_colors = ref_run(table, name, fr, w, h, ll, m, n)[0]
    assert colors[0].cpu().tolist() == ref_colors
    assert np.array_equal(pv[0].cpu().numpy(), mxn_ref.preview(table, fr, w, h, ll, m, n, ref_colors, 160, 120, 320))


def test_mxn_batch_validation(hsv, det, oracle_mod):
    """An invalid grid fails the batched calls and writes nothing."""
    import torch

    w, h, ll = 64, 8, 64
    dev = torch.from_numpy(oracle_mod.synth(1, w, h, ll, LAYOUT_OV7670, 1, 1)).cuda()
    b = hsv._batch(dev, w, h, ll, LAYOUT_OV7670)
    colors = torch.full((128,), SENTINEL, dtype=torch.int32, device="cuda")
    pv = torch.full((4 * 64,), 0x5A, dtype=torch.uint8, device="cuda")
    for m, n in ((0, 1), (1, 0), (11, 10), (-1, -1), (101, 1)):
        hsv._lib.trik_hsv_last_error()
        rc = hsv._lib.trik_hsv_mxn_batch(det._h, C.byref(b), m, n, C.c_void_p(colors.data_ptr()), None, None)
        assert rc != 0 and b"widthM" in hsv._lib.trik_hsv_last_error(), (m, n)
        rc = hsv._lib.trik_hsv_mxn_preview(det._h, C.byref(b), m, n, C.c_void_p(colors.data_ptr()), 32, 4, 64,
                                           C.c_void_p(pv.data_ptr()), 256, None)
        assert rc != 0, (m, n)
        with pytest.raises(hsv.TrikHsvError):
            det.mxn_batch(dev, w, h, ll, m, n)
    torch.cuda.synchronize()
    assert (colors.cpu().numpy() == SENTINEL).all() and (pv.cpu().numpy() == 0x5A).all()
    yuyv = hsv._batch(dev, 32, 8, 64, hsv.LAYOUT_YUYV)  # the packed layout is not this sensor's
    assert hsv._lib.trik_hsv_mxn_batch(det._h, C.byref(yuyv), 1, 1, C.c_void_p(colors.data_ptr()), None, None) != 0
    # 10 x 10 is the largest grid
    assert det.mxn_batch(dev, w, h, ll, 10, 10).shape == (1, 100)


def sensor(hsv, w, h, ll, ow, oh, oll, streams=1):
    s = hsv.MxnSensor(hsv._default_params(streams, fmt_in=hsv.FORMAT_YUV422P))
    assert s.set_params(w, h, ll, out_width=ow, out_height=oh, out_line_length=oll) == 0
    return s


def sentinel_out_args(hsv):
    oa = hsv._abi.MxnOutArgs()
    oa.base.size = C.sizeof(hsv._abi.MxnOutArgs)
    for i in range(100):
        oa.alg.outColor[i] = SENTINEL
    return oa


@pytest.mark.parametrize("geom", [(64, 8, 64, 2, 2, 32, 4, 64), (96, 20, 96, 3, 3, 48, 10, 100),
                                  (320, 240, 320, 3, 3, 320, 240, 640), (32, 4, 32, 5, 1, 16, 2, 32),
                                  (640, 480, 640, 10, 10, 320, 240, 640)])
def test_mxn_sensor_process(hsv, oracle_mod, table, geom):
    w, h, ll, m, n, ow, oh, oll = geom
    s = sensor(hsv, w, h, ll, ow, oh, oll)
    try:
        for name, fr in make_frames(oracle_mod, w, h, ll)[:2]:
            out = np.full(oh * oll + 32, 0xAB, np.uint8)
            oa = sentinel_out_args(hsv)
            rc, oa, colors = s.process(fr, m, n, out_buffer=out, out_args=oa, input_id=7)
            assert rc == hsv.IVIDTRANSCODE_EOK, hsv._abi.last_error()
            ref_colors = ref_run(table, name, fr, w, h, ll, m, n)[0]
            assert colors == ref_colors, (geom, name)
            assert all(oa.alg.outColor[i] == SENTINEL for i in range(m * n, 100))  # past M * N: untouched
            assert oa.base.encodedBuf[0].bufSize == oh * oll and oa.base.bitsConsumed == fr.size * 8
            assert oa.base.outputID[0] == 7 and oa.base.outBufsInUseFlag == 0
            want = mxn_ref.preview(table, fr, w, h, ll, m, n, ref_colors, ow, oh, oll)
            assert np.array_equal(out[:oh * oll].reshape(oh, oll), want), (geom, name)
            assert not out[oh * oll:].any()  # the glue's zero fill of the whole buffer
    finally:
        s.close()


def test_mxn_sensor_validation(hsv, oracle_mod, table):
    w, h, ll = 64, 8, 64
    fr = oracle_mod.synth(1, w, h, ll, LAYOUT_OV7670, 1, 2)
    s = sensor(hsv, w, h, ll, 32, 4, 64)
    try:
        for m, n in ((0, 2), (2, 0), (11, 10)):
            oa = sentinel_out_args(hsv)
            rc, oa, colors = s.process(fr, m, n, out_buffer=np.zeros(4 * 64, np.uint8), out_args=oa)
            assert rc == hsv.IVIDTRANSCODE_EFAIL and colors is None, (m, n)
            assert oa.base.extendedError & (1 << hsv._abi.XDM_CORRUPTEDDATA_BIT)
            assert all(oa.alg.outColor[i] == SENTINEL for i in range(100)), (m, n)
        # wrong size fields: EUNSUPPORTED + XDM_UNSUPPORTEDPARAM, as the other codecs (WFXNS:192-197)
        frb, ib, ob, keep = s._bufs(fr, np.zeros(4 * 64, np.uint8), None)
        for in_size, out_size in ((C.sizeof(hsv._abi.InArgs), C.sizeof(hsv._abi.MxnOutArgs)),
                                  (C.sizeof(hsv._abi.MxnInArgs), C.sizeof(hsv._abi.OutArgs))):
            ia = hsv._abi.MxnInArgs()
            ia.base.size, ia.base.numBytes = in_size, frb.size
            ia.alg = hsv._abi.MxnInArgsAlg(2, 2)
            oa = sentinel_out_args(hsv)
            oa.base.size = out_size
            rc = hsv._lib.TRIK_VIDTRANSCODE_CV_process(s._h, C.byref(ib), C.byref(ob), C.byref(ia), C.byref(oa))
            assert rc == hsv.IVIDTRANSCODE_EUNSUPPORTED
            assert oa.base.extendedError & (1 << hsv._abi.XDM_UNSUPPORTEDPARAM_BIT)
            assert all(oa.alg.outColor[i] == SENTINEL for i in range(100))
        # an input shorter than both planes: EFAIL + XDM_CORRUPTEDDATA
        rc, oa, _ = s.process(fr[:h * ll], 2, 2, out_buffer=np.zeros(4 * 64, np.uint8))
        assert rc == hsv.IVIDTRANSCODE_EFAIL and oa.base.extendedError & (1 << hsv._abi.XDM_CORRUPTEDDATA_BIT)
        # the packed-YUYV input format is not this codec's
        with pytest.raises(hsv.TrikHsvError):
            hsv.MxnSensor(hsv._default_params(1, fmt_in=hsv.FORMAT_YUV422))
        # still working after the failures
        rc, _, colors = s.process(fr, 2, 2, out_buffer=np.zeros(4 * 64, np.uint8))
        assert rc == 0 and colors == mxn_ref.run(table, fr, w, h, ll, 2, 2)[0]
    finally:
        s.close()


def test_mxn_sensor_zero_output_streams(hsv, oracle_mod, table):
    w, h, ll = 96, 20, 96
    fr = oracle_mod.synth(1, w, h, ll, LAYOUT_OV7670, 1, 4)
    s = sensor(hsv, w, h, ll, 48, 10, 96, streams=0)
    try:
        out = np.full(10 * 96, 0xAB, np.uint8)
        rc, _, colors = s.process(fr, 3, 3, out_buffer=out)
        assert rc == 0 and colors == mxn_ref.run(table, fr, w, h, ll, 3, 3)[0]
        assert (out == 0xAB).all()  # no output stream: the buffer is left alone
        rc, _, colors2 = s.process(fr, 3, 3)
        assert rc == 0 and colors2 == colors
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


def test_mxn_through_the_function_table(hsv, oracle_mod, table):
    """A framework-style caller: algAlloc, its own record, algInit, control and
    process through TRIK_VIDTRANSCODE_CV_MXN_FXNS, algFree."""
    w, h, ll, m, n, ow, oh, oll = 96, 20, 96, 3, 3, 48, 10, 100
    fr = oracle_mod.synth(1, w, h, ll, LAYOUT_OV7670, 1, 6)
    fx = TranscodeFxns.in_dll(hsv._lib, "TRIK_VIDTRANSCODE_CV_MXN_FXNS")
    recs = (MemRec * 16)()
    assert fx.ialg.algAlloc(None, None, recs) == 1
    raw = C.create_string_buffer(recs[0].size + 256)
    base = (C.addressof(raw) + 255) & ~255
    recs[0].base = base
    C.c_void_p.from_address(base).value = C.addressof(fx)  # IALG_Obj.fxns, as the framework stores it
    assert fx.ialg.algInit(base, recs, None, None) == hsv.IALG_EOK, hsv._abi.last_error()
    try:
        dyn = hsv.dynamic_params(w, h, ll, out_width=ow, out_height=oh, out_line_length=oll)
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
        ia = hsv._abi.MxnInArgs()
        ia.base.size, ia.base.numBytes = C.sizeof(hsv._abi.MxnInArgs), fr.size
        ia.alg = hsv._abi.MxnInArgsAlg(m, n)
        oa = sentinel_out_args(hsv)
        rc = fx.process(base, C.addressof(ib), C.addressof(ob), C.addressof(ia), C.addressof(oa))
        assert rc == hsv.IVIDTRANSCODE_EOK, hsv._abi.last_error()
        ref_colors = mxn_ref.run(table, fr, w, h, ll, m, n)[0]
        assert list(oa.alg.outColor[:m * n]) == ref_colors
        assert all(oa.alg.outColor[i] == SENTINEL for i in range(m * n, 100))
        assert np.array_equal(out.reshape(oh, oll), mxn_ref.preview(table, fr, w, h, ll, m, n, ref_colors, ow, oh, oll))
    finally:
        assert fx.ialg.algFree(base, recs) == 1
