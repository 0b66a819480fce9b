"""The exact autoDetectHsv on the GPU (trik_hsv_autorange.hip) against the
restatement (tests/autorange_ref.py) on the cases of tests/autorange_cases.py:
the score histogram and the start cell, the exact search and its six outputs,
and process() of the three codecs in both modes."""
import ctypes as C

import numpy as np
import pytest

import autorange_cases as AC
import autorange_ref as R

pytestmark = pytest.mark.gpu

KINDS = [R.OBJECT, R.LINE, R.WLINE]
CASES = [(k, i) for k in KINDS for i in range(len(AC.cases(k)))]
SENTINEL = 0xBEEF


@pytest.fixture(scope="module")
def hsv():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import trik_hsv

    return trik_hsv


def _upload(case):
    import torch

    return torch.from_numpy(case.data).cuda()[case.offset:]


def _u16(t):
    return (t.cpu().numpy().astype(np.int64) & 0xFFFF).tolist()


def _kw(case):
    return dict(n_frames=case.n, frame_stride=case.stride)


def _id(p):
    return f"{'object line wline'.split()[p[0]]}-{AC.cases(p[0])[p[1]].name}"


@pytest.mark.parametrize("p", CASES, ids=_id)
def test_auto_scores(hsv, p):
    case = AC.cases(p[0])[p[1]]
    want = case.want()
    dev = _upload(case)
    assert case.offset == 0 or dev.data_ptr() % 16 != 0
    scores, start = hsv.auto_scores(dev, case.width, case.height, case.line_length, case.kind, **_kw(case))
    scores, start = scores.cpu().numpy(), start.cpu().numpy().tolist()
    for i, w in enumerate(want):
        bad = np.flatnonzero(scores[i] != w["hist"])
        assert len(bad) == 0, (case.name, i, bad[:4], scores[i][bad[:4]], w["hist"][bad[:4]])
        assert start[i] == w["start"], (case.name, i)


@pytest.mark.parametrize("p", CASES, ids=_id)
def test_batch_auto_range_exact(hsv, p):
    case = AC.cases(p[0])[p[1]]
    want = case.want()
    out, best = hsv.batch_auto_range_exact(_upload(case), case.width, case.height, case.line_length, case.kind,
                                           **_kw(case))
    out, best = _u16(out), best.cpu().numpy().tolist()
    for i, w in enumerate(want):
        assert best[i] == w["best"], (case.name, i)
        assert out[i] == w["out"], (case.name, i)


@pytest.mark.parametrize("kind", KINDS)
def test_scene_batch(hsv, kind):
    """8 scene frames at 320 x 240 per kind; best_dev may be NULL."""
    import torch

    case = AC.scene_batch(kind)
    want = case.want()
    dev = _upload(case)
    scores, start = hsv.auto_scores(dev, case.width, case.height, case.line_length, kind)
    out, best = hsv.batch_auto_range_exact(dev, case.width, case.height, case.line_length, kind)
    assert np.array_equal(scores.cpu().numpy(), np.stack([w["hist"] for w in want]))
    assert start.cpu().numpy().tolist() == [w["start"] for w in want]
    assert best.cpu().numpy().tolist() == [w["best"] for w in want]
    assert _u16(out) == [w["out"] for w in want]
    assert any(w["start"][2] > 0 for w in want)
    b = hsv._batch(dev, case.width, case.height, case.line_length, R.layout_of(kind))
    out2 = torch.zeros((case.n, 6), dtype=torch.int16, device=dev.device)
    rc = hsv._lib.trik_hsv_batch_auto_range_exact(C.byref(b), kind, C.c_void_p(out2.data_ptr()), None,
                                                  C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0 and _u16(out2) == [w["out"] for w in want]


def test_refused_calls_write_nothing(hsv):
    import torch

    case = AC.cases(R.OBJECT)[1]
    dev = _upload(case)
    with pytest.raises(hsv.TrikHsvError):
        hsv.auto_scores(dev, case.width, case.height, case.line_length, 5, **_kw(case))
    b = hsv._batch(dev, case.width, case.height, case.line_length, hsv.LAYOUT_OV7670, case.n, case.stride)
    out = torch.full((case.n, 6), 0x1234, dtype=torch.int16, device=dev.device)
    for kind in (R.WLINE, 7):  # a layout that is not the kind's; an unknown kind
        assert hsv._lib.trik_hsv_batch_auto_range_exact(C.byref(b), kind, C.c_void_p(out.data_ptr()), None, None) != 0
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 0x1234).all()


# ---------------------------------------------------------------------------
# process()
# ---------------------------------------------------------------------------
def _sensor(hsv, kind, w, h, ll, ow, oh, oll):
    cls = {R.OBJECT: hsv.BlobSensor, R.LINE: hsv.LineSensor, R.WLINE: hsv.WebcamLineSensor}[kind]
    fmt = hsv.FORMAT_YUV422 if kind == R.WLINE else hsv.FORMAT_YUV422P
    s = cls(hsv._default_params(1, fmt, max(640, w), max(480, h)))
    assert s.set_params(w, h, ll, out_width=ow, out_height=oh, out_line_length=oll) == 0
    return s


def _process(hsv, s, kind, frame, out, auto_detect):
    """process() on OutArgs whose detect* hold a sentinel: (rc, targets, detect*)."""
    fr, ib, ob, keep = s._bufs(frame, out, None)
    if kind == R.OBJECT:
        ia, oa = hsv._abi.OV7670InArgs(), hsv._abi.OV7670OutArgs()
        ia.alg = hsv._abi.OV7670InArgsAlg(1, 0, 20, 80, 20, 60, 40, int(auto_detect))
    else:
        ia, oa = hsv._abi.InArgs(), hsv._abi.OutArgs()
        ia.alg = hsv._abi.InArgsAlg(0, 359, 0, 100, 0, 40, int(auto_detect))
    ia.base.size, oa.base.size = C.sizeof(ia), C.sizeof(oa)
    ia.base.numBytes = fr.size
    for f in ("detectHue", "detectHueTolerance", "detectSat", "detectSatTolerance", "detectVal",
              "detectValTolerance"):
        setattr(oa.alg, f, SENTINEL)
    rc = hsv._lib.TRIK_VIDTRANSCODE_CV_process(s._h, C.byref(ib), C.byref(ob), C.byref(ia), C.byref(oa))
    a = oa.alg
    if kind == R.OBJECT:
        targets = [(t.x, t.y, t.size) for t in a.target]
    else:
        targets = [(a.targetX, a.targetY, a.targetSize)]
    return rc, targets, [a.detectHue, a.detectHueTolerance, a.detectSat, a.detectSatTolerance, a.detectVal,
                         a.detectValTolerance]


@pytest.mark.parametrize("kind", KINDS)
def test_process_modes(hsv, kind):
    """Mode 0: detect* untouched.  Mode 1 with autoDetectHsv: detect* are the
    batched call's, targets and preview the same as in mode 0.  Mode 1 without
    autoDetectHsv: detect* untouched."""
    case = AC.scene_batch(kind)
    w, h, ll = case.width, case.height, case.line_length
    ow, oh, oll = 160, 120, 320
    out_b, _ = hsv.batch_auto_range_exact(_upload(case), w, h, ll, kind)
    out_b = _u16(out_b)
    assert out_b == [x["out"] for x in case.want()]
    s0, s1 = (_sensor(hsv, kind, w, h, ll, ow, oh, oll) for _ in range(2))
    try:
        assert s1.set_auto_detect(1) == 0 and s1.set_auto_detect(1) == 1
        for i in range(3):
            p0, p1, p2 = (np.full(oh * oll, 0xCD, np.uint8) for _ in range(3))
            rc0, t0, d0 = _process(hsv, s0, kind, case.frame(i), p0, True)
            rc1, t1, d1 = _process(hsv, s1, kind, case.frame(i), p1, True)
            assert rc0 == 0 and rc1 == 0
            assert d0 == [SENTINEL] * 6, "mode 0 must leave detect* alone"
            assert d1 == out_b[i], (kind, i)
            assert t1 == t0 and np.array_equal(p1, p0)
            # autoDetectHsv = 0 in mode 1 (a third handle would change nothing: the
            # line sensor's band state is the same after every run)
            rc2, t2, d2 = _process(hsv, s1, kind, case.frame(i), p2, False)
            assert rc2 == 0 and d2 == [SENTINEL] * 6 and t2 == t0 and np.array_equal(p2, p0)
        assert s1.set_auto_detect(0) == 1
        rc, _, d = _process(hsv, s1, kind, case.frame(0), np.zeros(oh * oll, np.uint8), True)
        assert rc == 0 and d == [SENTINEL] * 6
        with pytest.raises(ValueError):
            s1.set_auto_detect(2)
    finally:
        s0.close()
        s1.close()


def test_set_auto_detect_other_codecs(hsv):
    for cls in (hsv.ObjectSensor, hsv.MxnSensor, hsv.JpegSensor, hsv.EdgeLineSensor):
        s = cls()
        try:
            assert hsv._lib.trik_hsv_set_auto_detect(s._h, 1) == -1
            assert "only the ov7670 object sensor" in hsv._abi.last_error()
        finally:
            s.close()
