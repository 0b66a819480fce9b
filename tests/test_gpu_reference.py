"""The GPU against vectors recorded from the REFERENCE's own code
(tests/golden/reference_golden.json, written by
tests/golden/make_reference_golden.py from the reference's algorithm classes
built on the host).  Every golden case goes through the batched entry point of
its codec and through the codec's process(); OutArgs integers and the sha256 of
the preview or JPEG stream must equal the recorded values.  No reference and no
host build of it is needed here: the inputs are regenerated (their sha256 is
recorded too) and are a few frames of at most 320 x 240.

The webcam line sensor has no batched entry point, so it goes through
process() only; a line-sensor case with an explicit cross band goes through
the batched call only (process() carries the band from its own previous run).
"""
import hashlib
import json

import numpy as np
import pytest

from golden import make_reference_golden as mk
from golden.make_golden import RANGES
from gpu_util import LAYOUT_YUYV

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


@pytest.fixture(scope="module")
def ref_golden():
    with open(mk.OUT_PATH) as f:
        return json.load(f)


def cases(ref_golden, codec):
    """(case, recorded row, frame) of one codec; the input hash is checked here."""
    rows = ref_golden[codec]
    assert [r["name"] for r in rows] == [c[0] for c in mk.CODECS[codec]]
    for case, row in zip(mk.CODECS[codec], rows):
        fr = np.ascontiguousarray(mk.frame(codec, case))
        assert hashlib.sha256(fr.tobytes()).hexdigest() == row["frame_sha256"], case[0]
        yield case, row, fr


def same_stream(data, row, what):
    data = bytes(data)
    assert len(data) == row["stream_len"], (what, len(data), row["stream_len"])
    assert hashlib.sha256(data).hexdigest() == row["stream_sha256"], what


def sensor(hsv, cls, fmt, w, h, ll, ow, oh, oll):
    s = cls(hsv._default_params(1, fmt, max(640, w, ow), max(480, h, oh)))
    assert s.set_params(w, h, ll, out_width=ow, out_height=oh, out_line_length=oll) == 0
    return s


def test_object_sensor_vs_reference(hsv, det, ref_golden, oracle_mod):
    import torch

    n = 0
    for case, row, fr in cases(ref_golden, "object"):
        name, w, h, ll, _, _, _, rname, auto, ow, oh, oll = case
        rng, want = RANGES[rname], row["out"]
        dev = torch.from_numpy(fr).cuda()
        # the batched entry points: sums + targets, autoDetectHsv, preview
        sums, targets = det.process_batch(dev, w, h, ll, LAYOUT_YUYV, [rng])
        assert [int(v) & 0xFF for v in targets[0, 0, :3].cpu().tolist()] == [v & 0xFF for v in want["target"]], name
        if auto:
            got = hsv.batch_auto_range(dev, w, h, ll, LAYOUT_YUYV).cpu().numpy().astype(np.int64) & 0xFFFF
            assert got[0].tolist() == want["detect"], name
        pv = det.batch_preview(dev, w, h, ll, LAYOUT_YUYV, rng, sums, out_width=ow, out_height=oh,
                               out_line_length=oll)
        same_stream(pv[0].cpu().numpy().tobytes(), row, (name, "batch"))
        # the codec's process()
        s = sensor(hsv, hsv.ObjectSensor, hsv.FORMAT_YUV422, w, h, ll, ow, oh, oll)
        try:
            out = np.full(oh * oll + 16, 0xCD, np.uint8)
            rc, oa = s.process(fr, rng, out_buffer=out, auto_detect=bool(auto))
            assert rc == 0, hsv._abi.last_error()
            assert [oa.alg.targetX, oa.alg.targetY, oa.alg.targetSize] == want["target"], name
            if auto:
                assert [oa.alg.detectHue, oa.alg.detectHueTolerance, oa.alg.detectSat, oa.alg.detectSatTolerance,
                        oa.alg.detectVal, oa.alg.detectValTolerance] == want["detect"], name
            same_stream(out[:oh * oll].tobytes(), row, (name, "process"))
        finally:
            s.close()
        n += 1
    assert n == 8


def test_line_sensor_vs_reference(hsv, det, ref_golden, oracle_mod):
    import torch

    n = 0
    for case, row, fr in cases(ref_golden, "line"):
        name, w, h, ll, _, _, _, _, vf, vt, band, ow, oh, oll = case
        want = row["out"]
        dev = torch.from_numpy(fr).cuda()
        sums, targets = hsv.line_batch(dev, w, h, ll, vf, vt, band=band)
        assert sums[0].cpu().tolist() == want["sums"], name
        assert [int(v) & 0xFF for v in targets[0, :3].cpu().tolist()] == [v & 0xFF for v in want["target"]], name
        pv = det.line_preview(dev, w, h, ll, vf, vt, sums, out_width=ow, out_height=oh, out_line_length=oll)
        same_stream(pv[0].cpu().numpy().tobytes(), row, (name, "batch"))
        n += 1
        if band is not None:
            continue
        s = sensor(hsv, hsv.LineSensor, hsv.FORMAT_YUV422P, w, h, ll, ow, oh, oll)
        try:
            out = np.full(oh * oll + 16, 0xCD, np.uint8)
            rc, oa = s.process(fr, (0, 359, 0, 100, vf, vt), out_buffer=out)
            assert rc == 0, hsv._abi.last_error()
            assert [oa.alg.targetX, oa.alg.targetY, oa.alg.targetSize] == want["target"], name
            same_stream(out[:oh * oll].tobytes(), row, (name, "process"))
        finally:
            s.close()
        n += 1
    assert n == 8 + 7


def test_webcam_line_sensor_vs_reference(hsv, ref_golden, oracle_mod):
    n = 0
    for case, row, fr in cases(ref_golden, "wline"):
        name, w, h, ll, _, _, _, _, vf, vt, ow, oh, oll = case
        s = sensor(hsv, hsv.WebcamLineSensor, hsv.FORMAT_YUV422, w, h, ll, ow, oh, oll)
        try:
            out = np.full(oh * oll + 16, 0xCD, np.uint8)
            rc, oa = s.process(fr, (0, 359, 0, 100, vf, vt), out_buffer=out)
            assert rc == 0, hsv._abi.last_error()
            assert [oa.alg.targetX, oa.alg.targetY, oa.alg.targetSize] == row["out"]["target"], name
            same_stream(out[:oh * oll].tobytes(), row, (name, "process"))
        finally:
            s.close()
        n += 1
    assert n == 8


def test_blob_sensor_vs_reference(hsv, det, ref_golden, oracle_mod):
    import torch

    n = 0
    for case, row, fr in cases(ref_golden, "blob"):
        name, _, w, h, ll, _, _, rng_hsv, ow, oh, oll = case
        want = row["out"]
        dev = torch.from_numpy(fr).cuda()
        res = det.blob_batch(dev, w, h, ll, rng_hsv, meta=True)
        batch_targets = res["targets"][0, :, :3].cpu().numpy().astype(np.int8)
        # the fixture holds what the reference specifies: equal sizes in a canonical order (mk.blob_out)
        assert mk.blob_out(res["top"][0].cpu().numpy(), batch_targets, int(res["n_labels"][0])) == want, name
        pv = det.blob_preview(dev, w, h, ll, res["meta"], res["top"], out_width=ow, out_height=oh,
                              out_line_length=oll)
        same_stream(pv[0].cpu().numpy().tobytes(), row, (name, "batch"))
        s = sensor(hsv, hsv.BlobSensor, hsv.FORMAT_YUV422P, w, h, ll, ow, oh, oll)
        try:
            out = np.full(oh * oll + 16, 0xCD, np.uint8)
            rc, oa = s.process(fr, rng_hsv, out_buffer=out)
            assert rc == 0, hsv._abi.last_error()
            got = [v for i in range(8) for v in (oa.alg.target[i].x, oa.alg.target[i].y,
                                                 int(np.int8(np.uint8(oa.alg.target[i].size))))]
            assert got == batch_targets.reshape(-1).tolist(), name  # the batched call's, held to the fixture above
            same_stream(out[:oh * oll].tobytes(), row, (name, "process"))
        finally:
            s.close()
        n += 1
    assert n == 8


def test_mxn_sensor_vs_reference(hsv, det, ref_golden, oracle_mod):
    import torch

    n = 0
    for case, row, fr in cases(ref_golden, "mxn"):
        name, w, h, ll, _, m, k, ow, oh, oll = case
        want = row["out"]["colors"]
        dev = torch.from_numpy(fr).cuda()
        colors = det.mxn_batch(dev, w, h, ll, m, k)
        assert colors[0].cpu().tolist() == want, name
        pv = det.mxn_preview(dev, w, h, ll, m, k, colors, out_width=ow, out_height=oh, out_line_length=oll)
        same_stream(pv[0].cpu().numpy().tobytes(), row, (name, "batch"))
        s = sensor(hsv, hsv.MxnSensor, hsv.FORMAT_YUV422P, w, h, ll, ow, oh, oll)
        try:
            out = np.full(oh * oll + 16, 0xCD, np.uint8)
            rc, _, got = s.process(fr, m, k, out_buffer=out)
            assert rc == hsv.IVIDTRANSCODE_EOK, hsv._abi.last_error()
            assert got == want, name
            same_stream(out[:oh * oll].tobytes(), row, (name, "process"))
        finally:
            s.close()
        n += 1
    assert n == 8


def test_jpeg_encoder_vs_reference(hsv, det, ref_golden, oracle_mod):
    import torch

    n = 0
    for case, row, fr in cases(ref_golden, "jpeg"):
        name, (w, h, ll), _, q, bw = case
        dev = torch.from_numpy(fr).cuda()
        streams, sizes = det.jpeg_batch(dev, w, h, ll, q, bw)
        assert [int(sizes[0])] == row["out"]["size"], name
        same_stream(streams[0, :int(sizes[0])].cpu().numpy().tobytes(), row, (name, "batch"))
        # the declared output image is 16 x 2, so the stream's length alone decides the buffer
        s = sensor(hsv, hsv.JpegSensor, hsv.FORMAT_YUV422P, w, h, ll, 16, 2, 32)
        try:
            rc, oa, data = s.process(fr, q, bw, out_buffer=np.zeros(row["stream_len"] + 64, np.uint8))
            assert rc == hsv.IVIDTRANSCODE_EOK, hsv._abi.last_error()
            assert [int(oa.alg.size)] == row["out"]["size"], name
            same_stream(data, row, (name, "process"))
        finally:
            s.close()
        n += 1
    assert n == 8
