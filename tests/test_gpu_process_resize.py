"""process() on a live handle whose geometry changes: SETPARAMS to a smaller
geometry, to a larger one and back, one frame each, on one handle per sensor.
The handle's staging (the frame and preview buffers, the scale maps, the
multi-blob scratch) then grows, and is reused while larger than needed, instead
of starting empty as in every other process() test.  Each result is compared
with the oracle exactly as the sensor's own process() test compares it, on the
two smallest geometries that test runs."""
import numpy as np
import pytest

from gpu_util import LAYOUT_YUYV, T0

pytestmark = pytest.mark.gpu

RED = (0, 20, 80, 20, 50, 50)


@pytest.fixture(scope="module")
def hsv():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import trik_hsv

    return trik_hsv


def _ball(hsv, oracle_mod, s, geom, k, out):
    w, h, ll, ow, oh, oll = geom
    frame = oracle_mod.synth(1, w, h, ll, LAYOUT_YUYV, 1, 0x7A1C, first_frame=3 + k)
    rc, oa = s.process(frame, T0, out_buffer=out, auto_detect=True)
    assert rc == 0, hsv._abi.last_error()
    rc_o, want, preview = oracle_mod.run(frame, w, h, ll, LAYOUT_YUYV, T0, auto_detect=True, out_width=ow,
                                         out_height=oh, out_line_length=oll)
    assert rc_o == 0
    assert (oa.alg.targetX, oa.alg.targetY, oa.alg.targetSize) == (
        want["target_x"], want["target_y"], want["target_size"]), (geom, k)
    assert (oa.alg.detectHue, oa.alg.detectHueTolerance, oa.alg.detectSat, oa.alg.detectSatTolerance,
            oa.alg.detectVal, oa.alg.detectValTolerance) == (
        want["detect_hue"], want["detect_hue_tol"], want["detect_sat"], want["detect_sat_tol"],
        want["detect_val"], want["detect_val_tol"]), (geom, k)
    return preview


def _line(hsv, oracle_mod, s, geom, k, out):
    w, h, ll, ow, oh, oll = geom
    fr = oracle_mod.line_scene(w, h, ll, 1 + k, x0=None, slope=0.25)
    rc, oa = s.process(fr, (0, 359, 0, 100, 0, 30), out_buffer=out, auto_detect=True)
    assert rc == 0, hsv._abi.last_error()
    # (SETPARAMS runs setup, which puts the cross band back to its first-run rows: band=None)
    _, ref, ref_pv, _, _ = oracle_mod.line_run(fr, w, h, ll, 0, 30, band=None, out_width=ow, out_height=oh,
                                               out_line_length=oll)
    assert (oa.alg.targetX, oa.alg.targetY, oa.alg.targetSize) == (
        ref["target_x"], ref["target_y"], ref["target_size"]), (geom, k)
    assert (oa.alg.detectHue, oa.alg.detectVal) == (0, 0)
    return ref_pv


def _wline(hsv, oracle_mod, s, geom, k, out):
    w, h, ll, ow, oh, oll = geom
    fr = oracle_mod.wline_scene(w, h, ll, 1 + k, x0=None, slope=0.25)
    rc, oa = s.process(fr, (0, 359, 0, 100, 0, 30), out_buffer=out, auto_detect=True)
    assert rc == 0, hsv._abi.last_error()
    rrc, ref, ref_pv, _ = oracle_mod.wline_run(fr, w, h, ll, 0, 30, out_width=ow, out_height=oh,
                                               out_line_length=oll)
    assert rrc == 0
    assert (oa.alg.targetX, oa.alg.targetY, oa.alg.targetSize) == (
        ref["target_x"], ref["target_y"], ref["target_size"]), (geom, k)
    assert (oa.alg.detectHue, oa.alg.detectVal) == (0, 0)
    return ref_pv


def _blob(hsv, oracle_mod, s, geom, k, out):
    w, h, ll, ow, oh, oll = geom
    fr = oracle_mod.blob_scene(w, h, ll, 60 + k, noise=0.01 * k)
    # an explicit range on the first frame after every SETPARAMS, the oracle
    # from fresh state: whether the sticky range survives SETPARAMS is not asked
    rc, oa = s.process(fr, RED, out_buffer=out)
    assert rc == 0, hsv._abi.last_error()
    ref = oracle_mod.blob_run(fr, w, h, ll, hsv=RED, state=None, out_width=ow, out_height=oh, out_line_length=oll)
    got = [(oa.alg.target[i].x, oa.alg.target[i].y, oa.alg.target[i].size) for i in range(8)]
    assert got == [tuple(t) for t in ref["targets"].tolist()], (geom, k)
    return ref["preview"]


# sensor class, input format, the step, (smaller, larger) as (w, h, ll, ow, oh, oll)
SENSORS = {
    "ball": ("ObjectSensor", "FORMAT_YUV422", _ball,
             ((160, 120, 320, 320, 240, 640), (256, 240, 512, 100, 200, 200))),
    "line": ("LineSensor", "FORMAT_YUV422P", _line,
             ((320, 240, 320, 200, 150, 401), (320, 240, 324, 160, 120, 320))),
    "wline": ("WebcamLineSensor", "FORMAT_YUV422", _wline,
              ((64, 8, 128, 32, 4, 64), (320, 240, 704, 160, 120, 320))),
    "blob": ("BlobSensor", "FORMAT_YUV422P", _blob,
             ((320, 240, 352, 200, 150, 401), (640, 480, 640, 320, 240, 640))),
}


@pytest.mark.parametrize("name", list(SENSORS))
def test_process_after_geometry_change(hsv, oracle_mod, name):
    cls, fmt, step, (small, large) = SENSORS[name]
    s = getattr(hsv, cls)(hsv._default_params(1, getattr(hsv, fmt), 640, 480))
    try:
        for k, geom in enumerate((small, large, small)):
            w, h, ll, ow, oh, oll = geom
            assert s.set_params(w, h, ll, out_width=ow, out_height=oh, out_line_length=oll) == 0
            out = np.full(oh * oll + 16, 0xCD, np.uint8)
            preview = step(hsv, oracle_mod, s, geom, k, out)
            bad = np.flatnonzero(out[: oh * oll] != preview)
            assert bad.size == 0, f"{name} step {k}: {bad.size} preview bytes differ, first at {bad[:6].tolist()}"
            assert not out[oh * oll:].any()  # the bytes past the preview cleared
    finally:
        s.close()
