"""What tests/test_gpu_line_frame_ranges_preview.py relies on, checked without a GPU:

* tests/line_preview_ref.py equals oracle.line_run's and oracle.wline_run's
  previews byte for byte: scene frames at 640x480 -> 320x240, 320x240 -> 160x120
  and the non-2:1 240x320, with the frames' own sums and with an empty range;
* the case lists of tests/line_frame_ranges_preview_cases.py reach every form
  launch_line_frame_ranges_preview can pick, by its restatement forms(), for 64,
  256 and 304 CUs; on the reference's own output every frame of the "range
  follows the frame" batches differs from what its neighbours' ranges would
  give, and the edge cases of the target line do hit output columns 0 and W - 1;
* the ABI mirror and the method exist, and every argument refusal that comes
  before a device call returns non-zero with a message.
"""
import ctypes as C
import threading

import numpy as np
import pytest

import line_frame_ranges_preview_cases as LP
import line_preview_ref as LR
import line_ref
import preview_cases as pc
import preview_ref
from preview_ref import LAYOUT_OV7670, LAYOUT_YUYV

CUS = (64, 256, 304)


# ------------------------------------------------- the ABI and its refusals

def test_abi_mirror_and_method():
    from trik_hsv import Detector, _abi

    args, res = _abi.PROTOTYPES["trik_hsv_line_frame_ranges_preview"]
    assert len(args) == 10 and hasattr(_abi.load(), "trik_hsv_line_frame_ranges_preview")
    assert callable(Detector.line_frame_ranges_preview)


def _call(handle, batch, ranges, sums, ow, oh, oll, previews, stride):
    """(rc, message) of one call on a thread of its own (the error text is the
    calling thread's)."""
    from trik_hsv import _abi

    lib = _abi.load()
    got = []

    def run():
        rc = lib.trik_hsv_line_frame_ranges_preview(handle, C.byref(batch) if batch is not None else None, ranges, sums,
                                                    ow, oh, oll, previews, stride, None)
        got.append((rc, lib.trik_hsv_last_error()))

    th = threading.Thread(target=run)
    th.start()
    th.join()
    return got[0]


def test_argument_checks_need_no_gpu():
    """Every refusal that is decided before the handle is read: these checks
    take no device call, so a non-NULL pointer stands for the handle and for
    each buffer."""
    from trik_hsv import _abi

    store = (C.c_uint8 * 4096)()
    p = C.c_void_p(C.addressof(store))
    w, h, ow, oh = 64, 8, 32, 4

    def batch(**kw):
        args = dict(frames=C.addressof(store), frame_stride=2 * w * h, n_frames=2, width=w, height=h, line_length=2 * w,
                    layout=LAYOUT_YUYV)
        args.update(kw)
        return _abi.FrameBatch(**args)

    good = dict(handle=p, batch=batch(), ranges=p, sums=p, ow=ow, oh=oh, oll=2 * ow, previews=p, stride=oh * 2 * ow)
    bad = [("handle", dict(handle=None)), ("batch is NULL", dict(batch=None)), ("unknown layout", dict(batch=batch(layout=2))),
           ("width % 32", dict(batch=batch(width=33))), ("height % 4", dict(batch=batch(height=6))),
           ("n_frames < 0", dict(batch=batch(n_frames=-1))),
           ("line_length shorter", dict(batch=batch(line_length=2 * w - 1))),
           ("frame_stride shorter", dict(batch=batch(frame_stride=2 * w * h - 1))),
           ("frames is NULL", dict(batch=batch(frames=0))),
           ("line_length shorter", dict(batch=batch(layout=LAYOUT_OV7670, line_length=w - 1))),
           ("ranges is NULL", dict(ranges=None)), ("sums is NULL", dict(sums=None)),
           ("out_line_length", dict(oll=2 * ow - 1)), ("out_line_length", dict(ow=-1)), ("out_line_length", dict(oh=-1)),
           ("preview_stride smaller", dict(stride=oh * 2 * ow - 1)), ("previews is NULL", dict(previews=None))]
    for what, kw in bad:
        args = dict(good)
        args.update(kw)
        rc, err = _call(**args)
        assert rc != 0 and what.encode() in err, (what, rc, err)


# -------------------------------------------- the reference and the oracle

REF_GEOMS = [(640, 480, 320, 240), (320, 240, 160, 120), (640, 480, 240, 320)]
REF_PAIRS = [(0, 30), (20, 100), LP.EMPTY]


@pytest.mark.parametrize("geom", REF_GEOMS, ids=lambda g: "%dx%d_%dx%d" % g)
@pytest.mark.parametrize("layout", LP.LAYOUTS, ids=["yuyv", "ov7670"])
def test_reference_equals_the_oracle(oracle_mod, table, layout, geom):
    """One sampling of the scene, three ranges: own sums (with and without a
    target line) and the empty range, padded out_line_length included."""
    w, h, ow, oh = geom
    ll, oll = pc.line_length(w, layout), 2 * ow + 6
    scene = oracle_mod.line_scene if layout == LAYOUT_OV7670 else oracle_mod.wline_scene
    fr = scene(w, h, ll, 31, x0=w // 3, slope=0.2)
    smp = LR.sampled(table, fr[None, :], w, h, ll, layout, ow, oh)
    lines = 0
    for vf, vt in REF_PAIRS:
        if layout == LAYOUT_OV7670:
            rc, _, want, sums, _ = oracle_mod.line_run(fr, w, h, ll, vf, vt, out_width=ow, out_height=oh,
                                                      out_line_length=oll)
        else:
            rc, _, want, sums = oracle_mod.wline_run(fr, w, h, ll, vf, vt, out_width=ow, out_height=oh,
                                                     out_line_length=oll)
        assert rc == 0
        got = LR.previews(table, fr[None, :], w, h, ll, layout, ow, oh, oll, [(vf, vt)], [sums], smp)[0]
        assert np.array_equal(got, want), (layout, geom, vf, vt, np.flatnonzero(got != want)[:6].tolist())
        assert (sums[0] == 0) == ((vf, vt) == LP.EMPTY)
        lines += LR.target_column(sums) is not None
    assert lines == 2


# ------------------------------------------------------- the case lists

def test_no_scaled_from_is_to_plus_one():
    """line_frame_ranges_preview_cases' note on NARROWEST_EMPTY: over every
    uint16 no two bounds scale to neighbouring bytes."""
    s = sorted({line_ref.scale_val(v) for v in range(65536)})
    assert s[-1] == 255 and all(b - a >= 2 for a, b in zip(s, s[1:]))
    vf, vt = LP.NARROWEST_EMPTY
    assert vf == vt + 1 and line_ref.scale_val(vf) > line_ref.scale_val(vt)
    scaled = [(line_ref.scale_val(a), line_ref.scale_val(b)) for a, b in LP.EXHAUSTIVE_PAIRS]
    assert len(set(LP.EXHAUSTIVE_PAIRS)) == 64 and (0, 255) in scaled
    assert sum(a == b for a, b in scaled) >= 3 and sum(a > b for a, b in scaled) >= 2
    assert any(b > 100 for _, b in LP.EXHAUSTIVE_PAIRS)


@pytest.mark.parametrize("cus", CUS)
def test_case_lists_cover_every_form(cus):
    forms = {c.name: LP.forms_of(c, cus) for c in LP.all_cases(cus)}
    assert {(f["kernel"], f["layout"]) for f in forms.values()} == {(k, lay) for k in ("rows2", "gather") for lay in LP.LAYOUTS}
    rows2 = [f for f in forms.values() if f["kernel"] == "rows2"]
    # the ov7670 window always leaves output columns unwritten under 2:1 maps (WIN); YUYV never does
    assert all(f["win"] == (f["layout"] == LAYOUT_OV7670) for f in rows2)
    gathers = [f for f in forms.values() if f["kernel"] == "gather"]
    assert {(f["loads"], f["layout"]) for f in gathers} == {(ld, lay) for ld in ("aligned", "byte") for lay in LP.LAYOUTS}
    assert all(f["maps_lds"] for f in gathers)
    # ovl_ok never refuses alone: 2:1 maps rise in steps of 0 or 1
    assert all("maps" in f["refused"] for f in forms.values() if "ovl" in f["refused"])

    # a. fewer than 64 units (128 groups) a frame: one task each, idle lanes, waves that loop over frames
    for c in LP.follow_cases():
        f = forms[c.name]
        assert f["kernel"] == ("gather" if "gather" in c.name else "rows2") and f["segs"] == 1 and f["idle"] > 0, (c, f)
        assert f["tasks"] == c.n and (c.oll > 2 * c.ow) == (f["kernel"] == "gather"), (c, f)

    # b. the full grid, three rounds for every wave and a fourth for some
    for c in LP.grid_cases(cus):
        f = forms[c.name]
        assert f["kernel"] == ("gather" if "gather" in c.name else "rows2"), (c, f)
        assert f["grid"] == LP.BLOCKS_PER_CU * cus and f["min_tasks"] >= 3 and f["partial"], (c, f)
        assert f["max_tasks"] == f["min_tasks"] + 1 and (c.w, c.h) == (32, 8), (c, f)
        ps = LP.follow_pairs(c.n)
        for wave in (0, 1, f["waves"] - 1):  # a wave's successive tasks lie in other frames under other ranges
            frames = [t // f["segs"] for t in range(wave, f["tasks"], f["waves"])]
            assert len(frames) >= 3 and all(ps[a] != ps[b] for a, b in zip(frames, frames[1:])), (c, wave)

    # c. both kernels, whole tasks only
    for c in LP.exhaustive_cases():
        f = forms[c.name]
        assert f["kernel"] == ("gather" if "gather" in c.name else "rows2") and f["idle"] == 0 and c.n == 16, (c, f)

    # d. the target geometries: both forms at 32 wide and at 320 x 240
    assert [forms[c.name]["kernel"] for c in LP.target_cases()] == ["rows2"] * 2 + ["gather"] * 2 + ["rows2"] * 2 + ["gather"] * 2

    # e. 2:1 everywhere but the webcam glue's default output
    assert [forms[c.name]["kernel"] for c in LP.equal_cases()] == ["rows2", "rows2", "rows2", "gather"]

    # f. each refusing condition alone (out_w % 8 comes with the width test, preview_cases' docstring)
    for twin, refused in pc.refusal_cases():
        assert forms[twin.name]["kernel"] == "rows2" and not forms[twin.name]["refused"]
        for c in refused:
            cond = c.name.split("_", 2)[2]
            assert forms[c.name]["kernel"] == "gather", c
            assert forms[c.name]["refused"] == ([cond, "width"] if cond == "out_w" else [cond]), (c, forms[c.name])
    for c in pc.byte_path_cases():
        assert forms[c.name]["kernel"] == "gather" and forms[c.name]["loads"] == "byte", c
    for c in LP.placement_cases():
        if c.name.startswith("extra"):
            f = forms[c.name]
            want = {"frame_stride_odd": ("gather", ["frame_stride"]), "previews_2": ("gather", ["previews"]),
                    "gap": ("rows2", [])}[c.name.split("_", 2)[2]]
            assert (f["kernel"], f["refused"]) == want, (c, f)
            assert c.name.endswith("gap") or f["loads"] == "byte"


def test_ovl_ok_holds_wherever_the_maps_are_2_to_1():
    """The 2:1 form's `ovl` condition cannot fail alone, so no case breaks it."""
    for w in (32, 64, 96, 320, 640):
        for h in (8, 64, 240, 480):
            for ow in range(1, w + 9, 7):
                for oh in (h // 4, h // 2, h // 2 + 1, h):
                    for lay in LP.LAYOUTS:
                        if LP.rows2_maps(w, h, ow, oh, lay)[0] >= 0:
                            assert LP.ovl_ok(w, h, ow, oh), (w, h, ow, oh)


@pytest.mark.parametrize("c", LP.follow_cases(), ids=repr)
def test_every_frame_differs_under_its_neighbours_ranges(oracle_mod, table, c):
    host = LP.noise_frames(c, 11)
    smp = LR.sampled(table, LP.frames2d(host, c), c.w, c.h, c.ll, c.layout, c.ow, c.oh)
    sums = np.zeros((c.n, 3), np.int64)
    own, before, after = (LP.expected(table, host, c, LP.follow_pairs(c.n, s), sums, smp) for s in (0, -1, 1))
    assert (own != before).any(axis=1).all() and (own != after).any(axis=1).all()
    ps = LP.follow_pairs(c.n)
    assert LP.EMPTY in ps and LP.ABOVE_100 in ps and all(ps[f] != ps[f + 1] for f in range(c.n - 1))
    cyan = preview_ref.px565(LR.DETECTED)
    px = own.reshape(c.n, c.oh, c.oll)[:, :, :2 * c.ow].reshape(c.n, c.oh, c.ow, 2)
    hit = ((px[..., 0].astype(int) | (px[..., 1].astype(int) << 8)) == cyan).reshape(c.n, -1).any(axis=1)
    # the empty range detects nothing; the others something (in the smallest previews, nearly all of them)
    assert not any(hit[f] for f in range(c.n) if ps[f] == LP.EMPTY)
    assert sum(bool(hit[f]) for f in range(c.n) if ps[f] != LP.EMPTY) >= 0.9 * sum(p != LP.EMPTY for p in ps)
    if c.oll > 2 * c.ow:
        assert not own.reshape(c.n, c.oh, c.oll)[:, :, 2 * c.ow:].any()  # the line padding is zero


def _red_columns(p, c):
    """The output columns that are red on every row of preview p."""
    px = np.asarray(p).reshape(c.oh, c.oll)[:, :2 * c.ow].reshape(c.oh, c.ow, 2)
    red = (px[..., 0].astype(int) | (px[..., 1].astype(int) << 8)) == preview_ref.px565(LR.RED)
    return set(np.flatnonzero(red.all(axis=0)).tolist())


@pytest.mark.parametrize("c", LP.target_cases(), ids=repr)
def test_target_cases_reach_the_edges(table, c):
    cases = LP.target_sums(c.w)
    host = np.tile(LP.noise_frames(pc.Case("one", c.w, c.h, c.layout, c.ow, c.oh, 1), 5), c.n)
    pairs = [LP.EMPTY] * c.n  # (no detected pixel: red comes from the overlays alone)
    got = LP.expected(table, host, c, pairs, [s for _, s in cases])
    wi2wo, _ = preview_ref.maps(c.w, c.h, c.ow, c.oh)
    cols = {name: _red_columns(got[i], c) for i, (name, _) in enumerate(cases)}
    assert cols["cx_0"] == {wi2wo[0], wi2wo[1]} and 0 in cols["cx_0"]
    assert cols["cx_%d" % (c.w - 1)] == {wi2wo[c.w - 2], wi2wo[c.w - 1]} and wi2wo[c.w - 1] in cols["cx_%d" % (c.w - 1)]
    assert cols["past_the_frame"] == {wi2wo[c.w - 1]} == cols["unsigned_x"]
    assert cols["points_10"] == set() == cols["no_points"] == cols["high_points_only"] and cols["points_11"]
    assert cols["high_words"] == {wi2wo[x] for x in range(c.w // 4 + 2, c.w // 4 + 5)}
    assert len({got[i].tobytes() for i in range(c.n)}) >= 5
    if c.w == 32:  # all four thin lines clamp to source columns 0 and W - 1
        magenta = preview_ref.colour_pixels(got[cases.index(("no_points", (0, 77, 0)))].reshape(c.oh, c.oll), c.ow, LR.MAGENTA)
        assert {col for _, col in magenta} == {0, wi2wo[c.w - 1]}
