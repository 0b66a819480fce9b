"""What tests/test_gpu_frame_ranges_preview.py relies on, checked without a GPU:

* the case lists of tests/frame_ranges_preview_cases.py reach every form
  launch_frame_ranges_preview can pick, by its restatement plan(), for 64, 256
  and 304 CUs: both kernels in both layouts, tasks with idle lanes, waves that
  take three rounds and a partial fourth and change frame and range between
  them, each refusal of the 2:1 kernel alone, byte loads, maps in LDS and in
  memory;
* on the reference's own output: every frame of the "range follows the frame"
  batches looks different under its neighbours' ranges, the slot's other
  entries would give other pictures, rotating the sixteen ranges changes what
  every frame detects, a bound above 255 is the bound 255;
* the expectation (preview_ref.body over oracle.frame's mask, then
  preview_ref.preview) equals oracle.run's preview byte for byte on the
  closed-loop frames under their own ranges and on scene frames under the pool.
"""
import numpy as np
import pytest

import frame_ranges_cases as FC
import frame_ranges_preview_cases as PC
import preview_cases as pc
import preview_ref
from preview_ref import LAYOUT_OV7670, LAYOUT_YUYV

CUS = (64, 256, 304)
LAYOUTS = {LAYOUT_YUYV, LAYOUT_OV7670}


def test_abi_mirror_and_method():
    from trik_hsv import Detector, _abi

    args, res = _abi.PROTOTYPES["trik_hsv_frame_ranges_preview"]
    assert len(args) == 13 and hasattr(_abi.load(), "trik_hsv_frame_ranges_preview")
    assert callable(Detector.frame_ranges_preview)


def test_argument_checks_need_no_gpu():
    """The checks that come before any device call: NULL handle, n_ranges and t
    out of bounds, NULL ranges."""
    import ctypes as C
    import threading

    from trik_hsv import _abi

    lib = _abi.load()
    b = _abi.FrameBatch(0, 64 * 8, 1, 32, 8, 64, LAYOUT_YUYV)
    tail = (None, 1, 16, 4, 32, None, 128, None)
    got = []

    def call():  # (the error text is the calling thread's: a thread of its own leaves this one's as it is)
        got.append((lib.trik_hsv_frame_ranges_preview(None, C.byref(b), None, 1, 0, *tail), lib.trik_hsv_last_error()))

    th = threading.Thread(target=call)
    th.start()
    th.join()
    assert got[0][0] != 0 and b"handle" in got[0][1]


@pytest.mark.parametrize("cus", CUS)
def test_case_lists_cover_every_form(cus):
    plans = {c.name: PC.plan_of(c, cus) for c in PC.all_cases(cus)}
    assert {(p["kernel"], p["layout"]) for p in plans.values()} == {(k, lay) for k in ("rows2", "gather") for lay in LAYOUTS}
    gathers = [p for p in plans.values() if p["kernel"] == "gather"]
    assert {(p["loads"], p["layout"]) for p in gathers} == {(ld, lay) for ld in ("aligned", "byte") for lay in LAYOUTS}
    assert {(p["maps_lds"], p["layout"]) for p in gathers} == {(m, lay) for m in (False, True) for lay in LAYOUTS}
    assert {p["overlay_lds"] for p in plans.values()} == {False, True}
    assert all(p["guides"] == (p["kernel"] == "rows2") for p in plans.values())

    # a. one task per frame (two in the larger gather), with lanes that hold no unit; neighbouring waves hold
    # other frames and ranges
    for c in PC.follow_cases():
        p = plans[c.name]
        assert p["kernel"] == ("gather" if "gather" in c.name else "rows2"), (c, p)
        assert p["segs"] == (2 if c.name == "follow_gather_ov7670_96x8" else 1) and p["idle"] > 0, (c, p)
        assert p["tasks"] == c.n * p["segs"] and p["waves"] >= PC.WAVES, (c, p)
        rs = PC.follow_ranges(c.n)
        assert all(rs[f] != rs[f + 1] for f in range(c.n - 1)) and len(set(rs)) == 4

    # b. the full grid, three rounds for every wave and a fourth for some; the last task of a frame has idle
    # lanes; a wave's successive tasks lie in other frames under other ranges
    for c in PC.grid_cases(cus):
        p = plans[c.name]
        assert p["kernel"] == ("gather" if "gather" in c.name else "rows2"), (c, p)
        assert p["grid"] == PC.BLOCKS_PER_CU * cus and p["min_tasks"] >= 3 and p["partial"], (c, p)
        assert p["max_tasks"] == p["min_tasks"] + 1 and p["segs"] > 1 and p["idle"] > 0, (c, p)
        rs = PC.pool_ranges(c.n)
        assert len(set(rs)) == len(PC.POOL)
        for wave in (0, 1, p["waves"] - 1):
            frames = [t // p["segs"] for t in range(wave, p["tasks"], p["waves"])]
            assert len(frames) >= 3 and all(rs[a] != rs[b] for a, b in zip(frames, frames[1:])), (c, wave)

    # c. both kernels, whole tasks only, the gather's maps in LDS
    for c in PC.exhaustive_cases():
        p = plans[c.name]
        assert p["kernel"] == ("gather" if "gather" in c.name else "rows2") and p["idle"] == 0 and c.n == 16, (c, p)
        assert p["kernel"] == "rows2" or (p["maps_lds"] and p["loads"] == "aligned")

    # d. the circle geometries: the 2:1 kernel, the gather, the gather with unwritten output pixels
    assert [plans[c.name]["kernel"] for c in pc.circle_cases()] == ["rows2", "gather", "gather"]

    # e. a gap between previews under both kernels, line padding under the gather
    for c in PC.equal_cases():
        p = plans[c.name]
        assert c.preview_stride > c.pb and p["kernel"] == ("rows2" if "rows2" in c.name else "gather"), (c, p)
        assert p["kernel"] == "rows2" or c.oll > 2 * c.ow

    # f. each refusing condition alone (out_w % 8 with the width test, preview_cases' docstring)
    for twin, refused in pc.refusal_cases():
        assert plans[twin.name]["kernel"] == "rows2" and not plans[twin.name]["refused"]
        for c in refused:
            cond = c.name.split("_", 2)[2]
            assert plans[c.name]["kernel"] == "gather", c
            assert plans[c.name]["refused"] == ([cond, "width"] if cond == "out_w" else [cond]), (c, plans[c.name])
    for c in pc.byte_path_cases():
        assert plans[c.name]["kernel"] == "gather" and plans[c.name]["loads"] == "byte", c
    for c in PC.placement_cases():
        if c.name.startswith("maps_mem"):
            assert plans[c.name]["kernel"] == "gather" and not plans[c.name]["maps_lds"], c
            assert 2 * (c.ow + c.oh) > PC.MAP_LDS_BYTES and c.w < 65535 and not plans[c.name]["overlay_lds"]


def _bodies(oracle_mod, table, host, c, ranges):
    def one(f):
        fr = PC.frame_of(host, c, f)
        _, mask = oracle_mod.frame(fr, c.w, c.h, c.ll, c.layout, [PC.clamp255(ranges[f])], want_mask=True)
        return preview_ref.body(table, mask, fr, c.w, c.h, c.ll, c.layout, c.ow, c.oh, c.oll).reshape(-1)

    return np.stack([one(f) for f in range(c.n)])


@pytest.mark.parametrize("c", PC.follow_cases(), ids=repr)
def test_every_frame_differs_under_its_neighbours_ranges(oracle_mod, table, c):
    host = PC.follow_frames(table, c)
    rs = PC.follow_ranges(c.n)
    own = _bodies(oracle_mod, table, host, c, rs)
    before = _bodies(oracle_mod, table, host, c, [rs[f - 1] for f in range(c.n)])
    after = _bodies(oracle_mod, table, host, c, [rs[(f + 1) % c.n] for f in range(c.n)])
    assert (own != before).any(axis=1).all() and (own != after).any(axis=1).all()
    cyan = preview_ref.px565(preview_ref.DETECTED)
    px = own.reshape(c.n, c.oh, c.oll)[:, :, :2 * c.ow].reshape(c.n, c.oh, c.ow, 2)
    hit = ((px[..., 0].astype(int) | (px[..., 1].astype(int) << 8)) == cyan).reshape(c.n, -1)
    assert hit.any(axis=1).all() and not hit.all(axis=1).any()  # its own range paints some sampled pixels, not all
    assert len({fr.tobytes() for fr in host.reshape(c.n, c.fb)}) >= 4


def test_slot_entries_give_other_pictures(oracle_mod, table):
    for c in pc.circle_cases():
        fr = pc.corner_block(table, pc.T0, c.w, c.h, c.ll, c.layout, "centre")
        one = pc.Case("one", c.w, c.h, c.layout, c.ow, c.oh, 1)
        name, sums = pc.circle_sums(c.w, c.h)[0]
        want = PC.expected(oracle_mod, table, fr, one, [pc.T0], [sums])
        for other in PC.SLOT_OTHERS:
            assert not np.array_equal(PC.expected(oracle_mod, table, fr, one, [other], [sums]), want)
        assert not np.array_equal(PC.expected(oracle_mod, table, fr, one, [pc.T0], [PC.OTHER_SUMS]), want)


def test_sixteen_ranges_and_their_rotation(table):
    det = [pc.detect_table(table, PC.clamp255(r)) for r in PC.SIXTEEN]
    assert len(set(PC.SIXTEEN)) == 16 and PC.SIXTEEN[:12] == FC.POOL
    some = [bool(d.any()) and not bool(d.all()) for d in det]
    assert sum(some) >= 12 and det[4].all()  # (the full range detects everything)
    for f in range(16):  # frame f detects other triples under the rotated list
        assert not np.array_equal(det[f], det[(f + 1) % 16]), f
    assert PC.sixteen_ranges(1)[0] == PC.SIXTEEN[1] and PC.sixteen_ranges(0) == PC.SIXTEEN


def test_bounds_above_255_are_255():
    for wide in ((0, 359, 10, 300, 20, 300), (330, 20, 30, 65535, 30, 256), (0, 359, 256, 65535, 0, 100)):
        assert PC.clamp255(wide) != wide and pc.packed(wide) == pc.packed(PC.clamp255(wide))


def test_expectation_equals_oracle_run_on_the_loop_frames(oracle_mod, table):
    """The closed-loop frames under the ranges autoDetectHsv gives them: the
    restatement with the frames' own sums is oracle.run's preview."""
    c = PC.loop_case()
    host = FC.loop_frames(oracle_mod)
    ranges = PC.loop_ranges(oracle_mod)
    FC.check_loop(ranges)
    sums = PC.own_sums(oracle_mod, host, c, ranges)
    assert (sums[:, 0] > 0).any()
    want = PC.oracle_previews(oracle_mod, host, c, ranges)
    assert np.array_equal(PC.expected(oracle_mod, table, host, c, ranges, sums), want)
    shifted = PC.oracle_previews(oracle_mod, host, c, ranges[1:] + ranges[:1])
    assert (want != shifted).any(axis=1).sum() >= 2  # the ranges matter


@pytest.mark.parametrize("c", PC.equal_cases(), ids=repr)
def test_expectation_equals_oracle_run_on_scene_frames(oracle_mod, table, c):
    host = PC.scene_frames(oracle_mod, c)
    ranges = PC.pool_ranges(c.n)
    sums = PC.own_sums(oracle_mod, host, c, ranges)
    want = PC.oracle_previews(oracle_mod, host, c, ranges)
    assert np.array_equal(PC.expected(oracle_mod, table, host, c, ranges, sums), want)
    assert (sums[:, 0] > 0).sum() >= c.n // 2
    if c.oll > 2 * c.ow:
        assert not want.reshape(c.n, c.oh, c.oll)[:, :, 2 * c.ow:].any()  # the line padding is zero
