"""What tests/test_gpu_preview_shapes.py relies on, checked without a GPU:

* tests/preview_ref.py (maps, guide lines, clamp-then-map circle, body from
  the oracle's table and mask) equals oracle.run byte for byte on every
  corner-block frame, in both layouts and on each output geometry the GPU
  tests use -- and each placement shows what it is there for, asserted on
  oracle.run's own output;
* the case lists of tests/preview_cases.py reach every form the launcher can
  pick, by its restatement forms(), for 64, 256 and 304 CUs;
* the rows kernel's WIN form with GUIDES is unreachable from
  trik_hsv_batch_preview, and so is a refusal for out_w % 8 alone (a sweep of
  geometries through the restatement);
* the sampled-exhaustive batch holds every (Y, U, V) at a sampled pixel;
* the caller's-sums cases reach the clamps they name.
"""
import numpy as np
import pytest

import preview_cases as pc
import preview_ref
from preview_ref import LAYOUT_OV7670, LAYOUT_YUYV, MAGENTA, YELLOW

CUS = (64, 256, 304)

# (w, h, layout, ow, oh): the circle geometries in both layouts, and the frames
# whose overlay reads its maps from memory
REF_GEOMS = [(w, h, lay, ow, oh) for w, h, ow, oh in pc.CIRCLE_GEOMS for lay in (LAYOUT_YUYV, LAYOUT_OV7670)]
REF_GEOMS += [(c.w, c.h, c.layout, c.ow, c.oh) for c in pc.overlay_memory_cases()]


def _yellow(p, ow):
    return preview_ref.colour_pixels(p, ow, YELLOW)


@pytest.mark.parametrize("geom", REF_GEOMS, ids=["%dx%d_l%d_%dx%d" % g for g in REF_GEOMS])
def test_preview_ref_equals_oracle_run(oracle_mod, table, geom):
    w, h, layout, ow, oh = geom
    ll, oll = pc.line_length(w, layout), 2 * ow
    big = w > 640
    got_yellow, over_magenta, n = {}, 0, 0
    for rng in (pc.T0,) if big else (pc.T0, pc.V_BAND):
        for name in pc.PLACES:
            fr = pc.corner_block(table, rng, w, h, ll, layout, name)
            sums, mask = oracle_mod.frame(fr, w, h, ll, layout, [rng], want_mask=True)
            x0, y0, bw, bh = pc.place(name, w, h)
            inside = np.zeros((h, w), bool)
            inside[y0:y0 + bh, x0:x0 + bw] = True
            assert np.array_equal(mask != 0, inside), (name, "the block, and nothing else, is detected")
            body = preview_ref.body(table, mask, fr, w, h, ll, layout, ow, oh, oll)
            got = preview_ref.preview(body, w, h, ow, oh, oll, sums[0])
            rc, _, want = oracle_mod.run(fr, w, h, ll, layout, rng, out_width=ow, out_height=oh, out_line_length=oll)
            assert rc == 0
            bad = np.flatnonzero(got.reshape(-1) != want)
            assert bad.size == 0, (name, rng, bad[:6].tolist())
            n += 1
            # the claims, on oracle.run's output
            yellow = _yellow(want.reshape(oh, oll), ow)
            assert yellow, name
            got_yellow[(rng, name)] = len(yellow)
            lines = preview_ref.colour_pixels(preview_ref.preview(body, w, h, ow, oh, oll, (0, 0, 0)), ow, MAGENTA)
            over_magenta += len(yellow & lines)
        # the corner blocks and the centre block have one size, so one radius:
        # a corner's circle loses points to the clamp
        for corner in pc.CORNERS:
            assert got_yellow[(rng, corner)] < got_yellow[(rng, "centre")], (rng, corner, got_yellow)
    assert over_magenta > 0, "no circle pixel replaced a guide-line pixel"
    assert n == len(pc.PLACES) * (1 if big else 2)


# part B's geometries (w, h, layout, ow, oh): the exhaustive frame at identity scale, the sampled batch's frames
PART_B_GEOMS = [(c.w, c.h, c.layout, c.ow, c.oh) for c in pc.exhaustive_cases() if c.rng is pc.T0]


@pytest.mark.parametrize("geom", PART_B_GEOMS, ids=["%dx%d_l%d_%dx%d" % g for g in PART_B_GEOMS])
def test_preview_ref_equals_oracle_run_on_part_b_geometries(oracle_mod, table, geom):
    """One corner-block frame each: there preview_ref.preview, guide lines
    included, is the GPU test's only expectation."""
    w, h, layout, ow, oh = geom
    ll, oll = pc.line_length(w, layout), 2 * ow
    fr = pc.corner_block(table, pc.T0, w, h, ll, layout, "br")
    sums, mask = oracle_mod.frame(fr, w, h, ll, layout, [pc.T0], want_mask=True)
    assert int(sums[0][0]) == pc.BLOCK[0] * pc.BLOCK[1]
    got = preview_ref.preview(preview_ref.body(table, mask, fr, w, h, ll, layout, ow, oh, oll), w, h, ow, oh, oll, sums[0])
    rc, _, want = oracle_mod.run(fr, w, h, ll, layout, pc.T0, out_width=ow, out_height=oh, out_line_length=oll)
    assert rc == 0
    bad = np.flatnonzero(got.reshape(-1) != want)
    assert bad.size == 0, bad[:6].tolist()
    assert preview_ref.colour_pixels(want.reshape(oh, oll), ow, MAGENTA) and _yellow(want.reshape(oh, oll), ow)


def test_block_sizes_give_the_small_radii(oracle_mod, table):
    """The 1-pixel block gives n = 1 and the 2 x 2 block n = 4: radius 1 and 2."""
    for layout in (LAYOUT_YUYV, LAYOUT_OV7670):
        for name, n, radius in (("one", 1, 1), ("two", 4, 2)):
            fr = pc.corner_block(table, pc.T0, 96, 64, pc.line_length(96, layout), layout, name)
            sums, _ = oracle_mod.frame(fr, 96, 64, pc.line_length(96, layout), layout, [pc.T0])
            assert int(sums[0][0]) == n and preview_ref.centre_radius(sums[0])[2] == radius


@pytest.mark.parametrize("cus", CUS)
def test_case_lists_cover_every_form(cus):
    cases = pc.all_cases(cus)
    forms = {c.name: c.forms(cus) for c in cases}
    seen = {(f["kernel"], f["hue_free"], f["layout"]) for f in forms.values()}
    # every combination is reachable (a range and a layout do not bind the kernel)
    assert seen == {(k, hf, lay) for k in ("rows2", "gather") for hf in (False, True)
                    for lay in (LAYOUT_YUYV, LAYOUT_OV7670)}
    assert any(f["kernel"] == "rows2" and f["guides"] for f in forms.values())
    assert not any(f["kernel"] == "rows2" and (f["win"] or not f["guides"]) for f in forms.values())
    gathers = [f for f in forms.values() if f["kernel"] == "gather"]
    assert {f["gather_lds"] for f in gathers} == {False, True}
    assert {f["overlay_lds"] for f in forms.values()} == {False, True}
    assert {(f["overlay_lds"], f["kernel"]) for f in forms.values()} >= {(False, "rows2"), (False, "gather")}
    assert {f["layout"] for f in gathers if f["loads"] == "byte"} == {LAYOUT_YUYV, LAYOUT_OV7670}
    assert {f["layout"] for f in gathers if f["loads"] == "aligned"} == {LAYOUT_YUYV, LAYOUT_OV7670}
    # the ranges are what they are named for
    assert pc.hue_free(pc.V_BAND) and pc.hue_free(pc.SV_BAND) and not pc.hue_free(pc.T0)
    lo, hi, _ = pc.packed(pc.SV_BAND)
    assert 0 < lo[1] < hi[1] < 255 and pc.packed(pc.V_BAND)[0][1] == 0 and pc.packed(pc.V_BAND)[1][1] == 255

    # A: every lane takes at least three units (advance() feeds at least two
    # stored units), the last round is partial, the grid is the full one
    grid = pc.grid_cases(cus)
    outcomes = set()
    for c in grid:
        if c.entry == "batch":
            f = forms[c.name]
        else:  # the line and multi-blob previews run other instantiations of the same loop on the same grid
            assert pc.rows2_maps(c.w, c.h, c.ow, c.oh)[0] >= 0
            p = pc.rows2_plan(c.n, c.ow, c.oh, cus)
            f = {"kernel": "rows2", "grid": p["grid"], "min_units": p["min_units"], "max_units": p["max_units"],
                 "partial": p["partial"], "steps": p["steps"]}
        assert f["kernel"] == ("gather" if "gather" in c.name else "rows2"), c
        assert f["grid"] == 2 * cus and f["min_units"] >= 3 and f["partial"] and f["max_units"] == f["min_units"] + 1, (c, f)
        if f["kernel"] == "rows2":
            outcomes |= pc.advance_outcomes(c.n, c.ow, c.oh, cus)
    assert outcomes == {(False, False), (True, False), (False, True), (True, True)}
    steps = [forms[c.name]["steps"] for c in grid if c.entry == "batch" and forms[c.name]["kernel"] == "rows2"]
    assert any(s[2] != 0 for s in steps) and any(s[1] != 0 for s in steps)
    assert any(s[2] == 0 and s[1] == 0 for s in steps)  # the contrast: no carry at all
    # the line preview's written window leaves columns out (its WIN form)
    line = next(c for c in grid if c.entry == "line")
    wi2wo, _ = preview_ref.maps(line.w, line.h, line.ow, line.oh)
    assert wi2wo[5] > 0 and wi2wo[line.w - 5] < line.ow - 1

    # D: each refusing condition alone sends the aligned twin's call to the gather
    for twin, refused in pc.refusal_cases():
        assert forms[twin.name]["kernel"] == "rows2" and not forms[twin.name]["refused"]
        assert len(refused) == 7
        for c in refused:
            assert forms[c.name]["kernel"] == "gather", c
            assert pc.rows2_maps(c.w, c.h, c.ow, c.oh)[0] >= 0, (c, "the maps are the 2:1 ones")
            cond = c.name.split("_", 2)[2]
            # alone, but for out_w % 8: no width the entry point takes (w % 32 == 0) breaks it without
            # the width test (test_win_with_guides_is_unreachable sweeps for it)
            assert forms[c.name]["refused"] == ([cond, "width"] if cond == "out_w" else [cond]), (c, forms[c.name])
    for c in pc.byte_path_cases():
        assert forms[c.name]["kernel"] == "gather" and forms[c.name]["loads"] == "byte", c
    for c in pc.overlay_memory_cases():
        assert not forms[c.name]["overlay_lds"] and c.w + c.h > 8192


def test_win_with_guides_is_unreachable():
    """Over every output size of a few frames (widths the entry point takes:
    multiples of 32): wherever the maps are 2:1 with an unwritten column,
    2 * out_w > w, and launch_rows2 refuses; and wherever the maps are 2:1 and
    out_w % 8 != 0, the width test refuses as well, so that condition is never
    the only one."""
    windows = odd_widths = 0
    for w in (32, 64):
        for h in (4, 8, 16):
            for ow in range(1, w + 5):
                for oh in range(1, h + 3):
                    first, c0, c1, _ = pc.rows2_maps(w, h, ow, oh)
                    f = pc.forms(w, h, 2 * w, LAYOUT_YUYV, ow, oh, 2 * ow, 1, 0, h * 2 * w, 0, oh * 2 * ow, False, 64)
                    if first >= 0 and (c0 > 0 or c1 < ow):
                        windows += 1
                        assert 2 * ow > w and f["kernel"] == "gather", (w, h, ow, oh)
                    if first >= 0 and "out_w" in f["refused"]:
                        odd_widths += 1
                        assert "width" in f["refused"], (w, h, ow, oh)
                    if f["kernel"] == "rows2":
                        assert not f["win"] and f["guides"]
    assert windows > 0 and odd_widths > 0


@pytest.mark.parametrize("layout", [LAYOUT_YUYV, LAYOUT_OV7670])
def test_sampled_batch_holds_every_triple(layout):
    w, h, ow, oh, n = pc.SAMPLED
    ll = pc.line_length(w, layout)
    fb = pc.frame_bytes(w, h, ll, layout)
    batch = pc.sampled_batch(layout)
    assert batch.size == n * fb
    last_row, last_col = preview_ref.last_writers(w, h, ow, oh)
    assert last_row == list(range(1, h, 2)) and last_col == list(range(1, w, 2))  # the pixels the 2:1 maps sample
    seen = np.zeros(1 << 24, np.uint8)
    Y, U, V = pc.sampled_triples()
    for f in range(n):
        idx = preview_ref.yuv_index(batch[f * fb:(f + 1) * fb], w, h, ll, layout, last_row, last_col)
        assert np.array_equal(idx, Y[f].astype(np.int64) | (U[f].astype(np.int64) << 8) | (V[f].astype(np.int64) << 16))
        seen[idx.reshape(-1)] += 1
        if f == 0:  # the other taps hold other bytes: the even pixel's luma, the even row's everything
            other = preview_ref.yuv_index(batch[:fb], w, h, ll, layout, last_row, [c - 1 for c in last_col])
            assert np.array_equal(other & 255, 255 - (idx & 255))
            above = preview_ref.yuv_index(batch[:fb], w, h, ll, layout, [r - 1 for r in last_row], last_col)
            assert np.array_equal(above, idx ^ 0xFFFFFF)
    assert seen.min() == 1 and seen.max() == 1


@pytest.mark.parametrize("geom", pc.CIRCLE_GEOMS, ids=["%dx%d_%dx%d" % g for g in pc.CIRCLE_GEOMS])
def test_circle_sums_reach_their_clamps(geom):
    w, h, ow, oh = geom
    oll = 2 * ow
    blank = np.zeros((oh, oll), np.uint8)
    want = {name: preview_ref.preview(blank, w, h, ow, oh, oll, s) for name, s in pc.circle_sums(w, h)}
    yellow = {name: _yellow(p, ow) for name, p in want.items()}
    wi2wo, hi2ho = preview_ref.maps(w, h, ow, oh)
    for corner in pc.CORNERS:  # clamped: fewer pixels than at the centre, and other pixels than one step in
        assert len(yellow[corner + "_r2"]) < len(yellow["centre_r2"]), corner
        assert yellow[corner + "_r2"] != yellow["in_" + corner + "_r2"], corner
    sums = dict(pc.circle_sums(w, h))

    def outside(name):
        """(points left or right of the frame, points above or below it)"""
        pts = preview_ref.circle_points(*preview_ref.centre_radius(sums[name]))
        return sum(not 0 <= c < w for c, _ in pts), sum(not 0 <= r < h for _, r in pts)

    assert outside("centre_r2") == (0, 0)
    leaves = {"tl": (1, 1), "tr": (1, 1), "bl": (1, 1), "br": (1, 1), "top": (0, 1), "bottom": (0, 1),
              "left": (1, 0), "right": (1, 0), "in_tl": (1, 1), "in_tr": (1, 1), "in_bl": (1, 1), "in_br": (1, 1)}
    for name, want_out in leaves.items():  # which sides of the frame the circle crosses
        assert tuple(int(v > 0) for v in outside(name + "_r2")) == want_out, name
    for corner in pc.CORNERS:  # two pixels out at a corner, one when one step in
        assert outside(corner + "_r2") > outside("in_" + corner + "_r2") > (0, 0)
    assert yellow["centre_n1"] == yellow["centre_n3"] != yellow["centre_r2"]  # radius 1, 1, 2
    assert preview_ref.centre_radius((1, 0, 0))[2] == preview_ref.centre_radius((3, 0, 0))[2] == 1
    assert preview_ref.centre_radius((4, 0, 0))[2] == 2
    assert not yellow["no_points"] and preview_ref.colour_pixels(want["no_points"], ow, MAGENTA)
    assert yellow["low_word_x"] == yellow["low_word_y"] == yellow["centre_r2"]
    # the unsigned quotient is clamped to the last column / row (a signed one to the first)
    assert {c for _, c in yellow["unsigned_x"]} == {wi2wo[w - 1]}
    assert {r for r, _ in yellow["unsigned_y"]} == {hi2ho[h - 1]}
    rows = {r for r, _ in yellow["two_edges"]}
    cols = {c for _, c in yellow["two_edges"]}
    assert 0 in rows and wi2wo[w - 1] in cols and len(rows) > 2 and len(cols) > 2
    n, sx, sy = dict(pc.circle_sums(w, h))["huge"]
    assert preview_ref.centre_radius((n, sx, sy))[2] ** 2 > (w // 2) ** 2 + (h // 2) ** 2  # no point inside the frame
    assert all(r in (0, hi2ho[h - 1]) or c in (0, wi2wo[w - 1]) for r, c in yellow["huge"])  # only the frame's border
    # a circle pixel lands on a guide-line pixel
    lines = preview_ref.colour_pixels(want["no_points"], ow, MAGENTA)
    assert any(yellow[name] & lines for name in yellow)
