"""Every restatement of the reference against the reference's own code, built
on the host (oracle/ref, tests/ref_lib.py): the per-pixel path on all 2^24
triples, and whole setup() + run() of the six sensors against oracle.run,
oracle.line_run, oracle.wline_run, oracle.blob_run, mxn_ref and jpeg_ref.

All comparisons are exact.  Every test counts the cases that reached its
comparison and fails below the count it names.  The reference keeps its images
in 640 x 480 statics, so inputs larger than that cannot be driven; the input
families of the GPU tests are imported from their modules, not restated.
"""
from collections import Counter

import numpy as np
import pytest

import blob_patterns
import jpeg_cases
import jpeg_ref
import mxn_cases
import mxn_ref
import preview_cases
import ref_lib
import test_gpu_blob as gpu_blob
import test_gpu_line as gpu_line
import test_gpu_mxn as gpu_mxn
import test_gpu_wline as gpu_wline
from test_oracle_blob import target_py
from golden.make_golden import BLOB_CASES, CASES, LINE_CASES, RANGES, RUN_CASES

LAYOUT_YUYV, LAYOUT_OV7670 = 0, 1
OUTARGS = ("target_x", "target_y", "target_size")
DETECT = ("detect_hue", "detect_hue_tol", "detect_sat", "detect_sat_tol", "detect_val", "detect_val_tol")


@pytest.fixture(scope="module", autouse=True)
def _reference_build():
    ref_lib.require()


def fits(w, h):
    """The reference's static images hold 640 x 480."""
    return w <= 640 and h <= 480


# ---------------------------------------------------------------- pixel path

def test_pixel_path_webcam_exhaustive(table):
    """convert2xYuyvToRgb888 + convertRgb888ToHsv of the webcam detector on
    every (Y, U, V), for the first and for the second pixel of a word."""
    first, second = ref_lib.webcam_pixel_tables()
    compared = 0
    for got in (first, second):
        bad = np.flatnonzero(got != table)
        assert bad.size == 0, (bad.size, [(int(i), hex(int(got[i])), hex(int(table[i]))) for i in bad[:4]])
        compared += got.size
    assert compared == 2 << 24


def test_pixel_path_ov7670_exhaustive(table):
    """The ov7670 unpacking (OSEQ:369-381) and the per-pixel path on every
    (Y, U, V), every luma in each of the four positions of a 4-pixel group."""
    compared = 0
    for rot in range(4):
        got = ref_lib.ov7670_pixel_table(rot)
        bad = np.flatnonzero(got != table)
        assert bad.size == 0, (rot, bad.size, [(int(i), hex(int(got[i])), hex(int(table[i]))) for i in bad[:4]])
        compared += got.size
    assert compared == 4 << 24


# ------------------------------------------------------- webcam object sensor

def _same_run(oracle_mod, fr, w, h, ll, rng, auto, ow, oh, oll, what):
    rc, oa, pv = oracle_mod.run(fr, w, h, ll, LAYOUT_YUYV, rng, auto_detect=auto, out_width=ow,
                                out_height=oh, out_line_length=oll)
    rrc, roa, rpv = ref_lib.webcam_run(fr, w, h, ll, rng, auto, ow, oh, oll)
    assert rrc == rc == 0, what  # refusals are test_webcam_object_sensor_rejects'; a counted case is compared
    for k in OUTARGS + (DETECT if auto else ()):
        assert roa[k] == oa[k], (what, k, roa, oa)
    assert oa["detect_written"] == (1 if auto else 0), what
    assert np.array_equal(rpv, pv), (what, int(np.flatnonzero(rpv != pv)[0]))


# 32 x 4, 64 x 16 with a ragged line, 160 x 120, 320 x 240
OBJECT_GEOMS = [(32, 4, 64), (64, 16, 160), (160, 120, 320), (320, 240, 640)]


@pytest.mark.parametrize("geom", OBJECT_GEOMS, ids=["%dx%d_ll%d" % g for g in OBJECT_GEOMS])
def test_webcam_object_sensor(oracle_mod, geom):
    """Return code, target, the six detect fields and every preview byte:
    uniform and scene frames x the twelve golden ranges x autoDetectHsv off
    and on x a 2:1 and a 1:1 preview."""
    w, h, ll = geom
    n = 0
    for kind in (0, 1):
        fr = oracle_mod.synth(1, w, h, ll, LAYOUT_YUYV, kind, 0x7A1C, first_frame=2 + kind)
        for name, rng in RANGES.items():
            for auto in (False, True):
                for ow, oh, oll in ((w // 2, h // 2, w), (w, h, 2 * w + 6)):
                    _same_run(oracle_mod, fr, w, h, ll, rng, auto, ow, oh, oll, (geom, kind, name, auto, ow))
                    n += 1
    assert n == 2 * 12 * 2 * 2


def test_webcam_object_sensor_golden_cases(oracle_mod):
    """The inputs of tests/golden/make_golden.py that the webcam detector can
    take (packed YUYV, at most 640 x 480): CASES with every range of theirs,
    and RUN_CASES with their preview geometry."""
    n = empty = 0
    for name, w, h, ll, layout, kind, seed, fidx, rnames in CASES:
        if layout != LAYOUT_YUYV or not fits(w, h):
            continue
        if h == 0:
            # Not driven: the reference draws its guide lines through row 0 of an
            # empty image (WSEQ:84, 471-484).  Our side's extension:
            # accepted, no target, nothing detected, nothing drawn.
            fr = oracle_mod.synth(1, w, h, ll, layout, kind, seed, first_frame=fidx)
            for auto in (False, True):
                rc, oa, pv = oracle_mod.run(fr, w, h, ll, layout, RANGES[rnames[0]], auto_detect=auto,
                                            out_width=320, out_height=240, out_line_length=640)
                assert rc == 0 and not any(oa.values()) and pv.size == 240 * 640 and not pv.any(), (name, auto)
                empty += 1
            continue
        fr = oracle_mod.synth(1, w, h, ll, layout, kind, seed, first_frame=fidx)
        for r in (rnames if w * h <= 320 * 240 else rnames[:4]):
            _same_run(oracle_mod, fr, w, h, ll, RANGES[r], False, w // 2, h // 2, w, (name, r))
            n += 1
    for name, w, h, ll, layout, kind, seed, fidx, rname, auto, ow, oh, oll in RUN_CASES:
        if layout != LAYOUT_YUYV:
            continue
        fr = oracle_mod.synth(1, w, h, ll, layout, kind, seed, first_frame=fidx)
        _same_run(oracle_mod, fr, w, h, ll, RANGES[rname], bool(auto), ow, oh, oll, name)
        n += 1
    assert n == 1 + 4 + 4 + 12 + 12 + 5 and empty == 2


def test_webcam_object_sensor_corner_targets(oracle_mod, table):
    """The corner-block frames of tests/preview_cases.py (a target in each
    corner, on each edge, in the centre, the whole frame, one pixel, 2 x 2) on
    the 2:1, the 0.625 and the upscaled preview of the GPU tests: the target
    circle's points are clamped to the frame and then mapped (WSEQ:72-134)."""
    n = 0
    for w, h, ow, oh in preview_cases.CIRCLE_GEOMS:
        for rng in (preview_cases.T0, preview_cases.V_BAND):
            for name in preview_cases.PLACES:
                fr = preview_cases.corner_block(table, rng, w, h, 2 * w, LAYOUT_YUYV, name)
                _same_run(oracle_mod, fr, w, h, 2 * w, rng, False, ow, oh, 2 * ow, ((w, h, ow, oh), rng, name))
                n += 1
    assert n == 3 * 2 * 12


def test_webcam_object_sensor_rejects(oracle_mod):
    """setup() and run() refuse what the oracle refuses."""
    n = 0
    for w, h, ll, size in ((48, 4, 96, None), (32, 6, 64, None), (32, 4, 64, 32 * 4 * 2 - 1)):
        fr = np.zeros(h * ll if size is None else size, np.uint8)
        rc = oracle_mod.run(fr, w, h, ll, LAYOUT_YUYV, RANGES["T0"])[0]
        assert rc != 0 and ref_lib.webcam_run(fr, w, h, ll, RANGES["T0"])[0] != 0, (w, h, ll)
        n += 1
    assert n == 3


# ---------------------------------------------------------------- line sensors

def _same_line(oracle_mod, webcam, fr, w, h, ll, vf, vt, band, ow, oh, oll, what):
    if webcam:
        want = oracle_mod.wline_run(fr, w, h, ll, vf, vt, out_width=ow, out_height=oh, out_line_length=oll)
        got = ref_lib.wline_run(fr, w, h, ll, vf, vt, ow, oh, oll)
    else:
        want = oracle_mod.line_run(fr, w, h, ll, vf, vt, band=band, out_width=ow, out_height=oh,
                                   out_line_length=oll)
        got = ref_lib.line_run(fr, w, h, ll, vf, vt, band, ow, oh, oll)
    assert got[0] == want[0] == 0, what
    for k in OUTARGS:
        assert got[1][k] == want[1][k], (what, k, got[1], want[1])
    assert got[3].tolist() == want[3].tolist(), (what, got[3], want[3])
    assert np.array_equal(got[2], want[2]), (what, int(np.flatnonzero(got[2] != want[2])[0]))
    if not webcam:
        assert got[4] == want[4], what


def _line_scenes(w):
    """(seed, x0, slope, line width, valFrom, valTo): position, slope and width
    varied; a line that leaves the frame; no line at all; a frame that matches
    everywhere; an empty range."""
    return [(11, None, 0.25, 24, 0, 30), (12, w // 4, -0.5, 8, 0, 30), (13, 3 * w // 4, 1.5, 40, 0, 30),
            (14, w - 6, 0.75, 24, 0, 30), (15, 2, -0.25, 3, 0, 30), (16, None, 0.0, 0, 0, 30),
            (17, None, 0.25, 24, 0, 100), (18, None, 0.25, 24, 80, 20), (19, 0, 0.0, 1, 0, 12)]


def test_ov7670_line_sensor(oracle_mod):
    """Sums, OutArgs, the band state and every preview byte, on the geometries
    and scenes of tests/test_gpu_line.py plus the scenes above and uniform
    bytes, with the steady band, the (0, 0) band and one that covers all rows."""
    n = 0
    for w, h, ll, ow, oh, oll in gpu_line.GEOMS:
        scenes = [(s, x0, sl, 24, vf, vt) for s, x0, sl, vf, vt in gpu_line.SCENES]
        if (w, h) != (640, 480):
            scenes += _line_scenes(w)
        frames = [(sc, oracle_mod.line_scene(w, h, ll, sc[0], x0=sc[1], slope=sc[2], line_w=sc[3])) for sc in scenes]
        frames.append(((0, None, 0, 0, 20, 70), oracle_mod.synth(1, w, h, ll, LAYOUT_OV7670, 0, 0x11AE)))
        for sc, fr in frames:
            for band in (None, (0, 0), (0, h)):
                _same_line(oracle_mod, False, fr, w, h, ll, sc[4], sc[5], band, ow, oh, oll, ((w, h, ll), sc, band))
                n += 1
    assert n == (2 * 6 + 4 * 15) * 3
    for name, w, h, ll, seed, x0, slope, vf, vt, band, ow, oh, oll in LINE_CASES:
        fr = oracle_mod.line_scene(w, h, ll, seed, x0=x0, slope=slope)
        _same_line(oracle_mod, False, fr, w, h, ll, vf, vt, band, ow, oh, oll, name)
        n += 1
    assert n == 216 + 6


def test_webcam_line_sensor(oracle_mod):
    """The same for the webcam line sensor, on the geometries and scenes of
    tests/test_gpu_wline.py plus the scenes above and uniform bytes."""
    n = 0
    for w, h, ll, ow, oh, oll in gpu_wline.GEOMS:
        scenes = [(s, x0 if x0 is None or x0 < w else w // 3, sl, 24, vf, vt) for s, x0, sl, vf, vt in gpu_wline.SCENES]
        if (w, h) != (640, 480):
            scenes += _line_scenes(w)
        frames = [(sc, oracle_mod.wline_scene(w, h, ll, sc[0], x0=sc[1], slope=sc[2], line_w=sc[3])) for sc in scenes]
        frames.append(((0, None, 0, 0, 20, 70), oracle_mod.synth(1, w, h, ll, LAYOUT_YUYV, 0, 0x11AE)))
        for sc, fr in frames:
            _same_line(oracle_mod, True, fr, w, h, ll, sc[4], sc[5], None, ow, oh, oll, ((w, h, ll), sc))
            n += 1
    assert n == 2 * 7 + 4 * 16


def test_line_sensors_reject(oracle_mod):
    n = 0
    for w, h, ll in ((48, 4, 48), (32, 6, 32)):
        fr = np.zeros(2 * h * ll, np.uint8)
        assert oracle_mod.line_run(fr, w, h, ll, 0, 30)[0] != 0 and ref_lib.line_run(fr, w, h, ll, 0, 30)[0] != 0
        assert oracle_mod.wline_run(fr, w, h, 2 * ll, 0, 30, 16, 2)[0] != 0
        assert ref_lib.wline_run(fr, w, h, 2 * ll, 0, 30, 16, 2)[0] != 0
        n += 2
    assert n == 4


# ------------------------------------------------------ ov7670 multi-blob sensor

def _kept(cluster, w, h):
    """OSEQ:577-580: a cluster (size, sum x, sum y) gives a target and a mark
    only when its size in percent exceeds 4."""
    return target_py(cluster[1], cluster[2], cluster[0], w, h) is not None


def _own_targets(top, targets, w, h, what):
    """OSEQ:575-590: target[i] is what clusters[i] gives, zero when not kept."""
    for i, (c, t) in enumerate(zip(top, targets)):
        t_want = target_py(c[1], c[2], c[0], w, h) or (0, 0, 0)
        assert (t[0], t[1], t[2] & 255) == t_want, (what, i, c, t, t_want)


def _mark_pixels(clusters, w, h, ow, oh):
    """The output pixels (row, column) of drawFatPixel (OSEQ:99-118, 582-585)
    at the centres of the given clusters."""
    wi2wo, hi2ho = mxn_ref.scale_maps(w, h, ow, oh)
    out = set()
    for size, sx, sy in clusters:
        x, y = (sx // (size + 1)) * 4, (sy // (size + 1)) * 4
        for dx in (-1, 0, 1):
            for dy in (-1, 0, 1):
                out.add((hi2ho[min(max(y + dy, 0), h - 1)], wi2wo[min(max(x + dx, 0), w - 1)]))
    return out


def _same_blob(got, want, geom, what):
    """The bitmap, the label map, the label count, the sticky range, the 8
    largest clusters in order, the 8 targets and every preview byte.

    The one divergence: Clusterizer::postProcessing sorts
    with std::sort (CLU:126), which leaves the order of equal sizes to the
    library; the oracle orders them by ascending label.  Returns which of four
    paths the case took, each asserting all that the divergence leaves fixed:
      "equal"     the clusters agree position by position: everything equal;
      "unkept"    the order differs only among clusters that give no target
                  (merged labels of size 0, sizes of at most 4 percent):
                  targets and preview equal;
      "permuted"  clusters that give targets are ordered differently, the same
                  ones on both sides: their targets permute with them, the
                  preview is equal (the marks have one colour);
      "cut"       a tie group of kept clusters is cut at position 8, so the
                  two sides keep different members of it: each side's targets
                  are its own clusters', and the previews differ at most in
                  the 3 x 3 marks of the members only one side kept."""
    w, h, ow, oh, oll = geom
    assert got["rc"] == want["rc"] == 0, what
    assert got["state"] == want["state"], (what, got["state"], want["state"])
    assert np.array_equal(got["meta"], want["meta"]), what
    assert np.array_equal(got["labels"], want["labels"]), what
    assert got["n_labels"] == want["n_labels"], what
    gt, wt = [tuple(t) for t in got["top"].tolist()], [tuple(t) for t in want["top"].tolist()]
    g_tg, w_tg = [tuple(t) for t in got["targets"].tolist()], [tuple(t) for t in want["targets"].tolist()]
    same_preview = np.array_equal(got["preview"], want["preview"])
    if gt == wt:
        assert g_tg == w_tg, what
        assert same_preview, (what, int(np.flatnonzero(got["preview"] != want["preview"])[0]))
        return "equal"
    # sizes agree position by position; within one size both sides hold
    # clusters of the reference with that size, the same ones when the whole
    # group lies inside the first 8
    assert [t[0] for t in gt] == [t[0] for t in wt], (what, gt, wt)
    every = Counter(tuple(t) for t in got["sorted"].tolist())
    every[(0, 0, 0)] += max(0, 8 - got["n_labels"])  # the entries read past the label count
    for size in set(t[0] for t in wt):
        mine, theirs = Counter(t for t in wt if t[0] == size), Counter(t for t in gt if t[0] == size)
        assert not (mine - every) and not (theirs - every), (what, size, mine, theirs)
        if sum(c for t, c in every.items() if t[0] == size) == sum(mine.values()):
            assert mine == theirs, (what, size)
    # targets: each side's target[i] is its own clusters[i]'s, and equal
    # wherever the clusters are
    _own_targets(gt, g_tg, w, h, (what, "reference"))
    _own_targets(wt, w_tg, w, h, (what, "oracle"))
    for i in range(8):
        if gt[i] == wt[i]:
            assert g_tg[i] == w_tg[i], (what, i)
    g_kept = Counter(t for t in gt if _kept(t, w, h))
    w_kept = Counter(t for t in wt if _kept(t, w, h))
    if g_kept == w_kept:
        assert same_preview, (what, int(np.flatnonzero(got["preview"] != want["preview"])[0]))
        if all(gt[i] == wt[i] or not (_kept(gt[i], w, h) or _kept(wt[i], w, h)) for i in range(8)):
            assert g_tg == w_tg, what
            return "unkept"
        assert sorted(zip(gt, g_tg)) == sorted(zip(wt, w_tg)), what
        return "permuted"
    only = list(((g_kept - w_kept) + (w_kept - g_kept)).elements())
    assert len(set(t[0] for t in only)) == 1, (what, only)  # members of the one group cut at position 8
    allowed = _mark_pixels(only, w, h, ow, oh)
    a = got["preview"].reshape(oh, oll)[:, :2 * ow].reshape(oh, ow, 2)
    b = want["preview"].reshape(oh, oll)[:, :2 * ow].reshape(oh, ow, 2)
    differ = set(map(tuple, np.argwhere((a != b).any(axis=2)).tolist()))
    assert differ <= allowed, (what, sorted(differ - allowed)[:4])
    assert np.array_equal(got["preview"].reshape(oh, oll)[:, 2 * ow:], want["preview"].reshape(oh, oll)[:, 2 * ow:])
    return "cut"


def _blob_pair(oracle_mod, fr, w, h, ll, hsv, out=None):
    """(reference result, oracle result, geometry) of one frame."""
    ow, oh, oll = out if out is not None else (w // 2, h // 2, w)
    return (ref_lib.blob_run(fr, w, h, ll, hsv, ow, oh, oll),
            oracle_mod.blob_run(fr, w, h, ll, hsv=hsv, out_width=ow, out_height=oh, out_line_length=oll),
            (w, h, ow, oh, oll))


BLOB_PATTERN_GEOMS = [(6, 80), (12, 160), (9, 136)]  # (bh, bw), as tests/test_oracle_blob.py
# the most cases that may take _same_blob's ("permuted", "cut") paths per geometry
BLOB_PATTERN_TIES = {(6, 80): (2, 0), (12, 160): (1, 0), (9, 136): (1, 1)}


@pytest.mark.parametrize("geom", BLOB_PATTERN_GEOMS, ids=["%dx%d" % g for g in BLOB_PATTERN_GEOMS])
def test_blob_structured_bitmaps(oracle_mod, geom):
    """Every pattern of tests/blob_patterns.py (the label merging), with a
    padded line on the middle geometry."""
    bh, bw = geom
    w, h = 4 * bw, 4 * bh
    ll = w + 32 if bh == 12 else w
    pats = blob_patterns.patterns(bh, bw)
    pats["rand50"] = blob_patterns.rand(bh, bw, 0.5, 50)
    n = 0
    paths = Counter()
    for k, (name, meta) in enumerate(sorted(pats.items())):
        fr = blob_patterns.frame(meta, ll, seed=k)
        got, want, g = _blob_pair(oracle_mod, fr, w, h, ll, oracle_mod.RED_HSV)
        assert np.array_equal(want["meta"], meta), name
        paths[_same_blob(got, want, g, (geom, name))] += 1
        n += 1
    assert n == 18 == sum(paths.values())
    print("paths", geom, dict(paths))
    # the tolerant paths, as many as libstdc++'s order gives: more would widen what is accepted
    assert paths["permuted"] <= BLOB_PATTERN_TIES[geom][0] and paths["cut"] <= BLOB_PATTERN_TIES[geom][1]


def test_blob_scenes_and_dense_bitmaps(oracle_mod):
    """The geometries and cases of tests/test_gpu_blob.py that fit, dense
    random bitmaps at 160 x 120 and 320 x 240, and the golden BLOB_CASES."""
    n = 0
    paths = Counter()
    for w, h, ll in gpu_blob.GEOMS:
        if not fits(w, h):
            continue
        for case, fr in zip(gpu_blob.CASES, gpu_blob._frames(oracle_mod, w, h, ll, gpu_blob.CASES)):
            paths[_same_blob(*_blob_pair(oracle_mod, fr, w, h, ll, gpu_blob.RED), what=((w, h, ll), case))] += 1
            n += 1
    assert n == 5 * 6
    for (w, h), dens in (((160, 120), (0.3, 0.6, 0.9, 1.0)), ((320, 240), (0.45, 0.7, 0.97))):
        for d in dens:
            meta = blob_patterns.rand(h // 4, w // 4, d, int(100 * d))
            fr = blob_patterns.frame(meta, w, seed=int(100 * d))
            paths[_same_blob(*_blob_pair(oracle_mod, fr, w, h, w, oracle_mod.RED_HSV, (w, h, 2 * w)), what=(w, h, d))] += 1
            n += 1
    for name, kind, w, h, ll, seed, noise, dens, hsv, ow, oh, oll in BLOB_CASES:
        if kind == "scene":
            fr = oracle_mod.blob_scene(w, h, ll, seed, noise=noise)
        else:
            meta = (np.random.default_rng(seed).random((h // 4, w // 4)) < dens).astype(np.uint8)
            fr = oracle_mod.blob_frame(meta, ll, seed=seed)
        paths[_same_blob(*_blob_pair(oracle_mod, fr, w, h, ll, hsv, (ow, oh, oll)), what=name)] += 1
        n += 1
    assert n == 30 + 7 + 6 == sum(paths.values())
    print("paths", dict(paths))
    assert paths["permuted"] <= 1 and paths["cut"] <= 1  # more would widen what is accepted


def test_ov7670_multi_blob_corner_targets(oracle_mod, table):
    """The ov7670 counterpart of test_webcam_object_sensor_corner_targets.  The
    reference's ov7670 object sensor is the multi-blob one: it marks its
    targets with 3 x 3 squares and draws no circle, so the clamp-then-map
    circle is held to the reference by the webcam test alone.  The same
    placements as ov7670 frames, with blocks of 16 x 16 pixels (4 x 4
    metapixels, so the corner, edge and centre blocks give kept targets),
    through the multi-blob sensor under the same range in its centre and
    tolerance form, on the same three previews."""
    hsv = (15, 15, 75, 25, 65, 35)  # preview_cases.T0 as from / to: hue 0..30, sat 50..100, val 30..100
    assert oracle_mod.blob_range(hsv) == oracle_mod.pack_range(preview_cases.T0)
    n = marks = 0
    for w, h, ow, oh in preview_cases.CIRCLE_GEOMS:
        if w < 64:
            continue  # (32 x 16 holds 8 x 4 metapixels: no room for the blocks)
        for name in preview_cases.PLACES:
            fr = preview_cases.corner_block(table, preview_cases.T0, w, h, w, LAYOUT_OV7670, name, size=(16, 16))
            got, want, g = _blob_pair(oracle_mod, fr, w, h, w, hsv, out=(ow, oh, 2 * ow))
            assert _same_blob(got, want, g, ((w, h, ow, oh), name)) == "equal"
            marks += int(any(t[2] for t in want["targets"].tolist()))
            n += 1
    assert n == 2 * 12 and marks >= 2 * 9


def test_blob_sequence_keeps_its_range(oracle_mod):
    """One instance over a sequence of frames: setHsvRange changes between
    frames, frames without it keep the range, and an autoDetectHsv call leaves
    the range, the clusters and the preview alone (its detect* outputs come
    from an annealing seeded by the clock and are not compared)."""
    w, h, ll = 320, 240, 352
    frames = [oracle_mod.blob_scene(w, h, ll, 70 + k, noise=0.01 * (k % 3)) for k in range(4)]
    frames.append(oracle_mod.synth(1, w, h, ll, LAYOUT_OV7670, 1, 0x7A1C, first_frame=3))
    steps = [(0, oracle_mod.RED_HSV, False), (1, None, False), (4, (120, 40, 60, 40, 60, 40), False),
             (2, None, False), (4, None, False), (3, (350, 30, 70, 30, 50, 50), False), (0, None, False),
             (1, None, True), (2, (0, 20, 80, 20, 50, 50), True), (3, None, False)]
    state = None
    n = 0
    paths = Counter()
    with ref_lib.BlobSensor(w, h, ll) as sensor:
        for idx, hsv, auto in steps:
            got = sensor.run(frames[idx], hsv, auto)
            want = oracle_mod.blob_run(frames[idx], w, h, ll, hsv=hsv, state=state)
            paths[_same_blob(got, want, (w, h, w // 2, h // 2, w), (idx, hsv, auto))] += 1
            if auto:
                assert all(0 <= v <= 359 for v in got["detect"]), got["detect"]
            state = want["state"]
            n += 1
    assert n == 10 == sum(paths.values())
    print("paths", dict(paths))
    assert paths["permuted"] == 0 and paths["cut"] == 0


def test_blob_rejects(oracle_mod):
    n = 0
    for w, h, ll in ((48, 4, 48), (32, 6, 32)):
        fr = np.zeros(2 * h * ll, np.uint8)
        assert oracle_mod.blob_run(fr, w, h, ll, hsv=oracle_mod.RED_HSV)["rc"] != 0
        assert ref_lib.blob_run(fr, w, h, ll, oracle_mod.RED_HSV)["rc"] != 0
        n += 1
    assert n == 2


# ------------------------------------------------------------------------ MxN

def _same_mxn(table, fr, w, h, ll, m, n, ow, oh, oll, what):
    colors, bins, ties = mxn_ref.run(table, fr, w, h, ll, m, n)
    rc, got, pv = ref_lib.mxn_run(fr, w, h, ll, m, n, ow, oh, oll)
    assert rc == 0, what
    assert got == colors, (what, got, colors)
    want = mxn_ref.preview(table, fr, w, h, ll, m, n, colors, ow, oh, oll)
    assert np.array_equal(pv, want), (what, np.argwhere(pv != want)[0].tolist())
    return bins, ties


GRIDS = [(1, 1), (2, 2), (3, 3), (2, 4), (10, 10), (7, 5)]  # (7, 5) divides neither image
MXN_GEOMS = [((64, 8, 64), [(1, 1), (1, 2), (2, 1), (2, 2)]), ((96, 24, 128), GRIDS), ((320, 240, 320), GRIDS)]


@pytest.mark.parametrize("geom,grids", MXN_GEOMS, ids=["%dx%d_ll%d" % g for g, _ in MXN_GEOMS])
def test_mxn_sensor(oracle_mod, table, geom, grids):
    """outColor and every preview byte: uniform, scene and single-colour frames
    on each grid, with a 2:1 preview."""
    w, h, ll = geom
    cnt = 0
    for name, fr in gpu_mxn.make_frames(oracle_mod, w, h, ll):
        for m, n in grids:
            _same_mxn(table, fr, w, h, ll, m, n, w // 2, h // 2, w + 2, (geom, name, m, n))
            cnt += 1
    assert cnt == 3 * len(grids)


def test_mxn_tie_frames(table):
    """The crafted tie frames of tests/test_gpu_mxn.py: the bin that reaches
    the shared count first wins, in the reference's own loop."""
    color_of = {b: mxn_ref.bin_color(b) for b in range(mxn_ref.N_BINS)}
    cnt = 0
    for fr, (m, n), want in gpu_mxn.crafted_tie_frames(gpu_mxn.yuv_of_bin_map(table)):
        bins, ties = _same_mxn(table, fr, 64, 8, 64, m, n, 32, 4, 64, (m, n))
        assert all(ties) and bins == want
        rc, got, _ = ref_lib.mxn_run(fr, 64, 8, 64, m, n)
        assert rc == 0 and got == [color_of[b] for b in want]
        cnt += len(want)
    assert cnt == 5


def test_mxn_shape_frames(table):
    """The frames of tests/mxn_cases.py, the inputs tests/test_gpu_mxn_shapes.py
    judges the GPU by: every edge, split and whole-frame cell in the
    reference's own loop, and the preview geometries (gaps, overlaps, clamped
    squares, outputs larger than the input) in its own preview pass.  The
    reference gives colours only; the contenders of a cell differ in colour
    from each other and from every other bin of the frame, so the colour of
    the cell names its winner."""
    pal = mxn_cases.Palette(table)
    color_of = {b: mxn_ref.bin_color(b) for b in range(mxn_ref.N_BINS)}
    cnt = 0
    edges = mxn_cases.edge_cases(pal)
    splits, bigs = mxn_cases.split_cases(pal), mxn_cases.big_cases(pal)
    for c in edges + splits + bigs:
        w, h, m, n = c.geom
        k = c.cell[0] * n + c.cell[1]
        if isinstance(c, mxn_cases.EdgeCase):
            win, lose = (c.X, [c.Y, pal.C]) if c.kind == "lead" else (c.Y, [c.X, pal.C])
        elif isinstance(c, mxn_cases.SplitCase):
            win = mxn_ref.winner_sequential(c.bins.reshape(-1).tolist())
            lose = [b for b in set(c.bins.reshape(-1).tolist()) if b != win]
        else:
            win = pal.A if c.name == "big_tie" else pal.C
            lose = [b for b in (pal.A, pal.B, pal.C, pal.noise[0]) if b != win]
        assert all(color_of[b] != color_of[win] for b in lose), c
        bins, _ = _same_mxn(table, pal.frame(c.bins), w, h, w, m, n, w // 2, h // 2, w, c.name)
        assert bins[k] == win, c
        rc, got, _ = ref_lib.mxn_run(pal.frame(c.bins), w, h, w, m, n)
        assert rc == 0 and got[k] == color_of[win], (c, got[k])
        cnt += 1
    for w, h, ll, m, n, ow, oh, oll in mxn_cases.PREVIEW_GEOMS:
        for i in range(mxn_cases.PREVIEW_FRAMES):
            fr = pal.frame(mxn_cases.preview_body(pal, w, h, i), ll)
            _same_mxn(table, fr, w, h, ll, m, n, ow, oh, oll, (w, h, ll, m, n, ow, oh, oll))
            cnt += 1
    assert cnt == len(edges) + len(splits) + len(bigs) + 4 * 2
    assert len(edges) >= 250 and len(splits) == 10 and len(bigs) == 2


def test_mxn_gpu_test_geometries(oracle_mod, table):
    """The grids and previews of tests/test_gpu_mxn.py (GEOMS, PREVIEWS), the
    uniform-byte frame of each (ties decide real cells at 1 x 100)."""
    cnt = 0
    tied = False
    for w, h, ll, m, n in gpu_mxn.GEOMS:
        name, fr = gpu_mxn.make_frames(oracle_mod, w, h, ll)[0]
        _, ties = _same_mxn(table, fr, w, h, ll, m, n, w // 2, h // 2, w, (w, h, ll, m, n))
        tied = tied or ((m, n) == (1, 100) and any(ties))
        cnt += 1
    for w, h, ll, m, n, ow, oh, oll in gpu_mxn.PREVIEWS:
        name, fr = gpu_mxn.make_frames(oracle_mod, w, h, ll)[1]
        _same_mxn(table, fr, w, h, ll, m, n, ow, oh, oll, (w, h, ll, m, n, ow, oh, oll))
        cnt += 1
    assert tied and cnt == 9 + 6


def test_mxn_color_of_every_bin(table):
    """HSVtoRGB through the reference: one single-colour frame per reachable
    bin (the float-then-double conversion of MSEQ:480-517)."""
    yuv = gpu_mxn.yuv_of_bin_map(table)
    cnt = 0
    for b, (y, u, v) in sorted(yuv.items()):
        fr = gpu_mxn.single_colour(32, 4, 32, y, u, v)
        rc, got, _ = ref_lib.mxn_run(fr, 32, 4, 32, 1, 1)
        assert rc == 0 and got == [mxn_ref.bin_color(b)], (b, got)
        cnt += 1
    assert cnt == len(yuv) >= 256


# ----------------------------------------------------------------------- JPEG

def _same_jpeg(oracle_mod, geom, name, q, bw):
    w, h, ll = geom
    fr = jpeg_cases.frames_of(oracle_mod, geom)[name]
    want = jpeg_cases.ref(oracle_mod, geom, name, q, bw)[0]
    got = ref_lib.jpeg_encode(fr, w, h, ll, q, bw)
    assert len(got) == len(want), (geom, name, q, bw, len(got), len(want))
    assert got == want, (geom, name, q, bw, next(i for i in range(len(got)) if got[i] != want[i]))


@pytest.mark.parametrize("geom", jpeg_cases.SMALL, ids=["%dx%d_ll%d" % g for g in jpeg_cases.SMALL])
def test_jpeg_small_cases(oracle_mod, geom):
    """Every stream of jpeg_cases.small_cases() of one geometry, byte for byte.
    96 x 24 has lineLength 128: the reference strides by width and never reads
    lineLength, so it gets the compacted planes, and its stream must equal
    jpeg_ref's on the padded frame (our documented extension)."""
    n = 0
    for g, name, q, bw in jpeg_cases.small_cases():
        if g == geom:
            _same_jpeg(oracle_mod, g, name, q, bw)
            n += 1
    assert n == 8 * 2 * (7 if geom == (64, 64, 64) else 6)


def test_jpeg_mid_cases(oracle_mod):
    n = 0
    for g, name, q, bw in jpeg_cases.mid_cases():
        _same_jpeg(oracle_mod, g, name, q, bw)
        n += 1
    assert n == 24


def test_jpeg_vga_cases(oracle_mod):
    n = 0
    for name, q, bw in jpeg_cases.VGA_CASES:
        _same_jpeg(oracle_mod, jpeg_cases.VGA, name, q, bw)
        n += 1
    assert n == 2


def test_jpeg_padded_line_is_ignored_by_the_reference(oracle_mod):
    """The exact divergence: fed a padded frame as it is, the reference reads
    it with a stride of `width` (JENC:734-752), so its stream is jpeg_ref's of
    the frame's first 2 * w * h bytes taken as unpadded planes."""
    w, h, ll = 96, 24, 128
    fr = jpeg_cases.frames_of(oracle_mod, (w, h, ll))["scene"]
    with ref_lib.Instance("ov7670_jpeg", w, h, ll) as inst:
        out = np.zeros(4 * w * h + 4096, np.uint8)
        n = inst.lib.ref_run(inst.handle, fr.ctypes.data, fr.size, out.ctypes.data, out.size, 75, 0)
    assert 0 < n <= out.size
    assert out[:n].tobytes() == jpeg_ref.encode(fr[:2 * w * h], w, h, w, 75, False)[0]
    assert out[:n].tobytes() != jpeg_ref.encode(fr, w, h, ll, 75, False)[0]
