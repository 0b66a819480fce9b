"""Generate tests/golden/reference_golden.json from the REFERENCE's own code.

Run from the repo root, with a reference checkout present (oracle/ref builds
it on the host):  python tests/golden/make_reference_golden.py

oracle_golden.json is written by our restatements; this file is written by the
reference's algorithm classes (setup() + run(), driven through tests/ref_lib.py)
and is what tests/test_gpu_reference.py holds the GPU against on a machine
that has no reference.  Inputs are regenerated from generator, seed and frame
index or from a named pattern, not stored.  Per case the file holds the
sha256 of the input frame (pins the generator), the OutArgs integers, and the
length and sha256 of the preview or JPEG stream -- hashes only, no images.

About eight cases per codec, each list with the smallest geometry, a ragged
lineLength and a 320 x 240 frame; the JPEG list with an aligned tail, stuffed
bytes, a ZRL code and a non-zero coefficient 63 (tests/test_reference_golden.py
asserts those shapes).  The multi-blob rows hold only what the reference
specifies (blob_out below: the order of equal-sized clusters is not).  The
generator refuses to write a case on which the restatement and the reference
still differ -- for the multi-blob sensor that is a tie group of kept clusters
cut at position 8, where the previews differ: such a case belongs in
tests/test_reference_cpu.py.
"""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (os.path.join(HERE, ".."), os.path.join(HERE, "..", "..", "oracle")):
    if os.path.abspath(_p) not in [os.path.abspath(q) for q in sys.path]:
        sys.path.insert(0, os.path.abspath(_p))
import blob_patterns  # noqa: E402
import jpeg_cases  # noqa: E402
import jpeg_ref  # noqa: E402
import mxn_ref  # noqa: E402
import oracle as O  # noqa: E402
from golden.make_golden import RANGES  # noqa: E402

OUT_PATH = os.path.join(HERE, "reference_golden.json")
RED = (0, 20, 80, 20, 50, 50)

# webcam object sensor: name, w, h, ll, kind, seed, frame, range, auto, ow, oh, oll
OBJECT = [
    ("obj_32x4_uniform_T0", 32, 4, 64, 0, 1, 0, "T0", 0, 16, 2, 32),
    ("obj_64x16_ragged_scene_T3_auto", 64, 16, 160, 1, 0x7A1C, 3, "T3_wrap", 1, 32, 8, 70),
    ("obj_160x120_scene_T1_auto", 160, 120, 320, 1, 0x7A1C, 3, "T1", 1, 80, 60, 166),
    ("obj_320x240_scene_T0_auto", 320, 240, 640, 1, 0x7A1C, 3, "T0", 1, 160, 120, 320),
    ("obj_320x240_uniform_full_scale0.625", 320, 240, 640, 0, 0x7A1C, 2, "full", 0, 200, 150, 401),
    ("obj_320x240_scene_empty_point_no_circle", 320, 240, 640, 1, 3, 1, "empty_point", 1, 160, 120, 320),
    ("obj_320x240_scene_wrap_359_0", 320, 240, 704, 1, 7, 0, "wrap_359_0", 0, 160, 120, 320),
    ("obj_320x240_scene_grey_auto", 320, 240, 640, 1, 7, 5, "grey", 1, 160, 120, 320),
]

# ov7670 line sensor: name, w, h, ll, seed, x0, slope, line width, valFrom, valTo, band, ow, oh, oll
LINE = [
    ("line_64x8_edge", 64, 8, 64, 4, 2, 0.0, 24, 0, 30, None, 32, 4, 64),
    ("line_320x240_ragged_steady", 320, 240, 352, 1, None, 0.25, 24, 0, 30, None, 160, 120, 320),
    ("line_320x240_leaves_frame", 320, 240, 320, 14, 314, 0.75, 24, 0, 30, None, 200, 150, 401),
    ("line_320x240_no_line", 320, 240, 320, 16, None, 0.0, 0, 0, 30, None, 160, 120, 320),
    ("line_320x240_all_match", 320, 240, 320, 17, None, 0.25, 24, 0, 100, None, 160, 120, 320),
    ("line_320x240_empty_range", 320, 240, 324, 18, None, 0.25, 24, 80, 20, None, 160, 120, 320),
    ("line_320x240_band_0_0", 320, 240, 320, 2, 30, -0.5, 24, 0, 30, (0, 0), 160, 120, 320),
    ("line_320x240_portrait_bright", 320, 240, 384, 3, 40, 0.0, 24, 50, 100, None, 240, 320, 480),
]

# webcam line sensor: name, w, h, ll, seed, x0, slope, line width, valFrom, valTo, ow, oh, oll
WLINE = [
    ("wline_64x8_edge", 64, 8, 128, 5, 2, 0.0, 24, 0, 100, 32, 4, 64),
    ("wline_320x240_ragged_steady", 320, 240, 704, 1, None, 0.25, 24, 0, 30, 160, 120, 320),
    ("wline_320x240_leaves_frame", 320, 240, 640, 14, 314, 0.75, 24, 0, 30, 200, 150, 401),
    ("wline_320x240_no_line", 320, 240, 640, 16, None, 0.0, 0, 0, 30, 160, 120, 320),
    ("wline_320x240_all_match", 320, 240, 640, 17, None, 0.25, 24, 0, 100, 320, 240, 640),
    ("wline_320x240_empty_range", 320, 240, 640, 18, None, 0.25, 24, 80, 20, 160, 120, 320),
    ("wline_320x240_thin_dark", 320, 240, 640, 6, 300, 0.1, 3, 0, 12, 160, 120, 320),
    ("wline_320x240_portrait", 320, 240, 640, 2, 30, -0.5, 24, 0, 30, 240, 320, 480),
]

# ov7670 multi-blob sensor: name, source, w, h, ll, seed, arg, hsv, ow, oh, oll;
# source "scene" (arg = noise), "pattern" (arg = a name of blob_patterns), "rand" (arg = density)
BLOB = [
    ("blob_32x4_full", "pattern", 32, 4, 32, 1, "full", RED, 16, 2, 32),
    ("blob_320x240_ragged_two_discs", "scene", 320, 240, 352, 1, 0.0, RED, 160, 120, 320),
    ("blob_320x240_discs_salt", "scene", 320, 240, 320, 2, 0.01, RED, 200, 150, 401),
    ("blob_320x24_comb_up", "pattern", 320, 24, 320, 3, "comb_up", RED, 160, 12, 320),
    ("blob_320x24_serpentine", "pattern", 320, 24, 320, 4, "serpentine", RED, 160, 12, 320),
    ("blob_320x24_vees", "pattern", 320, 24, 352, 5, "vees", RED, 160, 12, 320),
    ("blob_320x240_dense_tie_of_16", "rand", 320, 240, 320, 6, 0.7, RED, 160, 120, 320),
    ("blob_320x240_no_match", "scene", 320, 240, 320, 6, 0.0, (180, 10, 50, 10, 50, 10), 160, 120, 320),
]

# ov7670 MxN sensor: name, w, h, ll, content, m, n, ow, oh, oll; content
# "uniform" / "scene" / "single" (tests/test_gpu_mxn.py make_frames) or "tie4" /
# "tie1" (its crafted tie frames)
MXN = [
    ("mxn_64x8_tie_2x2", 64, 8, 64, "tie4", 2, 2, 32, 4, 64),
    ("mxn_64x8_tie_1x1", 64, 8, 64, "tie1", 1, 1, 32, 4, 64),
    ("mxn_96x24_ragged_scene_3x3", 96, 24, 128, "scene", 3, 3, 48, 12, 100),
    ("mxn_96x24_ragged_uniform_7x5", 96, 24, 128, "uniform", 7, 5, 96, 24, 192),
    ("mxn_320x240_scene_3x3", 320, 240, 320, "scene", 3, 3, 160, 120, 320),
    ("mxn_320x240_uniform_10x10", 320, 240, 320, "uniform", 10, 10, 160, 120, 320),
    ("mxn_320x240_scene_2x4_portrait", 320, 240, 320, "scene", 2, 4, 240, 320, 480),
    ("mxn_320x240_single_1x1", 320, 240, 352, "single", 1, 1, 160, 120, 331),
]

# ov7670 JPEG encoder: name, (w, h, ll), content of tests/jpeg_cases.py, quality, black and white
JPEG = [
    ("jpeg_32x8_uniform_q75", (32, 8, 32), "uniform", 75, False),
    ("jpeg_32x8_checker_q75_aligned_tail", (32, 8, 32), "checker", 75, False),
    ("jpeg_96x24_ragged_scene_q50", (96, 24, 128), "scene", 50, False),
    ("jpeg_64x64_basis_q50_bw_zrl_coef63", (64, 64, 64), "basis", 50, True),
    ("jpeg_64x64_checker_q100_stuffed", (64, 64, 64), "checker", 100, False),
    ("jpeg_64x16_uniform_q1", (64, 16, 64), "uniform", 1, False),
    ("jpeg_320x240_scene_q50", (320, 240, 320), "scene", 50, False),
    ("jpeg_320x240_uniform_q100_bw", (320, 240, 320), "uniform", 100, True),
]

CODECS = {"object": OBJECT, "line": LINE, "wline": WLINE, "blob": BLOB, "mxn": MXN, "jpeg": JPEG}

_cache = {}


def table():
    if "table" not in _cache:
        _cache["table"] = O.yuv_table(closed=False)
    return _cache["table"]


def frame(codec, case):
    """The input frame of a case (uint8, flat)."""
    if codec == "object":
        name, w, h, ll, kind, seed, fidx = case[:7]
        return O.synth(1, w, h, ll, O.LAYOUT_YUYV, kind, seed, first_frame=fidx)
    if codec in ("line", "wline"):
        name, w, h, ll, seed, x0, slope, lw = case[:8]
        scene = O.line_scene if codec == "line" else O.wline_scene
        return scene(w, h, ll, seed, x0=x0, slope=slope, line_w=lw)
    if codec == "blob":
        name, source, w, h, ll, seed, arg = case[:7]
        if source == "scene":
            return O.blob_scene(w, h, ll, seed, noise=arg)
        meta = blob_patterns.patterns(h // 4, w // 4)[arg] if source == "pattern" else \
            blob_patterns.rand(h // 4, w // 4, arg, seed)
        return blob_patterns.frame(meta, ll, seed=seed)
    if codec == "mxn":
        import test_gpu_mxn as gm

        name, w, h, ll, content = case[:5]
        if content in ("tie4", "tie1"):
            ties = gm.crafted_tie_frames(gm.yuv_of_bin_map(table()))
            return ties[0 if content == "tie4" else 1][0]
        return dict(gm.make_frames(O, w, h, ll))[content]
    name, geom, content = case[:3]
    return jpeg_cases.frames_of(O, geom)[content]


UNSPECIFIED = -1


def blob_out(top, targets, n_labels):
    """The 8 largest clusters (size, sum x, sum y) and the 8 targets as the
    fixture records them: only what the reference specifies.  It orders equal
    sizes by std::sort (CLU:126), which specifies no order among them, so
      * a run of equal sizes is recorded in a canonical order (its (cluster,
        target) pairs sorted), whatever order a library or a port gives it;
      * entries of size 0 (labels merged into another, which keep their sums)
        give no target and have their sums recorded as 0;
      * with more than 8 clusters the last run may continue past position 8,
        so which of its members are seen is unspecified: its sums and targets
        are recorded as UNSPECIFIED (sizes stay)."""
    t = np.asarray(top, np.int64).reshape(8, 3)
    g = np.asarray(targets, np.int64).reshape(8, -1)[:, :3]
    rows = [(tuple(int(v) for v in t[i]), tuple(int(v) for v in g[i])) for i in range(8)]
    rows = [((0, 0, 0), tg) if c[0] == 0 else (c, tg) for c, tg in rows]
    out = []
    i = 0
    while i < 8:
        j = i
        while j < 8 and rows[j][0][0] == rows[i][0][0]:
            j += 1
        run = sorted(rows[i:j])
        if j == 8 and int(n_labels) > 8 and rows[i][0][0] > 0:
            run = [((c[0], UNSPECIFIED, UNSPECIFIED), (UNSPECIFIED,) * 3) for c, _ in run]
        out += run
        i = j
    return {"targets": [v for _, tg in out for v in tg], "top": [v for c, _ in out for v in c],
            "n_labels": [int(n_labels)]}


def restated(codec, case, fr):
    """(named OutArgs integers, preview or JPEG bytes) by our restatements."""
    if codec == "object":
        name, w, h, ll, _, _, _, rname, auto, ow, oh, oll = case
        rc, oa, pv = O.run(fr, w, h, ll, O.LAYOUT_YUYV, RANGES[rname], bool(auto), ow, oh, oll)
        assert rc == 0, name
        out = {"target": [oa["target_x"], oa["target_y"], oa["target_size"]]}
        if auto:
            out["detect"] = [oa[k] for k in ("detect_hue", "detect_hue_tol", "detect_sat", "detect_sat_tol",
                                             "detect_val", "detect_val_tol")]
        return out, pv.tobytes()
    if codec == "line":
        name, w, h, ll, _, _, _, _, vf, vt, band, ow, oh, oll = case
        rc, oa, pv, sums, _ = O.line_run(fr, w, h, ll, vf, vt, band=band, out_width=ow, out_height=oh,
                                         out_line_length=oll)
        assert rc == 0, name
        return {"target": [oa["target_x"], oa["target_y"], oa["target_size"]], "sums": sums.tolist()}, pv.tobytes()
    if codec == "wline":
        name, w, h, ll, _, _, _, _, vf, vt, ow, oh, oll = case
        rc, oa, pv, sums = O.wline_run(fr, w, h, ll, vf, vt, ow, oh, oll)
        assert rc == 0, name
        return {"target": [oa["target_x"], oa["target_y"], oa["target_size"]], "sums": sums.tolist()}, pv.tobytes()
    if codec == "blob":
        name, _, w, h, ll, _, _, hsv, ow, oh, oll = case
        r = O.blob_run(fr, w, h, ll, hsv=hsv, out_width=ow, out_height=oh, out_line_length=oll)
        assert r["rc"] == 0, name
        return blob_out(r["top"], r["targets"], r["n_labels"]), r["preview"].tobytes()
    if codec == "mxn":
        name, w, h, ll, _, m, n, ow, oh, oll = case
        colors = mxn_ref.run(table(), fr, w, h, ll, m, n)[0]
        pv = mxn_ref.preview(table(), fr, w, h, ll, m, n, colors, ow, oh, oll)
        return {"colors": [int(c) for c in colors]}, pv.tobytes()
    name, (w, h, ll), _, q, bw = case
    data = jpeg_ref.encode(fr, w, h, ll, q, bw)[0]
    return {"size": [len(data)]}, data


def referenced(codec, case, fr):
    """The same by the reference's own classes (needs the host build)."""
    import ref_lib as R

    if codec == "object":
        name, w, h, ll, _, _, _, rname, auto, ow, oh, oll = case
        rc, oa, pv = R.webcam_run(fr, w, h, ll, RANGES[rname], bool(auto), ow, oh, oll)
        assert rc == 0, name
        out = {"target": [oa["target_x"], oa["target_y"], oa["target_size"]]}
        if auto:
            out["detect"] = [oa[k] for k in R.DETECT_KEYS]
        return out, pv.tobytes()
    if codec == "line":
        name, w, h, ll, _, _, _, _, vf, vt, band, ow, oh, oll = case
        rc, oa, pv, sums, _ = R.line_run(fr, w, h, ll, vf, vt, band, ow, oh, oll)
        assert rc == 0, name
        return {"target": [oa[k] for k in R.OUTARG_KEYS], "sums": sums.tolist()}, pv.tobytes()
    if codec == "wline":
        name, w, h, ll, _, _, _, _, vf, vt, ow, oh, oll = case
        rc, oa, pv, sums = R.wline_run(fr, w, h, ll, vf, vt, ow, oh, oll)
        assert rc == 0, name
        return {"target": [oa[k] for k in R.OUTARG_KEYS], "sums": sums.tolist()}, pv.tobytes()
    if codec == "blob":
        name, _, w, h, ll, _, _, hsv, ow, oh, oll = case
        r = R.blob_run(fr, w, h, ll, hsv, ow, oh, oll)
        assert r["rc"] == 0, name
        return blob_out(r["top"], r["targets"], r["n_labels"]), r["preview"].tobytes()
    if codec == "mxn":
        name, w, h, ll, _, m, n, ow, oh, oll = case
        rc, colors, pv = R.mxn_run(fr, w, h, ll, m, n, ow, oh, oll)
        assert rc == 0, name
        return {"colors": colors}, pv.tobytes()
    name, (w, h, ll), _, q, bw = case
    data = R.jpeg_encode(fr, w, h, ll, q, bw)
    return {"size": [len(data)]}, data


def record(case, fr, out, stream):
    return {"name": case[0], "frame_sha256": hashlib.sha256(np.ascontiguousarray(fr).tobytes()).hexdigest(),
            "out": out, "stream_len": len(stream), "stream_sha256": hashlib.sha256(stream).hexdigest()}


def main():
    import ref_lib as R

    if not R.available() or not R._state.get("tree"):
        raise SystemExit("needs a reference checkout ($TRIK_REFERENCE): the values come from its code")
    doc = {"generator": "tests/golden/make_reference_golden.py",
           "source": "the reference's algorithm classes, built on the host by oracle/ref/Makefile"}
    for codec, cases in CODECS.items():
        rows = []
        for case in cases:
            fr = frame(codec, case)
            got = record(case, fr, *referenced(codec, case, fr))
            ours = record(case, fr, *restated(codec, case, fr))
            assert got == ours, ("the restatement and the reference differ", codec, case[0], got, ours)
            rows.append(got)
        doc[codec] = rows
    with open(OUT_PATH, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", sum(len(c) for c in CODECS.values()), "cases,", os.path.getsize(OUT_PATH), "bytes")


if __name__ == "__main__":
    main()
