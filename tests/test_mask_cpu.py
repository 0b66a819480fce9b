"""The detection-mask reference (tests/mask_ref.py) against the oracle, and the
coverage claims of tests/mask_cases.py asserted on the reference's own output:
no GPU.  tests/test_gpu_mask.py compares trik_hsv_mask_batch with the same
reference on the same cases."""
import ctypes as C

import numpy as np
import pytest

import mask_cases as MC
import mask_ref as MR

YUYV, OV7670 = MC.LAYOUT_YUYV, MC.LAYOUT_OV7670
LAYOUTS = [YUYV, OV7670]


def _oracle_planes(oracle_mod, buf, i, ranges):
    """bool [n, T, h, w] from oracle.frame(..., want_mask=True), 8 ranges a call."""
    t = len(ranges[0])
    out = np.zeros((i.n, t, i.h, i.w), bool)
    fb = MC.in_stride(i) - i.stride_pad
    for f in range(i.n):
        frame = buf[i.off + f * MC.in_stride(i):][:fb]
        for g in range(0, t, 8):
            group = [MR.as_inargs(r) for r in ranges[f][g:g + 8]]
            _, m = oracle_mod.frame(frame, i.w, i.h, MC.in_ll(i), i.layout, group, want_mask=True)
            for k in range(len(group)):
                out[f, g + k] = (m >> k) & 1
    return out


# ---- the reference is the oracle's mask -------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("pad", [0, 12])
def test_ref_is_the_oracles_mask(oracle_mod, table, layout, pad):
    """Both layouts, dense and padded line_length, 16 ranges in two groups of 8,
    a rotation per frame."""
    i = MC.In(layout, 96, 8, 4, pad=pad, stride_pad=5, off=3)
    buf = MC.uniform_input(i, 11 + layout)
    ranges = [[MC.EXH_RANGES[(f + k) % 16] for k in range(16)] for f in range(i.n)]
    det = MR.planes(oracle_mod, table, buf[i.off:], MC.in_stride(i), i.n, i.w, i.h, MC.in_ll(i), layout, ranges)
    assert np.array_equal(det, _oracle_planes(oracle_mod, buf, i, ranges))
    assert det.any() and not det.all()


@pytest.mark.parametrize("layout", LAYOUTS)
def test_ref_is_the_oracles_mask_on_the_range_edges(oracle_mod, table, layout):
    """One 320 x 240 scene frame and one of uniform bytes under every edge range
    the oracle's InArgs bytes hold (as_inargs: above 255 is 255)."""
    w, h = 320, 240
    ll = MC.in_ll(MC.In(layout, w, h, 1))
    scene = oracle_mod.synth(1, w, h, ll, layout, 1, 0x7A1C, first_frame=100)
    i = MC.In(layout, w, h, 2)
    buf = np.concatenate([scene, MC.uniform_input(MC.In(layout, w, h, 1), 5)])
    ranges = [MC.EDGE_RANGES] * 2
    det = MR.planes(oracle_mod, table, buf, MC.in_stride(i), 2, w, h, ll, layout, ranges)
    assert np.array_equal(det, _oracle_planes(oracle_mod, buf, i, ranges))
    by = dict(zip(MC.EDGE_RANGES, det[1]))
    assert by[MC.FULL].all() and by[MC.FULL_WRAP].all() and not by[MC.EMPTY_V].any()
    for r in (MC.WRAP_HALF, MC.WRAP_NARROW, MC.FROM_EQ_TO, MC.SV_ABOVE_100, MC.V_ABOVE_255):
        assert by[r].any() and not by[r].all(), r
    # above 255 behaves as 255, and 255 as 100 percent
    assert np.array_equal(by[MC.V_ABOVE_255], MR.detect(oracle_mod, *MR.hsv_of(table, buf[MC.in_stride(i):], 0, 1, w, h,
                                                                           ll, layout), (0, 359, 0, 100, 50, 100))[0])


def test_pack_of_wide_values():
    assert MR.as_inargs((400, 500, 200, 250, 0, 255)) == (400, 500, 200, 250, 0, 255)
    assert MR.as_inargs((0, 359, 0, 65535, 256, 300)) == (0, 359, 0, 255, 255, 255)


def test_layouts_bits_and_bytes():
    det = np.zeros((1, 2, 2, 32), bool)
    det[0, 0, 0, [0, 9, 31]] = True
    det[0, 1, 1, 8] = True
    buf = MR.lay_out(det, MR.BITS, np.full(64, 7, np.uint8), 3, 40, 12, 5)
    assert buf[3:7].tolist() == [0x01, 0x02, 0x00, 0x80] and int(buf[3:7].view("<u4")[0]) == 1 | 1 << 9 | 1 << 31
    assert buf[3 + 12 + 5:3 + 12 + 9].tolist() == [0, 1, 0, 0]
    assert (buf == 7).sum() == 64 - 16
    by = MR.lay_out(det, MR.BYTES, np.full(256, 7, np.uint8), 0, 128, 64, 32)
    assert by[[0, 9, 31]].tolist() == [255] * 3 and by[:32].sum() == 3 * 255 and by[64 + 32 + 8] == 255
    assert (by == 7).sum() == 256 - 128


# ---- the labels ---------------------------------------------------------------------
def test_labels():
    assert [MC.label(r) for r in MC.SMALL_RANGES] == ["mixed", "mixed", "mixed", "full", "empty"]
    assert [MC.label(r) for r in MC.EXH_RANGES].count("pool") == 12
    assert MC.EMPTY_V[4] > MC.EMPTY_V[5] and MC.WRAP_HALF[0] > MC.WRAP_HALF[1]
    assert MC.window(6)[0] > MC.window(6)[1] and len({MC.window(k) for k in range(12)}) == 12


# ---- 1. the exhaustive frames ------------------------------------------------------------
def test_exhaustive_covers_every_triple_under_every_range():
    w, h, n = MC.EXH["w"], MC.EXH["h"], MC.EXH["n"]
    idx = {}
    for layout in LAYOUTS:
        i = MC.In(layout, w, h, n)
        idx[layout] = np.concatenate([MR.CR.gather(MC.exhaustive_frames(layout)[f * MC.in_stride(i):], w, h, MC.in_ll(i),
                                                   layout).reshape(-1) for f in range(n)])
    assert np.array_equal(np.sort(idx[YUYV]), np.arange(1 << 24, dtype=np.uint32))
    assert np.array_equal(idx[YUYV], idx[OV7670])  # the same triple at every pixel: one reference for both
    ranges = MC.exhaustive_ranges()
    assert len(MC.EXH_RANGES) == 16 and all(sorted(r) == sorted(MC.EXH_RANGES) for r in ranges)
    assert ranges[1][0] == MC.EXH_RANGES[1]
    labels = [MC.label(r) for r in MC.EXH_RANGES]
    assert labels.count("full") == 3 and labels.count("empty") == 1
    assert any(r[0] > r[1] for r in MC.EXH_RANGES) and MC.POINT in MC.EXH_RANGES


def test_exhaustive_cases_reach_both_kernels():
    seen = set()
    for case in MC.EXHAUSTIVE:
        i, o = MC.exhaustive_case(*case)
        kernel = MC.form(i, o, 16)
        assert kernel == ("vec" if case[2] == 0 and case[3] == 0 else "generic")
        seen.add((i.layout, o.form, kernel))
    assert len(seen) == 8 and len(MC.EXHAUSTIVE) == 8
    assert {c[2:] for c in MC.EXHAUSTIVE} == {(0, 0), (1, 0), (0, 1)}


# ---- 2. smallest geometries ------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
def test_small_geometries_hold_their_claims(oracle_mod, table, layout):
    shapes = set()
    for k, i in enumerate(MC.small_inputs(layout)):
        ranges = MC.small_ranges(i)
        buf = MC.uniform_input(i, 100 + k)
        det = MR.planes(oracle_mod, table, buf[i.off:], MC.in_stride(i), i.n, i.w, i.h, MC.in_ll(i), layout, ranges)
        MC.check_planes(det, ranges, MC.case_id(i, MC.Out(0)))
        shapes.add((i.w, i.h, i.n))
        for f in MC.FORMS:
            aligned = i.off % 16 == 0 and MC.in_ll(i) % 16 == 0 and (i.n == 1 or MC.in_stride(i) % 16 == 0)
            assert MC.form(i, MC.Out(f), 5) == ("vec" if aligned else "generic")
    assert {(32, 4, 1), (32, 4, 3), (32, 4, 300), (64, 4, 2), (32, 8, 2), (96, 8, 3), (544, 4, 2), (2080, 4, 2)} <= shapes
    kernels = {MC.form(i, MC.Out(0), 5) for i in MC.small_inputs(layout)}
    assert kernels == {"vec", "generic"}


# ---- 3. T ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
def test_t_sets_hold_their_claims(oracle_mod, table, layout):
    assert MC.T_VALUES == (1, 3, 4, 5, 8, 9, 64) and max(MC.T_VALUES) == MC.MAX_RANGES
    i = MC.T_IN[layout]
    buf = MC.uniform_input(i, 40 + layout)
    H, S, V = MR.hsv_of(table, buf, MC.in_stride(i), i.n, i.w, i.h, MC.in_ll(i), layout)
    for t in MC.T_VALUES:
        ranges = MC.t_sets(i.n, t)
        assert all(len(set(r)) == t for r in ranges)
        assert len({tuple(r) for r in ranges}) == (i.n if t < 3 else min(i.n, t))  # another set in every frame
        det = MR.planes(oracle_mod, table, buf, MC.in_stride(i), i.n, i.w, i.h, MC.in_ll(i), layout, ranges)
        MC.check_planes(det, ranges, ("T", t))
        labels = [MC.label(r) for r in ranges[0]]
        assert "mixed" in labels and (t < 3 or ("full" in labels and "empty" in labels))
        # a frame under its neighbour's set would differ, and so would a set read one tuple off
        for f in range(i.n - 1):
            other = MR.planes(oracle_mod, table, buf[f * MC.in_stride(i):], 0, 1, i.w, i.h, MC.in_ll(i), layout,
                              [ranges[f + 1]])
            assert not np.array_equal(other[0], det[f]), (t, f)
        # the padding tuples would change the result if they were read as a range
        assert not np.array_equal(MR.detect(oracle_mod, H[0], S[0], V[0], MC.PAD_RANGE), det[0, 0])
        for f in MC.FORMS:
            assert MC.form(i, MC.Out(f), t) == "vec"
            assert MC.form(i, MC.Out(f, row_pad=1), t) == "generic"


# ---- 4. range edges ---------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
def test_edge_input_holds_its_claims(oracle_mod, table, layout):
    from convert_cases import sentinel

    assert np.array_equal(MC.sentinel(1000), sentinel(1000)) and MC.sentinel(5000).min() == 3
    i = MC.In(layout, 96, 8, 2)
    buf = MC.uniform_input(i, 61 + layout)
    ranges = [MC.EDGE_RANGES] * 2
    det = MR.planes(oracle_mod, table, buf, MC.in_stride(i), i.n, i.w, i.h, MC.in_ll(i), layout, ranges)
    MC.check_planes(det, ranges, "edges")
    labels = [MC.label(r) for r in MC.EDGE_RANGES]
    assert labels.count("mixed") == 3 and labels.count("full") == 2 and labels.count("empty") == 1
    assert any(max(r[2:]) > 255 for r in MC.EDGE_RANGES) and any(100 < max(r[2:]) <= 255 for r in MC.EDGE_RANGES)


# ---- 5. placement ------------------------------------------------------------------------------------
def test_placements_reach_both_kernels_and_every_padding():
    for layout in LAYOUTS:
        i = MC.PITCH_IN[layout]
        for f in MC.FORMS:
            width = 4 if f == MC.BITS else 8
            kernels = {}
            for o in MC.pitch_outs(f):
                _, frame_stride, plane_stride, row_pitch, _ = MC.out_geometry(o, i.w, i.h, i.n, 5)
                aligned = all(v % width == 0 for v in (o.off, frame_stride, plane_stride, row_pitch))
                assert MC.form(i, o, 5) == ("vec" if aligned else "generic"), o
                kernels.setdefault(MC.form(i, o, 5), []).append(o)
            assert len(kernels["vec"]) >= 5 and len(kernels["generic"]) >= 5
            # each padding alone on the vector kernel, and a 4-byte one that only the bits' stores take
            alone = [o for o in kernels["vec"] if sum(1 for v in o[1:] if v) == 1]
            assert {next(k for k, v in enumerate(o[1:]) if v) for o in alone} == {0, 1, 2, 3}
            assert (MC.form(i, MC.Out(f, row_pad=4), 5) == "vec") == (f == MC.BITS)
            assert (MC.form(i, MC.Out(f, off=4), 5) == "vec") == (f == MC.BITS)
    # a single range's plane_stride and a single frame's strides are no addresses
    one = MC.In(YUYV, 96, 8, 1, stride_pad=3)
    assert MC.form(one, MC.Out(MC.BITS, plane_pad=3, frame_pad=1), 1) == "vec"
    assert MC.form(one, MC.Out(MC.BITS, plane_pad=3), 2) == "generic"


@pytest.mark.parametrize("layout", LAYOUTS)
def test_placement_input_holds_its_claims(oracle_mod, table, layout):
    i = MC.PITCH_IN[layout]
    ranges = MC.small_ranges(i)
    buf = MC.uniform_input(i, 7 + layout)
    det = MR.planes(oracle_mod, table, buf, MC.in_stride(i), i.n, i.w, i.h, MC.in_ll(i), layout, ranges)
    MC.check_planes(det, ranges, "placement")


# ---- 6. one-hot columns --------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("width", MC.COLUMN_WIDTHS)
def test_one_hot_columns_are_one_hot(oracle_mod, table, layout, width):
    i = MC.In(layout, width, MC.COLUMN_H, width)
    buf = MC.one_hot_columns(width, layout)
    assert buf.size == MC.in_size(i)
    det = MR.planes(oracle_mod, table, buf, MC.in_stride(i), width, width, MC.COLUMN_H, MC.in_ll(i), layout,
                    [[MC.COLUMN_RANGE]] * width)
    assert np.array_equal(det, MC.one_hot_planes(width))
    bits = MR.dense(det, MR.BITS)
    for c in range(width):
        assert bits[c, 0, 0].tolist() == [1 << (c & 7) if b == c >> 3 else 0 for b in range(width // 8)]
    assert MC.form(i, MC.Out(MC.BITS), 1) == "vec" and MC.form(i, MC.Out(MC.BYTES), 1) == "vec"


# ---- 8. the loop frames ----------------------------------------------------------------------------------
def test_loop_frames_as_planes(oracle_mod):
    v = MC.LOOP
    host = MC.loop_frames(oracle_mod)
    fb = v["h"] * 2 * v["w"]
    twin = MC.ov7670_twin(host[:fb], v["w"], v["h"])
    assert twin.size == fb
    a = MR.CR.gather(host[:fb], v["w"], v["h"], 2 * v["w"], YUYV)
    assert np.array_equal(a, MR.CR.gather(twin, v["w"], v["h"], v["w"], OV7670))


# ---- 9. the C ABI without a GPU -------------------------------------------------------------------------
FAKE = 0x10000  # a non-NULL, 16-byte aligned address nothing reads


@pytest.fixture(scope="module")
def abi():
    from trik_hsv import _abi

    return _abi


def _batch(abi, n=2, w=64, h=8, ll=128, layout=0, stride=None, frames=FAKE):
    return abi.FrameBatch(frames, h * ll * (2 if layout == 1 else 1) if stride is None else stride, n, w, h, ll,
                          layout)


def _out(abi, form=0, w=64, h=8, t=3, out=FAKE, row=None, plane=None, frame=None):
    row = MC.row_bytes(form, w) if row is None else row
    plane = h * row if plane is None else plane
    frame = (t - 1) * plane + h * row if frame is None else frame
    return abi.MaskOut(out, frame, plane, row, form)


def _call(abi, b, o, ranges=FAKE, t=3, stride=18, stream=None):
    return abi.load().trik_hsv_mask_batch(C.byref(b) if b is not None else None, C.c_void_p(ranges), t, stride,
                                          C.byref(o) if o is not None else None, stream)


def refusals(abi):
    """(what, batch or None, out or None, keyword arguments of _call, a word of
    the message): each refusal of the header, one at a time."""
    ok = lambda: _batch(abi)  # noqa: E731
    cases = [("NULL batch", None, _out(abi), {}, "NULL"), ("NULL out", ok(), None, {}, "NULL"),
             ("NULL frames", _batch(abi, frames=None), _out(abi), {}, "frames"),
             ("NULL ranges", ok(), _out(abi), dict(ranges=None), "ranges"),
             ("NULL out->out", ok(), _out(abi, out=None), {}, "out->out"),
             ("unknown layout", _batch(abi, layout=2), _out(abi), {}, "layout"),
             ("form 2", ok(), _out(abi, form=2), {}, "form"), ("form -1", ok(), _out(abi, form=-1), {}, "form"),
             ("no range", ok(), _out(abi, t=1), dict(t=0, stride=0), "n_ranges"),
             ("negative n_ranges", ok(), _out(abi, t=1), dict(t=-1, stride=0), "n_ranges"),
             ("65 ranges", ok(), _out(abi, t=65), dict(t=65, stride=0), "n_ranges"),
             ("ranges stride 1", ok(), _out(abi), dict(stride=1), "ranges_frame_stride"),
             ("ranges stride 6 T - 1", ok(), _out(abi), dict(stride=17), "ranges_frame_stride"),
             ("ranges stride -6 T", ok(), _out(abi), dict(stride=-18), "ranges_frame_stride"),
             ("ranges stride -1", ok(), _out(abi), dict(stride=-1), "ranges_frame_stride")]
    for what, bad in (("width % 32", _batch(abi, w=33)), ("height % 4", _batch(abi, h=6)),
                      ("negative width", _batch(abi, w=-32)), ("short line_length", _batch(abi, ll=127)),
                      ("short ov7670 line_length", _batch(abi, layout=1, ll=63)),
                      ("short frame_stride", _batch(abi, stride=8 * 128 - 1)), ("n_frames < 0", _batch(abi, n=-1)),
                      ("width past int16", _batch(abi, w=32768, ll=65536))):
        cases.append((what, bad, _out(abi, w=bad.width, h=bad.height), {}, ""))
    for f in MC.FORMS:
        rb = MC.row_bytes(f, 64)
        cases += [(f"row_pitch form {f}", ok(), _out(abi, f, row=rb - 1, plane=8 * rb, frame=24 * rb), {}, "row_pitch"),
                  (f"negative row_pitch form {f}", ok(), _out(abi, f, row=-rb, plane=8 * rb, frame=24 * rb), {}, "row_pitch"),
                  (f"plane_stride form {f}", ok(), _out(abi, f, plane=8 * rb - 1, frame=24 * rb), {}, "plane_stride"),
                  (f"planes interleaved by rows form {f}", ok(), _out(abi, f, row=3 * rb, plane=rb, frame=24 * rb), {},
                   "plane_stride"),
                  (f"frame_stride form {f}", ok(), _out(abi, f, frame=24 * rb - 1), {}, "frame_stride"),
                  (f"frame_stride of one frame form {f}", _batch(abi, n=1), _out(abi, f, frame=24 * rb - 1), {},
                   "frame_stride"),
                  (f"frame_stride below padded planes form {f}", ok(), _out(abi, f, plane=8 * rb + 16, frame=24 * rb + 31),
                   {}, "frame_stride"),
                  (f"plane_stride past int64 form {f}", ok(), _out(abi, f, plane=1 << 62, frame=(1 << 63) - 1), {},
                   "frame_stride")]
    return cases


def test_mask_batch_refuses(abi):
    seen = set()
    for what, b, o, kw, word in refusals(abi):
        rc = _call(abi, b, o, **kw)
        assert rc != 0, what
        msg = abi.last_error()
        assert msg and word in msg, (what, msg)
        seen.add(what)
    assert len(seen) == 15 + 8 + 2 * 8


def test_mask_batch_degenerate_calls_touch_nothing(abi):
    """n_frames == 0, and width or height 0, return 0 before any GPU call
    (there is no GPU here, and the addresses are not memory)."""
    for f in MC.FORMS:
        assert _call(abi, _batch(abi, n=0, frames=None), _out(abi, f, out=None), ranges=None) == 0
        assert _call(abi, _batch(abi, n=0), _out(abi, f)) == 0
        assert _call(abi, _batch(abi, w=0, ll=0, stride=0), _out(abi, f, w=0)) == 0
        assert _call(abi, _batch(abi, h=0, stride=0), _out(abi, f, h=0), stride=0) == 0


def test_library_exports_mask_batch(abi):
    args, res = abi.PROTOTYPES["trik_hsv_mask_batch"]
    assert len(args) == 6 and res is C.c_int32
    assert hasattr(abi.load(), "trik_hsv_mask_batch")
    assert C.sizeof(abi.MaskOut) == 32 and abi.MaskOut.row_pitch.offset == 24 and abi.MaskOut.form.offset == 28
    import trik_hsv

    assert callable(trik_hsv.mask_batch)
    assert (trik_hsv.MASK_BITS, trik_hsv.MASK_BYTES) == (0, 1) == (MC.BITS, MC.BYTES)
    assert abi.MAX_RANGES == MC.MAX_RANGES


def test_struct_layout_matches_c(abi, tmp_path):
    import os
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "trik_hsv.h"\nint main(void){\n'
                   '  printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(TrikHsvMaskOut), offsetof(TrikHsvMaskOut, out),\n'
                   '         offsetof(TrikHsvMaskOut, frame_stride), offsetof(TrikHsvMaskOut, plane_stride),\n'
                   '         offsetof(TrikHsvMaskOut, row_pitch), offsetof(TrikHsvMaskOut, form));\n'
                   '  printf("%d %d %d\\n", TRIK_HSV_MASK_BITS, TRIK_HSV_MASK_BYTES, TRIK_HSV_MAX_RANGES);\n'
                   '  return 0;\n}\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(root, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    m = abi.MaskOut
    assert [int(x) for x in out[:6]] == [C.sizeof(m), m.out.offset, m.frame_stride.offset, m.plane_stride.offset,
                                         m.row_pitch.offset, m.form.offset]
    assert [int(x) for x in out[6:]] == [abi.MASK_BITS, abi.MASK_BYTES, abi.MAX_RANGES]
