"""CPU-only checks of the colour conversion: tests/convert_ref.py against the
oracle's per-pixel code and against oracle.frame's masks; the claims of
tests/convert_cases.py, stated on the reference output; every argument the C
ABI refuses, refused before any GPU call (no pointer is dereferenced on the
host); the library's export and the Python surface."""
import ctypes as C

import numpy as np
import pytest

import convert_cases as CC
import convert_ref as CR

FAKE = 0x10000  # a non-NULL, 16-byte aligned address nothing reads


@pytest.fixture(scope="module")
def abi():
    from trik_hsv import _abi

    return _abi


# ---- convert_ref against the oracle -------------------------------------------
def _small_frame(layout, w, h, seed, pad=0):
    i = CC.In(layout, w, h, 1, pad=pad)
    return i, CC.uniform_input(i, seed)


@pytest.mark.parametrize("layout", [CC.LAYOUT_YUYV, CC.LAYOUT_OV7670])
@pytest.mark.parametrize("size", [(32, 4, 0), (64, 8, 0), (64, 8, 12)])
def test_ref_is_the_oracles_pixel_code(oracle_mod, table, layout, size):
    """Every pixel: RGB from trik_oracle_pair_rgb_c64x on the pixel's YUYV word,
    HSV from trik_oracle_hsv_c64x on that RGB."""
    w, h, pad = size
    i, buf = _small_frame(layout, w, h, 7 * w + h + layout, pad)
    ent = CR.entries(table, buf, CC.in_stride(i), 1, w, h, CC.in_ll(i), layout)[0]
    idx = CR.gather(buf, w, h, CC.in_ll(i), layout)
    for r in range(h):
        for c in range(0, w, 2):
            y0, y1 = int(idx[r, c]) & 255, int(idx[r, c + 1]) & 255
            u, v = (int(idx[r, c]) >> 8) & 255, int(idx[r, c]) >> 16
            assert (int(idx[r, c + 1]) >> 8) == (int(idx[r, c]) >> 8)  # a pair shares its chroma
            rgb = oracle_mod.pair_rgb(y0 | (u << 8) | (y1 << 16) | (v << 24))
            for k in (0, 1):
                hsv = oracle_mod.lib().trik_oracle_hsv_c64x(rgb[k])
                assert int(ent[r, c + k]) == (rgb[k] << 32) | hsv, (r, c + k)
    # the raw bytes of the gather, restated: packed words, or planes with V even / U odd
    ll = CC.in_ll(i)
    for r, c in ((0, 0), (1, 5), (h - 1, w - 1), (2, w - 2)):
        if layout == CC.LAYOUT_YUYV:
            p = r * ll + 4 * (c // 2)
            want = int(buf[p + 2 * (c % 2)]) | (int(buf[p + 1]) << 8) | (int(buf[p + 3]) << 16)
        else:
            cr = h * ll + r * ll
            want = int(buf[r * ll + c]) | (int(buf[cr + (c | 1)]) << 8) | (int(buf[cr + (c & ~1)]) << 16)
        assert int(idx[r, c]) == want


@pytest.mark.parametrize("layout", [CC.LAYOUT_YUYV, CC.LAYOUT_OV7670])
@pytest.mark.parametrize("size", [(32, 4), (64, 8)])
def test_ref_is_what_the_oracles_frame_detects(oracle_mod, table, layout, size):
    """Through oracle.frame: under the point range of one pixel's own H, S, V
    (as InArgs numbers that scale back to those bytes) the mask is set exactly
    where convert_ref's HSV equals that pixel's."""
    w, h = size
    i, buf = _small_frame(layout, w, h, 31 * w + layout)
    ent = CR.entries(table, buf, CC.in_stride(i), 1, w, h, CC.in_ll(i), layout)[0]
    hsv = (ent & np.uint64(0xFFFFFF)).astype(np.uint32)

    def unscale(b, full):  # the InArgs value that (v * 255) / full maps to b, or None
        v = -(-b * full // 255)
        return v if v * 255 // full == b else None

    # InArgs saturation and value have 101 steps: the pixels whose S and V bytes one of them maps to
    # (every H byte has a hue), the first five in raster order
    points = [(r, c) for r in range(h) for c in range(w)
              if None not in (unscale((int(hsv[r, c]) >> 8) & 255, 100), unscale(int(hsv[r, c]) >> 16, 100))][:5]
    assert len(points) == 5 and all(unscale(b, 359) is not None for b in range(256))
    checked = 0
    for r, c in points:
        e = int(hsv[r, c])
        H, S, V = e & 255, (e >> 8) & 255, e >> 16
        rng = (unscale(H, 359), unscale(H, 359), unscale(S, 100), unscale(S, 100), unscale(V, 100), unscale(V, 100))
        f, t, x = oracle_mod.pack_range(rng)
        assert (f, t, x) == (e, e, 0)
        _, mask = oracle_mod.frame(buf, w, h, CC.in_ll(i), layout, [rng], want_mask=True)
        assert np.array_equal(mask != 0, hsv == e) and mask[r, c]
        checked += 1
    assert checked == 5


def test_planes_and_dense_forms(table):
    ent = table[np.array([[[0x123456, 0xFFFFFF, 0, 0x80FF10]]])]
    e = [int(x) for x in ent[0, 0]]
    hp, rp = CR.planes(ent, CR.HSV_PLANES), CR.planes(ent, CR.RGB_PLANES)
    assert hp.shape == rp.shape == (1, 3, 1, 4) and hp.dtype == np.uint8
    for k, x in enumerate(e):
        assert hp[0, :, 0, k].tolist() == [x & 255, (x >> 8) & 255, (x >> 16) & 255]
        assert rp[0, :, 0, k].tolist() == [(x >> 48) & 255, (x >> 40) & 255, (x >> 32) & 255]
        assert x >> 56 == 0 and (x >> 24) & 255 == 0
    assert CR.dense(ent, CR.RGB888HSV).dtype == np.int64 and CR.dense(ent, CR.RGB888HSV).tolist() == [[e]]


# ---- the case lists' claims -------------------------------------------------
def test_exhaustive_set_holds_every_triple_in_each_pixel_position():
    """Over the 64 frames, pixel 0 of a word takes every even Y with every
    (U, V) and pixel 1 every odd Y; the set and its twin hold each of the 2^24
    triples exactly once, so each word position meets its half, and the
    conversion of a pixel does not depend on its position (one table)."""
    w, h, n = CC.EXH["w"], CC.EXH["h"], CC.EXH["n"]
    for layout in (CC.LAYOUT_YUYV, CC.LAYOUT_OV7670):
        host = CC.exhaustive_frames(layout)
        ll = CC.row_bytes(w, layout)
        stride = CC.frame_bytes(w, h, ll, layout)
        assert host.size == n * stride
        idx = np.stack([CR.gather(host[f * stride:], w, h, ll, layout) for f in range(n)])
        assert ((idx[..., 0::2] & 1) == 0).all() and ((idx[..., 1::2] & 1) == 1).all()
        assert (np.bincount(idx.reshape(-1), minlength=1 << 24) == 1).all()


def test_exhaustive_cases_take_their_kernels():
    kinds = [CC.form(*CC.exhaustive_case(*c)) for c in CC.EXHAUSTIVE]
    assert kinds == ["vec"] * 6 + ["generic"] * 4
    assert {(c[0], c[1]) for c in CC.EXHAUSTIVE[:6]} == {(l, f) for l in (0, 1) for f in CC.FORMS}
    assert sorted((c[1], bool(c[2]), bool(c[3])) for c in CC.EXHAUSTIVE[6:]) == \
        [(CC.RGB888HSV, False, True), (CC.RGB888HSV, True, False), (CC.HSV_PLANES, False, True),
         (CC.HSV_PLANES, True, False)]


def test_ov7670_cases_tell_the_chroma_order_and_the_lumas(table):
    """Every ov7670 input of the small and pitch cases changes its output when
    U and V are swapped, and when pixel 1 of a pair takes pixel 0's luma."""
    for k, i in enumerate(CC.small_inputs(CC.LAYOUT_OV7670) + [CC.PITCH_IN[CC.LAYOUT_OV7670]]):
        buf = CC.uniform_input(i, 100 + k)
        ll, st = CC.in_ll(i), CC.in_stride(i)
        ent = CR.entries(table, buf[i.off:], st, i.n, i.w, i.h, ll, i.layout)
        for f in range(i.n):
            fr = buf[i.off + f * st:i.off + f * st + CC.frame_bytes(i.w, i.h, ll, i.layout)]
            swapped, same_luma = fr.copy(), fr.copy()
            for r in range(i.h):
                c = swapped[i.h * ll + r * ll:i.h * ll + r * ll + i.w].reshape(-1, 2)
                c[:] = c[:, ::-1].copy()
                y = same_luma[r * ll:r * ll + i.w].reshape(-1, 2)
                y[:, 1] = y[:, 0]
            for other in (swapped, same_luma):
                assert (CR.entries(table, other, st, 1, i.w, i.h, ll, i.layout)[0] != ent[f]).any()


def test_small_cases_cover_what_they_name():
    for layout in (CC.LAYOUT_YUYV, CC.LAYOUT_OV7670):
        ins = CC.small_inputs(layout)
        assert [(i.w, i.h, i.n) for i in ins[:5]] == [(32, 4, 1), (32, 4, 2), (32, 4, 3), (64, 4, 2), (32, 8, 2)]
        rb = CC.row_bytes(64, layout)
        assert {CC.in_ll(i) for i in ins if i.pad} == {rb + 16, rb + 4}
        for f in CC.FORMS:
            px = 8 if f == CC.RGB888HSV else 16  # pixels per unit of the vector kernel
            # frames of fewer units than a wave's 64, a whole batch of them too
            assert 3 * 32 * 4 // px < 64
            # a per-frame unit count that is no multiple of a workgroup's 256, in a batch of several workgroups
            assert (96 * 20 // px) % 256 != 0 and 3 * 96 * 20 // px > 256
            assert 64 % (640 // px) != 0 and (640 // px) % 64 != 0  # waves cross row ends mid-wave
            want = {"vec": 0, "generic": 0}
            for i in ins:
                kind = CC.form(i, CC.Out(f))
                want[kind] += 1
                odd = i.n > 1 and CC.in_stride(i) % 2 == 1
                if i.pad == 4 or i.off == 1 or odd or (i.off == 8):
                    assert kind == "generic", i
                else:
                    assert kind == "vec", i
            assert want["vec"] >= 8 and want["generic"] >= 4
        assert any(i.n > 1 and i.stride_pad % 2 == 1 and CC.in_stride(i) > CC.frame_bytes(i.w, i.h, CC.in_ll(i), layout)
                   for i in ins)


def test_pitch_cases_have_padding_in_rows_planes_and_frames():
    for f in CC.FORMS:
        outs = CC.pitch_outs(f)
        i = CC.PITCH_IN[CC.LAYOUT_YUYV]
        kinds = [CC.form(i, o) for o in outs]
        for field in ("row_pad", "frame_pad") + (("plane_pad",) if f != CC.RGB888HSV else ()):
            others = [x for x in ("row_pad", "plane_pad", "frame_pad") if x != field]
            alone = [o for o in outs if getattr(o, field) and not any(getattr(o, x) for x in others) and not o.off]
            # alone: once on the vector kernel, once on the generic one
            assert {CC.form(i, o) for o in alone} == {"vec", "generic"}, (f, field)
        assert any(o.row_pad and o.frame_pad and (f == CC.RGB888HSV or o.plane_pad) and k == "vec"
                   for o, k in zip(outs, kinds))
        assert any(o.row_pad and o.frame_pad and (f == CC.RGB888HSV or o.plane_pad) and o.off and k == "generic"
                   for o, k in zip(outs, kinds))
        assert any(o.off % 8 == 0 and o.off and k == "generic" for o, k in zip(outs, kinds))  # 8-byte stores
        assert any(o.off % 2 == 1 for o in outs)
        for o in outs:  # the padding is real: bytes of the buffer that no pixel covers
            off, fs, ps, rp, size = CC.out_geometry(o, i.w, i.h, i.n)
            ent = np.zeros((i.n, i.h, i.w), np.uint64)
            marks = CR.lay_out(ent, f, np.full(size, 1, np.uint8), off, fs, ps, rp)
            covered = int((marks == 0).sum())
            assert covered == i.n * i.h * i.w * (8 if f == CC.RGB888HSV else 3)
            assert (marks[:off] == 1).all() and (marks[-CC.GUARD:] == 1).all()
            if o.row_pad or o.plane_pad or o.frame_pad:
                assert size - 2 * CC.GUARD - o.off > covered


def test_sentinel_is_never_zero_and_has_no_power_of_two_period():
    s = CC.sentinel(4096)
    assert s.min() >= 3 and not np.array_equal(s[:2048], s[2048:]) and not np.array_equal(s[16:32], s[:16])


# ---- the C ABI without a GPU --------------------------------------------------
def _batch(abi, n=2, w=64, h=8, ll=128, layout=0, stride=None, frames=FAKE):
    return abi.FrameBatch(frames, h * ll * (2 if layout == 1 else 1) if stride is None else stride, n, w, h, ll,
                          layout)


def _out(abi, form=0, w=64, h=8, out=FAKE, row=None, plane=None, frame=None):
    row = (8 * w if form == 0 else w) if row is None else row
    plane = (0 if form == 0 else h * row) if plane is None else plane
    frame = (2 * plane + h * row) if frame is None else frame
    return abi.ConvertOut(out, frame, plane, row, form)


def refusals(abi):
    """(what, batch or None, out or None, a word of the message): each refusal
    of the header, one at a time."""
    ok = lambda: _batch(abi)  # noqa: E731
    cases = [("NULL batch", None, _out(abi), "NULL"), ("NULL out", ok(), None, "NULL"),
             ("NULL frames", _batch(abi, frames=None), _out(abi), "frames"),
             ("NULL out->out", ok(), _out(abi, out=None), "out->out"),
             ("unknown layout", _batch(abi, layout=2), _out(abi), "layout"),
             ("form 3", ok(), _out(abi, form=3), "form"), ("form -1", ok(), _out(abi, form=-1), "form")]
    for what, bad in (("width % 32", _batch(abi, w=33)), ("height % 4", _batch(abi, h=6)),
                      ("negative width", _batch(abi, w=-32)), ("short line_length", _batch(abi, ll=127)),
                      ("short ov7670 line_length", _batch(abi, layout=1, ll=63)),
                      ("short frame_stride", _batch(abi, stride=8 * 128 - 1)), ("n_frames < 0", _batch(abi, n=-1)),
                      ("width past int16", _batch(abi, w=32768, ll=65536))):
        cases.append((what, bad, _out(abi, w=bad.width, h=bad.height), ""))
    for f in (0, 1, 2):
        rb = 512 if f == 0 else 64
        cases += [(f"row_pitch form {f}", ok(), _out(abi, f, row=rb - 1, plane=8 * rb, frame=24 * rb), "row_pitch"),
                  (f"negative row_pitch form {f}", ok(), _out(abi, f, row=-rb, plane=8 * rb, frame=24 * rb), "row_pitch"),
                  (f"frame_stride form {f}", ok(), _out(abi, f, frame=(8 if f == 0 else 24) * rb - 1), "frame_stride")]
        if f:
            cases += [(f"plane_stride form {f}", ok(), _out(abi, f, plane=8 * rb - 1, frame=24 * rb), "plane_stride"),
                      (f"frame_stride below padded planes form {f}", ok(),
                       _out(abi, f, plane=8 * rb + 16, frame=24 * rb + 31), "frame_stride")]
    return cases


def call(abi, b, o, stream=None):
    return abi.load().trik_hsv_convert_batch(C.byref(b) if b is not None else None,
                                             C.byref(o) if o is not None else None, stream)


def test_convert_batch_refuses(abi):
    seen = set()
    for what, b, o, word in refusals(abi):
        rc = call(abi, b, o)
        assert rc != 0, what
        msg = abi.last_error()
        assert msg and word in msg, (what, msg)
        seen.add(what)
    assert len(seen) >= 7 + 8 + 3 * 3 + 2 * 2


def test_convert_batch_single_frame_stride_is_checked(abi):
    """The output's frame_stride is checked for one frame too."""
    assert call(abi, _batch(abi, n=1), _out(abi, frame=8 * 512 - 1)) != 0
    assert "frame_stride" in abi.last_error()


def test_convert_batch_degenerate_calls_touch_nothing(abi):
    """n_frames == 0, and width or height 0, return 0 before any GPU call
    (there is no GPU here, and the addresses are not memory)."""
    for f in (0, 1, 2):
        assert call(abi, _batch(abi, n=0, frames=None), _out(abi, f, out=None)) == 0
        assert call(abi, _batch(abi, n=0), _out(abi, f)) == 0
        assert call(abi, _batch(abi, w=0, ll=0, stride=0), _out(abi, f, w=0)) == 0
        assert call(abi, _batch(abi, h=0, stride=0), _out(abi, f, h=0)) == 0


def test_library_exports_convert_batch(abi):
    args, res = abi.PROTOTYPES["trik_hsv_convert_batch"]
    assert len(args) == 3 and res is C.c_int32
    assert hasattr(abi.load(), "trik_hsv_convert_batch")
    assert C.sizeof(abi.ConvertOut) == 32 and abi.ConvertOut.row_pitch.offset == 24 and abi.ConvertOut.form.offset == 28
    import trik_hsv

    assert callable(trik_hsv.convert_batch)
    assert (trik_hsv.CONVERT_RGB888HSV, trik_hsv.CONVERT_HSV_PLANES, trik_hsv.CONVERT_RGB_PLANES) == (0, 1, 2)
    assert (CC.RGB888HSV, CC.HSV_PLANES, CC.RGB_PLANES) == (0, 1, 2)


def test_struct_layout_matches_c(abi, tmp_path):
    import os
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "trik_hsv.h"\nint main(void){\n'
                   '  printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(TrikHsvConvertOut), offsetof(TrikHsvConvertOut, out),\n'
                   '         offsetof(TrikHsvConvertOut, frame_stride), offsetof(TrikHsvConvertOut, plane_stride),\n'
                   '         offsetof(TrikHsvConvertOut, row_pitch), offsetof(TrikHsvConvertOut, form));\n'
                   '  printf("%d %d %d\\n", TRIK_HSV_CONVERT_RGB888HSV, TRIK_HSV_CONVERT_HSV_PLANES,\n'
                   '         TRIK_HSV_CONVERT_RGB_PLANES);\n  return 0;\n}\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(root, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    m = abi.ConvertOut
    assert [int(x) for x in out[:6]] == [C.sizeof(m), m.out.offset, m.frame_stride.offset, m.plane_stride.offset,
                                         m.row_pitch.offset, m.form.offset]
    assert [int(x) for x in out[6:]] == [abi.CONVERT_RGB888HSV, abi.CONVERT_HSV_PLANES, abi.CONVERT_RGB_PLANES]
