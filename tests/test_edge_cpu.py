"""CPU-only checks of the ov7670 edge-line sensor: the test reference itself
(tests/edge_ref.py: its vectorised forms against the literal loops, the
per-row uint16 wrap, the parity of the Sobel magnitude, the int32 line column),
the inputs of the GPU sweeps (tests/edge_cases.py: that each reaches what it is
meant to reach, stated on the reference's output), the host-side OutArgs
(trik_hsv_edge_targets runs without a GPU), and the new exports: the symbols
and the function table bind from plain C."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import edge_cases
import edge_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("geom", [(32, 4), (64, 8), (96, 12)])
def test_vectorised_map_equals_scalar_loops(geom):
    w, h = geom
    rng = np.random.default_rng(w * 1000 + h)
    for kind in ("bytes", "binary"):
        fr = rng.integers(0, 256, 2 * w * h, dtype=np.uint8)
        if kind == "binary":
            fr[:w * h] = rng.integers(0, 2, w * h, dtype=np.uint8) * 255
        for thr in (50, 255):
            want = edge_ref.edge_map_scalar(fr, w, h, thr)
            got = edge_ref.edge_map(fr, w, h, thr)
            assert np.array_equal(got, want), (geom, kind, thr)
            # the bytes the loop never writes
            flat = got.reshape(-1)
            assert flat[0] == 0 and flat[w * (h - 2) - 1] == 0 and not got[h - 2:].any()


@pytest.mark.parametrize("geom", [(32, 4, 16, 2, 32), (64, 8, 128, 16, 256), (64, 8, 48, 6, 100)])
def test_vectorised_preview_equals_scalar_loops(geom):
    w, h, ow, oh, oll = geom
    rng = np.random.default_rng(7 * w + h)
    fr = rng.integers(0, 256, 2 * w * h, dtype=np.uint8)
    emap, (p, sx), _ = edge_ref.run(fr, w, h)
    for points in (p, 0):
        want = edge_ref.preview_scalar(fr, w, h, emap, points, sx, ow, oh, oll)
        assert np.array_equal(edge_ref.preview(fr, w, h, emap, points, sx, ow, oh, oll), want), (geom, points)


@pytest.mark.parametrize("geom", [(32, 4), (64, 8), (96, 12), (384, 4)])
def test_vectorised_sums_equal_scalar_loops(geom):
    w, h = geom
    rng = np.random.default_rng(w * 1000 + h + 1)
    frames = [rng.integers(0, 256, 2 * w * h, dtype=np.uint8), edge_ref.level_frame(w, h, 1020)]
    for fr in frames:
        for thr in (0, 50, 255):
            emap = edge_ref.edge_map(fr, w, h, thr)
            for wrap in (True, False):
                assert edge_ref.sums(emap, wrap) == edge_ref.sums_scalar(emap, wrap), (geom, thr, wrap)
    # the level frame detects every window pixel: at 384 columns the wrap decides its column sum
    p, sx = edge_ref.sums(edge_ref.edge_map(frames[1], w, h))
    assert p == (h - 2) * (w - 31)
    assert (edge_ref.sums(edge_ref.edge_map(frames[1], w, h), wrap=False)[1] != sx) == (w >= 384)


def test_preview_line_column_is_an_int32():
    """targetX is an int32_t (ESEQ:399): a quotient with bit 31 set is negative
    and clamps to column 0, in the loops and in the vectorised form alike."""
    w, h = 64, 8
    rng = np.random.default_rng(9)
    fr = rng.integers(0, 256, 2 * w * h, dtype=np.uint8)
    emap = edge_ref.edge_map(fr, w, h)
    cases = [(1, -1, 0), (1, 1 << 31, 0), (1, (1 << 32) - 5, 0), (2, -1, w - 1), (3, (1 << 32) - 1, w - 1),
             (1, 20, 20), (1, w + 500, w - 1), (1 << 32, 5, None), (0, 5, None)]
    for points, sum_x, col in cases:
        want = edge_ref.preview_scalar(fr, w, h, emap, points, sum_x, w, h, 2 * w)
        assert np.array_equal(edge_ref.preview(fr, w, h, emap, points, sum_x, w, h, 2 * w), want), (points, sum_x)
        px = want.view("<u2")
        line = (px == edge_ref.LINE_PIXEL).all(axis=0)  # H = 8: the line spans every row
        assert np.flatnonzero(line).tolist() == ([] if col is None else [col]), (points, sum_x)


@pytest.mark.parametrize("level", [0, 2, 6, 50, 52, 254, 256, 300, 1020])
def test_level_frame_has_one_magnitude(level):
    for w, h in ((64, 8), (2048, 68)):
        H, V = edge_ref.hv(edge_ref.level_frame(w, h, level), w, h)
        H, V = H.reshape(h, w)[:h - 2, 1:w - 1], V.reshape(h, w)[:h - 2, 1:w - 1]
        assert (np.abs(H) == level).all() and not V.any()
        assert (H[0::4] == level).all() and (H[2::4] == -level).all()
        o = edge_ref.sobel(edge_ref.level_frame(w, h, level), w, h).reshape(h, w)
        assert (o[:h - 2, 1:w - 1] == min(level, 255)).all() and not o[h - 2:].any()


def test_sweep_inputs_cover_what_they_claim():
    """The inputs of the GPU threshold sweep, on the reference: the noise
    ladder holds every even magnitude and one past the cap in each sign
    quadrant, the two axis frames hold them with H = 0 and with V = 0, and the
    last-row frame detects in map row H-3 alone."""
    edge_cases.check_ladder(edge_cases.noise_ladder())
    edge_cases.check_axis(edge_cases.h0_frame(), *edge_cases.H0_GEOM, "h0")
    edge_cases.check_axis(edge_cases.v0_frame(), *edge_cases.V0_GEOM, "v0")
    for w in (64, 320):
        for h in (20, 36, 292, 308):
            edge_cases.check_last_row(edge_cases.last_row_frame(w, h), w, h)
    # a level frame at threshold t: all of the window or nothing
    w, h = 64, 8
    for level in edge_cases.SWEEP_LEVELS:
        o = edge_ref.sobel(edge_ref.level_frame(w, h, level), w, h)
        for thr in range(256):
            p, _ = edge_ref.sums(edge_ref.threshold(o, w, h, thr))
            assert p == ((h - 2) * (w - 31) if level > thr or level >= 255 else 0), (level, thr)


def test_preview_inputs_hold_every_luma_with_every_chroma():
    w, h = edge_cases.PREVIEW_GEOM
    chroma = edge_cases.preview_chroma(w, h)
    seen = np.zeros(1 << 24, bool)
    for level in edge_cases.PREVIEW_LEVELS:
        fr = edge_cases.preview_frame(level, chroma)
        edge_cases.preview_triples(fr, edge_ref.edge_map(fr, w, h, 255), seen)
    lumas = sorted(set(np.flatnonzero(seen) >> 16))
    assert lumas == list(range(0, 256, 2)) + [255]
    assert int(seen.sum()) == 129 * 65536


def test_row_sums_wrap_at_384_columns():
    """384 x 4, rows 0, 0, 255, 255: both live rows detect every window pixel
    (|H| = 1020); a row's column sum 16 + .. + 368 = 67776 wraps to 2240."""
    w, h = 384, 4
    fr = np.full(2 * w * h, 128, np.uint8)
    fr[:2 * w] = 0
    fr[2 * w:4 * w] = 255
    emap = edge_ref.edge_map(fr, w, h)
    assert (emap[:2, 16:w - 15] == 255).all() and not emap[2:].any()
    assert edge_ref.sums(emap, wrap=False) == (706, 2 * 67776)
    assert edge_ref.sums(emap) == (706, 2 * 2240)
    # 352 columns: 16 + .. + 336 = 56496, no wrap yet
    w = 352
    fr = np.full(2 * w * h, 128, np.uint8)
    fr[:2 * w] = 0
    fr[2 * w:4 * w] = 255
    emap = edge_ref.edge_map(fr, w, h)
    assert edge_ref.sums(emap) == edge_ref.sums(emap, wrap=False) == (642, 2 * 56496)


def test_sobel_magnitude_is_even_so_the_live_boundary_is_50_52():
    w, h = 64, 8
    o = edge_ref.sobel(edge_ref.single_pixel(w, h, 3, 30, 100, 125), w, h)
    assert o.max() == 50 and (o == 50).sum() == 8
    assert edge_ref.run(edge_ref.single_pixel(w, h, 3, 30, 100, 125), w, h)[1] == (0, 0)
    fr = edge_ref.single_pixel(w, h, 3, 30, 100, 126)
    o = edge_ref.sobel(fr, w, h)
    assert o.max() == 52 and (o == 52).sum() == 8
    emap, (p, sx), _ = edge_ref.run(fr, w, h)
    # the 8 windows around the pixel: map rows 1..3 (shifted up one row), columns 29..31
    assert p == 8 and sx == 3 * (29 + 31) + 2 * 30
    assert (emap[1:4, 29:32] == 255).sum() == 8 and emap[2, 30] == 0
    rng = np.random.default_rng(5)
    fr = rng.integers(0, 256, 2 * w * h, dtype=np.uint8)
    assert not (edge_ref.sobel(fr, w, h) % 2)[edge_ref.sobel(fr, w, h) < 255].any()


def test_host_targets_equal_reference():
    import trik_hsv

    for w, h in ((320, 240), (640, 480), (32, 4), (2048, 2048)):
        for points in (0, 1, 10, 68782):
            for mean in (0, 16, w // 2 - 1, w // 2, w - 16, w - 1):
                for extra in (0, points // 2):
                    sum_x = mean * points + extra
                    assert trik_hsv.edge_targets(points, sum_x, w, h) == edge_ref.targets(points, sum_x, w, h), \
                        (w, h, points, sum_x)
    # hand-worked: 68782 points (every window pixel of 320 x 240 above the last two rows), centred
    assert edge_ref.targets(68782, 68782 * 160, 320, 240) == (0, -100, 105)  # ceil(sqrt(21894.02)) = 148; 59200 / 560
    assert edge_ref.targets(1, 16, 320, 240) == (-90, -100, 0)
    assert edge_ref.targets(0, 5, 320, 240) == (0, 0, 0)


XDAIS_PROG = r"""
#include <stdio.h>
#include "trik_hsv.h"
int main(void) {
  const TRIK_IVIDTRANSCODE_Fxns* f = &TRIK_VIDTRANSCODE_CV_EDGE_LINE_FXNS;
  TRIK_IALG_MemRec m[16];
  TRIK_IALG_Fxns* parent = NULL;
  int n = f->ialg.algAlloc(NULL, &parent, m);
  if (n != 1 || m[0].size < sizeof(TRIK_IALG_Obj) || m[0].attrs != TRIK_IALG_PERSIST) return 10;
  if (f->ialg.implementationId != (const void*)f || !f->process || !f->control || !f->ialg.algInit ||
      !f->ialg.algFree) return 20;
  if (f->ialg.algInit == TRIK_VIDTRANSCODE_CV_OV7670_FXNS.ialg.algInit) return 30;
  if (!&TRIK_VIDTRANSCODE_CV_create_edge_line || !&trik_hsv_edge_batch || !&trik_hsv_edge_preview) return 40;
  TrikHsvTargetSums s = {68782, 68782LL * 160, 0};
  TrikHsvTarget t = {1, 1, 1, 1};
  if (trik_hsv_edge_targets(&s, 320, 240, &t)) return 50;
  printf("%d %d %d\n", t.x, t.y, t.size);
  return 0;
}
"""


def test_edge_table_links_from_c_without_gpu():
    lib_dir = os.path.join(ROOT, "trik-media-sensors-dsp_amd", "trik_hsv")
    with tempfile.TemporaryDirectory() as d:
        c, exe = os.path.join(d, "x.c"), os.path.join(d, "x")
        open(c, "w").write(XDAIS_PROG)
        subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-Wno-address", f"-I{os.path.join(ROOT, 'include')}",
                        c, f"-L{lib_dir}", "-ltrik_hsv", f"-Wl,-rpath,{lib_dir}", "-o", exe], check=True)
        r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    assert tuple(int(v) for v in r.stdout.split()) == edge_ref.targets(68782, 68782 * 160, 320, 240)


def test_edge_symbols_are_exported():
    from trik_hsv import _abi

    lib = _abi.load()
    for name in ("trik_hsv_edge_batch", "trik_hsv_edge_preview", "trik_hsv_edge_targets",
                 "TRIK_VIDTRANSCODE_CV_create_edge_line"):
        assert getattr(lib, name)
    assert C.c_void_p.in_dll(lib, "TRIK_VIDTRANSCODE_CV_EDGE_LINE_FXNS")
