"""mxn_hist_kernel and mxn_preview_kernel on the inputs of tests/mxn_cases.py:
every cell edge (each (c0 % 4, col_step % 4) a grid can produce, every border
and every adjacent pixel decisive), ties whose contenders sit in one slot, in
two slots, waves and loop trips, winners that lead in no wave, counts and
positions above 2^16, and previews whose every square pixel names its cell.
tests/test_mxn_shapes_cpu.py asserts what each input reaches; here the GPU's
bins, colours and preview bytes are compared with tests/mxn_ref.py, bit-exact.

Every batch call writes into sentinel-filled outputs one cell longer than the
batch: nothing past n_frames * m * n may change."""
import ctypes as C

import numpy as np
import pytest

import mxn_cases as mc
import mxn_ref
from gpu_util import LAYOUT_OV7670

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A5A5A
SENTINEL16 = 0x5A5A


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
def pal(table):
    return mc.Palette(table)


@pytest.fixture(scope="module")
def edges(pal):
    return mc.by_geometry(mc.edge_cases(pal))


_REF = {}


def ref(table, pal, case):
    """(colors, bins) of mxn_ref.run on a case's frame, computed once."""
    if case.name not in _REF:
        w, h, m, n = case.geom
        _REF[case.name] = mxn_ref.run(table, pal.frame(case.bins), w, h, w, m, n)[:2]
    return _REF[case.name]


def run_batch(hsv, det, dev, geom, ll, n_frames, frame_stride=None):
    """trik_hsv_mxn_batch into sentinel-filled outputs one cell longer than the
    batch: (colors, bins) as int lists per frame.  Detector.mxn_batch
    allocates its own outputs, so the sentinels need the C entry point it
    wraps; check() sends every aligned batch through the wrapper as well."""
    import torch

    w, h, m, n = geom
    cells = m * n
    b = hsv._batch(dev, w, h, ll, LAYOUT_OV7670, n_frames, frame_stride)
    colors = torch.full((n_frames * cells + cells,), SENTINEL, dtype=torch.int32, device="cuda")
    bins = torch.full((n_frames * cells + cells,), SENTINEL16, dtype=torch.int16, device="cuda")
    rc = hsv._lib.trik_hsv_mxn_batch(det._h, C.byref(b), m, n, C.c_void_p(colors.data_ptr()),
                                     C.c_void_p(bins.data_ptr()), None)
    assert rc == 0, hsv._lib.trik_hsv_last_error()
    torch.cuda.synchronize()
    colors, bins = colors.cpu().numpy(), bins.cpu().numpy()
    assert (colors[n_frames * cells:] == SENTINEL).all() and (bins[n_frames * cells:] == SENTINEL16).all()
    return colors[:n_frames * cells].reshape(n_frames, cells).tolist(), bins[:n_frames * cells].reshape(n_frames, cells).tolist()


def check(hsv, det, table, pal, geom, cases, ll=None, base=0, pad=0):
    """The cases of one geometry as one batch: frames `pad` bytes apart beyond
    their size, the first `base` bytes past a 4-byte boundary."""
    import torch

    w, h, m, n = geom
    ll = w if ll is None else ll
    fb = 2 * h * ll
    stride = fb + pad
    host = np.full(base + len(cases) * stride, 0xEE, np.uint8)
    for i, c in enumerate(cases):
        host[base + i * stride:base + i * stride + fb] = pal.frame(c.bins, ll)
    dev = torch.from_numpy(host).cuda()
    assert dev.data_ptr() % 4 == 0
    colors, bins = run_batch(hsv, det, dev[base:], geom, ll, len(cases), stride)
    for i, c in enumerate(cases):
        want = ref(table, pal, c)
        assert bins[i] == want[1], (c, ll, base, pad)
        assert colors[i] == want[0], (c, ll, base, pad)
    if (ll, base, pad) == (w, 0, 0):
        wc, wb = det.mxn_batch(dev, w, h, ll, m, n, bins=True)
        assert wc.cpu().numpy().tolist() == colors and wb.cpu().numpy().tolist() == bins


def test_mxn_edges(hsv, det, table, pal, edges):
    """Every border pixel counted, no adjacent pixel counted: one batch per
    geometry, so the cases also neighbour each other across frames."""
    n = 0
    for geom, cases in edges:
        check(hsv, det, table, pal, geom, cases)
        # the cell each frame was made for holds the tie (or the one-pixel lead) the case says
        for c in cases:
            k = c.cell[0] * c.form.n + c.cell[1]
            win, lose = (c.X, c.Y) if c.kind == "lead" else (c.Y, c.X)
            assert ref(table, pal, c)[1][k] == win
            # the colour names the winner too: the contenders' colours differ
            assert ref(table, pal, c)[0][k] == mxn_ref.bin_color(win) != mxn_ref.bin_color(lose)
        n += len(cases)
    assert n == 2 * sum(len(mc.edge_targets(mc.form(*g))) for g in mc.EDGE_GEOMS)


def test_mxn_empty_cells(hsv, det, table, pal, edges):
    """row_step == 0: every cell is empty, bin 0 and colour 0, whatever the frame holds."""
    geom = mc.EMPTY_GEOM
    cases = [c for g, cs in edges if g == (32, 4, 4, 6) for c in cs][:4]
    import torch

    dev = torch.from_numpy(np.concatenate([pal.frame(c.bins) for c in cases])).cuda()
    colors, bins = run_batch(hsv, det, dev, geom, 32, len(cases))
    for i, c in enumerate(cases):
        want = mxn_ref.run(table, pal.frame(c.bins), 32, 4, 32, geom[2], geom[3])
        assert want[1] == [0] * 5 and want[0] == [0] * 5
        assert bins[i] == want[1] and colors[i] == want[0]


def test_mxn_edges_odd_base(hsv, det, table, pal, edges):
    """The byte-load path by the frame address alone: one frame a call, one byte past a 4-byte boundary."""
    for geom, cases in edges:
        for c in cases:
            check(hsv, det, table, pal, geom, [c], base=1)


def test_mxn_edges_odd_stride(hsv, det, table, pal, edges):
    """The byte-load path by the frame stride alone (2 mod 4, and odd): aligned base and lines."""
    for geom, cases in edges:
        check(hsv, det, table, pal, geom, cases, pad=2)
        check(hsv, det, table, pal, geom, cases, pad=1)


def test_mxn_edges_line_length_2_mod_4(hsv, det, table, pal, edges):
    """The byte-load path by the line length alone: width + 2, which the entry
    point accepts (any line_length >= width); base and stride stay aligned."""
    for geom, cases in edges:
        assert (2 * geom[1] * (geom[0] + 2)) % 4 == 0
        check(hsv, det, table, pal, geom, cases, ll=geom[0] + 2)


def test_mxn_split(hsv, det, table, pal):
    """Cells of more than 256 groups: sums over waves, last positions over
    slots, waves and trips, and the lanes after the peel rounds."""
    for geom, cases in mc.by_geometry(mc.split_cases(pal)):
        check(hsv, det, table, pal, geom, cases)
        check(hsv, det, table, pal, geom, cases, ll=geom[0] + 2)  # the same through byte loads


def test_mxn_big(hsv, det, table, pal):
    """The whole 640 x 480 frame as one cell: two bins tied above 2^16 pixels
    with last positions above 2^17, and 307,200 pixels of one bin."""
    cases = mc.big_cases(pal)
    check(hsv, det, table, pal, mc.BIG_GEOM, cases)
    assert ref(table, pal, cases[0])[1] == [pal.A] and ref(table, pal, cases[1])[1] == [pal.C]


@pytest.mark.parametrize("geom", mc.PREVIEW_GEOMS)
def test_mxn_preview_names_its_cells(hsv, det, table, pal, geom):
    """The caller's colours, all different and none a body pixel's: the whole
    out_h x out_ll buffer against the reference, padding and unwritten pixels
    zero; then into a sentinel-filled buffer one row longer."""
    import torch

    w, h, ll, m, n, ow, oh, oll = geom
    nf = mc.PREVIEW_FRAMES
    frames = [pal.frame(mc.preview_body(pal, w, h, i), ll) for i in range(nf)]
    body565 = np.concatenate([mxn_ref.px565(mxn_ref.frame_pixels(table, fr, w, h, ll)[0]).reshape(-1) for fr in frames])
    colors = mc.preview_colors(body565, nf, m * n)
    want = [mxn_ref.preview(table, frames[i], w, h, ll, m, n, colors[i].tolist(), ow, oh, oll) for i in range(nf)]
    dev = torch.from_numpy(np.concatenate(frames)).cuda()
    dcol = torch.from_numpy(colors).cuda()
    pv = det.mxn_preview(dev, w, h, ll, m, n, dcol, out_width=ow, out_height=oh, out_line_length=oll).cpu().numpy()
    for i in range(nf):
        assert np.array_equal(pv[i], want[i]), (geom, i, np.argwhere(pv[i] != want[i])[:4].tolist())
        assert not pv[i][:, 2 * ow:].any()
    stride = (oh + 1) * oll
    buf = torch.full((nf * stride,), 0x5A, dtype=torch.uint8, device="cuda")
    b = hsv._batch(dev, w, h, ll, LAYOUT_OV7670)
    rc = hsv._lib.trik_hsv_mxn_preview(det._h, C.byref(b), m, n, C.c_void_p(dcol.data_ptr()), ow, oh, oll,
                                       C.c_void_p(buf.data_ptr()), stride, None)
    assert rc == 0, hsv._lib.trik_hsv_last_error()
    torch.cuda.synchronize()
    got = buf.cpu().numpy().reshape(nf, oh + 1, oll)
    for i in range(nf):
        assert np.array_equal(got[i, :oh], want[i]), (geom, i)
        assert (got[i, oh] == 0x5A).all()
