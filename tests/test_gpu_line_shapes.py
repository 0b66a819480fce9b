"""The ov7670 line sensor's kernels through their own geometry (csrc/
trik_hsv_line.hip): every workgroup shape line_geom picks (idle lanes, row
offsets past the last row, a partial last iteration, a short last segment, the
forced single segment, a second column chunk under several row segments), the
cross band at every offset relative to the rows per iteration, the unrolled
loop and the segment edges, the lane-to-column formula one column at a time,
the generic kernel on misaligned input, the OutArgs at the points threshold
and past 2^32 in the column sum, and the target line's column clamps in both
preview paths.  Every comparison is exact, against tests/line_ref.py (held to
the oracle by tests/test_line_cpu.py, which also checks what each input of
tests/line_cases.py reaches)."""
import numpy as np
import pytest

import line_cases
import line_ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hsv():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import trik_hsv

    return trik_hsv


def _band(h, band):
    return line_ref.default_band(h) if band is None else band


def _targets(t):
    """int8 [N, 4] of line_batch -> [(targetX, targetY, targetSize)]."""
    return [(x, y, s & 0xFF) for x, y, s, _ in t.cpu().tolist()]


def _frames(buf, n, stride, fb, off=0):
    return [buf[off + f * stride:off + f * stride + fb] for f in range(n)]


def _check(hsv, table, dev, frames, w, h, ll, bands, **kw):
    """line_batch over `frames` (resident in `dev`) = line_ref, at both RANGES
    and every band: sums and OutArgs of every frame."""
    for vf, vt in line_cases.RANGES:
        dets = [line_ref.detect(table, fr, w, h, ll, vf, vt) for fr in frames]
        for band in bands:
            sums, targets = hsv.line_batch(dev, w, h, ll, vf, vt, band=band, n_frames=len(frames), **kw)
            want = [line_ref.sums_of(d, _band(h, band)) for d in dets]
            assert sums.cpu().tolist() == want, (w, h, len(frames), vf, vt, band)
            assert _targets(targets) == [line_ref.targets(*s, w, h) for s in want], (w, h, vf, vt, band)


@pytest.mark.parametrize("shape", line_cases.SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_line_shapes(hsv, table, shape):
    """Each workgroup shape on noise frames, under every band of
    line_cases.bands."""
    import torch

    w, h, n = shape
    buf = line_cases.shape_noise(w, h, n)
    dev = torch.from_numpy(np.array(buf)).cuda()
    _check(hsv, table, dev, _frames(buf, n, 2 * h * w, 2 * h * w), w, h, w, line_cases.bands(h))


def test_line_batch_takes_setup_geometries_only(hsv):
    """Widths of 17 units or of 8 or 16 columns, and heights below 4, never
    reach the kernels: the entry point refuses what setup() refuses
    (LSEQ:328-332).  line_cases.SHAPES holds the smallest frames it takes."""
    import torch

    dev = torch.zeros(2 * 136 * 36, dtype=torch.uint8, device="cuda")
    for w, h in ((136, 36), (16, 8), (8, 8), (24, 4), (64, 1), (64, 3), (100, 20)):
        with pytest.raises(hsv.TrikHsvError):
            hsv.line_batch(dev, w, h, w, 0, 70, n_frames=1)


def test_line_forced_single_segment_equals_segments(hsv):
    """The 1024-frame call (one segment of 104 rows) and the 7-frame call (two
    segments, 56 + 44 rows) agree on the frames they share."""
    import torch

    w, h = 64, 100
    dev = torch.from_numpy(np.array(line_cases.shape_noise(w, h, 1024))).cuda()
    for vf, vt in line_cases.RANGES:
        many, many_t = hsv.line_batch(dev, w, h, w, vf, vt, band=(50, 60), n_frames=1024)
        few, few_t = hsv.line_batch(dev, w, h, w, vf, vt, band=(50, 60), n_frames=7)
        assert torch.equal(many[:7], few) and torch.equal(many_t[:7], few_t)
        assert int(few[:, 2].min()) > 0


def test_line_every_band_64x36(hsv, table):
    """Every band (s, e), 0 <= s <= e < 36, on one 64 x 36 frame (rpi 8, five
    iterations): 666 launches, the results copied back once."""
    import torch

    w, h = 64, 36
    buf = line_cases.shape_noise(w, h, 1)
    dev = torch.from_numpy(np.array(buf)).cuda()
    bands = [(s, e) for s in range(h) for e in range(s, h)]
    assert len(bands) == 666
    for vf, vt in line_cases.RANGES:
        det = line_ref.detect(table, buf, w, h, w, vf, vt)
        got = torch.stack([hsv.line_batch(dev, w, h, w, vf, vt, band=b)[0][0] for b in bands]).cpu().tolist()
        assert got == [line_ref.sums_of(det, b) for b in bands], (vf, vt)


@pytest.mark.parametrize("n", [1, 7])
def test_line_single_row_bands_64x100(hsv, table, n):
    """Every band (r, r) of 64 x 100: two segments of 56 and 44 rows."""
    import torch

    w, h = 64, 100
    buf = line_cases.shape_noise(w, h, n)
    dev = torch.from_numpy(np.array(buf)).cuda()
    frames = _frames(buf, n, 2 * h * w, 2 * h * w)
    vf, vt = line_cases.RANGES[0]
    dets = [line_ref.detect(table, fr, w, h, w, vf, vt) for fr in frames]
    got = torch.stack([hsv.line_batch(dev, w, h, w, vf, vt, band=(r, r), n_frames=n)[0]
                       for r in range(h)]).cpu().tolist()
    assert got == [[line_ref.sums_of(d, (r, r)) for d in dets] for r in range(h)]


@pytest.mark.parametrize("width", line_cases.COLUMN_WIDTHS)
def test_line_one_hot_columns(hsv, width):
    """Frame c has column c dark, so its sums name the column every
    accumulator slot of every lane stands for."""
    import torch

    dev = torch.from_numpy(line_cases.one_hot_columns(width)).cuda()
    sums, _ = hsv.line_batch(dev, width, 8, width, *line_cases.COLUMN_RANGE, n_frames=width)
    assert sums.cpu().tolist() == line_cases.one_hot_expected(width)


@pytest.mark.parametrize("case", line_cases.GENERIC, ids=lambda c: "w%d_ll%d_n%d_pad%d_off%d" % c)
def test_line_generic_kernel(hsv, table, case):
    """line_sums_kernel on what the fast kernel refuses."""
    import torch

    w, ll, n, pad, off = case
    h = line_cases.GENERIC_H
    buf, off, stride = line_cases.generic_noise(case)
    dev = torch.from_numpy(buf).cuda()
    assert dev.data_ptr() % 16 == 0
    _check(hsv, table, dev[off:], _frames(buf, n, stride, 2 * h * ll, off), w, h, ll, line_cases.bands(h),
           frame_stride=stride)


def test_line_targets_points_threshold(hsv, table):
    """10 points give no target, 11 do (LSEQ:462)."""
    import torch

    w, h = 64, 8
    for count in (10, 11):
        fr = line_cases.dark_pixels(w, h, count)
        sums, targets = hsv.line_batch(torch.from_numpy(fr).cuda(), w, h, w, *line_cases.COLUMN_RANGE)
        want = line_ref.sums(table, fr, w, h, w, *line_cases.COLUMN_RANGE)
        assert sums[0].cpu().tolist() == want and want[0] == count
        assert _targets(targets)[0] == line_ref.targets(*want, w, h)
        assert (_targets(targets)[0] == (0, 0, 0)) == (count == 10)


def test_line_column_sum_past_2_32(hsv, oracle_mod, table):
    """4096 x 600 with every window pixel detected.  sum_x is the exact
    64-bit value; the OutArgs and the preview's target line come from its low
    word, as the reference's int32 gives them."""
    import torch

    w, h = 4096, 600
    fr = line_cases.noise(w, h, w, 1, 4096)
    dev = torch.from_numpy(fr).cuda()
    sums, targets = hsv.line_batch(dev, w, h, w, 0, 100)
    want = line_ref.sums(table, fr, w, h, w, 0, 100)
    assert want[1] > 2**32 and sums[0].cpu().tolist() == want
    _, oa, ref_pv, _, _ = oracle_mod.line_run(fr, w, h, w, 0, 100)
    assert _targets(targets)[0] == line_ref.targets(*want, w, h) == (oa["target_x"], oa["target_y"], oa["target_size"])
    det = hsv.Detector()
    try:
        pv = det.line_preview(dev, w, h, w, 0, 100, sums)
    finally:
        det.close()
    assert np.array_equal(pv[0].cpu().numpy().reshape(-1), ref_pv)


# 64 x 8 -> 32 x 4: the 2:1 maps, the overlay drawn by preview_rows2_kernel;
# 64 x 8 -> 40 x 5: other maps, the preview body and then line_overlay_kernel
@pytest.mark.parametrize("out", [(32, 4), (40, 5)])
def test_line_preview_target_line_from_sums(hsv, oracle_mod, out):
    """The target line's column clamps, reached with the caller's sums (a
    frame's own never put the line at an edge: the window ends 5 columns in)."""
    import torch

    w, h = 64, 8
    ow, oh = out
    oll = 2 * ow
    fr = line_cases.floor(w, h)
    _, _, p0, s0, _ = oracle_mod.line_run(fr, w, h, w, *line_cases.COLUMN_RANGE, out_width=ow, out_height=oh,
                                          out_line_length=oll)
    assert s0[0] <= 10  # so P0 has no target line
    p0 = p0.reshape(oh, oll)
    shift = min(ow / w, oh / h)
    wi2wo = [int(i * shift) for i in range(w)]
    hi2ho = [int(i * shift) for i in range(h)]
    red = p0[hi2ho[h // 2], 2 * wi2wo[5]:2 * wi2wo[5] + 2].copy()  # a pixel of P0's band line
    assert red.any()

    def with_line(cx):
        p = p0.copy()
        for row in range(h):
            for c in range(cx - 1, cx + 2):
                oc = wi2wo[min(max(c, 0), w - 1)]
                p[hi2ho[row], 2 * oc:2 * oc + 2] = red
        return p

    centres = [0, 1, 2, w // 2, w - 3, w - 2, w - 1]
    sums = [[11, 11 * cx, 0] for cx in centres] + [[10, 10 * (w // 2), 0], [11, 2**32 + 11 * (w // 2), 0], [0, 0, 0]]
    want = [with_line(cx) for cx in centres] + [p0, with_line(w // 2), p0]
    # (the clamps show: the line is narrower at column 0 than at 1, and at w - 1 than at w - 3)
    assert not np.array_equal(want[0], want[1]) and not np.array_equal(want[6], want[4])
    n = len(sums)
    dev = torch.from_numpy(np.tile(fr, n)).cuda()
    det = hsv.Detector()
    try:
        pv = det.line_preview(dev, w, h, w, *line_cases.COLUMN_RANGE, torch.tensor(sums, dtype=torch.int64).cuda(),
                              out_width=ow, out_height=oh, out_line_length=oll, n_frames=n)
    finally:
        det.close()
    pv = pv.cpu().numpy()
    for i in range(n):
        assert np.array_equal(pv[i], want[i]), (out, sums[i])
