"""The ov7670 edge-line sensor on the GPU against tests/edge_ref.py (TI's
documented natural-C semantics of the three IMGLIB calls plus ESEQ =
trik/ov7670/edge_line_sensor/include/internal/cv_ball_detector_seqpass.hpp):
sums, targets, the thresholded map and the preview bytes, bit-exact, through
edge_batch / Detector.edge_preview (trik_hsv_edge_batch / trik_hsv_edge_preview),
EdgeLineSensor.process (TRIK_VIDTRANSCODE_CV_create_edge_line) and the exported
XDAIS function table.  Every lane layout and row segmentation of the fast
kernel, every threshold and every colour of the preview run on the inputs of
tests/edge_cases.py, whose coverage is asserted on the reference's output."""
import ctypes as C

import numpy as np
import pytest

import edge_cases
import edge_ref
from gpu_util import LAYOUT_OV7670

pytestmark = pytest.mark.gpu


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


_REF = {}


def ref_run(key, frame, w, h, thr=50):
    """edge_ref.run, computed once per (frame, threshold) and shared."""
    k = (key, w, h, thr)
    if k not in _REF:
        _REF[k] = edge_ref.run(frame, w, h, thr)
    return _REF[k]


def binary_frame(w, h, seed):
    rng = np.random.default_rng(seed)
    fr = rng.integers(0, 256, 2 * w * h, dtype=np.uint8)
    fr[:w * h] = rng.integers(0, 2, w * h, dtype=np.uint8) * 255
    return fr


def steps_frame(w, h):
    """Rows 0, 0, 255, 255, ...: |H| = 1020 on every live row, so every window
    pixel is detected and, from 384 columns, every row's column sum wraps."""
    fr = np.full(2 * w * h, 128, np.uint8)
    fr[:w * h].reshape(h, w)[(np.arange(h) % 4) >= 2] = 255
    fr[:w * h].reshape(h, w)[(np.arange(h) % 4) < 2] = 0
    return fr


def make_frames(oracle_mod, w, h):
    """Uniform bytes, a scene, random {0, 255} luma, single-pixel frames (one
    inside the window, one whose edges straddle its left end), the steps."""
    return [("uniform", oracle_mod.synth(1, w, h, w, LAYOUT_OV7670, 0, 0x51DE)),
            ("scene", oracle_mod.synth(1, w, h, w, LAYOUT_OV7670, 1, 0x7A1C, first_frame=3)),
            ("binary", binary_frame(w, h, 11 * w + h)),
            ("pixel", edge_ref.single_pixel(w, h, 1, w // 2)),
            ("pixel16", edge_ref.single_pixel(w, h, h - 2, 16)),
            ("steps", steps_frame(w, h))]


def upload(frames):
    import torch

    return torch.from_numpy(np.concatenate([fr for _, fr in frames])).cuda()


# 32x4: a one-column window and two live rows; 352x8: the widest frame whose
# row sums cannot wrap; 384x4 and 640x8: the wrap frames; 320x240: the TRIK frame.
# The fast kernel's other shapes: 160x8 (a row takes 32 lanes), 64x52 (row
# segments of 17, 17 and 16 rows), 1024x4 (16 columns per lane), 1056x4 and
# 2048x4 (32 columns per lane; the cap)
GEOMS = [(32, 4), (64, 8), (96, 12), (352, 8), (384, 4), (640, 8), (320, 240), (160, 8), (64, 52), (1024, 4),
         (1056, 4), (2048, 4)]


def check_frames(hsv, frames, w, h):
    """Sums, targets and the map of every frame, the fast and the generic
    kernel, against the reference.  `frames` begins with make_frames()."""
    geom = (w, h)
    refs = [ref_run(name, fr, w, h) for name, fr in frames]
    assert refs[5][1][0] == (h - 2) * (w - 31)  # the steps: every window pixel of every live row
    for i in (0, 5):  # from 384 columns the per-row uint16 wrap decides the uniform and the steps frames' sums
        assert (edge_ref.sums(refs[i][0], wrap=False)[1] != refs[i][1][1]) == (w >= 384), (geom, i)
    assert refs[2][1][0] > 0 and refs[3][1][0] > 0
    dev = upload(frames)
    sums, targets = hsv.edge_batch(dev, w, h, w)  # the fast kernel
    sums_m, targets_m, emap = hsv.edge_batch(dev, w, h, w, edges=True)  # the generic kernel, with the map
    sums, targets, sums_m, targets_m, emap = (t.cpu().numpy() for t in (sums, targets, sums_m, targets_m, emap))
    for i, (name, _) in enumerate(frames):
        want_map, (p, sx), tg = refs[i]
        assert sums[i].tolist() == [p, sx, 0], (geom, name, "fast")
        assert sums_m[i].tolist() == [p, sx, 0], (geom, name, "generic")
        assert targets[i, :3].tolist() == [tg[0], tg[1], tg[2] - 256 * (tg[2] > 127)], (geom, name)
        assert np.array_equal(targets_m[i], targets[i])
        assert np.array_equal(emap[i], want_map), (geom, name)
        # the wrap columns, the two bytes and the two rows the Sobel loop never writes
        assert np.array_equal(emap[i][:, 0], want_map[:, 0]) and np.array_equal(emap[i][:, -1], want_map[:, -1])
        flat = emap[i].reshape(-1)
        assert flat[0] == 0 and flat[w * (h - 2) - 1] == 0 and not emap[i][h - 2:].any()
    # the wrap columns carry values (they mix two rows): the comparison above is not of zeros
    assert refs[0][0][:h - 2, 0].any() and refs[0][0][:h - 2, -1].any()


@pytest.mark.parametrize("geom", GEOMS)
def test_edge_batch_vs_reference(hsv, oracle_mod, geom):
    w, h = geom
    check_frames(hsv, make_frames(oracle_mod, w, h), w, h)


# (width, dwords per lane, lane group): the classes of the fast kernel's lane
# layout that GEOMS leaves out.  Full groups (a row takes every lane of its
# group, so the column halos of its end lanes come from the neighbouring
# group or wrap inside the wave): 128, 256, 512, 1280; partial groups: 480
# (60 of 64 lanes), 544 and 992 (34 and 62 of 64), 1120 (56 of 64), 2016 (63
# of 64).  GEOMS holds the others: 32..96 (2, 16), 160 (2, 32), 352 and 384
# (2, 64), 320 (5, 16), 640 (5, 32), 1024 (4, 64), 1056 and 2048 (8, 64).
LAYOUTS = [(128, 2, 16), (256, 2, 32), (480, 2, 64), (512, 2, 64), (544, 4, 64), (992, 4, 64), (1120, 5, 64),
           (1280, 5, 64), (2016, 8, 64)]


@pytest.mark.parametrize("layout", LAYOUTS, ids=lambda v: "w%d-q%d-g%d" % v)
def test_edge_every_lane_layout(hsv, oracle_mod, layout):
    """Seven frames of H = 8 (one row segment each): no multiple of the 4 or 2
    groups a wave holds, so a wave's last live group sits beside an idle group
    and every other one beside another frame's."""
    w, q, group = layout
    assert w % (4 * q) == 0 and w // (4 * q) <= group and (group == 16 or w // (4 * q) > group // 2)
    h = 8
    frames = make_frames(oracle_mod, w, h) + [("uniform2", oracle_mod.synth(1, w, h, w, LAYOUT_OV7670, 0, 0x0DD5))]
    assert group == 64 or len(frames) % (64 // group)
    check_frames(hsv, frames, w, h)


HEIGHT_FRAMES = (0, 1, 2, 5)  # of make_frames: uniform, scene, binary, steps


# h - 2 output rows in segments of at most (h - 2) / 16: 20 is the last height
# with one segment (18 rows), 36 the first with two (17 + 17); 292 gives 18
# segments of 17 rows whose last holds one row; 308 gives 18 segments of 17
# rows where 19 are allowed.  64 columns: 2 dwords per lane, 320: 5.
@pytest.mark.parametrize("w", [64, 320])
@pytest.mark.parametrize("h", [20, 36, 292, 308])
def test_edge_heights(hsv, oracle_mod, w, h):
    all_frames = make_frames(oracle_mod, w, h)
    frames = [all_frames[i] for i in HEIGHT_FRAMES] + [("lastrow", edge_cases.last_row_frame(w, h))]
    edge_cases.check_last_row(frames[-1][1], w, h)  # points > 0, all of them in map row h - 3
    refs = [ref_run(name, fr, w, h) for name, fr in frames]
    assert refs[3][1][0] == (h - 2) * (w - 31) and refs[2][1][0] > 0
    dev = upload(frames)
    sums, targets = hsv.edge_batch(dev, w, h, w)
    sums_m, targets_m, emap = hsv.edge_batch(dev, w, h, w, edges=True)
    sums, targets, sums_m, targets_m, emap = (t.cpu().numpy() for t in (sums, targets, sums_m, targets_m, emap))
    for i, (name, _) in enumerate(frames):
        want_map, (p, sx), tg = refs[i]
        assert sums[i].tolist() == [p, sx, 0], (w, h, name, "fast")
        assert sums_m[i].tolist() == [p, sx, 0], (w, h, name, "generic")
        assert targets[i, :3].tolist() == [tg[0], tg[1], tg[2] - 256 * (tg[2] > 127)], (w, h, name)
        assert np.array_equal(targets_m[i], targets[i])
        assert np.array_equal(emap[i], want_map), (w, h, name)


# (frames, width, height): 512 frames of 64 x 2048 take 64 row segments of 32
# rows (the last of 30) where the height allows 127; 32768 frames of 64 x 36
# take one segment where the height allows two.  Smaller batches stay at the
# height's cap, as every other test here does.
@pytest.mark.parametrize("shape", [(512, 64, 2048), (32768, 64, 36)])
def test_edge_segments_follow_the_batch(hsv, oracle_mod, shape):
    """Frame i = distinct[i % 7]: every frame's sums and targets, from both kernels."""
    import torch

    n, w, h = shape
    frames = make_frames(oracle_mod, w, h) + [("lastrow", edge_cases.last_row_frame(w, h))]
    refs = [ref_run(name, fr, w, h) for name, fr in frames]
    assert all(r[1][0] > 0 for r in refs[2:]) and len({r[1] for r in refs}) == 7  # seven different results
    idx = np.arange(n) % 7
    want_sums = np.array([[r[1][0], r[1][1], 0] for r in refs], np.int64)[idx]
    want_tg = np.array([[r[2][0], r[2][1], r[2][2] - 256 * (r[2][2] > 127)] for r in refs], np.int8)[idx]
    dev = upload(frames).reshape(7, 2 * w * h)[torch.from_numpy(idx).cuda()].reshape(-1)
    assert dev.numel() == n * 2 * w * h
    sums, targets = hsv.edge_batch(dev, w, h, w)
    assert np.array_equal(sums.cpu().numpy(), want_sums)
    assert np.array_equal(targets.cpu().numpy()[:, :3], want_tg)
    sums_m, targets_m, emap = hsv.edge_batch(dev, w, h, w, edges=True)
    assert np.array_equal(sums_m.cpu().numpy(), want_sums)
    assert torch.equal(targets_m, targets)
    for i in (0, 1, 2, 3, 4, 5, 6, n - 1):
        assert np.array_equal(emap[i].cpu().numpy(), refs[i % 7][0]), (shape, i)


def sweep_inputs():
    """name -> (frames, width, height) of the threshold sweep."""
    w, h = 64, 8
    return {"levels": ([edge_ref.level_frame(w, h, lv) for lv in edge_cases.SWEEP_LEVELS], w, h),
            "ladder": ([edge_cases.noise_ladder()],) + edge_cases.LADDER_GEOM,
            "h0": ([edge_cases.h0_frame()],) + edge_cases.H0_GEOM,
            "v0": ([edge_cases.v0_frame()],) + edge_cases.V0_GEOM}


@pytest.mark.parametrize("name", ["levels", "ladder", "h0", "v0"])
def test_edge_every_threshold(hsv, name):
    """Thresholds 0 .. 255, both kernels, sums against the reference.  The
    inputs put every even magnitude 2 .. 254 and one past 255 next to every
    threshold: as a whole window (the level frames: all of it or nothing is
    detected), in each sign quadrant of (H, V) (the ladder) and on the axes
    H = 0 and V = 0."""
    import torch

    frames, w, h = sweep_inputs()[name]
    if name == "ladder":
        edge_cases.check_ladder(frames[0])
    elif name != "levels":
        edge_cases.check_axis(frames[0], w, h, name)
    sobels = [edge_ref.sobel(fr, w, h) for fr in frames]
    want = np.array([[edge_ref.sums(edge_ref.threshold(o, w, h, thr)) + (0,) for o in sobels] for thr in range(256)])
    if name == "levels":
        full = (h - 2) * (w - 31)
        for j, level in enumerate(edge_cases.SWEEP_LEVELS):
            for thr in range(256):
                assert want[thr, j, 0] == (full if level > thr or level >= 255 else 0), (level, thr)
    else:
        assert len(set(want[0::2, 0, 0].tolist())) == 128  # every even threshold selects another set
    # what the reference implies: fewer points as the threshold grows, magnitudes are even, 255 = 254
    assert (np.diff(want[:, :, 0], axis=0) <= 0).all()
    assert np.array_equal(want[0:254:2], want[1:254:2]) and np.array_equal(want[254], want[255])
    dev = torch.from_numpy(np.concatenate(frames)).cuda()
    fast = torch.stack([hsv.edge_batch(dev, w, h, w, thr)[0] for thr in range(256)]).cpu().numpy()
    generic = torch.stack([hsv.edge_batch(dev, w, h, w, thr, edges=True)[0] for thr in range(256)]).cpu().numpy()
    for thr in range(256):
        assert np.array_equal(fast[thr], want[thr]), (name, thr, "fast")
        assert np.array_equal(generic[thr], want[thr]), (name, thr, "generic")


def test_edge_thresholds(hsv):
    """49, 50, 51, 52 and 255 on one frame: low-amplitude noise (magnitudes
    around 50) left, {0, 255} right.  O is even: 50 and 51 select the same
    pixels, 49 more, 52 fewer; 255 detects only where |H| + |V| >= 255."""
    w, h = 96, 12
    rng = np.random.default_rng(3)
    fr = rng.integers(0, 256, 2 * w * h, dtype=np.uint8)
    y = fr[:w * h].reshape(h, w)
    y[:, :48] = 100 + rng.integers(0, 30, (h, 48))
    y[:, 48:] = rng.integers(0, 2, (h, 48)) * 255
    dev = upload([("t", fr)])
    got = {}
    for thr in (49, 50, 51, 52, 255):
        want_map, (p, sx), tg = ref_run("thr", fr, w, h, thr)
        sums, targets = hsv.edge_batch(dev, w, h, w, thr)
        sums_m, _, emap = hsv.edge_batch(dev, w, h, w, thr, edges=True)
        assert sums[0].tolist() == [p, sx, 0] and sums_m[0].tolist() == [p, sx, 0], thr
        assert np.array_equal(emap[0].cpu().numpy(), want_map), thr
        got[thr] = p
    o = edge_ref.sobel(fr, w, h).reshape(h, w)[:, 16:w - 15]
    assert got[255] == int((o >= 255).sum()) > 0
    assert got[49] > got[50] == got[51] > got[52] > got[255]


@pytest.mark.parametrize("geom", [(64, 8), (384, 4), (320, 240)])
def test_edge_window_edges(hsv, geom):
    """A lone bright pixel at input column x marks map columns x-1 .. x+1:
    edges up to column 15 and from column W-15 are not counted, those at
    columns 16 and W-16 are."""
    w, h = geom
    cases = [(14, 0, 0), (15, 3, 3 * 16), (w - 14, 0, 0), (w - 15, 3, 3 * (w - 16))]
    if h == 4:  # two live rows: the pixel (input row 1) marks map rows 0 and 1, not three rows
        cases = [(x, n * 2 // 3, sx * 2 // 3) for x, n, sx in cases]
    frames = [(f"x{x}", edge_ref.single_pixel(w, h, 1 if h == 4 else 3, x)) for x, _, _ in cases]
    sums, _ = hsv.edge_batch(upload(frames), w, h, w)
    sums_m, _, _ = hsv.edge_batch(upload(frames), w, h, w, edges=True)
    for i, (x, n, sx) in enumerate(cases):
        assert ref_run(("edge", x), frames[i][1], w, h)[1] == (n, sx), (geom, x)
        assert sums[i].tolist() == [n, sx, 0] and sums_m[i].tolist() == [n, sx, 0], (geom, x)


@pytest.mark.parametrize("geom", [(64, 8), (640, 8)])
def test_edge_frames_are_isolated(hsv, oracle_mod, geom):
    """Three different frames, frame_stride larger than a frame with 0xFF
    between them: map row H-3 takes nothing from the next frame, rows H-2 and
    H-1 are 0, and every frame's results are its own."""
    import torch

    w, h = geom
    fb, stride = 2 * w * h, 2 * w * h + 64
    frames = make_frames(oracle_mod, w, h)[:3]
    host = np.full(3 * stride, 0xFF, np.uint8)
    for i, (_, fr) in enumerate(frames):
        host[i * stride:i * stride + fb] = fr
    dev = torch.from_numpy(host).cuda()
    sums, targets = hsv.edge_batch(dev, w, h, w, n_frames=3, frame_stride=stride)
    sums_m, _, emap = hsv.edge_batch(dev, w, h, w, n_frames=3, frame_stride=stride, edges=True)
    for i, (name, fr) in enumerate(frames):
        want_map, (p, sx), tg = ref_run(name, fr, w, h)
        assert sums[i].tolist() == [p, sx, 0] and sums_m[i].tolist() == [p, sx, 0], (geom, name)
        got = emap[i].cpu().numpy()
        assert np.array_equal(got, want_map) and not got[h - 2:].any(), (geom, name)


@pytest.mark.parametrize("geom", [(96, 12), (640, 8)])
def test_edge_misaligned_frames(hsv, oracle_mod, geom):
    """Frames at an odd address and an odd stride: the generic kernel, equal results."""
    import torch

    w, h = geom
    fb, stride = 2 * w * h, 2 * w * h + 3
    frames = make_frames(oracle_mod, w, h)[:3]
    host = np.zeros(1 + 3 * stride, np.uint8)
    for i, (_, fr) in enumerate(frames):
        host[1 + i * stride:1 + i * stride + fb] = fr
    dev = torch.from_numpy(host).cuda()
    sums, targets = hsv.edge_batch(dev[1:], w, h, w, n_frames=3, frame_stride=stride)
    for i, (name, fr) in enumerate(frames):
        _, (p, sx), tg = ref_run(name, fr, w, h)
        assert sums[i].tolist() == [p, sx, 0], (geom, name)
        assert [int(v) & 255 for v in targets[i, :3].tolist()] == [v & 255 for v in tg], (geom, name)


# (w, h, ow, oh, oll): 1:1; the TRIK default 2:1; a portrait output (shift
# 0.75); 2x up (the gaps stay zero); H = 8 (the line's rows clamp to the frame);
# a padded output line
PREVIEWS = [(64, 8, 64, 8, 128), (320, 240, 320, 240, 640), (320, 240, 160, 120, 320), (320, 240, 240, 320, 480),
            (64, 8, 128, 16, 256), (96, 12, 48, 6, 100)]


@pytest.mark.parametrize("geom", PREVIEWS)
def test_edge_preview_vs_reference(hsv, det, oracle_mod, geom):
    w, h, ow, oh, oll = geom
    flat = np.full(2 * w * h, 90, np.uint8)  # no edge: points = 0, no line
    frames = make_frames(oracle_mod, w, h)[:4] + [("flat", flat)]
    dev = upload(frames)
    sums, _ = hsv.edge_batch(dev, w, h, w)
    pv = det.edge_preview(dev, w, h, w, sums, out_width=ow, out_height=oh, out_line_length=oll).cpu().numpy()
    assert pv.shape == (len(frames), oh, oll)
    for i, (name, fr) in enumerate(frames):
        emap, (p, sx), _ = ref_run(name, fr, w, h)
        assert p == 0 if name == "flat" else p > 0 or name != "binary"
        want = edge_ref.preview(fr, w, h, emap, p, sx, ow, oh, oll)
        assert np.array_equal(pv[i], want), (geom, name)
        px = pv[i][:, :2 * ow].copy().view("<u2")
        if name == "flat":
            assert not (px == edge_ref.LINE_PIXEL).any()
        elif h == 8:  # rows 4 +- 99 clamp to 0 .. 7: the line spans every mapped output row
            col = edge_ref.scale_maps(w, h, ow, oh)[0][min(sx // p, w - 1)]
            rows = sorted(set(edge_ref.scale_maps(w, h, ow, oh)[1]))
            assert (px[rows, col] == edge_ref.LINE_PIXEL).all()
    if (ow, oh) == (2 * w, 2 * h):  # odd output rows and columns are never written
        assert not pv[:, 1::2].any() and not pv[:, :, 2::4].any() and not pv[:, :, 3::4].any()


@pytest.mark.parametrize("thr", [0, 49, 255])
def test_edge_preview_thresholds(hsv, det, oracle_mod, thr):
    """The TRIK default geometry at other thresholds than 50: the luma of the
    conversion is the map at that threshold."""
    w, h, ow, oh, oll = PREVIEWS[2]
    frames = make_frames(oracle_mod, w, h)[:4]
    dev = upload(frames)
    sums, _ = hsv.edge_batch(dev, w, h, w, thr)
    pv = det.edge_preview(dev, w, h, w, sums, thr, out_width=ow, out_height=oh, out_line_length=oll).cpu().numpy()
    lumas = set()
    for i, (name, fr) in enumerate(frames):
        emap, (p, sx), _ = ref_run(name, fr, w, h, thr)
        assert sums[i].tolist() == [p, sx, 0]
        assert np.array_equal(pv[i], edge_ref.preview(fr, w, h, emap, p, sx, ow, oh, oll)), (thr, name)
        lumas |= set(np.unique(emap).tolist())
    assert lumas <= set(range(0, min(thr, 254) + 1, 2)) | {255} and {0, 255} <= lumas
    assert thr == 0 or max(lumas - {255}) in (thr - 1, 254)  # up to the threshold, not up to 50


def test_edge_preview_every_colour(hsv, det):
    """129 level frames at threshold 255, 1:1: the map holds 0, 2, .., 254 and
    255, and the chroma plane every (cb, cr) pair beside each of them, so the
    conversion sees every triple it can be given."""
    import torch

    w, h = edge_cases.PREVIEW_GEOM
    chroma = edge_cases.preview_chroma(w, h)
    frames = [edge_cases.preview_frame(level, chroma) for level in edge_cases.PREVIEW_LEVELS]
    refs = [edge_ref.run(fr, w, h, 255) for fr in frames]
    seen = np.zeros(1 << 24, bool)
    for fr, (emap, _, _) in zip(frames, refs):
        edge_cases.preview_triples(fr, emap, seen)
    assert int(seen.sum()) == 129 * 65536
    dev = torch.from_numpy(np.concatenate(frames)).cuda()
    sums, _ = hsv.edge_batch(dev, w, h, w, 255)
    want_sums = np.array([[p, sx, 0] for _, (p, sx), _ in refs], np.int64)
    assert np.array_equal(sums.cpu().numpy(), want_sums) and want_sums[-1, 0] == (h - 2) * (w - 31)
    pv = det.edge_preview(dev, w, h, w, torch.from_numpy(want_sums).cuda(), 255, out_width=w, out_height=h,
                          out_line_length=2 * w).cpu().numpy()
    for i, (fr, (emap, (p, sx), _)) in enumerate(zip(frames, refs)):
        want = edge_ref.preview(fr, w, h, emap, p, sx, w, h, 2 * w)
        assert np.array_equal(pv[i], want), edge_cases.PREVIEW_LEVELS[i]


def test_edge_preview_takes_the_callers_sums(hsv, det, oracle_mod):
    """The line column is int32(uint32(int32(sum_x)) / uint32(points)) clamped
    to 0 .. w-1, whatever sums the caller passes."""
    import torch

    w, h = 64, 8
    fr = oracle_mod.synth(1, w, h, w, LAYOUT_OV7670, 1, 0x7A1C, first_frame=3)
    # (points, sum_x, the line's column): in range, the upper clamp, a negative int32 (the lower clamp), no points
    cases = [(1, 0, 0), (1, w - 1, w - 1), (1, w + 500, w - 1), (2, 2**31 - 1, w - 1), (1, -1, 0),
             (3, 2**32 - 1, w - 1), (0, 5, None)]
    dev = torch.from_numpy(np.tile(fr, len(cases))).cuda()
    sums = torch.tensor([[p, sx, 0] for p, sx, _ in cases], dtype=torch.int64).cuda()
    pv = det.edge_preview(dev, w, h, w, sums, out_width=w, out_height=h, out_line_length=2 * w).cpu().numpy()
    emap = edge_ref.edge_map(fr, w, h)
    for i, (p, sx, col) in enumerate(cases):
        want = edge_ref.preview(fr, w, h, emap, p, sx, w, h, 2 * w)
        assert np.array_equal(pv[i], want), (p, sx)
        line = (pv[i].copy().view("<u2") == edge_ref.LINE_PIXEL).all(axis=0)  # H = 8: the line spans every row
        assert np.flatnonzero(line).tolist() == ([] if col is None else [col]), (p, sx)


def sensor(hsv, w, h, ow, oh, oll, streams=1):
    s = hsv.EdgeLineSensor(hsv._default_params(streams, fmt_in=hsv.FORMAT_YUV422P))
    assert s.set_params(w, h, w, out_width=ow, out_height=oh, out_line_length=oll) == 0, hsv._abi.last_error()
    return s


@pytest.mark.parametrize("geom", [(32, 4, 16, 2, 32), (64, 8, 64, 8, 128), (384, 4, 192, 2, 384),
                                  (320, 240, 320, 240, 640), (320, 240, 240, 320, 480)])
def test_edge_sensor_process(hsv, det, oracle_mod, geom):
    w, h, ow, oh, oll = geom
    s = sensor(hsv, w, h, ow, oh, oll)
    try:
        for name, fr in make_frames(oracle_mod, w, h)[:3]:
            out = np.full(oh * oll + 32, 0xAB, np.uint8)
            rc, oa = s.process(fr, out_buffer=out, hsv_range=(1, 2, 3, 4, 5, 6), auto_detect=True, input_id=7)
            assert rc == hsv.IVIDTRANSCODE_EOK, hsv._abi.last_error()
            emap, (p, sx), tg = ref_run(name, fr, w, h)
            assert (oa.alg.targetX, oa.alg.targetY, oa.alg.targetSize) == tg, (geom, name)
            assert oa.base.encodedBuf[0].bufSize == oh * oll and oa.base.bitsConsumed == fr.size * 8
            assert oa.base.outputID[0] == 7 and oa.base.outBufsInUseFlag == 0
            want = edge_ref.preview(fr, w, h, emap, p, sx, ow, oh, oll)
            assert np.array_equal(out[:oh * oll].reshape(oh, oll), want), (geom, name)
            assert not out[oh * oll:].any()  # the glue's zero fill of the whole buffer
            # process() = edge_batch + edge_preview
            import torch

            dev = torch.from_numpy(fr).cuda()
            sums, targets = hsv.edge_batch(dev, w, h, w)
            assert targets[0, :2].tolist() == [oa.alg.targetX, oa.alg.targetY]
            pv = det.edge_preview(dev, w, h, w, sums, out_width=ow, out_height=oh, out_line_length=oll)
            assert np.array_equal(pv[0].cpu().numpy(), out[:oh * oll].reshape(oh, oll))
    finally:
        s.close()


def test_edge_sensor_validation(hsv, det, oracle_mod):
    import torch

    w, h = 64, 8
    fr = oracle_mod.synth(1, w, h, w, LAYOUT_OV7670, 1, 2)
    s = sensor(hsv, w, h, 32, 4, 64)
    try:
        # SETPARAMS: a padded input line, a width that is no multiple of 32, a height that is no multiple of 4
        for bad in ((64, 8, 96), (48, 8, 48), (64, 6, 64), (4096, 8, 4096)):
            assert s.set_params(*bad, out_width=32, out_height=4, out_line_length=64) != 0, bad
            rc, oa = s.process(fr, out_buffer=np.zeros(4 * 64, np.uint8))
            assert rc == hsv.IVIDTRANSCODE_EFAIL, bad  # no algorithm until a valid SETPARAMS
        assert s.set_params(w, h, w, out_width=32, out_height=4, out_line_length=64) == 0
        # an input shorter than both planes, an output smaller than the preview
        rc, oa = s.process(fr[:w * h], out_buffer=np.zeros(4 * 64, np.uint8))
        assert rc == hsv.IVIDTRANSCODE_EFAIL and oa.base.extendedError & (1 << hsv._abi.XDM_CORRUPTEDDATA_BIT)
        rc, oa = s.process(fr, out_buffer=np.zeros(4 * 64 - 1, np.uint8))
        assert rc == hsv.IVIDTRANSCODE_EFAIL
        # the packed-YUYV input format is not this codec's
        with pytest.raises(hsv.TrikHsvError):
            hsv.EdgeLineSensor(hsv._default_params(1, fmt_in=hsv.FORMAT_YUV422))
        # still working after the failures
        rc, oa = s.process(fr, out_buffer=np.zeros(4 * 64, np.uint8))
        assert rc == 0 and (oa.alg.targetX, oa.alg.targetY, oa.alg.targetSize) == edge_ref.run(fr, w, h)[2]
    finally:
        s.close()
    # the batched calls: a padded line, the packed layout, a threshold out of range
    dev = torch.from_numpy(np.zeros(2 * 8 * 96, np.uint8)).cuda()
    with pytest.raises(hsv.TrikHsvError):
        hsv.edge_batch(dev, 64, 8, 96)
    with pytest.raises(hsv.TrikHsvError):
        hsv.edge_batch(dev, 64, 8, 64, 256)
    sums, _ = hsv.edge_batch(dev, 64, 8, 64)
    with pytest.raises(hsv.TrikHsvError):
        det.edge_preview(dev, 64, 8, 96, sums)
    with pytest.raises(hsv.TrikHsvError):  # the host-side OutArgs: a frame without columns
        hsv.edge_targets(1, 1, 0, 240)
    yuyv = hsv._abi.FrameBatch(dev.data_ptr(), 2 * 8 * 64, 1, 32, 8, 64, 0)
    assert hsv._lib.trik_hsv_edge_batch(C.byref(yuyv), 50, C.c_void_p(sums.data_ptr()), None, None, None) != 0


def test_edge_sensor_zero_output_streams(hsv, oracle_mod):
    w, h = 96, 12
    fr = oracle_mod.synth(1, w, h, w, LAYOUT_OV7670, 1, 4)
    s = sensor(hsv, w, h, 48, 6, 96, streams=0)
    try:
        out = np.full(6 * 96, 0xAB, np.uint8)
        rc, oa = s.process(fr, out_buffer=out)
        assert rc == 0 and (oa.alg.targetX, oa.alg.targetY, oa.alg.targetSize) == edge_ref.run(fr, w, h)[2]
        assert (out == 0xAB).all()  # no output stream: the buffer is left alone
    finally:
        s.close()


class MemRec(C.Structure):
    _fields_ = [("size", C.c_uint32), ("alignment", C.c_int32), ("space", C.c_int32), ("attrs", C.c_int32),
                ("base", C.c_void_p)]


class IalgFxns(C.Structure):
    _fields_ = [("implementationId", C.c_void_p), ("algActivate", C.c_void_p),
                ("algAlloc", C.CFUNCTYPE(C.c_int32, C.c_void_p, C.c_void_p, C.POINTER(MemRec))),
                ("algControl", C.c_void_p), ("algDeactivate", C.c_void_p),
                ("algFree", C.CFUNCTYPE(C.c_int32, C.c_void_p, C.POINTER(MemRec))),
                ("algInit", C.CFUNCTYPE(C.c_int32, C.c_void_p, C.POINTER(MemRec), C.c_void_p, C.c_void_p)),
                ("algMoved", C.c_void_p), ("algNumAlloc", C.c_void_p)]


class TranscodeFxns(C.Structure):
    _fields_ = [("ialg", IalgFxns),
                ("process", C.CFUNCTYPE(C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p)),
                ("control", C.CFUNCTYPE(C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p))]


def test_edge_through_the_function_table(hsv, oracle_mod):
    """A framework-style caller: algAlloc, its own record, algInit, control and
    process through TRIK_VIDTRANSCODE_CV_EDGE_LINE_FXNS, algFree.  The detect*
    OutArgs keep the caller's values."""
    w, h, ow, oh, oll = 96, 12, 48, 6, 100
    fr = binary_frame(w, h, 6)
    fx = TranscodeFxns.in_dll(hsv._lib, "TRIK_VIDTRANSCODE_CV_EDGE_LINE_FXNS")
    recs = (MemRec * 16)()
    assert fx.ialg.algAlloc(None, None, recs) == 1
    raw = C.create_string_buffer(recs[0].size + 256)
    base = (C.addressof(raw) + 255) & ~255
    recs[0].base = base
    C.c_void_p.from_address(base).value = C.addressof(fx)  # IALG_Obj.fxns, as the framework stores it
    assert fx.ialg.algInit(base, recs, None, None) == hsv.IALG_EOK, hsv._abi.last_error()
    try:
        dyn = hsv.dynamic_params(w, h, w, out_width=ow, out_height=oh, out_line_length=oll)
        st = hsv._abi.Status()
        assert fx.control(base, hsv.XDM_SETPARAMS, C.addressof(dyn), C.addressof(st)) == 0
        out = np.full(oh * oll, 0xAB, np.uint8)
        ib = hsv._abi.BufDesc1()
        ib.numBufs = 1
        ib.descs[0].buf = fr.ctypes.data
        ib.descs[0].bufSize = fr.size
        ob = hsv._abi.BufDesc()
        ob_arr, sz_arr = (C.c_void_p * 1)(out.ctypes.data), (C.c_int32 * 1)(out.nbytes)
        ob.bufs, ob.numBufs, ob.bufSizes = ob_arr, 1, sz_arr
        ia = hsv._abi.InArgs()
        ia.base.size, ia.base.numBytes = C.sizeof(hsv._abi.InArgs), fr.size
        oa = hsv._abi.OutArgs()
        oa.base.size = C.sizeof(hsv._abi.OutArgs)
        oa.alg = hsv._abi.OutArgsAlg(99, 99, 99, 11, 12, 13, 14, 15, 16)
        rc = fx.process(base, C.addressof(ib), C.addressof(ob), C.addressof(ia), C.addressof(oa))
        assert rc == hsv.IVIDTRANSCODE_EOK, hsv._abi.last_error()
        emap, (p, sx), tg = edge_ref.run(fr, w, h)
        assert p > 0 and (oa.alg.targetX, oa.alg.targetY, oa.alg.targetSize) == tg
        assert [oa.alg.detectHue, oa.alg.detectHueTolerance, oa.alg.detectSat, oa.alg.detectSatTolerance,
                oa.alg.detectVal, oa.alg.detectValTolerance] == [11, 12, 13, 14, 15, 16]
        assert np.array_equal(out.reshape(oh, oll), edge_ref.preview(fr, w, h, emap, p, sx, ow, oh, oll))
    finally:
        assert fx.ialg.algFree(base, recs) == 1
