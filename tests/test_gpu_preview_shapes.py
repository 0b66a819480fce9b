"""The object sensors' RGB565X preview (trik_hsv_batch_preview and
ObjectSensor.process: preview_rows2_kernel, preview_gather_kernel and
overlay_kernel of trik-media-sensors-dsp_amd/csrc/trik_hsv_operator.hip) through every form the launcher
can pick, byte for byte:

A. the grid-stride loops: batches large enough that every lane of
   preview_rows2_kernel takes three units or more (every wave of
   preview_gather_kernel three chunks), every frame different, each preview
   against oracle.run of its frame -- and the line sensor's and the multi-blob
   sensor's instantiations of the rows kernel against oracle.line_run and
   oracle.blob_run;
B. every (Y, U, V) through the preview's own colour arithmetic, RGB565X
   packing and detection, in both kernels, both layouts, a hue-bounded and a
   hue-free range;
C. the target circle from the caller's sums: centres on corners and edges, the
   smallest and the largest radii, sums whose low words decide; and the
   corner-block frames through ObjectSensor.process;
D. the launcher's other branches: the overlay's maps read from memory, each
   condition under which the rows kernel must refuse, the gather's byte loads
   and stores.

The inputs and the launcher's restated decision are tests/preview_cases.py's;
tests/test_preview_cpu.py asserts what each input reaches and holds
tests/preview_ref.py to oracle.run.  Each test asserts the restated decision
for the device's own CU count before it runs.
"""
import ctypes as C
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import preview_cases as pc
import preview_ref
from preview_ref import LAYOUT_OV7670, LAYOUT_YUYV

pytestmark = pytest.mark.gpu

SEED = 0x51A9
SENTINEL = 0xA5
LINE_RANGE = (0, 70)
WORKERS = min(16, os.cpu_count() or 1)


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


def _cus():
    import torch

    return torch.cuda.get_device_properties(0).multi_processor_count


def _threaded(fn, n):
    """[fn(f) for f in range(n)], the frames split among threads (the oracle's
    calls release the GIL)."""
    if n < 4 * WORKERS:
        return [fn(f) for f in range(n)]
    parts = [range(i * n // WORKERS, (i + 1) * n // WORKERS) for i in range(WORKERS)]
    with ThreadPoolExecutor(WORKERS) as ex:
        return [r for part in ex.map(lambda rg: [fn(f) for f in rg], parts) for r in part]


def _oracle_previews(oracle_mod, host, c, outargs=False):
    """oracle.run of every frame of case c (frames at c.frame_stride in host)."""
    def one(f):
        fr = host[f * c.frame_stride:f * c.frame_stride + c.fb]
        rc, oa, pv = oracle_mod.run(fr, c.w, c.h, c.ll, c.layout, c.rng, out_width=c.ow, out_height=c.oh,
                                    out_line_length=c.oll)
        assert rc == 0
        return (oa, pv) if outargs else pv

    return _threaded(one, c.n)


def _same(got, want, what):
    """got, want: uint8 [n, bytes]."""
    got, want = np.asarray(got).reshape(len(want), -1), np.asarray(want)
    bad = np.flatnonzero((got != want).any(axis=1))
    if bad.size:
        f = int(bad[0])
        at = np.flatnonzero(got[f] != want[f])
        raise AssertionError("%s: %d of %d previews differ, first %d at bytes %s: got %s, want %s" % (
            what, bad.size, len(want), f, at[:6].tolist(), got[f][at[:6]].tolist(), want[f][at[:6]].tolist()))


def _synth(hsv, c):
    """c.n different frames on the device: kind 0 (uniform bytes) and kind 1
    (scene) alternate.  Returns (device tensor, host copy)."""
    import torch

    dev = torch.empty(c.n * c.fb, dtype=torch.uint8, device="cuda")
    hsv.synth(dev, c.w, c.h, c.ll, c.layout, 0, SEED, first_frame=0, n_frames=(c.n + 1) // 2, frame_stride=2 * c.fb)
    hsv.synth(dev[c.fb:], c.w, c.h, c.ll, c.layout, 1, SEED, first_frame=1, n_frames=c.n // 2, frame_stride=2 * c.fb)
    host = dev.cpu().numpy()
    rows = host.reshape(c.n, c.fb)
    assert len({r.tobytes() for r in rows}) == c.n, "every frame is different"
    return dev, host


def _place(c, host):
    """The case's frames on the device at its offset from a 16-byte boundary."""
    import torch

    span = (c.n - 1) * c.frame_stride + c.fb
    raw = torch.full((span + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
    assert raw.data_ptr() % 16 == 0
    frames = raw[c.frames_offset:c.frames_offset + span]
    frames.copy_(torch.from_numpy(np.ascontiguousarray(host[:span])))
    return frames


def _call(hsv, det, c, frames, *args, sums_pitch=1):
    """The case's preview entry point through the C ABI: trik_hsv_batch_preview
    (args: sums), trik_hsv_line_preview (val_from, val_to, sums) or
    trik_hsv_blob_preview (meta, top), on `frames` (a device tensor that starts
    at the first frame), the previews at the case's offset and stride inside a
    sentinel-filled buffer -- so a preview byte the kernels do not write
    shows, and so does a write outside the previews.  Returns uint8 [n, pb]."""
    import torch

    assert frames.data_ptr() % 16 == c.frames_offset
    pspan = (c.n - 1) * c.preview_stride + c.pb
    raw_p = torch.full((pspan + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
    assert raw_p.data_ptr() % 16 == 0
    b = hsv._abi.FrameBatch(frames.data_ptr(), c.frame_stride, c.n, c.w, c.h, c.ll, c.layout)
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    tail = (c.ow, c.oh, c.oll, C.c_void_p(raw_p.data_ptr() + c.previews_offset), c.preview_stride,
            C.c_void_p(torch.cuda.current_stream().cuda_stream))
    if c.entry == "batch":
        arr, _ = hsv._ranges([c.rng])
        rc = hsv._lib.trik_hsv_batch_preview(det._h, C.byref(b), arr, ptr(args[0]), sums_pitch, *tail)
    elif c.entry == "line":
        rc = hsv._lib.trik_hsv_line_preview(det._h, C.byref(b), int(args[0]), int(args[1]), ptr(args[2]), *tail)
    else:
        rc = hsv._lib.trik_hsv_blob_preview(det._h, C.byref(b), ptr(args[0]), ptr(args[1]), *tail)
    assert rc == 0, hsv._abi.last_error()
    out = raw_p.cpu().numpy()
    keep = np.ones(out.size, bool)
    for f in range(c.n):
        keep[c.previews_offset + f * c.preview_stride:c.previews_offset + f * c.preview_stride + c.pb] = False
    assert (out[keep] == SENTINEL).all(), (c, "bytes outside the previews were written")
    if c.preview_stride == c.pb:
        return out[c.previews_offset:c.previews_offset + c.n * c.pb].reshape(c.n, c.pb)
    return np.stack([out[c.previews_offset + f * c.preview_stride:][:c.pb] for f in range(c.n)])


def _frame_sums(hsv, det, c, frames):
    sums, _ = det.process_batch(frames, c.w, c.h, c.ll, c.layout, [c.rng], n_frames=c.n, frame_stride=c.frame_stride)
    return sums


# ---------------------------------------------------------------- A. grid passes

def _grid_case(name):
    return next(c for c in pc.grid_cases(_cus()) if c.name == name)


def _assert_rounds(c, plan):
    assert plan["grid"] == 2 * _cus() and plan["min_units"] >= 3 and plan["partial"], (c, plan)


GRID_NAMES = [c.name for c in pc.grid_cases(1) if c.entry == "batch"]


@pytest.mark.parametrize("name", GRID_NAMES)
def test_grid_passes(hsv, det, oracle_mod, name):
    """Every lane (wave) of the full grid takes three units (chunks) or more,
    the last round is partial; frame f's preview is oracle.run of frame f."""
    c = _grid_case(name)
    f = c.forms(_cus())
    assert f["kernel"] == ("gather" if "gather" in name else "rows2") and f["hue_free"] == pc.hue_free(c.rng), f
    _assert_rounds(c, f)
    dev, host = _synth(hsv, c)
    sums = _frame_sums(hsv, det, c, dev)
    pv = _call(hsv, det, c, dev, sums)
    want = _oracle_previews(oracle_mod, host, c)
    _same(pv, want, (name, f))
    assert int((sums[:, 0, 0] > 0).sum()) > c.n // 4  # circles are drawn: the overlay reads frame f's sums


def test_grid_passes_line_preview(hsv, det, oracle_mod):
    """The OVL instantiation (the line sensor's preview on 2:1 maps): the
    later rounds read the advanced frame's sums for its target line."""
    c = _grid_case("grid_line")
    assert pc.rows2_maps(c.w, c.h, c.ow, c.oh)[0] >= 0
    _assert_rounds(c, pc.rows2_plan(c.n, c.ow, c.oh, _cus()))
    dev, host = _synth(hsv, c)
    vf, vt = LINE_RANGE
    sums, _ = hsv.line_batch(dev, c.w, c.h, c.ll, vf, vt, n_frames=c.n)
    pv = _call(hsv, det, c, dev, vf, vt, sums)

    def one(f):
        rc, _, p, s, _ = oracle_mod.line_run(host[f * c.fb:(f + 1) * c.fb], c.w, c.h, c.ll, vf, vt, out_width=c.ow,
                                             out_height=c.oh, out_line_length=c.oll)
        assert rc == 0
        return p, int(s[0]), int(s[1]) // max(int(s[0]), 1)

    ref = _threaded(one, c.n)
    _same(pv, [r[0] for r in ref], "line_preview")
    drawn = {r[2] for r in ref if r[1] > 10}
    assert len(drawn) > 8, "the target lines stand at many columns"


def test_grid_passes_blob_preview(hsv, det, oracle_mod):
    """The META instantiation (the multi-blob preview on 2:1 maps): the later
    rounds read the advanced frame's metapixels."""
    c = _grid_case("grid_blob")
    assert pc.rows2_maps(c.w, c.h, c.ow, c.oh)[0] >= 0
    _assert_rounds(c, pc.rows2_plan(c.n, c.ow, c.oh, _cus()))
    dev, host = _synth(hsv, c)
    res = det.blob_batch(dev, c.w, c.h, c.ll, oracle_mod.RED_HSV, meta=True)
    pv = _call(hsv, det, c, dev, res["meta"], res["top"])

    def one(f):
        r = oracle_mod.blob_run(host[f * c.fb:(f + 1) * c.fb], c.w, c.h, c.ll, hsv=oracle_mod.RED_HSV, out_width=c.ow,
                                out_height=c.oh, out_line_length=c.oll)
        assert r["rc"] == 0
        return r["preview"], r["meta"].tobytes()

    ref = _threaded(one, c.n)
    _same(pv, [r[0] for r in ref], "blob_preview")
    assert len({r[1] for r in ref}) > c.n // 4, "the frames' metapixel bitmaps differ"


# ------------------------------------------ B. every (Y, U, V) through the preview

_shared = {}


def _triple_mask(oracle_mod, rng):
    """The oracle's detection of every (Y, U, V) under rng, uint8 [2^24]
    indexed as the table: oracle.frame's mask of the exhaustive YUYV frame (in
    bands of rows, threaded), read back per triple."""
    if ("mask", rng) not in _shared:
        from gpu_util import exhaustive_yuyv_frame

        fr, w, h, ll = exhaustive_yuyv_frame()
        bands = 16
        rows = h // bands
        parts = _threaded(lambda i: oracle_mod.frame(fr[i * rows * ll:(i + 1) * rows * ll], w, rows, ll, LAYOUT_YUYV,
                                                     [rng], want_mask=True)[1], bands)
        mask = np.concatenate(parts).reshape(-1)
        t = np.arange(1 << 24, dtype=np.int64)
        Y, U, V = t & 255, (t >> 8) & 255, t >> 16
        # gpu_util.exhaustive_yuyv_frame: pair p = U | V << 8 | (Y >> 1) << 16, pixel 2 p + (Y & 1)
        _shared[("mask", rng)] = mask[2 * (U | (V << 8) | ((Y >> 1) << 16)) + (Y & 1)]
    return _shared[("mask", rng)]


def _frames_of(kind, layout):
    """The exhaustive frame / the sampled batch of a layout (the last one built is kept)."""
    if _shared.get("frames_key") != (kind, layout):
        _shared["frames_key"], _shared["frames"] = None, None
        _shared["frames"] = pc.exhaustive_frame(layout) if kind == "gather" else pc.sampled_batch(layout)
        _shared["frames_key"] = (kind, layout)
    return _shared["frames"]


def _triple_report(table, host, c, got, want, limit=5):
    """The first differing output pixels as (Y, U, V, got, want)."""
    last_row, last_col = preview_ref.last_writers(c.w, c.h, c.ow, c.oh)
    out = []
    for f in range(c.n):
        g = got[f].reshape(c.oh, c.oll)[:, :2 * c.ow].reshape(c.oh, c.ow, 2)
        w_ = want[f].reshape(c.oh, c.oll)[:, :2 * c.ow].reshape(c.oh, c.ow, 2)
        for r, col in np.argwhere((g != w_).any(axis=2))[:limit].tolist():
            idx = int(preview_ref.yuv_index(host[f * c.fb:(f + 1) * c.fb], c.w, c.h, c.ll, c.layout, [last_row[r]],
                                            [last_col[col]])[0, 0])
            out.append((idx & 255, (idx >> 8) & 255, idx >> 16, hex(int(g[r, col, 0]) | int(g[r, col, 1]) << 8),
                        hex(int(w_[r, col, 0]) | int(w_[r, col, 1]) << 8)))
        if len(out) >= limit:
            break
    return out[:limit]


@pytest.mark.parametrize("c", pc.exhaustive_cases(), ids=repr)
def test_every_triple(hsv, det, oracle_mod, table, c):
    """gather: the exhaustive frame at identity scale.  rows2: the
    sampled-exhaustive batch, every triple at a pixel the 2:1 maps sample
    (there also under a hue-free range that bounds the saturation).
    Expected: preview_ref.body from the oracle's table and mask, plus the
    guide lines; the sums hold no points, so no circle."""
    import torch

    kind, layout, rng = ("gather" if "gather" in c.name else "rows2"), c.layout, c.rng
    f = c.forms(_cus())
    assert f["kernel"] == kind and f["hue_free"] == (rng is not pc.T0) and (kind == "gather" or f["guides"]), f
    host = _frames_of(kind, layout)
    mask = _triple_mask(oracle_mod, rng)
    assert 0 < int(mask.sum()) < mask.size
    dev = torch.from_numpy(host).cuda()
    sums = torch.zeros((c.n, 3), dtype=torch.int64, device="cuda")
    sums[:, 1:] = 12345  # (no points: the sums of x and y must not matter)
    pv = _call(hsv, det, c, dev, sums)
    want = _threaded(lambda i: preview_ref.preview(
        preview_ref.body(table, mask, host[i * c.fb:(i + 1) * c.fb], c.w, c.h, c.ll, c.layout, c.ow, c.oh, c.oll),
        c.w, c.h, c.ow, c.oh, c.oll, (0, 0, 0)).reshape(-1), c.n)
    want = np.stack(want)
    if not np.array_equal(pv, want):
        raise AssertionError("%s: (Y, U, V, got, want) %s" % (c, _triple_report(table, host, c, pv, want)))


# ------------------------------------------- C. the circle from the caller's sums

@pytest.mark.parametrize("geom", pc.CIRCLE_GEOMS, ids=["%dx%d_%dx%d" % g for g in pc.CIRCLE_GEOMS])
@pytest.mark.parametrize("layout", [LAYOUT_YUYV, LAYOUT_OV7670], ids=["yuyv", "ov7670"])
def test_circle_from_callers_sums(hsv, det, oracle_mod, table, layout, geom):
    """One frame tiled, one sums row per preview (preview_cases.circle_sums);
    expected: preview_ref.preview over the frame's own body."""
    import torch

    w, h, ow, oh = geom
    cases = pc.circle_sums(w, h)
    c = pc.Case("circle", w, h, layout, ow, oh, len(cases))
    f = c.forms(_cus())
    assert (f["kernel"], f["guides"]) == (("rows2", True) if (ow, oh) == (w // 2, h // 2) else ("gather", False)), f
    fr = pc.corner_block(table, c.rng, w, h, c.ll, layout, "centre")
    _, mask = oracle_mod.frame(fr, w, h, c.ll, layout, [c.rng], want_mask=True)
    assert mask.any()
    body = preview_ref.body(table, mask, fr, w, h, c.ll, layout, ow, oh, c.oll)
    want = [preview_ref.preview(body, w, h, ow, oh, c.oll, s).reshape(-1) for _, s in cases]
    assert not np.array_equal(want[0], want[-1])
    # pitch 2: the rows between hold other sums
    sums = torch.full((c.n, 2, 3), 7, dtype=torch.int64)
    sums[:, 0] = torch.tensor([list(s) for _, s in cases], dtype=torch.int64)
    pv = _call(hsv, det, c, _place(c, np.tile(fr, c.n)), sums.cuda(), sums_pitch=2)
    for i, (name, s) in enumerate(cases):
        assert np.array_equal(pv[i], want[i]), (geom, name, s, np.flatnonzero(pv[i] != want[i])[:6].tolist())


@pytest.mark.parametrize("geom", pc.CIRCLE_GEOMS, ids=["%dx%d_%dx%d" % g for g in pc.CIRCLE_GEOMS])
@pytest.mark.parametrize("layout", [LAYOUT_YUYV, LAYOUT_OV7670], ids=["yuyv", "ov7670"])
def test_process_corner_targets(hsv, oracle_mod, table, layout, geom):
    """The corner-block frames through the codec's process(): the sums come
    from the kernels; preview and OutArgs against oracle.run."""
    w, h, ow, oh = geom
    ll, oll = pc.line_length(w, layout), 2 * ow
    fmt = hsv.FORMAT_YUV422 if layout == LAYOUT_YUYV else hsv.FORMAT_YUV422P
    s = hsv.ObjectSensor(hsv._default_params(1, fmt, 640, 480))
    try:
        assert s.set_params(w, h, ll, out_width=ow, out_height=oh, out_line_length=oll) == 0
        for rng in (pc.T0, pc.V_BAND):
            for name in pc.PLACES:
                fr = pc.corner_block(table, rng, w, h, ll, layout, name)
                out = np.full(oh * oll + 16, 0xCD, np.uint8)
                rc, oa = s.process(fr, rng, out_buffer=out)
                rc_o, want, preview = oracle_mod.run(fr, w, h, ll, layout, rng, out_width=ow, out_height=oh,
                                                     out_line_length=oll)
                assert rc == rc_o == 0
                assert (oa.alg.targetX, oa.alg.targetY, oa.alg.targetSize) == (
                    want["target_x"], want["target_y"], want["target_size"]), (name, rng)
                bad = np.flatnonzero(out[:oh * oll] != preview)
                assert bad.size == 0, (name, rng, bad[:6].tolist())
                assert not out[oh * oll:].any()  # the zero fill of the whole buffer (WFXNS:234)
    finally:
        s.close()


# --------------------------------------------------- D. launcher branches

def _corner_frames(table, c, names):
    fr = [pc.corner_block(table, c.rng, c.w, c.h, c.ll, c.layout, name) for name in names]
    host = np.zeros((c.n - 1) * c.frame_stride + c.fb, np.uint8)
    for f in range(c.n):
        host[f * c.frame_stride:f * c.frame_stride + c.fb] = fr[f % len(fr)]
    return host


@pytest.mark.parametrize("c", pc.overlay_memory_cases(), ids=repr)
def test_overlay_maps_from_memory(hsv, det, oracle_mod, table, c):
    """w + h > 8192: overlay_kernel<false> draws the circle (and, after the
    gather, the guide lines) through the maps in memory; corner targets."""
    f = c.forms(_cus())
    assert not f["overlay_lds"] and f["kernel"] == ("rows2" if "2to1" in c.name else "gather"), f
    host = _corner_frames(table, c, ("tl", "br"))
    dev = _place(c, host)
    sums = _frame_sums(hsv, det, c, dev)
    assert int(sums[:, 0, 0].min()) > 0
    pv = _call(hsv, det, c, dev, sums)
    _same(pv, _oracle_previews(oracle_mod, host, c), (c, f))


def _noise_frames(oracle_mod, c):
    return oracle_mod.synth(c.n, c.w, c.h, c.ll, c.layout, 1, SEED, first_frame=5, frame_stride=c.frame_stride)


def _run_placed(hsv, det, oracle_mod, c):
    """Case c on scene frames with their own sums, against oracle.run."""
    import torch

    host = _noise_frames(oracle_mod, c)
    sums = _frame_sums(hsv, det, c, torch.from_numpy(host).cuda())  # (from an aligned copy of the frames)
    pv = _call(hsv, det, c, _place(c, host), sums)
    _same(pv, _oracle_previews(oracle_mod, host, c), (c, c.forms(_cus())))
    return pv


@pytest.mark.parametrize("layout", [LAYOUT_YUYV, LAYOUT_OV7670], ids=["yuyv", "ov7670"])
def test_rows_kernel_refusals(hsv, det, oracle_mod, layout):
    """2:1 maps: the aligned call runs the rows kernel; six of launch_rows2's
    conditions, each broken alone, and out_w % 8 with the width test it cannot
    be parted from (preview_cases' docstring), send the call to the gather,
    which must write the same previews."""
    twin, refused = pc.refusal_cases()[0 if layout == LAYOUT_YUYV else 1]
    assert twin.forms(_cus())["kernel"] == "rows2"
    _run_placed(hsv, det, oracle_mod, twin)
    for c in refused:
        f = c.forms(_cus())
        assert f["kernel"] == "gather" and f["refused"][0] == c.name.split("_", 2)[2], (c, f)
        _run_placed(hsv, det, oracle_mod, c)


@pytest.mark.parametrize("c", pc.byte_path_cases(), ids=repr)
def test_gather_byte_path(hsv, det, oracle_mod, c):
    """aligned4 == 0, one cause at a time: fetch_yuv's byte loads in both
    layouts and the byte stores; nothing outside the previews is written."""
    f = c.forms(_cus())
    assert f["kernel"] == "gather" and f["loads"] == "byte", f
    _run_placed(hsv, det, oracle_mod, c)
