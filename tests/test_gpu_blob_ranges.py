"""The multi-blob sensor for several HSV ranges per call, on ov7670 and packed
YUYV frames (trik_hsv_blob_batch_ranges): every (frame, range) slot against
the oracle's run of the ov7670 frame with that range as the sticky state
(tests/test_oracle_blob_ranges.py ties the YUYV twin, the packed-state form
and every frame builder to the oracle on the CPU) -- bitmap, label map, label
count, the 8 largest clusters and the 8 targets, bit-exact."""
import ctypes as C

import numpy as np
import pytest

import blob_ranges_cases as cases

pytestmark = pytest.mark.gpu

OV, YUYV = 1, 0
SENTINEL = 0x5A


@pytest.fixture(scope="module")
def hsv():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import trik_hsv

    return trik_hsv


@pytest.fixture
def det(hsv):
    d = hsv.Detector()
    yield d
    d.close()


_frames_cache, _ref_cache = {}, {}


def _geom_frames(oracle_mod, w, h, ll):
    """Two mosaics of clusterer patterns, a scene and uniform random bytes."""
    key = (w, h, ll)
    if key not in _frames_cache:
        bh, bw = h // 4, w // 4
        _frames_cache[key] = [cases.mosaic(cases.pattern_stack(bh, bw, 4, 0), ll, seed=1),
                              cases.mosaic(cases.pattern_stack(bh, bw, 4, 5), ll, seed=2),
                              oracle_mod.blob_scene(w, h, ll, 3, noise=0.03),
                              np.random.default_rng(4).integers(0, 256, 2 * h * ll, dtype=np.uint8)]
    return _frames_cache[key]


def _ref(oracle_mod, key, fr, w, h, ll, rng):
    """One oracle run per (frame, range), shared by the tests and layouts."""
    k = (key, w, h, ll, rng)
    if k not in _ref_cache:
        _ref_cache[k] = cases.expect(oracle_mod, fr, w, h, ll, rng)
    return _ref_cache[k]


def _device_batch(frames, w, h, ll, layout, ll_yuyv=None, stride=None, offset=0):
    """The frames (ov7670, host) as one device tensor of `layout`; returns
    (tensor, line length, frame stride)."""
    import torch

    if layout == YUYV:
        frames = [cases.to_yuyv(fr, w, h, ll, ll_yuyv, seed=i) for i, fr in enumerate(frames)]
        ll = ll_yuyv
    fb = len(frames[0])
    stride = fb if stride is None else stride
    host = np.full(offset + stride * len(frames), 0xA5, np.uint8)
    for i, fr in enumerate(frames):
        host[offset + i * stride: offset + i * stride + fb] = fr
    return torch.from_numpy(host).cuda()[offset:], ll, stride


def _run(det, frames, w, h, ll, ranges, layout, **kw):
    dev, ll_dev, stride = _device_batch(frames, w, h, ll, layout, **kw)
    res = det.blob_batch_ranges(dev, w, h, ll_dev, ranges, layout=layout, n_frames=len(frames), frame_stride=stride,
                                meta=True, labels=True)
    return {k: v.cpu() for k, v in res.items()}


def _check_all(oracle_mod, res, frames, keys, w, h, ll, ranges, what):
    for f, fr in enumerate(frames):
        for t, rng in enumerate(ranges):
            cases.check_slot(res, f, t, _ref(oracle_mod, keys[f], fr, w, h, ll, rng), (what, "frame", f, "range", t))


LAYOUTS = [("ov7670", OV, 0), ("yuyv", YUYV, 0), ("yuyv_padded", YUYV, 16)]


@pytest.mark.parametrize("t", [1, 2, 4, 5, 9])
@pytest.mark.parametrize("layout", LAYOUTS, ids=[x[0] for x in LAYOUTS])
@pytest.mark.parametrize("geom", [(32, 4, 32), (64, 32, 80), (352, 96, 352), (320, 240, 352)])
def test_every_slot_vs_oracle(hsv, det, oracle_mod, geom, layout, t):
    """T = 4: one full group; 5: a last group of one range; 9: three groups."""
    w, h, ll = geom
    _, lay, pad = layout
    frames = _geom_frames(oracle_mod, w, h, ll)
    ranges = cases.ranges_for(t)
    res = _run(det, frames, w, h, ll, ranges, lay, ll_yuyv=2 * w + pad)
    assert det.last_hot_kernel() == hsv.HOT_STRIPE
    _check_all(oracle_mod, res, frames, [(geom, i) for i in range(len(frames))], w, h, ll, ranges, (geom, layout, t))


@pytest.mark.parametrize("hot", ["stripe", "chroma"])
def test_same_as_the_single_range_call(hsv, oracle_mod, hot):
    """ov7670: slot (f, t) is bit-identical to blob_batch with range t's
    centre/tolerance, whichever bitmap kernel that call runs; the hot-kernel
    setting does not reach the ranges call."""
    import torch

    w, h, ll = 320, 240, 320
    frames = _geom_frames(oracle_mod, w, h, ll)
    dev, _, _ = _device_batch(frames, w, h, ll, OV)
    d = hsv.Detector(hot=hsv.HOT_CHROMA if hot == "chroma" else hsv.HOT_STRIPE)
    try:
        res = d.blob_batch_ranges(dev, w, h, ll, [hsv.blob_range_of(x) for x in cases.ALL_HSV], meta=True, labels=True)
        assert d.last_hot_kernel() == hsv.HOT_STRIPE
        for t, x in enumerate(cases.ALL_HSV):
            one = d.blob_batch(dev, w, h, ll, x, meta=True, labels=True)
            assert d.last_hot_kernel() == (hsv.HOT_CHROMA if hot == "chroma" else hsv.HOT_STRIPE)
            for key in ("targets", "top", "n_labels", "meta", "labels"):
                assert torch.equal(res[key][:, t], one[key]), (hot, t, key)
    finally:
        d.close()


@pytest.mark.parametrize("layout", LAYOUTS[:2], ids=["ov7670", "yuyv"])
def test_byte_lanes(det, oracle_mod, layout):
    """The four ranges of a group count side by side in one register."""
    _, lay, _ = layout
    # one colour under four nested ranges that all hold it: counts (16, 16, 16, 16)
    red = cases.mosaic(np.ones((1, 1, 8), np.uint8), counts=np.full((1, 1, 8), 16))
    nested = [(340, 20, 60, 100, 0, 100), cases.from_to(cases.WRAP_HSV), (0, 359, 0, 100, 0, 100),
              (300, 60, 50, 100, 0, 100)]
    res = _run(det, [red], 32, 4, 32, nested, lay, ll_yuyv=64)
    assert res["meta"].all()
    _check_all(oracle_mod, res, [red], ["red"], 32, 4, 32, nested, "nested")
    # k = 0..16 in range 0 next to fixed counts 2, 3 and 16 in the same metapixels
    fr, k = cases.lane_ladder()
    res = _run(det, [fr], 96, 4, 96, cases.LANE_RANGES, lay, ll_yuyv=192)
    meta = res["meta"][0].numpy()
    assert np.array_equal(meta[0, 0], k > 2), meta[0, 0]
    assert not meta[1].any() and meta[2].all() and meta[3].all()
    _check_all(oracle_mod, res, [fr], ["lanes"], 96, 4, 96, cases.LANE_RANGES, "ladder")
    # the ladder in each lane in turn, the other lanes holding other colours' ladders
    frames, counts = zip(*[cases.ladder(t) for t in range(4)])
    ranges = cases.ranges_for(4)
    res = _run(det, list(frames), 96, 4, 96, ranges, lay, ll_yuyv=192)
    for t in range(4):
        for r in range(4):
            want = counts[t] > 2 if r == t else np.zeros(24, bool)
            assert np.array_equal(res["meta"][t, r, 0].numpy(), want), (t, r)
    _check_all(oracle_mod, res, frames, [("ladder", t) for t in range(4)], 96, 4, 96, ranges, "ladders")


def test_byte_load_path(det, oracle_mod):
    """Batches that are not 4-byte aligned: an ov7670 line length of 322, and
    YUYV frames at a base pointer 2 bytes off with a line length of 2w + 2."""
    ranges = cases.ranges_for(5)
    w, h, ll = 320, 48, 322
    frames = _geom_frames(oracle_mod, w, h, ll)
    res = _run(det, frames, w, h, ll, ranges, OV)
    _check_all(oracle_mod, res, frames, [((w, h, ll), i) for i in range(4)], w, h, ll, ranges, "ov7670 ll 322")
    w, h, ll = 64, 32, 80
    frames = _geom_frames(oracle_mod, w, h, ll)
    res = _run(det, frames, w, h, ll, ranges, YUYV, ll_yuyv=2 * w + 2, offset=2)
    _check_all(oracle_mod, res, frames, [((w, h, ll), i) for i in range(4)], w, h, ll, ranges, "yuyv + 2")


@pytest.mark.parametrize("layout", LAYOUTS[:2], ids=["ov7670", "yuyv"])
def test_grid_stride(det, oracle_mod, layout):
    """32 frames of 320 x 240 are 153,600 metapixels: more than one grid pass
    (2 x CUs x 256, 131,072 at 256 CUs) holds."""
    _, lay, _ = layout
    w, h, ll = 320, 240, 352
    four = _geom_frames(oracle_mod, w, h, ll)
    frames = [four[(i + i // 4) % 4] for i in range(32)]
    keys = [((w, h, ll), (i + i // 4) % 4) for i in range(32)]
    ranges = cases.ranges_for(2)
    res = _run(det, frames, w, h, ll, ranges, lay, ll_yuyv=2 * w)
    _check_all(oracle_mod, res, frames, keys, w, h, ll, ranges, "grid stride")


@pytest.mark.parametrize("n,t,crosses", [(1100, 4, True), (1100, 3, False), (1400, 3, True)])
def test_chunk_boundary(hsv, det, oracle_mod, n, t, crosses):
    """More slots than BLOB_CHUNK_SLOTS: 1100 frames x 4 ranges are 4400 slots
    in chunks of 1024 frames.  With 3 ranges a chunk is 1365 frames (4095
    slots, the constant does not divide): 1100 frames stay just inside one
    chunk, 1400 frames cross into a second."""
    chunk = max(1, hsv.BLOB_CHUNK_SLOTS // t)
    assert (n > chunk) == crosses and (n * t > hsv.BLOB_CHUNK_SLOTS) == crosses
    w, h, ll = 32, 4, 32
    # one tall mosaic, cut into frames of one metapixel row
    tall = cases.mosaic(np.stack([np.random.default_rng(10 + i).random((n, 8)) < 0.5 for i in range(4)]), seed=n)
    y, c = tall[: 4 * n * ll].reshape(n, 4 * ll), tall[4 * n * ll:].reshape(n, 4 * ll)
    frames = [np.concatenate([y[f], c[f]]) for f in range(n)]
    ranges = cases.ranges_for(t)
    res = _run(det, frames, w, h, ll, ranges, OV)
    for f, fr in enumerate(frames):
        edge = next((b for b in range(chunk, n, chunk) if f in (b - 1, b)), None)
        where = f"frame {f}" + (f" (chunk boundary between frames {edge - 1} and {edge})" if edge else "")
        for r, rng in enumerate(ranges):
            cases.check_slot(res, f, r, cases.expect(oracle_mod, fr, w, h, ll, rng), (where, "range", r))


def _raw(hsv, det_h, b, ranges, outs, n_ranges=None, null=()):
    """trik_hsv_blob_batch_ranges itself on sentinel-filled outputs."""
    arr, n = hsv._ranges(ranges)
    ptr = {k: (None if k in null else C.c_void_p(v.data_ptr())) for k, v in outs.items()}
    return hsv._lib.trik_hsv_blob_batch_ranges(
        det_h, C.byref(b) if b is not None else None, None if "ranges" in null else arr,
        n if n_ranges is None else n_ranges, ptr["targets"], ptr["top"], ptr["meta"], ptr["labels"], ptr["n_labels"],
        None)


def _sentinels(n, t, w, h):
    import torch

    shape = {"targets": (n, t, 8, 4), "top": (n, t, 8, 12), "meta": (n, t, h // 4, w // 4),
             "labels": (n, t, h // 4, w // 4 * 2), "n_labels": (n, t, 4)}
    return {k: torch.full(s, SENTINEL, dtype=torch.uint8, device="cuda") for k, s in shape.items()}


def _untouched(outs):
    import torch

    torch.cuda.synchronize()
    return all(bool((v == SENTINEL).all()) for v in outs.values())


def test_strided_and_empty(hsv, det, oracle_mod):
    import torch

    w, h, ll = 64, 32, 80
    frames = _geom_frames(oracle_mod, w, h, ll)
    ranges = cases.ranges_for(3)
    keys = [((w, h, ll), i) for i in range(4)]
    for lay, kw in ((OV, dict(stride=2 * h * ll + 24)), (YUYV, dict(ll_yuyv=2 * w, stride=2 * w * h + 40))):
        res = _run(det, frames, w, h, ll, ranges, lay, **kw)
        _check_all(oracle_mod, res, frames, keys, w, h, ll, ranges, ("strided", lay))
    # no frame: nothing is touched
    dev, _, _ = _device_batch(frames, w, h, ll, OV)
    outs = _sentinels(2, 3, w, h)
    b = hsv._batch(dev, w, h, ll, OV, n_frames=0)
    assert _raw(hsv, det._h, b, ranges, outs) == 0 and _untouched(outs)
    res = det.blob_batch_ranges(dev, w, h, ll, ranges, n_frames=0, meta=True, labels=True)
    assert res["targets"].shape == (0, 3, 8, 4) and res["meta"].shape == (0, 3, 8, 16)
    # frames without pixels: zeros
    for lay in (OV, YUYV):
        res = det.blob_batch_ranges(torch.zeros(64, dtype=torch.uint8, device="cuda"), 0, 0, 0, ranges, layout=lay,
                                    n_frames=3, frame_stride=0)
        assert res["targets"].shape == (3, 3, 8, 4)
        assert not res["targets"].any() and not res["top"].any() and not res["n_labels"].any()


def test_rejections(hsv, det):
    """Each rejected call: the return code, the message, nothing written."""
    import torch

    ranges = cases.ranges_for(2)
    dev = torch.zeros(2 * 64 * 64, dtype=torch.uint8, device="cuda")
    good = hsv._abi.FrameBatch(dev.data_ptr(), 2 * 64 * 64, 1, 64, 64, 64, OV)

    def batch(**kw):
        b = hsv._abi.FrameBatch(dev.data_ptr(), 2 * 64 * 64, 1, 64, 64, 64, OV)
        for k, v in kw.items():
            setattr(b, k, v)
        return b

    rejected = [
        ("handle is NULL", dict(h=None)),
        ("batch is NULL", dict(b=None)),
        ("n_ranges", dict(null=("ranges",))),
        ("targets is NULL", dict(null=("targets",))),
        ("unknown layout", dict(b=batch(layout=2))),
        ("n_ranges", dict(n_ranges=0)),
        ("n_ranges", dict(n_ranges=hsv._abi.MAX_RANGES + 1)),
        ("width % 32", dict(b=batch(width=48))),
        ("height % 4", dict(b=batch(height=62))),
        ("too large", dict(b=batch(width=8224, line_length=8224, height=4))),
        ("too large", dict(b=batch(width=4096, line_length=4096, height=4096))),
        ("line_length", dict(b=batch(layout=YUYV))),  # a YUYV row of 64 pixels is 128 bytes
    ]
    for text, kw in rejected:
        outs = _sentinels(1, 2, 64, 64)
        rc = _raw(hsv, kw.get("h", det._h), kw.get("b", good), ranges, outs, n_ranges=kw.get("n_ranges"),
                  null=kw.get("null", ()))
        assert rc == hsv.IVIDTRANSCODE_EFAIL, text
        assert text in hsv._abi.last_error(), (text, hsv._abi.last_error())
        assert _untouched(outs), text
    # the accepted call, for contrast, writes
    outs = _sentinels(1, 2, 64, 64)
    assert _raw(hsv, det._h, good, ranges, outs) == 0 and not _untouched(outs)
    # and the single-range call still refuses YUYV
    alg = hsv._abi.OV7670InArgsAlg(1, *cases.RED_HSV, 0)
    outs = _sentinels(1, 1, 64, 64)
    rc = hsv._lib.trik_hsv_blob_batch(det._h, C.byref(batch(layout=YUYV, height=32, line_length=128)), C.byref(alg),
                                      C.c_void_p(outs["targets"].data_ptr()), None, None, None, None, None)
    assert rc != 0 and "ov7670" in hsv._abi.last_error() and _untouched(outs)


def test_handle_state(hsv, det, oracle_mod):
    """One handle: a single-range batch, a ranges batch of a geometry with the
    unpacked statistics (1056 x 1024: 17 + 24 + 24 bits), a single-range batch
    again -- each runs on the statistics buffer the one before left behind."""
    import blob_patterns
    import torch

    w, h, ll = 320, 240, 352
    small = _geom_frames(oracle_mod, w, h, ll)
    dev, _, _ = _device_batch(small, w, h, ll, OV)

    def single(tag):
        res = det.blob_batch(dev, w, h, ll, cases.RED_HSV, meta=True, labels=True)
        for i, fr in enumerate(small):
            blob_patterns.check_frame(res, i, _ref(oracle_mod, ((w, h, ll), i), fr, w, h, ll,
                                                   cases.from_to(cases.RED_HSV)), (tag, i))

    single("before")
    bw, bh = 1056 // 4, 1024 // 4
    big = [cases.mosaic(np.stack([blob_patterns.rand(bh, bw, 0.5, 80), blob_patterns.rand(bh, bw, 0.2, 81)]), seed=8)]
    ranges = cases.ranges_for(2)
    res = _run(det, big, 1056, 1024, 1056, ranges, OV)
    _check_all(oracle_mod, res, big, ["big"], 1056, 1024, 1056, ranges, "unpacked")
    single("after")
    torch.cuda.synchronize()
