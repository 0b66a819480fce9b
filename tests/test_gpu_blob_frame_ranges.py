"""trik_hsv_blob_frame_ranges_batch on the GPU: the multi-blob sensor with HSV
ranges per frame, read on the device.  Slot (f, t) against the oracle's run of
the ov7670 frame f with the slot's six numbers as the sticky state -- bitmap,
label map, label count, the 8 largest clusters and the 8 targets, bit-exact --
on the cases of tests/blob_frame_ranges_cases.py, ov7670 batches and their
packed-YUYV twins.  tests/test_blob_frame_ranges_cpu.py asserts every coverage
claim of those cases on the oracle's output."""
import ctypes as C

import numpy as np
import pytest

import blob_frame_ranges_cases as BF
import blob_patterns
import blob_ranges_cases as BR

pytestmark = pytest.mark.gpu

OV, YUYV = BF.OV, BF.YUYV
LAYOUTS = [pytest.param(OV, id="ov7670"), pytest.param(YUYV, id="yuyv")]


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


def _ranges_dev(ranges):
    import torch

    return torch.tensor(ranges, dtype=torch.int32).to(torch.int16).cuda()


def _device_batch(c, layout, ll_dev=None, stride=None, offset=0):
    """The case's frames (their YUYV twins for that layout) as one device
    tensor: (tensor, line length, frame stride)."""
    import torch

    frames, ll = c["frames"], c["ll"]
    if layout == YUYV:
        ll_dev = 2 * c["w"] if ll_dev is None else ll_dev
        frames = [BR.to_yuyv(fr, c["w"], c["h"], ll, ll_dev, seed=i) for i, fr in enumerate(frames)]
        ll = ll_dev
    host, stride = BF.host_batch(frames, stride, offset)
    return torch.from_numpy(host).cuda()[offset:], ll, stride


def _run(det, c, layout, *, top=True, meta=True, labels=True, stream=None, **kw):
    dev, ll, stride = _device_batch(c, layout, **kw)
    res = det.blob_frame_ranges_batch(dev, c["w"], c["h"], ll, _ranges_dev(c["ranges"]),
                                      layout=layout, n_frames=len(c["frames"]), frame_stride=stride, top=top,
                                      meta=meta, labels=labels, stream=stream)
    return {k: v.cpu() for k, v in res.items() if v is not None}


def _check(oracle_mod, res, c, what):
    """Every slot in full (blob_ranges_cases.check_slot)."""
    want = BF.expect_all(oracle_mod, c)
    for f, row in enumerate(want):
        for t, ref in enumerate(row):
            BF.check_frame(res, f, t, ref, (c["name"], what, "frame", f, "range", t))
    return want


def _check_stats(res, want, what):
    """targets, top and n_labels of every slot, whole arrays at once."""
    top = np.array([[r["top"] for r in row] for row in want])
    tg = np.array([[r["targets"] for r in row] for row in want])
    nl = np.array([[r["n_labels"] for r in row] for row in want])
    got_tg = res["targets"].numpy()
    bad = np.argwhere((res["top"].numpy() != top).any(axis=(2, 3)) | (got_tg[..., :3] != tg).any(axis=(2, 3)) |
                      (res["n_labels"].numpy() != nl))
    assert len(bad) == 0, (what, "slots (frame, range) differ", bad[:6].tolist())
    assert not got_tg[..., 3].any(), what


# ---- 1. the threshold at every count ---------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
def test_threshold_at_every_count(det, oracle_mod, layout):
    """k = 0..16 pixels of a metapixel: the bitmap is k > 2, at T = 1 and in
    byte lane 0 of four with fixed counts 2, 3 and 16 beside it."""
    c, counts = BF.ladders()
    res = _run(det, c, layout)
    for t in range(4):
        assert np.array_equal(res["meta"][t, 0, 0].numpy(), counts[t] > 2), t
    _check(oracle_mod, res, c, layout)
    c, k = BF.lanes()
    res = _run(det, c, layout)
    meta = res["meta"][0].numpy()
    assert np.array_equal(meta[0, 0], k > 2), meta[0, 0]
    assert not meta[1].any() and meta[2].all() and meta[3].all()  # counts 2, 3, 16: no lane leaks
    _check(oracle_mod, res, c, layout)


# ---- 2. ranges are per frame -----------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
def test_ranges_are_per_frame(det, oracle_mod, layout):
    """8 mosaics, frame f under the palette rotated by f: a kernel that read
    frame 0's set for everyone would be right in no slot but those of f % 4 == 0."""
    c = BF.rotated()
    own, shared = BF.expect_all(oracle_mod, c), BF.rotated_under_frame0(oracle_mod)
    for f in range(8):
        for t in range(4):
            assert BF.same_result(own[f][t], shared[f][t]) == (f % 4 == 0), (f, t)
    _check(oracle_mod, _run(det, c, layout), c, layout)


# ---- 3. equal sets equal the shared call -------------------------------------------
@pytest.mark.parametrize("t", BF.EQUAL_T)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_equal_sets_equal_the_shared_call(det, layout, t):
    """One set for all frames: tensors identical to blob_batch_ranges'.  T = 5
    and 8: the group tail and a second group; 64: the most."""
    import torch

    frames = BF.equal_frames()
    ranges = BR.ranges_for(t)
    c = BF.case("equal", frames, 64, 32, 64, [ranges] * len(frames))
    dev, ll, stride = _device_batch(c, layout)
    shared = det.blob_batch_ranges(dev, 64, 32, ll, ranges, layout=layout, meta=True, labels=True)
    own = det.blob_frame_ranges_batch(dev, 64, 32, ll, _ranges_dev(c["ranges"]), layout=layout, top=True, meta=True,
                                      labels=True)
    assert shared["meta"].any() and not shared["meta"].all()
    for key in ("targets", "top", "n_labels", "meta", "labels"):
        assert torch.equal(own[key], shared[key]), (t, key)


# ---- 4. geometry ---------------------------------------------------------------------
@pytest.mark.parametrize("name", list(BF.GEOMETRY))
@pytest.mark.parametrize("layout", LAYOUTS)
def test_geometry(det, oracle_mod, layout, name):
    """The smallest frame; a metapixel row that fills no wave; the widest
    frame; a tall one; VGA; 3000 tiny frames with a range each."""
    c = BF.geometry(name)
    res = _run(det, c, layout)
    if len(c["frames"]) <= 8:
        want = _check(oracle_mod, res, c, layout)
    else:
        want = BF.expect_all(oracle_mod, c)
        _check_stats(res, want, (name, layout))
        meta = np.array([[r["meta"] for r in row] for row in want])
        assert np.array_equal(res["meta"].numpy(), meta), name
    assert sum(r["meta"].any() for row in want for r in row) > len(want) // 2


# ---- 5. chunks -------------------------------------------------------------------------
@pytest.mark.parametrize("t", list(BF.CHUNKS))
@pytest.mark.parametrize("layout", LAYOUTS)
def test_chunks(hsv, det, oracle_mod, layout, t):
    """More slots than BLOB_CHUNK_SLOTS, a ragged second chunk, a distinct set
    per frame: the ranges pointer advances with the chunk.  The bitmaps go
    through the handle's scratch (meta is not asked for)."""
    assert hsv.BLOB_CHUNK_SLOTS == BF.CHUNK_SLOTS
    c = BF.chunked(t)
    res = _run(det, c, layout, meta=False, labels=False)
    _check_stats(res, BF.expect_all(oracle_mod, c), (t, layout))


# ---- 6. load paths -----------------------------------------------------------------------
@pytest.mark.parametrize("name", list(BF.LOADS))
@pytest.mark.parametrize("layout", LAYOUTS)
def test_load_paths(det, oracle_mod, layout, name):
    c = BF.load_case(name)
    ll, stride, offset = BF.load_geometry(name, layout)
    dev, ll_dev, stride_dev = _device_batch(c, layout, ll_dev=ll, stride=stride, offset=offset)
    assert (ll_dev, stride_dev) == (ll, stride)
    bits = dev.data_ptr() | stride | ll
    assert {"dwords": bits % 8 == 4, "bytes": dev.data_ptr() % 2 == 1 and ll % 2 == 1, "aligned16": bits % 16 == 0}[name]
    res = _run(det, c, layout, ll_dev=ll, stride=stride, offset=offset)
    _check(oracle_mod, res, c, (name, layout))


# ---- 7. dense random bytes -------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
def test_dense_random_bytes(det, oracle_mod, layout):
    c = BF.dense(oracle_mod)
    want = BF.expect_all(oracle_mod, c)
    assert all(0.25 < r["meta"].mean() < 0.75 for row in want for r in row)
    res = _run(det, c, layout)
    _check_stats(res, want, layout)
    assert np.array_equal(res["meta"].numpy(), np.array([[r["meta"] for r in row] for row in want]))
    assert np.array_equal(res["labels"].numpy().view(np.uint16), np.array([[r["labels"] for r in row] for row in want]))


# ---- 8. edge ranges, one per frame ---------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
def test_edge_ranges_per_frame(det, oracle_mod, layout):
    """Full, point, hue wrap, From == To, From == To + 1, and a saturation and a
    value of 400, which behave as 255."""
    c = BF.edges()
    want = _check(oracle_mod, _run(det, c, layout), c, layout)
    assert want[0][0]["meta"].all()


# ---- 9. optional outputs, frames without pixels -----------------------------------------------------
def test_optional_outputs_and_empty_geometry(hsv, det):
    import torch

    c = BF.rotated()
    dev, ll, stride = _device_batch(c, OV)
    rng = _ranges_dev(c["ranges"])
    full = det.blob_frame_ranges_batch(dev, 64, 32, ll, rng, top=True, meta=True, labels=True)
    only = det.blob_frame_ranges_batch(dev, 64, 32, ll, rng)
    assert only["top"] is None and only["n_labels"] is None and only["meta"] is None and only["labels"] is None
    assert torch.equal(only["targets"], full["targets"]) and full["targets"].any()
    # the call itself, every optional pointer NULL
    tg = torch.full((8, 4, 8, 4), 0x5A, dtype=torch.int8, device="cuda")
    b = hsv._batch(dev, 64, 32, ll, OV)
    rc = hsv._lib.trik_hsv_blob_frame_ranges_batch(det._h, C.byref(b), C.c_void_p(rng.data_ptr()), 4,
                                                   C.c_void_p(tg.data_ptr()), None, None, None, None, None)
    torch.cuda.synchronize()
    assert rc == 0 and torch.equal(tg, full["targets"])
    # frames without pixels: zeros; no frame: nothing is touched
    for lay in (OV, YUYV):
        res = det.blob_frame_ranges_batch(torch.zeros(64, dtype=torch.uint8, device="cuda"), 0, 0, 0, rng[:3, :2].contiguous(),
                                          layout=lay, n_frames=3, frame_stride=0, top=True)
        assert res["targets"].shape == (3, 2, 8, 4)
        assert not res["targets"].any() and not res["top"].any() and not res["n_labels"].any()
    b = hsv._batch(dev, 64, 32, ll, OV, n_frames=0)
    tg.fill_(0x5A)
    assert hsv._lib.trik_hsv_blob_frame_ranges_batch(det._h, C.byref(b), None, 4, C.c_void_p(tg.data_ptr()), None,
                                                     None, None, None, None) == 0
    torch.cuda.synchronize()
    assert bool((tg == 0x5A).all())


# ---- 10. stream order ------------------------------------------------------------------------------------
def test_ranges_are_read_in_stream_order(det, oracle_mod):
    """Set A, a call, set B copied over it from pinned memory without waiting,
    a second call: each output matches its own set."""
    import torch

    c = BF.rotated()
    set_a, set_b = BF.stream_sets()
    ca, cb = dict(c, ranges=set_a), dict(c, ranges=set_b)
    dev, ll, stride = _device_batch(c, OV)
    pinned_b = torch.tensor(set_b, dtype=torch.int32).to(torch.int16).pin_memory()
    ranges = _ranges_dev(set_a)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        out1 = det.blob_frame_ranges_batch(dev, 64, 32, ll, ranges, top=True, meta=True, labels=True, stream=s)
        ranges.copy_(pinned_b, non_blocking=True)
        out2 = det.blob_frame_ranges_batch(dev, 64, 32, ll, ranges, top=True, meta=True, labels=True, stream=s)
    s.synchronize()
    _check(oracle_mod, {k: v.cpu() for k, v in out1.items()}, ca, "first call")
    _check(oracle_mod, {k: v.cpu() for k, v in out2.items()}, cb, "second call")


# ---- 11. the closed loop on the device ------------------------------------------------------------------------
def test_closed_loop_on_the_device(hsv, det, oracle_mod):
    """batch_auto_range_exact(OV7670_OBJECT) -> ranges_of_detect -> the call, on
    one stream with no host step between: slot f is the sensor's own run of
    frame f with the detected centre/tolerance range."""
    import torch

    v = BF.LOOP
    w, h = v["w"], v["h"]
    c = BF.case("loop", BF.loop_frames(), w, h, w, [[(0,) * 6]] * v["n"])
    dev, ll, stride = _device_batch(c, OV)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        det_dev, _ = hsv.batch_auto_range_exact(dev, w, h, ll, hsv.AUTO_OV7670_OBJECT, stream=s)
        rng_dev = hsv.ranges_of_detect(det_dev, stream=s)
        res = det.blob_frame_ranges_batch(dev, w, h, ll, rng_dev, top=True, meta=True, labels=True, stream=s)
    s.synchronize()
    detect = (det_dev.cpu().numpy().astype(np.int64) & 0xFFFF).tolist()
    want = BF.loop_expect(oracle_mod, detect)
    BF.check_loop(detect, want)
    res = {k: x.cpu() for k, x in res.items()}
    for f, ref in enumerate(want):
        BF.check_frame(res, f, 0, ref, ("loop", f, detect[f]))


# ---- 12. scratch reuse -----------------------------------------------------------------------------------------
def test_scratch_reuse_on_one_handle(hsv, det, oracle_mod):
    """The call, blob_batch, the call again: the clusterer's statistics are back
    at zero after each, the table-free path leaves the handle's tables usable,
    and the hot-kernel report is left as blob_batch set it."""
    c = BF.rotated()
    want = BF.expect_all(oracle_mod, c)
    dev, ll, stride = _device_batch(c, OV)
    rng = _ranges_dev(c["ranges"])

    def ours(tag):
        res = det.blob_frame_ranges_batch(dev, 64, 32, ll, rng, top=True)
        _check_stats({k: x.cpu() for k, x in res.items() if x is not None}, want, tag)

    ours("first")
    one = det.blob_batch(dev, 64, 32, ll, BR.RED_HSV, meta=True, labels=True)
    reported = det.last_hot_kernel()
    for f, fr in enumerate(c["frames"]):
        blob_patterns.check_frame(one, f, BF.expect(oracle_mod, c["keys"][f], fr, 64, 32, 64, BR.from_to(BR.RED_HSV)),
                                  ("blob_batch between", f))
    ours("again")
    assert det.last_hot_kernel() == reported
    one = det.blob_batch(dev, 64, 32, ll, BR.RED_HSV, meta=True, labels=True)
    blob_patterns.check_frame(one, 3, BF.expect(oracle_mod, c["keys"][3], c["frames"][3], 64, 32, 64,
                                                BR.from_to(BR.RED_HSV)), "blob_batch after")
