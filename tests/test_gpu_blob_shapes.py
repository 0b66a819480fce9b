"""Every blob_ccl_kernel instantiation, both statistics layouts and both
overlay forms on structured bitmaps (tests/blob_patterns.py), bit-exact
against the oracle (oracle/trik_oracle.c:trik_oracle_blob_run) through
Detector.blob_batch / blob_preview and BlobSensor.process.

Which kernel a geometry runs is restated here from launch_blob (variant()
below) and asserted per case, so the table cannot drift from the launcher
unnoticed:

  w x h        bw x bh     kernel           statistics   what it adds
  256 x 48     64 x 12     <1, exact>       packed       all 64 lanes used
  288 x 36     72 x 9      <2, exact>       packed       tail lanes; bh % 8 != 0
  544 x 48     136 x 12    <3, exact>       packed       lanes >= 46 empty
  640 x 4      160 x 1     <3, exact>       packed       one row
  1024 x 36    256 x 9     <4, exact>       packed
  1280 x 48    320 x 12    <5, exact>       packed
  1056 x 36    264 x 9     <5, exact>       packed       tail lanes
  1312 x 24    328 x 6     <8>, K = 6       packed       j < K guards
  2048 x 24    512 x 6     <8>, K = 8       packed
  2080 x 24    520 x 6     <16>, K = 9      packed
  4096 x 24    1024 x 6    <16>, K = 16     packed
  4128 x 24    1032 x 6    <32>, K = 17     packed
  8160 x 64    2040 x 16   <32>, K = 32     packed       overlay maps from memory
  1056 x 1024  264 x 256   <5, exact>       three int32  sizes past 65535, read from
  1024 x 1056  256 x 264   <4, exact>       three int32  memory in the top-8 passes

The sweep batches stage the bitmap in LDS; 640 x 48 and 1312 x 24 run again
at 2 * CUs + 3 frames, where the clusterer reads it from L2, as it does for
the last three rows (bitmap and eq table together past 40 KiB).
"""
import numpy as np
import pytest

import blob_patterns
from blob_patterns import check_frame
from test_gpu_blob import RED, _blob_sensor

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hsv():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import trik_hsv

    return trik_hsv


def _bits(v):
    return int(v).bit_length()


def variant(w, h, n_frames, cus):
    """launch_blob's choices for a batch, restated: (KMAX, exact, K), whether
    the statistics are packed into one u64 per label (bit sum <= 63), whether
    the bitmap is staged in LDS, whether the top-8 passes read sizes from LDS."""
    bw, bh = w // 4, h // 4
    k = (bw + 63) // 64
    kmax = k if k <= 5 else 8 if k <= 8 else 16 if k <= 16 else 32
    ml = ((bw + 1) // 2) * ((bh + 1) // 2) + 1
    bit_sum = _bits(bw * bh) + _bits(bh * bw * (bw - 1) // 2) + _bits(bw * bh * (bh - 1) // 2)
    eq_bytes = 2 * ((ml + 1) & ~1)
    return {"kernel": (kmax, k <= 5, k), "bit_sum": bit_sum, "packed": bit_sum <= 63,
            "staged": n_frames < 2 * cus and eq_bytes + bw * bh <= 40 * 1024, "lds_sizes": bw * bh < 65536}


def _cus():
    import torch

    return torch.cuda.get_device_properties(0).multi_processor_count


_cache = {}


def _pattern_frames(oracle_mod, w, h, ll):
    """The geometry's pattern frames and their oracle results, built once."""
    key = (w, h, ll)
    if key not in _cache:
        pats = blob_patterns.patterns(h // 4, w // 4)
        frames = [blob_patterns.frame(m, ll, seed=i) for i, m in enumerate(pats.values())]
        refs = [oracle_mod.blob_run(fr, w, h, ll, hsv=RED, preview=False) for fr in frames]
        for m, ref in zip(pats.values(), refs):
            assert np.array_equal(ref["meta"], m)
        _cache[key] = (list(pats), frames, refs)
    return _cache[key]


def _to_host(res):
    return {k: v.cpu() for k, v in res.items() if v is not None}


# (w, h, ll) -> (KMAX, exact, K); padded lines: a multiple of 16, and one that is not a multiple of 4
SWEEP = [((256, 48, 256), (1, True, 1)),
         ((288, 36, 288), (2, True, 2)), ((288, 36, 304), (2, True, 2)), ((288, 36, 290), (2, True, 2)),
         ((544, 48, 544), (3, True, 3)),
         ((640, 4, 640), (3, True, 3)), ((640, 4, 656), (3, True, 3)), ((640, 4, 642), (3, True, 3)),
         ((1024, 36, 1024), (4, True, 4)),
         ((1280, 48, 1280), (5, True, 5)),
         ((1056, 36, 1056), (5, True, 5)),
         ((1312, 24, 1312), (8, False, 6)), ((1312, 24, 1328), (8, False, 6)), ((1312, 24, 1314), (8, False, 6)),
         ((2048, 24, 2048), (8, False, 8)),
         ((2080, 24, 2080), (16, False, 9)),
         ((4096, 24, 4096), (16, False, 16)),
         ((4128, 24, 4128), (32, False, 17))]


@pytest.mark.parametrize("geom,kernel", SWEEP, ids=["%dx%d_ll%d" % g for g, _ in SWEEP])
def test_blob_variant_sweep(hsv, oracle_mod, geom, kernel):
    """All patterns of a geometry as the frames of one batch (bitmap staged in
    LDS, packed statistics), on both bitmap kernels where the lines allow it."""
    import torch

    w, h, ll = geom
    names, frames, refs = _pattern_frames(oracle_mod, w, h, ll)
    v = variant(w, h, len(frames), _cus())
    assert v["kernel"] == kernel and v["staged"] and v["packed"] and v["lds_sizes"], v
    dev = torch.from_numpy(np.concatenate(frames)).cuda()
    aligned = w % 16 == 0 and ll % 16 == 0
    for hot in (hsv.HOT_AUTO, hsv.HOT_CHROMA) if aligned else (hsv.HOT_AUTO,):
        det = hsv.Detector(hot=hot)
        try:
            res = _to_host(det.blob_batch(dev, w, h, ll, RED, meta=True, labels=True))
            assert det.last_hot_kernel() == (hsv.HOT_CHROMA if hot == hsv.HOT_CHROMA else hsv.HOT_STRIPE)
            for i, ref in enumerate(refs):
                check_frame(res, i, ref, (geom, hot, names[i]))
        finally:
            det.close()


@pytest.mark.parametrize("geom,kernel", [((640, 48, 640), (3, True, 3)), ((1312, 24, 1312), (8, False, 6))],
                         ids=["640x48", "1312x24"])
def test_blob_patterns_from_l2(hsv, oracle_mod, geom, kernel):
    """2 * CUs + 3 frames: the clusterer reads the bitmap from L2, not LDS.
    The pattern frames cycled; every frame of the batch is compared."""
    import torch

    w, h, ll = geom
    names, frames, refs = _pattern_frames(oracle_mod, w, h, ll)
    n = 2 * _cus() + 3
    v = variant(w, h, n, _cus())
    assert v["kernel"] == kernel and not v["staged"] and v["packed"], v
    dev = torch.from_numpy(np.concatenate([frames[i % len(frames)] for i in range(n)])).cuda()
    det = hsv.Detector()
    try:
        res = _to_host(det.blob_batch(dev, w, h, ll, RED, meta=True, labels=True))
        for i in range(n):
            check_frame(res, i, refs[i % len(frames)], (geom, i, names[i % len(frames)]))
    finally:
        det.close()


def _named_frames(oracle_mod, w, h, names):
    """(frame, oracle result) per name: a pattern's, or "rand50"."""
    bh, bw = h // 4, w // 4
    pats = blob_patterns.patterns(bh, bw)
    out = []
    for i, name in enumerate(names):
        meta = blob_patterns.rand(bh, bw, 0.5, 50) if name == "rand50" else pats[name]
        fr = blob_patterns.frame(meta, w, seed=100 + i)
        ref = oracle_mod.blob_run(fr, w, h, w, hsv=RED, preview=False)
        assert np.array_equal(ref["meta"], meta)
        out.append((fr, ref))
    return out


UNPACKED = [((1056, 1024), (5, True, 5)), ((1024, 1056), (4, True, 4))]


@pytest.mark.parametrize("geom,kernel", UNPACKED, ids=["1056x1024", "1024x1056"])
def test_blob_unpacked_statistics(hsv, oracle_mod, geom, kernel):
    """Size, sum x and sum y need 65 bits: three int32 atomics per run, the
    fold and the top-8 passes on memory, and a cluster of more than 65535
    metapixels -- top keeps the int32 size, the target takes getSize()'s
    uint16_t (CLU:155)."""
    import torch

    w, h = geom
    names = ["full", "rand50", "bridges_rtl"]
    v = variant(w, h, len(names), _cus())
    assert v["bit_sum"] > 63 and not v["packed"] and not v["lds_sizes"] and v["kernel"] == kernel, v
    cases = _named_frames(oracle_mod, w, h, names)
    full = cases[0][1]
    size = int(full["top"][0, 0])
    assert size == (w // 4) * (h // 4) - 1 > 0xFFFF
    # OSEQ:563-590 on the wrapped and on the whole size differ: the truncation decides target[0]
    pct = lambda s: (int(np.ceil(np.float32(int(np.sqrt(np.float32(s)))) / np.float32(3.1415927))) * 400) \
        // (w // 4 + h // 4)  # noqa: E731
    assert int(full["targets"][0, 2]) == pct(size & 0xFFFF) != pct(size)
    dev = torch.from_numpy(np.concatenate([fr for fr, _ in cases])).cuda()
    det = hsv.Detector()
    try:
        res = _to_host(det.blob_batch(dev, w, h, w, RED, meta=True, labels=True))
        for i, (_, ref) in enumerate(cases):
            check_frame(res, i, ref, (geom, names[i]))
    finally:
        det.close()


def test_blob_stats_layout_handover(hsv, oracle_mod):
    """One handle, packed -> unpacked -> packed -> unpacked -> packed: the
    statistics buffer is indexed as u64[f * ml + k] by one layout and as
    int32[3 * (f * ml + k)] by the other over the same bytes, and is only zero
    for the next batch if every wave zeroed what it used in its own layout.
    iso_grid uses every label slot of its frame, the last one included."""
    import torch

    seq = [(640, 480), (1056, 1024), (640, 480), (1024, 1056), (320, 240)]
    want = [True, False, True, False, True]
    det = hsv.Detector()
    try:
        for (w, h), packed in zip(seq, want):
            assert variant(w, h, 2, _cus())["packed"] == packed
            cases = _named_frames(oracle_mod, w, h, ["rand45", "iso_grid"])
            assert cases[1][1]["n_labels"] == ((w // 4 + 1) // 2) * ((h // 4 + 1) // 2) + 1
            dev = torch.from_numpy(np.concatenate([fr for fr, _ in cases])).cuda()
            res = _to_host(det.blob_batch(dev, w, h, w, RED, meta=True, labels=True))
            for i, (_, ref) in enumerate(cases):
                check_frame(res, i, ref, ((w, h), i))
    finally:
        det.close()


def test_blob_overlay_maps_from_memory(hsv, oracle_mod):
    """4 * (W + H) > 32 KiB: blob_overlay_kernel reads the scale maps from
    memory, not LDS.  8160 x 64 full is one cluster of 32639 metapixels, kept
    (size 11), so the overlay draws a mark."""
    import torch

    w, h = 8160, 64
    assert 4 * (w + h) > 32 * 1024
    v = variant(w, h, 2, _cus())
    assert v["kernel"] == (32, False, 32) and v["packed"], v
    cases = _named_frames(oracle_mod, w, h, ["full", "rand45"])
    assert cases[0][1]["targets"][0, 2] > 4
    dev = torch.from_numpy(np.concatenate([fr for fr, _ in cases])).cuda()
    det = hsv.Detector()
    try:
        res = det.blob_batch(dev, w, h, w, RED, meta=True, labels=True)
        for i, (_, ref) in enumerate(cases):
            check_frame(res, i, ref, i)
        for ow, oh, oll in ((w // 2, h // 2, w), (1000, 40, 2003)):
            pv = det.blob_preview(dev, w, h, w, res["meta"], res["top"], out_width=ow, out_height=oh,
                                  out_line_length=oll).cpu().numpy()
            for i, (fr, _) in enumerate(cases):
                ref = oracle_mod.blob_run(fr, w, h, w, hsv=RED, out_width=ow, out_height=oh, out_line_length=oll)
                assert np.array_equal(pv[i].reshape(-1), ref["preview"]), (i, ow)
    finally:
        det.close()


def _corner_frames(oracle_mod, w, h):
    """Four frames with one solid strip each in a frame corner, large enough
    to be kept.  The mark's source point is (sum / (size + 1)) * 4 per axis:
    a two-metapixel strip along the left or top edge puts it on column or row
    0, where the 3 x 3 mark reaches -1 and is clamped (OSEQ:92-108)."""
    bh, bw = h // 4, w // 4
    metas = [np.zeros((bh, bw), np.uint8) for _ in range(4)]
    metas[0][:20, :2] = 1          # top left, down the left edge
    metas[1][:2, bw - 20:] = 1     # top right, along the top edge
    metas[2][bh - 20:, :2] = 1     # bottom left
    metas[3][bh - 20:, bw - 2:] = 1  # bottom right: the mark stays inside (the point is a multiple of 4)
    frames = [blob_patterns.frame(m, w, seed=200 + i) for i, m in enumerate(metas)]
    marks = []
    for fr in frames:
        ref = oracle_mod.blob_run(fr, w, h, w, hsv=RED, preview=False)
        size, sx, sy = (int(t) for t in ref["top"][0])
        assert size == 39 and ref["targets"][0, 2] > 0  # kept
        marks.append(((sx // (size + 1)) * 4, (sy // (size + 1)) * 4))
    assert marks[0][0] == 0 and marks[1][1] == 0 and marks[2][0] == 0  # the clamped ones
    assert marks[3][0] >= w - 16 and marks[3][1] == marks[2][1]
    return frames


@pytest.mark.parametrize("out", [(160, 120, 320), (200, 150, 401)], ids=["160x120", "200x150"])
def test_blob_corner_marks(hsv, oracle_mod, out):
    """Kept targets in the frame corners through blob_batch + blob_preview and
    through BlobSensor.process: previews byte for byte, nothing written past
    the output buffer."""
    import torch

    w, h = 320, 240
    ow, oh, oll = out
    frames = _corner_frames(oracle_mod, w, h)
    refs = [oracle_mod.blob_run(fr, w, h, w, hsv=RED, out_width=ow, out_height=oh, out_line_length=oll)
            for fr in frames]
    dev = torch.from_numpy(np.concatenate(frames)).cuda()
    det = hsv.Detector()
    try:
        res = det.blob_batch(dev, w, h, w, RED, meta=True, labels=True)
        pv = det.blob_preview(dev, w, h, w, res["meta"], res["top"], out_width=ow, out_height=oh,
                              out_line_length=oll).cpu().numpy()
        for i, ref in enumerate(refs):
            check_frame(res, i, ref, i)
            assert np.array_equal(pv[i].reshape(-1), ref["preview"]), i
    finally:
        det.close()
    s = _blob_sensor(hsv, w, h, w, ow, oh, oll)
    try:
        for i, (fr, ref) in enumerate(zip(frames, refs)):
            # the output buffer is the first oh * oll + 16 bytes of arena: the 16 past
            # the preview come back zero (as in test_blob_sensor_process_vs_oracle),
            # what lies past the buffer keeps its pattern
            arena = np.full(oh * oll + 16 + 256, 0xCD, np.uint8)
            buf = arena[: oh * oll + 16]
            rc, oa = s.process(fr, RED, out_buffer=buf)
            assert rc == 0
            got = [(oa.alg.target[k].x, oa.alg.target[k].y, oa.alg.target[k].size) for k in range(8)]
            assert got == [tuple(t) for t in ref["targets"].tolist()], i
            assert np.array_equal(buf[: oh * oll], ref["preview"]), i
            assert not buf[oh * oll:].any(), i
            assert (arena[oh * oll + 16:] == 0xCD).all(), i
    finally:
        s.close()
