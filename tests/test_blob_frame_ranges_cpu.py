"""CPU-only checks of the per-frame-range multi-blob call: the ctypes mirror has
the prototype and the library the symbol, every argument the C ABI refuses is
refused before any GPU call (there is no GPU here, and no pointer is
dereferenced on the host), and the inputs of tests/test_gpu_blob_frame_ranges.py
(tests/blob_frame_ranges_cases.py) reach what they are meant to reach, stated
on the oracle's output."""
import ctypes as C

import numpy as np
import pytest

import blob_frame_ranges_cases as BF
import blob_ranges_cases as BR

FAKE = 0x10000  # a non-NULL address nothing reads
OV, YUYV = BF.OV, BF.YUYV


@pytest.fixture(scope="module")
def abi():
    from trik_hsv import _abi

    return _abi


def _batch(abi, n=2, w=64, h=8, ll=64, layout=OV, stride=None, frames=FAKE):
    return abi.FrameBatch(frames, h * ll * (2 if layout == OV else 1) if stride is None else stride, n, w, h, ll,
                          layout)


def _refused(abi, rc):
    assert rc != 0
    msg = abi.last_error()
    assert msg, "a refused call leaves a message"
    return msg


def test_prototype_and_symbol(abi):
    args, res = abi.PROTOTYPES["trik_hsv_blob_frame_ranges_batch"]
    assert len(args) == 10 and res is C.c_int32
    assert hasattr(abi.load(), "trik_hsv_blob_frame_ranges_batch")
    import trik_hsv

    assert callable(trik_hsv.Detector.blob_frame_ranges_batch)
    assert BF.CHUNK_SLOTS == abi.BLOB_CHUNK_SLOTS


def test_refusals_come_before_any_gpu_call(abi):
    """A handle that is only an address: a refused call never looks into it."""
    call = abi.load().trik_hsv_blob_frame_ranges_batch
    ok = _batch(abi)

    def run(h=FAKE, b=ok, ranges=FAKE, t=1, targets=FAKE):
        return call(h, C.byref(b) if b is not None else None, ranges, t, targets, None, None, None, None, None)

    assert "handle" in _refused(abi, run(h=None))
    assert "batch is NULL" in _refused(abi, run(b=None))
    assert "targets" in _refused(abi, run(targets=None))
    assert "ranges" in _refused(abi, run(ranges=None))
    assert "layout" in _refused(abi, run(b=_batch(abi, layout=2)))
    assert "width % 32" in _refused(abi, run(b=_batch(abi, w=48)))
    assert "height % 4" in _refused(abi, run(b=_batch(abi, h=6)))
    assert "too large" in _refused(abi, run(b=_batch(abi, w=8224, ll=8224, h=4)))
    assert "too large" in _refused(abi, run(b=_batch(abi, w=4096, ll=4096, h=4096)))  # more than 30,000 labels
    assert "line_length" in _refused(abi, run(b=_batch(abi, layout=YUYV, stride=8 * 64)))  # a YUYV row is 128 bytes
    for t in (0, -1, abi.MAX_RANGES + 1):
        assert "n_ranges" in _refused(abi, run(t=t))


def test_empty_batch_touches_nothing(abi):
    """n_frames == 0 returns 0 with every buffer NULL: nothing is enqueued."""
    call = abi.load().trik_hsv_blob_frame_ranges_batch
    for t in (1, abi.MAX_RANGES):
        for layout in (OV, YUYV):
            b = _batch(abi, n=0, frames=None, layout=layout, ll=128)
            assert call(FAKE, C.byref(b), None, t, None, None, None, None, None, None) == 0


# ---- the case file's claims, on the oracle ------------------------------------
def _counts(oracle_mod, c, f, t):
    """Per-metapixel pixel counts of slot (f, t), from the oracle's mask."""
    _, mask = oracle_mod.frame(c["frames"][f], c["w"], c["h"], c["ll"], OV, [BF.clamped(c["ranges"][f][t])],
                               want_mask=True)
    return BR.counts_of(mask.reshape(c["h"], c["w"]), 0)


def test_ladders_reach_every_count(oracle_mod):
    c, counts = BF.ladders()
    for t in range(4):
        assert sorted(set(counts[t].tolist())) == list(range(17))
        assert np.array_equal(_counts(oracle_mod, c, t, 0)[0], counts[t]), t
        want = BF.expect(oracle_mod, c["keys"][t], c["frames"][t], 96, 4, 96, c["ranges"][t][0])
        assert np.array_equal(want["meta"][0], counts[t] > 2)
    c, k = BF.lanes()
    assert sorted(set(k.tolist())) == list(range(17))
    assert np.array_equal(_counts(oracle_mod, c, 0, 0)[0], k)
    for t, n in zip((1, 2, 3), BR.LANE_COUNTS):
        assert (_counts(oracle_mod, c, 0, t) == n).all(), (t, n)


def test_rotated_sets_are_per_frame(oracle_mod):
    """Distinct sets per residue of f mod 4, and no slot of a frame f with f % 4
    != 0 would come out the same under frame 0's set."""
    c = BF.rotated()
    assert len({tuple(rs) for rs in c["ranges"]}) == 4 and c["ranges"][4] == c["ranges"][0]
    assert all(len(set(rs)) == 4 for rs in c["ranges"])
    own, shared = BF.expect_all(oracle_mod, c), BF.rotated_under_frame0(oracle_mod)
    for f in range(8):
        for t in range(4):
            assert BF.same_result(own[f][t], shared[f][t]) == (f % 4 == 0), (f, t)


def test_equal_set_ranges_are_distinct():
    for t in BF.EQUAL_T:
        rs = BR.ranges_for(t)
        assert len(rs) == t and len(set(rs)) == (t if t <= 8 else 46), t  # (the value floor stops at the ceiling)


def test_geometry_cases(abi):
    from_name = {k: v[:2] for k, v in BF.GEOMETRY.items()}
    assert from_name["32x4"] == (32, 4) and from_name["96x12"] == (96, 12) and from_name["8192x4"] == (8192, 4)
    assert from_name["32x2048"] == (32, 2048) and from_name["640x480"] == (640, 480)
    assert (96 // 4) * 1 % 16 != 0 and (96 // 4) % 16 != 0  # a metapixel row of 24 fills no wave's 16
    c = BF.geometry("3000x32x4")
    assert len(c["frames"]) == 3000 and len({rs[0] for rs in c["ranges"]}) == 3000
    for name, (w, h, n, t) in BF.GEOMETRY.items():
        assert w % 32 == 0 and h % 4 == 0 and w <= 8192 and ((w // 4 + 1) // 2) * ((h // 4 + 1) // 2) + 1 <= 30000
        assert n * t <= BF.CHUNK_SLOTS  # one chunk: the chunk cases cross it


def test_chunk_cases_cross_once_with_a_ragged_chunk():
    for t, n in BF.CHUNKS.items():
        per, last, chunks = BF.chunk_split(n, t)
        assert chunks == 2 and 0 < last < per and (n - last) == per, (t, n)
        assert n * t > BF.CHUNK_SLOTS > per * t - t
        c = BF.chunked(t)
        sets = [tuple(rs) for rs in c["ranges"]]
        assert len(set(sets)) == n  # a ranges pointer that does not advance shows
        assert set(sets[per:]).isdisjoint(sets[:last])
    assert BF.chunk_split(825, 5)[0] == 819 and BF.chunk_split(1030, 4)[0] == 1024


def test_chunk_results_differ_from_the_first_chunks(oracle_mod):
    """The last chunk's frames under the first frames' sets give other results
    in most slots: a stale ranges pointer cannot pass."""
    for t in BF.CHUNKS:
        c = BF.chunked(t)
        per, last, _ = BF.chunk_split(len(c["frames"]), t)
        differ = 0
        for i in range(last):
            f = per + i
            for k in range(t):
                a = BF.expect(oracle_mod, c["keys"][f], c["frames"][f], 32, 8, 32, c["ranges"][f][k])
                b = BF.expect(oracle_mod, c["keys"][f], c["frames"][f], 32, 8, 32, c["ranges"][i][k])
                differ += not BF.same_result(a, b)
        assert differ > last * t // 2, (t, differ)


def test_load_cases_take_their_paths():
    """line_length + 12 keeps dword loads (no 8-byte ones); + 3 with an odd
    frame stride and a base offset of 1 leaves only bytes; the plain batch is
    16-byte aligned throughout."""
    for layout in (OV, YUYV):
        ll, stride, off = BF.load_geometry("dwords", layout)
        assert ll % 4 == 0 and ll % 8 != 0 and stride % 4 == 0 and off == 0
        ll, stride, off = BF.load_geometry("bytes", layout)
        assert ll % 2 == 1 and stride % 2 == 1 and off == 1
        ll, stride, off = BF.load_geometry("aligned16", layout)
        assert ll % 16 == 0 and stride % 16 == 0 and off == 0
    for name in BF.LOADS:
        c = BF.load_case(name)
        assert c["ll"] == BF.LOAD_W + BF.LOADS[name][0] and len(c["frames"]) == 3
        assert len({tuple(rs) for rs in c["ranges"]}) == 3


def test_load_case_results_are_not_trivial(oracle_mod):
    for name in BF.LOADS:
        c = BF.load_case(name)
        metas = [r["meta"] for row in BF.expect_all(oracle_mod, c) for r in row]
        assert sum(m.any() and not m.all() for m in metas) >= len(metas) // 2, name


def test_dense_case_shares(oracle_mod):
    c = BF.dense(oracle_mod)
    assert len(c["frames"]) == 8 and all(len(set(rs)) == 4 for rs in c["ranges"])
    assert len({tuple(rs) for rs in c["ranges"]}) == 8
    for row in BF.expect_all(oracle_mod, c):
        for r in row:
            assert 0.25 < r["meta"].mean() < 0.75


def test_edge_case_ranges(oracle_mod):
    c = BF.edges()
    assert [rs[0] for rs in c["ranges"]] == BF.EDGE
    assert BF.clamped(BF.EDGE[5])[3] == 255 and BF.clamped(BF.EDGE[6])[5] == 255
    want = BF.expect_all(oracle_mod, c)
    assert want[0][0]["meta"].all()  # the full range holds every pixel
    # the clamped bounds are the scaled 100 % bounds: the same packed range
    assert oracle_mod.pack_range(BF.clamped(BF.EDGE[5])) == oracle_mod.pack_range((0, 359, 10, 100, 0, 100))
    assert oracle_mod.pack_range(BF.clamped(BF.EDGE[2]))[2] == 1  # the wrap is packed as one
    assert sum(r[0]["meta"].any() for r in want) >= 5


def test_stream_sets_differ(oracle_mod):
    c = BF.rotated()
    a, b = BF.stream_sets()
    differ = 0
    for f, fr in enumerate(c["frames"]):
        for t in range(4):
            differ += not BF.same_result(BF.expect(oracle_mod, c["keys"][f], fr, 64, 32, 64, a[f][t]),
                                         BF.expect(oracle_mod, c["keys"][f], fr, 64, 32, 64, b[f][t]))
    assert differ >= 16, differ  # half of the 32 slots


def test_closed_loop_frames_on_the_restated_detector(oracle_mod, table):
    """The loop's claims, foreseen on the CPU with the detector's restatement
    (tests/autorange_ref.py): at least two distinct ranges, a kept target."""
    import autorange_ref as R

    v = BF.LOOP
    detect = [R.detect(table, fr, v["w"], v["h"], v["w"], R.OBJECT)["out"] for fr in BF.loop_frames()]
    assert all(max(d) <= 255 or d[0] < 360 for d in detect)
    BF.check_loop(detect, BF.loop_expect(oracle_mod, detect))
