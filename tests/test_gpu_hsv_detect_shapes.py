"""trik_hsv_batch_auto_range (the webcam object sensor's autoDetectHsv) on the
GPU, all six outputs of every frame against hsv_detect_ref's restatement of
HsvRangeDetector::detect, through each of its three kernels:

  vec    auto_range_vec_kernel<YUYV | OV7670>: 16-byte aligned batches;
  k1024  auto_range_kernel<1024>: the same frames 4 bytes past a 16-byte
         boundary, at most 32 of them per call;
  k256   auto_range_kernel<256>: the same, more than 32 frames (a batch is
         padded with copies of its own frames where it has fewer).

hsv_detect_cases.form() says which kernel a call takes; every call asserts it.
What the cases cover, and that each would change the expected output if the
kernel were wrong in the way it is aimed at, is asserted without a GPU in
test_hsv_detect_cpu.py.

  A  every zone-edge class of the chunked kernel (the pixels of a row's first
     and last chunk that it counts and subtracts again), one frame per zone
     alteration that frame would expose, minimal and padded lines;
  B  ties: one channel, two, all three; three values; the deciding last
     occurrences in the final partial pass or in different waves of a pass;
     later occurrences of the winner outside the zone; zones of 81, 289 and
     1089 pixels;
  C  zones of more than 1024 chunks: a lane's run state crosses load batches;
  D  every (Y, U, V) in each pixel of a pair, through both layouts' word
     assembly (vec) and both column parities of the fallback's pixel fetch;
  E  every (Y, U, V) again with its S, then its V, checked exactly: a frame
     whose output changes if the kernel's value is one off."""
import numpy as np
import pytest

import hsv_detect_cases as C
import hsv_detect_ref as R

pytestmark = pytest.mark.gpu

YUYV, OV = C.LAYOUT_YUYV, C.LAYOUT_OV7670
LAYOUTS = [YUYV, OV]
FORMS = ["vec", "k1024", "k256"]
OFFSET = 4  # bytes past a 16-byte boundary of the fallback kernels' batches


@pytest.fixture(scope="module")
def hsv():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import trik_hsv

    return trik_hsv


@pytest.fixture(scope="module")
def table_dev(hsv, table):
    import torch

    return torch.from_numpy((table & 0xFFFFFFFF).astype(np.int32)).cuda()


@pytest.fixture(scope="module")
def memo():
    """References computed once and shared by the three kernels' runs."""
    return {}


def _call(hsv, dev, w, h, ll, layout, n, kind, **kw):
    f = C.form(w, h, ll, layout, n, dev.data_ptr() % 16, kw.get("frame_stride"))
    assert f.kernel == kind, (f, kind)
    return hsv.batch_auto_range(dev, w, h, ll, layout, n_frames=n, **kw).cpu().numpy().astype(np.int64) & 0xFFFF


def _place(frames, offset):
    """Host or device frames [n, bytes] on the device at `offset` bytes past a 16-byte boundary."""
    import torch

    src = torch.from_numpy(frames) if isinstance(frames, np.ndarray) else frames
    raw = torch.empty(src.numel() + 16, dtype=torch.uint8, device="cuda")
    assert raw.data_ptr() % 16 == 0
    dev = raw[offset:offset + src.numel()]
    dev.view(src.shape).copy_(src)
    return dev


def _run(hsv, frames, w, h, ll, layout, kind):
    """frames (numpy uint8 [n, frame bytes]) through kernel `kind`: [n, 6]."""
    n, fb = frames.shape
    assert fb == C.frame_bytes(w, h, ll, layout) and fb % 16 == 0
    if kind == "vec":
        return _call(hsv, _place(frames, 0), w, h, ll, layout, n, kind)
    if kind == "k256":
        padded = frames[np.arange(max(n, C.WIDE_FRAMES + 1)) % n]
        return _call(hsv, _place(padded, OFFSET), w, h, ll, layout, padded.shape[0], kind)[:n]
    dev = _place(frames, OFFSET)
    return np.concatenate([_call(hsv, dev[i * fb:], w, h, ll, layout, min(C.WIDE_FRAMES, n - i), kind)
                           for i in range(0, n, C.WIDE_FRAMES)])


def _want(table, frames, w, h, ll, layout):
    return np.asarray([R.detect(table, fr, w, h, ll, layout) for fr in frames], np.int64)


def _check(got, want, names):
    bad = np.flatnonzero((got != want).any(1))
    assert bad.size == 0, [(names[i], got[i].tolist(), want[i].tolist()) for i in bad[:6]]


# ---------------------------------------------------------------------------
# A. zone edges
# ---------------------------------------------------------------------------
def _edge_batches(memo, table, layout):
    key = ("edge", layout)
    if key not in memo:
        out = []
        for w, h in C.edge_geometries(layout):
            for pad in (0, 16):
                ll = C.min_ll(w, layout) + pad
                whats = C.edge_alterations(w, h)
                frames = np.stack([C.edge_frame(w, h, ll, layout, a) for a in whats])
                out.append((w, h, ll, whats, frames, _want(table, frames, w, h, ll, layout)))
        memo[key] = out
    return memo[key]


@pytest.mark.parametrize("kind", FORMS)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_zone_edges(hsv, table, memo, layout, kind):
    classes = set()
    for w, h, ll, whats, frames, want in _edge_batches(memo, table, layout):
        classes.add(C.edge_class(C.form(w, h, ll, layout, len(whats))))
        _check(_run(hsv, frames, w, h, ll, layout, kind), want, [(w, h, ll, a) for a in whats])
    assert classes == C.reachable_edge_classes(layout)


# ---------------------------------------------------------------------------
# B. ties
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind", FORMS)
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("h", C.TIE_HEIGHTS)
def test_ties(hsv, table, memo, h, layout, kind):
    w, ll = C.TIE_WIDTH, C.min_ll(C.TIE_WIDTH, layout)
    key = ("tie", h, layout)
    if key not in memo:
        frames = C.tie_frames(h, layout)
        memo[key] = frames, _want(table, frames, w, h, ll, layout)
    frames, want = memo[key]
    _check(_run(hsv, frames, w, h, ll, layout, kind), want, [c[0] for c in C.tie_cases(h)])


# ---------------------------------------------------------------------------
# C. more than one load batch of chunks
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind", FORMS)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_more_chunks_than_a_load_batch(hsv, table, memo, layout, kind):
    w, h = C.BIG[layout]
    ll = C.min_ll(w, layout)
    assert C.form(w, h, ll, layout, 1).total > C.VEC_BATCH_CHUNKS
    key = ("big", layout)
    if key not in memo:
        # the frame, and an edge frame of the same geometry (counts across batches, no tie)
        frames = np.stack([C.big_frame(layout), C.edge_frame(w, h, ll, layout, "R+")])
        memo[key] = frames, _want(table, frames, w, h, ll, layout)
    frames, want = memo[key]
    _check(_run(hsv, frames, w, h, ll, layout, kind), want, ["big", "edge"])


# ---------------------------------------------------------------------------
# frame strides that are no multiple of 16
# ---------------------------------------------------------------------------
def test_unaligned_frame_stride(hsv, table):
    """An aligned batch of several frames whose stride is no multiple of 16
    falls back (frames after the first are not aligned); a single frame with
    such a stride stays with the chunked kernel."""
    import torch

    w, h, layout = C.TIE_WIDTH, 32, YUYV
    ll = C.min_ll(w, layout)
    fb = C.frame_bytes(w, h, ll, layout)
    frames = C.tie_frames(h, layout)[:4]
    want = _want(table, frames, w, h, ll, layout)
    stride = fb + 8
    dev = torch.full((4 * stride,), 0x5A, dtype=torch.uint8, device="cuda")
    assert dev.data_ptr() % 16 == 0
    dev.view(4, stride)[:, :fb] = torch.from_numpy(frames).cuda()
    _check(_call(hsv, dev, w, h, ll, layout, 4, "k1024", frame_stride=stride), want, list(range(4)))
    _check(_call(hsv, dev, w, h, ll, layout, 1, "vec", frame_stride=stride), want[:1], [0])
    _check(_call(hsv, dev[2 * stride:], w, h, ll, layout, 1, "vec", frame_stride=stride), want[2:3], [2])


# ---------------------------------------------------------------------------
# D, E. every (Y, U, V)
# ---------------------------------------------------------------------------
SWEEP_FORMS = [(YUYV, "vec"), (OV, "vec"), (YUYV, "k256")]


def _sweep(hsv, words, want, tr, w, h, layout, kind):
    frames = C.to_layout(words, layout)
    del words
    n = frames.shape[0]
    dev = _place(frames, OFFSET) if kind == "k256" else frames.reshape(-1)
    assert dev.data_ptr() % 16 == (OFFSET if kind == "k256" else 0)
    f = C.form(w, h, C.min_ll(w, layout), layout, n, dev.data_ptr() % 16)
    assert f.kernel == kind
    got = hsv.batch_auto_range(dev, w, h, C.min_ll(w, layout), layout, n_frames=n).long() & 0xFFFF
    bad = (got != want).any(1).nonzero()[:, 0][:6]
    assert bad.numel() == 0, [(hex(int(tr[i])), got[i].tolist(), want[i].tolist()) for i in bad]


@pytest.mark.parametrize("part", range(C.N_SLICES))
@pytest.mark.parametrize("layout,kind", SWEEP_FORMS)
@pytest.mark.parametrize("geom", sorted(C.D_GEOMS))
def test_every_triple_in_each_pixel_of_a_pair(hsv, table_dev, geom, layout, kind, part):
    import torch

    w, h, _ = C.D_GEOMS[geom]
    tr = torch.arange(part * C.SLICE, (part + 1) * C.SLICE, device="cuda")
    _sweep(hsv, C.d_words(tr, geom), C.d_expected(tr, table_dev), tr, w, h, layout, kind)


@pytest.fixture(scope="module")
def e_tabs(hsv, table):
    import torch

    return {ch: torch.from_numpy(C.e_tables(table, ch)).cuda() for ch in (1, 2)}


@pytest.mark.parametrize("part", range(C.N_SLICES))
@pytest.mark.parametrize("layout,kind", SWEEP_FORMS)
@pytest.mark.parametrize("ch", [1, 2])
def test_every_triple_s_and_v_exactly(hsv, table_dev, e_tabs, ch, layout, kind, part):
    import torch

    tr = torch.arange(part * C.SLICE, (part + 1) * C.SLICE, device="cuda")
    t = C.e_triples(tr, e_tabs[ch], table_dev, ch)
    _sweep(hsv, C.e_words(t), C.e_expected(t, table_dev), tr, 32, 12, layout, kind)
