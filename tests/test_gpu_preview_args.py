"""The argument checks of the five preview entry points (trik_hsv_batch_preview,
_line_preview, _blob_preview, _mxn_preview, _edge_preview) through the C ABI
itself: which call is refused, with which trik_hsv_last_error() text, and which
call returns 0 without touching the previews.

Frames are 64 x 8, N = 2, previews 32 x 4 with line length 64: the smallest
shape all five take (the multi-blob sensor needs width % 32 and height % 4, the
edge-line sensor height >= 3 and line_length == width)."""
import ctypes as C

import pytest

pytestmark = pytest.mark.gpu

W, H, N = 64, 8, 2
OW, OH, OLL = 32, 4, 64
PB = OH * OLL  # bytes of one preview
SENTINEL = 0xA5
ENTRIES = ["batch", "batch_yuyv", "line", "blob", "mxn", "edge"]  # batch_preview on either layout
OV7670_ONLY = ENTRIES[2:]
SENSOR = {"line": "line", "blob": "multi-blob", "mxn": "MxN", "edge": "edge-line"}
GEOMETRY = "preview geometry: need out_line_length >= 2*out_width"


@pytest.fixture(scope="module")
def hsv():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import trik_hsv

    return trik_hsv


@pytest.fixture(scope="module")
def env(hsv):
    """One handle and every device buffer the five calls read, all valid."""
    import torch

    det = hsv.Detector()
    g = torch.Generator().manual_seed(7)
    e = {
        "det": det,
        "frames": torch.randint(0, 256, (N * 2 * H * W,), dtype=torch.uint8, generator=g).cuda(),
        "sums": torch.zeros((N, 3), dtype=torch.int64, device="cuda"),
        "meta": torch.zeros((N, H // 4, W // 4), dtype=torch.uint8, device="cuda"),
        "top": torch.zeros((N, 8, 3), dtype=torch.int32, device="cuda"),
        "colors": torch.zeros((N, 1), dtype=torch.int32, device="cuda"),
    }
    yield e
    det.close()


def _batch(hsv, env, entry, layout=None, n=N, width=W, line_length=None):
    if layout is None:
        layout = hsv.LAYOUT_YUYV if entry == "batch_yuyv" else hsv.LAYOUT_OV7670
    if line_length is None:
        line_length = 2 * width if layout == hsv.LAYOUT_YUYV else width
    return hsv._abi.FrameBatch(env["frames"].data_ptr(), 2 * H * W, n, width, H, line_length, layout)


def _previews():
    import torch

    return torch.full((N * PB,), SENTINEL, dtype=torch.uint8, device="cuda")


def _call(hsv, env, entry, b, previews, *, handle=True, ow=OW, oh=OH, oll=OLL, stride=PB, sums_pitch=1):
    """The entry point on batch b with every other argument valid; `previews`
    is a tensor or None (NULL).  Returns (code, trik_hsv_last_error())."""
    import torch

    lib = hsv._lib
    h = env["det"]._h if handle else None
    p = C.c_void_p(previews.data_ptr()) if previews is not None else None
    ptr = lambda k: C.c_void_p(env[k].data_ptr())  # noqa: E731
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    tail = (ow, oh, oll, p, stride, s)
    if entry.startswith("batch"):
        arr = (hsv._abi.InArgsAlg * 1)(hsv._abi.InArgsAlg(0, 359, 0, 100, 0, 100, 0))
        rc = lib.trik_hsv_batch_preview(h, C.byref(b), arr, ptr("sums"), sums_pitch, *tail)
    elif entry == "line":
        rc = lib.trik_hsv_line_preview(h, C.byref(b), 0, 100, ptr("sums"), *tail)
    elif entry == "blob":
        rc = lib.trik_hsv_blob_preview(h, C.byref(b), ptr("meta"), ptr("top"), *tail)
    elif entry == "mxn":
        rc = lib.trik_hsv_mxn_preview(h, C.byref(b), 1, 1, ptr("colors"), *tail)
    else:
        rc = lib.trik_hsv_edge_preview(h, C.byref(b), 50, ptr("sums"), *tail)
    torch.cuda.synchronize()
    return rc, hsv._abi.last_error()


def _refused(hsv, env, entry, message, b=None, previews="sentinel", **kw):
    pv = _previews() if isinstance(previews, str) else previews
    rc, err = _call(hsv, env, entry, _batch(hsv, env, entry) if b is None else b, pv, **kw)
    assert rc != 0, (entry, "accepted")
    assert err == message, (entry, err)
    if pv is not None:
        assert bool((pv == SENTINEL).all()), (entry, "a refused call wrote the previews")


@pytest.mark.parametrize("entry", ENTRIES)
def test_null_handle(hsv, env, entry):
    _refused(hsv, env, entry, "handle is NULL", handle=False)


@pytest.mark.parametrize("entry", ENTRIES)
def test_line_length_shorter_than_a_row(hsv, env, entry):
    _refused(hsv, env, entry, GEOMETRY + (", sums_pitch >= 1" if entry.startswith("batch") else ""), oll=2 * OW - 1)


@pytest.mark.parametrize("entry", ENTRIES[:2])
def test_batch_preview_sums_pitch_zero(hsv, env, entry):
    _refused(hsv, env, entry, GEOMETRY + ", sums_pitch >= 1", sums_pitch=0)


@pytest.mark.parametrize("entry", ENTRIES)
def test_stride_smaller_than_a_preview(hsv, env, entry):
    _refused(hsv, env, entry, "preview_stride smaller than one preview", stride=PB - 1)


@pytest.mark.parametrize("entry", ENTRIES)
def test_null_previews(hsv, env, entry):
    _refused(hsv, env, entry, "previews is NULL" if entry.startswith("batch") else "NULL buffer", previews=None)


@pytest.mark.parametrize("entry", OV7670_ONLY)
def test_packed_layout_refused(hsv, env, entry):
    _refused(hsv, env, entry, "the %s sensor takes the ov7670 layout (YUV422P)" % SENSOR[entry],
             b=_batch(hsv, env, entry, layout=hsv.LAYOUT_YUYV))


@pytest.mark.parametrize("entry", ENTRIES)
def test_no_frames_returns_zero_untouched(hsv, env, entry):
    pv = _previews()
    rc, err = _call(hsv, env, entry, _batch(hsv, env, entry, n=0), pv)
    assert rc == 0, (entry, err)
    assert bool((pv == SENTINEL).all()), entry


@pytest.mark.parametrize("entry", ENTRIES)
def test_no_preview_rows_returns_zero_untouched(hsv, env, entry):
    pv = _previews()
    rc, err = _call(hsv, env, entry, _batch(hsv, env, entry), pv, oh=0)
    assert rc == 0, (entry, err)
    assert bool((pv == SENTINEL).all()), entry


@pytest.mark.parametrize("entry", ["mxn", "edge"])
def test_frames_without_pixels_zero_both_previews(hsv, env, entry):
    """width = 0: the two entry points that handle it themselves write the
    zero fill alone.  (The other three are not called with such a batch.)"""
    pv = _previews()
    rc, err = _call(hsv, env, entry, _batch(hsv, env, entry, width=0, line_length=0), pv)
    assert rc == 0, (entry, err)
    assert bool((pv == 0).all()), entry
