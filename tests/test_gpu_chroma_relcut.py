"""The chroma-run kernel's cut, applied by one packed subtract on descriptors
stored relative to it (trik_hsv_chroma.hip: chroma_desc_rel, select2), on
frames crafted from the blocks that have a cut -- against the CPU oracle,
bit-exact.

The blocks with a cut A > 0 of the bench's 4-range set come from the CPU model
(tests/golden/relcut_blocks.json, held to the model by
tests/test_chroma_model_relcut.py): 366 blocks of 16 chromas.  The frames hold

* every such chroma with all 256 Y, each as pixel 0 and as pixel 1 of a word
  (word j of a chroma: Y0 = j, Y1 = 255 - j; 3.0 M pixels): verification mode
  (the per-pixel masks and the sums) and the hot kernel proper (the sums);
* the same chromas with Y at and next to their block's cut in one frame of
  640x16, 640x32 and 640x48 -- 1, 2 and 3 steps of the hot loop, which takes
  two steps per round and leaves at an odd count;
* one 32x4 frame in the ov7670 layout, and one call of the multi-blob sensor's
  bitmap on the chroma-run tables.
"""
import json
import os

import numpy as np
import pytest

from blob_patterns import check_frame
from gpu_util import BENCH_RANGES, LAYOUT_OV7670, LAYOUT_YUYV, sums_from_mask

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "relcut_blocks.json")


@pytest.fixture(scope="module")
def hsv():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import trik_hsv

    return trik_hsv


@pytest.fixture(scope="module")
def chroma(hsv):
    d = hsv.Detector(hot=hsv.HOT_CHROMA)
    yield d
    d.close()


@pytest.fixture(scope="module")
def cut_chromas():
    """(c, A): the chromas c = U | V << 8 of the blocks with a cut, and that cut."""
    with open(FIXTURE) as f:
        fx = json.load(f)
    assert [tuple(r) for r in fx["ranges"]] == BENCH_RANGES
    b, A = np.asarray(fx["blocks"], np.uint32), np.asarray(fx["cuts"], np.uint32)
    assert len(b) > 300 and (A > 0).all()
    # block b = (V << 4) | (U >> 4): its chromas are U = 16 (b & 15) + i, V = b >> 4
    c = (((b >> 4) << 8) | ((b & 15) << 4))[:, None] + np.arange(16, dtype=np.uint32)[None, :]
    return c.reshape(-1), np.repeat(A, 16)


def _words(c, y0, y1):
    """YUYV words (bytes Y0, U, Y1, V) as uint32."""
    return (y0 | ((c & 255) << 8) | (y1 << 16) | ((c >> 8) << 24)).astype("<u4")


def _yuyv_frame(words, w, h):
    """An h x w YUYV frame of the given words (the rest grey), line length 2 w."""
    fr = np.full(h * w // 2, 0x80808080, "<u4")
    assert len(words) <= len(fr)
    fr[: len(words)] = words
    return fr.view(np.uint8)


def _near_cut_words(c, A):
    """Per chroma, Y at and next to the cut in both pixel positions: kind by
    kind, so that any prefix holds whole kinds of as many chromas as fit."""
    lo, hi = A - 1, np.minimum(A + 1, 255)
    kinds = [(lo, A), (A, lo), (hi, A), (A, hi), (lo, lo), (A, A)]
    return np.concatenate([_words(c, a, b) for a, b in kinds])


def _to_dev(arr):
    import torch

    return torch.from_numpy(np.ascontiguousarray(arr)).cuda()


@pytest.fixture(scope="module")
def full_frame(cut_chromas, oracle_mod):
    """Every cut-block chroma x all 256 Y in both pixel positions, and the oracle's masks."""
    c, _ = cut_chromas
    j = np.arange(256, dtype=np.uint32)
    words = _words(c[:, None], j[None, :], 255 - j[None, :]).reshape(-1)
    w = 640
    h = (len(words) + w // 2 - 1) // (w // 2)
    h = (h + 3) // 4 * 4  # (the reference takes heights that are multiples of 4)
    h += 4 if h % 16 == 0 else 0  # and a last step with rows past the frame
    frame = _yuyv_frame(words, w, h)
    assert 2 * len(words) >= 2_900_000
    _, want = oracle_mod.frame(frame, w, h, 2 * w, LAYOUT_YUYV, BENCH_RANGES, want_mask=True)
    return frame, w, h, want


def test_cut_chromas_all_y_masks(hsv, chroma, full_frame):
    frame, w, h, want = full_frame
    masks, sums = chroma.batch_masks(_to_dev(frame), w, h, 2 * w, LAYOUT_YUYV, BENCH_RANGES)
    assert chroma.last_hot_kernel() == hsv.HOT_CHROMA
    got = masks[0].cpu().numpy()
    bad = np.count_nonzero(got != want)
    assert bad == 0, f"{bad} pixels differ; first at {np.argwhere(got != want)[:5].tolist()}"
    assert sums[0].cpu().numpy().tolist() == sums_from_mask(want, 4).tolist()


def test_cut_chromas_all_y_sums(hsv, chroma, full_frame):
    frame, w, h, want = full_frame
    sums, _ = chroma.process_batch(_to_dev(frame), w, h, 2 * w, LAYOUT_YUYV, BENCH_RANGES)
    assert chroma.last_hot_kernel() == hsv.HOT_CHROMA
    assert sums[0].cpu().numpy().tolist() == sums_from_mask(want, 4).tolist()


@pytest.mark.parametrize("h", [16, 32, 48])
def test_cut_chromas_one_two_three_steps(hsv, chroma, oracle_mod, cut_chromas, h):
    w = 640
    frame = _yuyv_frame(_near_cut_words(*cut_chromas)[: h * w // 2], w, h)
    _, want = oracle_mod.frame(frame, w, h, 2 * w, LAYOUT_YUYV, BENCH_RANGES, want_mask=True)
    assert want.any()
    dev = _to_dev(frame)
    sums, _ = chroma.process_batch(dev, w, h, 2 * w, LAYOUT_YUYV, BENCH_RANGES)
    assert chroma.last_hot_kernel() == hsv.HOT_CHROMA
    assert sums[0].cpu().numpy().tolist() == sums_from_mask(want, 4).tolist()
    masks, msums = chroma.batch_masks(dev, w, h, 2 * w, LAYOUT_YUYV, BENCH_RANGES)
    assert np.array_equal(masks[0].cpu().numpy(), want)
    assert msums[0].cpu().numpy().tolist() == sums_from_mask(want, 4).tolist()


def _ov7670_frame(words, w, h):
    """The YUYV words as an ov7670 frame (luma plane, then the chroma plane:
    even byte V, odd byte U), line length w."""
    px = _yuyv_frame(words, w, h).reshape(h, w // 2, 4)
    ylum = np.stack([px[..., 0], px[..., 2]], -1).reshape(-1)
    chrom = np.stack([px[..., 3], px[..., 1]], -1).reshape(-1)
    return np.concatenate([ylum, chrom])


def test_cut_chromas_ov7670_32x4(hsv, chroma, oracle_mod, cut_chromas):
    c, A = cut_chromas
    w, h = 32, 4
    # 64 words: chromas of blocks spread over the cut blocks, Y around the cut
    pick = np.arange(32) * (len(c) // 32)
    words = _near_cut_words(c[pick], A[pick])[: h * w // 2]
    frame = _ov7670_frame(words, w, h)
    _, want = oracle_mod.frame(frame, w, h, w, LAYOUT_OV7670, BENCH_RANGES, want_mask=True)
    dev = _to_dev(frame)
    masks, msums = chroma.batch_masks(dev, w, h, w, LAYOUT_OV7670, BENCH_RANGES)
    assert chroma.last_hot_kernel() == hsv.HOT_CHROMA
    assert np.array_equal(masks[0].cpu().numpy(), want)
    assert msums[0].cpu().numpy().tolist() == sums_from_mask(want, 4).tolist()
    sums, _ = chroma.process_batch(dev, w, h, w, LAYOUT_OV7670, BENCH_RANGES)
    assert sums[0].cpu().numpy().tolist() == sums_from_mask(want, 4).tolist()


# the bench's first range (hue 0..30, sat 50..100, val 30..100) as the sensor's
# centre and tolerance
BLOB_RANGE = (15, 15, 75, 25, 65, 35)


def test_cut_chromas_blob_bitmap(hsv, chroma, oracle_mod, cut_chromas):
    """The multi-blob sensor's bitmap kernel reads the same tables: one frame
    of the near-cut words, the bitmap, labels, clusters and targets against
    the oracle."""
    w, h = 640, 96
    frame = _ov7670_frame(_near_cut_words(*cut_chromas)[: h * w // 2], w, h)
    res = chroma.blob_batch(_to_dev(frame), w, h, w, BLOB_RANGE, meta=True, labels=True)
    assert chroma.last_hot_kernel() == hsv.HOT_CHROMA
    ref = oracle_mod.blob_run(frame, w, h, w, hsv=BLOB_RANGE, preview=False)
    assert ref["meta"].any()
    check_frame(res, 0, ref, "near-cut words")
