"""The chroma-run kernel's exact path takes flagged words whole
(trik_hsv_chroma.hip: select2w zeroes both pixels of a flagged word, the drain
computes both exactly without looking the chroma up again) -- against the CPU
oracle, bit-exact, on frames crafted from the CPU model of the tables
(tests/test_chroma_model.py) for the bench's 4 ranges and its first range
alone.

* Every window chroma and every exception chroma, in words with pixel 0 in the
  flagged zone and pixel 1 outside it, the reverse, and both inside; Y at b2,
  b2 + 1, b1 - 1 and b1, and at the cut A and A - 1 for chromas of cut blocks.
  Packed into batches of 640x16, 640x32 and 640x48 frames (1, 2 and 3 steps of
  the hot loop), YUYV and ov7670: the sums, and the verification mode's mask of
  every pixel.
* Pieces (4 words) with 2, 3 and 4 flagged words: the drain's re-queue.
* Frames of flagged words only: every append of a step finds the queue full.
* trik_hsv_batch_sums and the fused step, on 1, 2 and 17 frames.

Not vacuous: for every input the number of words the kernel's exact path
resolved (the count behind Detector.chroma_measured_share, tests/
test_gpu_auto.py) equals the model's number of flagged words, exactly, and
that number is positive (checked on the CPU first).
"""
import numpy as np
import pytest

from gpu_util import LAYOUT_OV7670, LAYOUT_YUYV, sums_from_mask
from test_chroma_model import BENCH, KEXC, build, profiles

pytestmark = pytest.mark.gpu

W = 640
GREY = 0x80808080


@pytest.fixture(scope="module")
def hsv():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import trik_hsv

    return trik_hsv


class Model:
    """The tables of one range set (CPU model) and the words made from them."""

    def __init__(self, oracle_mod, ranges):
        self.ranges = ranges
        runs, _, cut = build(profiles(oracle_mod, ranges))
        self.b1, self.b2 = runs & 255, runs >> 8
        self.exc = runs == KEXC
        self.A = np.repeat(cut, 16)
        Y = np.arange(256)[None, :]
        # flagged[c, Y]: the pixel raises its word's flag
        self.flagged = self.exc[:, None] | ((Y < self.b1[:, None]) & (Y > self.b2[:, None]))
        self.window = ~self.exc & (self.b1 > self.b2 + 1)

    def word_flagged(self, words):
        w = np.asarray(words, np.uint32)
        c = ((w >> 8) & 255) | ((w >> 24) << 8)
        return self.flagged[c, w & 255] | self.flagged[c, (w >> 16) & 255]

    def count(self, words):
        return int(self.word_flagged(words).sum())

    def combination_words(self):
        """Every window and exception chroma in every pixel combination."""
        out = []
        c = np.flatnonzero(self.window).astype(np.uint32)
        b1, b2, A = (v[c].astype(np.uint32) for v in (self.b1, self.b2, self.A))
        lo_in, hi_in, lo_out, hi_out = b2 + 1, b1 - 1, b2, b1  # inside / outside the window
        for i in (lo_in, hi_in):
            for o in (lo_out, hi_out):
                out += [_words(c, i, o), _words(c, o, i)]  # one pixel inside
        out += [_words(c, lo_in, hi_in), _words(c, hi_in, lo_in)]  # both inside
        cutb = A > 0
        for y in (A[cutb] - 1, A[cutb]):  # at and below the cut, beside a window pixel
            out += [_words(c[cutb], y, lo_in[cutb]), _words(c[cutb], hi_in[cutb], y)]
        c = np.flatnonzero(self.exc).astype(np.uint32)
        A = self.A[c].astype(np.uint32)
        for y0, y1 in ((0, 255), (255, 0), (128, 17)):
            out.append(_words(c, np.uint32(y0), np.uint32(y1)))
        cutb = A > 0
        out += [_words(c[cutb], A[cutb] - 1, A[cutb]), _words(c[cutb], A[cutb], A[cutb] - 1)]
        return np.concatenate(out)

    def clean_words(self, n, rng):
        """n words that raise no flag: window chromas with both Y outside."""
        c = rng.choice(np.flatnonzero(self.window), n).astype(np.uint32)
        w = _words(c, self.b2[c].astype(np.uint32), self.b1[c].astype(np.uint32))
        assert not self.word_flagged(w).any()
        return w

    def flagged_words(self, n, rng):
        """n flagged words: window words with one pixel inside, exception words."""
        c = rng.choice(np.flatnonzero(self.window), n).astype(np.uint32)
        w = _words(c, (self.b2[c] + 1).astype(np.uint32), self.b1[c].astype(np.uint32))
        if self.exc.any():  # (the one-range set has no exception chroma)
            e = rng.choice(np.flatnonzero(self.exc), n).astype(np.uint32)
            we = _words(e, rng.integers(0, 256, n).astype(np.uint32), rng.integers(0, 256, n).astype(np.uint32))
            w = np.where(rng.integers(0, 2, n) == 0, w, we).astype(np.uint32)
        assert self.word_flagged(w).all()
        return w


def _words(c, y0, y1):
    """YUYV words (bytes Y0, U, Y1, V) as uint32."""
    return (y0 | ((c & 255) << 8) | (y1 << 16) | ((c >> 8) << 24)).astype(np.uint32)


@pytest.fixture(scope="module", params=[4, 1], ids=["bench4", "range1"])
def model(request, oracle_mod):
    m = Model(oracle_mod, BENCH[: request.param])
    assert m.window.sum() > 0 and (m.exc.sum() > 0 or request.param == 1)
    return m


def _yuyv_batch(words, h):
    """The words in frames of W x h YUYV (the rest grey): [n, h * W / 2] uint32."""
    per = h * W // 2
    n = (len(words) + per - 1) // per
    fr = np.full(n * per, GREY, np.uint32)
    fr[: len(words)] = words
    return fr.reshape(n, per)


def _bytes(batch, layout, h):
    """The batch's frames as bytes: YUYV (line length 2 W) or ov7670 (luma plane,
    then the chroma plane: even byte V, odd byte U; line length W)."""
    px = np.ascontiguousarray(batch).astype("<u4").view(np.uint8).reshape(len(batch), h * W // 2, 4)
    if layout == LAYOUT_YUYV:
        return px.reshape(-1)
    ylum = np.stack([px[..., 0], px[..., 2]], -1).reshape(len(batch), -1)
    chrom = np.stack([px[..., 3], px[..., 1]], -1).reshape(len(batch), -1)
    return np.concatenate([ylum, chrom], axis=1).reshape(-1)


def _to_dev(arr):
    import torch

    return torch.from_numpy(np.ascontiguousarray(arr)).cuda()


def _resolved_words(hsv, dev, n, h, layout, ranges):
    """Words the exact path resolved in one launch over the batch: a fresh
    handle's first call gives the counter's base, the eight calls after it one
    readback; the share it reports is their words over theirs launched."""
    import torch

    ll = 2 * W if layout == LAYOUT_YUYV else W
    det = hsv.Detector(hot=hsv.HOT_CHROMA)
    try:
        for _ in range(9):
            det.process_batch(dev, W, h, ll, layout, ranges, n_frames=n)
            torch.cuda.synchronize()
        assert det.last_hot_kernel() == hsv.HOT_CHROMA
        share = det.chroma_measured_share()
    finally:
        det.close()
    assert share >= 0, "no measured share after nine launches"
    got = share * (n * (W // 2) * h)
    assert abs(got - round(got)) < 1e-3, got
    return int(round(got))


def _check(hsv, oracle_mod, model, batch, h, layout, masks=True):
    """Sums, verification-mode masks and the resolved-word count of one batch."""
    ranges, T, n = model.ranges, len(model.ranges), len(batch)
    want_words = model.count(batch.reshape(-1))
    assert want_words > 0  # (on the CPU, before anything runs on the GPU)
    ll = 2 * W if layout == LAYOUT_YUYV else W
    host = _bytes(batch, layout, h)
    fb = oracle_mod.frame_bytes(W, h, ll, layout)
    want_s, want_t = oracle_mod.batch(host, fb, n, W, h, ll, layout, ranges, n_threads=8)
    dev = _to_dev(host)
    det = hsv.Detector(hot=hsv.HOT_CHROMA)
    try:
        sums, tg = det.process_batch(dev, W, h, ll, layout, ranges, n_frames=n)
        assert det.last_hot_kernel() == hsv.HOT_CHROMA
        assert np.array_equal(sums.cpu().numpy(), want_s)
        assert np.array_equal(tg[:, :, :3].cpu().numpy(), want_t)
        if masks:
            got_m, msums = det.batch_masks(dev, W, h, ll, layout, ranges, n_frames=n)
            got_m = got_m.cpu().numpy()
            for f in range(n):
                _, want_m = oracle_mod.frame(host[f * fb:(f + 1) * fb], W, h, ll, layout, ranges, want_mask=True)
                bad = np.count_nonzero(got_m[f] != want_m)
                assert bad == 0, f"frame {f}: {bad} pixels differ; first at {np.argwhere(got_m[f] != want_m)[:5].tolist()}"
                assert sums_from_mask(want_m, T).tolist() == want_s[f].tolist()
            assert np.array_equal(msums.cpu().numpy(), want_s)
    finally:
        det.close()
    got_words = _resolved_words(hsv, dev, n, h, layout, ranges)
    print(f"exact-path words: kernel {got_words}, model {want_words}")
    assert got_words == want_words
    return dev, want_s, want_t


@pytest.mark.parametrize("layout", [LAYOUT_YUYV, LAYOUT_OV7670], ids=["yuyv", "ov7670"])
@pytest.mark.parametrize("h", [16, 32, 48])
def test_every_pixel_combination(hsv, oracle_mod, model, h, layout):
    words = model.combination_words()
    assert model.word_flagged(words).all()  # (every word has a pixel in the flagged zone)
    _check(hsv, oracle_mod, model, _yuyv_batch(words, h), h, layout)


@pytest.mark.parametrize("layout", [LAYOUT_YUYV, LAYOUT_OV7670], ids=["yuyv", "ov7670"])
def test_several_flagged_words_in_one_piece(hsv, oracle_mod, model, layout):
    """Pieces with 2, 3 and 4 flagged words (at every position among the 4):
    a drained record goes back to the queue with its remaining bits."""
    rng = np.random.default_rng(5)
    h, n = 32, 2
    pieces = n * h * W // 8
    words = model.clean_words(4 * pieces, rng).reshape(pieces, 4)
    pats = [p for p in range(16) if bin(p).count("1") >= 2]  # which of a piece's words are flagged
    pat = np.array([pats[i % len(pats)] for i in range(pieces)])
    sel = ((pat[:, None] >> np.arange(4)[None, :]) & 1).astype(bool)
    words[sel] = model.flagged_words(int(sel.sum()), rng)
    per_piece = model.word_flagged(words.reshape(-1)).reshape(pieces, 4).sum(1)
    assert set(per_piece.tolist()) == {2, 3, 4}
    _check(hsv, oracle_mod, model, words.reshape(n, -1), h, layout)


@pytest.mark.parametrize("layout", [LAYOUT_YUYV, LAYOUT_OV7670], ids=["yuyv", "ov7670"])
def test_full_queue(hsv, oracle_mod, model, layout):
    """Every word of every lane flagged in both piece slots of three
    consecutive steps: each append finds the queue full and drains first, and
    every record is drained four times."""
    rng = np.random.default_rng(6)
    h, n = 48, 2
    words = model.flagged_words(n * h * W // 2, rng)
    assert model.count(words) == len(words)
    _check(hsv, oracle_mod, model, words.reshape(n, -1), h, layout)


@pytest.mark.parametrize("n", [1, 2, 17])
def test_call_paths(hsv, oracle_mod, model, n):
    """trik_hsv_batch_sums (adds into the caller's sums) and the fused step
    (trik_hsv_process_batch_totals) on the first n frames of the 640x16 batch."""
    import torch

    h = 16
    # (the words repeated to fill 17 frames: the one-range set makes two)
    batch = np.resize(model.combination_words(), (17, h * W // 2))[:n]
    dev, want_s, want_t = _check(hsv, oracle_mod, model, batch, h, LAYOUT_YUYV, masks=False)
    ranges, T = model.ranges, len(model.ranges)
    det = hsv.Detector(hot=hsv.HOT_CHROMA)
    try:
        sums = torch.zeros((n, T, 3), dtype=torch.int64, device="cuda")
        det.batch_sums(dev, W, h, 2 * W, LAYOUT_YUYV, ranges, sums, n_frames=n)
        assert det.last_hot_kernel() == hsv.HOT_CHROMA
        assert np.array_equal(sums.cpu().numpy(), want_s)
        for _ in range(2):  # (the fused step leaves its scratch clean for the next launch)
            s2, t2, tot = det.process_batch_totals(dev, W, h, 2 * W, LAYOUT_YUYV, ranges, n_frames=n)
            torch.cuda.synchronize()
            assert det.last_hot_kernel() == hsv.HOT_CHROMA
            assert np.array_equal(s2.cpu().numpy(), want_s)
            assert np.array_equal(t2[:, :, :3].cpu().numpy(), want_t)
            assert np.array_equal(tot.cpu().numpy(), want_s.sum(0))
    finally:
        det.close()
