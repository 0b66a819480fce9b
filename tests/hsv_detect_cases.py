"""Inputs for the tests of trik_hsv_batch_auto_range's three kernels
(test_hsv_detect_cpu.py, test_gpu_hsv_detect_shapes.py), and form(): which
kernel launch_auto_range starts for a call.  Test code, not product.

Crafted frames keep to the pixel formats' constraint that the two pixels of a
pair share U and V: colours that must be placed pixel by pixel differ in Y
only.  At (U 90, V 200), Y 60 / 100 / 180 / 21 give HSV (1, 254, 165),
(7, 230, 211), (9, 142, 255) and (0, 255, 120), so
every output differs between any two of them.

(launch_auto_range's guard "the zone's last chunk lies in its row" cannot
fail for a batch it is given: the line length is a multiple of 16 and at
least the row's bytes, so the 16-byte chunk holding the zone's last pixel ends
inside the line.  form() restates the guard; no case reaches its other side.)
"""
from collections import namedtuple

import numpy as np

import hsv_detect_ref as R

LAYOUT_YUYV, LAYOUT_OV7670 = R.LAYOUT_YUYV, R.LAYOUT_OV7670
VEC_BATCH_CHUNKS = 4 * 256  # kVecBatch x kRangeBlock: a lane's chunks of one load batch are this far apart
WIDE_FRAMES = 32            # kRangeWideFrames: up to here the fallback has 1024 lanes per frame

Form = namedtuple("Form", "kernel k0 per_row lo_f hi_l total")


def frame_bytes(w, h, ll, layout):
    return h * ll * (2 if layout == LAYOUT_OV7670 else 1)


def min_ll(w, layout):
    return 2 * w if layout == LAYOUT_YUYV else w


def form(w, h, ll, layout, n, base_offset=0, frame_stride=None):
    """launch_auto_range's decision for one call: kernel 'vec' (the chunked
    two-pass kernel, with its geometry), 'k1024' or 'k256' (the fallbacks)."""
    stride = frame_bytes(w, h, ll, layout) if frame_stride is None else frame_stride
    if n <= 0:
        return None
    if base_offset % 16 == 0 and (n <= 1 or stride % 16 == 0) and ll % 16 == 0:
        pxc = 8 if layout == LAYOUT_YUYV else 16
        r0, r1, c0, c1 = R.zone(w, h)
        zw, zh = c1 - c0, r1 - r0
        k0 = cpr = 0
        if zw > 0 and zh > 0:
            k0 = c0 // pxc
            cpr = (c1 - 1) // pxc + 1 - k0
        if 16 * (k0 + cpr) <= ll:
            per_row = cpr if cpr > 0 else 1
            return Form("vec", k0, per_row, c0 - k0 * pxc, c1 - (k0 + per_row - 1) * pxc, cpr * zh if cpr > 0 else 0)
    return Form("k1024" if n <= WIDE_FRAMES else "k256", None, None, None, None, None)


def edge_class(f):
    """The chunked kernel's zone-edge class of a form: the pixels it subtracts
    in a row's first and last chunk, and whether those are one chunk."""
    return f.lo_f, f.hi_l, f.per_row == 1


# ---------------------------------------------------------------------------
# frames from pixel planes
# ---------------------------------------------------------------------------
def slots(ll, layout):
    """Pixel slots of a line, padding included."""
    return ll // 2 if layout == LAYOUT_YUYV else ll


def luma_frame(Y, U, V, layout):
    """A frame of one (U, V) from its luma plane Y [h, slots] (uint8)."""
    h, p = Y.shape
    if layout == LAYOUT_YUYV:
        fr = np.empty((h, p // 2, 4), np.uint8)
        fr[..., 0], fr[..., 1], fr[..., 2], fr[..., 3] = Y[:, 0::2], U, Y[:, 1::2], V
        return fr.reshape(-1)
    chroma = np.empty((h, p), np.uint8)
    chroma[:, 0::2], chroma[:, 1::2] = V, U
    return np.concatenate([Y.astype(np.uint8).reshape(-1), chroma.reshape(-1)])


UV = (90, 200)
LUMA = (100, 180, 60, 21)  # colours 0..3 at UV; 0 and 1 are A and P of the edge frames


def _zone_index(w, h):
    """(rows, cols) of the zone's pixels in scan order."""
    r0, r1, c0, c1 = R.zone(w, h)
    if r0 >= r1 or c0 >= c1:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    rr, cc = np.meshgrid(np.arange(r0, r1), np.arange(c0, c1), indexing="ij")
    return rr.reshape(-1), cc.reshape(-1)


def seq_frame(w, h, ll, layout, seq, outside, lumas=LUMA, uv=UV):
    """The zone's pixels in scan order take colours lumas[seq]; every other
    pixel slot, line padding included, lumas[outside]."""
    Y = np.full((h, slots(ll, layout)), lumas[outside], np.uint8)
    rr, cc = _zone_index(w, h)
    Y[rr, cc] = np.asarray(lumas, np.uint8)[np.asarray(seq)]
    return luma_frame(Y, uv[0], uv[1], layout)


# ---------------------------------------------------------------------------
# A. zone edges
# ---------------------------------------------------------------------------
ALTERATIONS = ("L+", "R+", "T+", "B+", "L-", "R-", "T-", "B-")
EDGE_WIDTH, EDGE_HEIGHTS = 64, range(8, 108, 4)
SWEEP_WIDTHS, SWEEP_HEIGHTS = (32, 64, 96), range(4, 220, 4)


def reachable_edge_classes(layout):
    """Every zone-edge class the chunked kernel meets with width % 32 == 0."""
    out = set()
    for w in SWEEP_WIDTHS:
        for h in SWEEP_HEIGHTS:
            f = form(w, h, min_ll(w, layout), layout, 1)
            if f.kernel == "vec" and f.total:
                out.add(edge_class(f))
    return out


def edge_geometries(layout):
    """The smallest (w, h) of each zone-edge class, width 64."""
    seen, out = set(), []
    for h in EDGE_HEIGHTS:
        f = form(EDGE_WIDTH, h, min_ll(EDGE_WIDTH, layout), layout, 1)
        if f.kernel == "vec" and f.total and edge_class(f) not in seen:
            seen.add(edge_class(f))
            out.append((EDGE_WIDTH, h))
    return out


def edge_alterations(w, h):
    """The alterations a frame can be built for: all eight, but for the
    one-pixel zone widened right or below (a tie there keeps the earlier
    pixel, whatever the added pixels hold)."""
    r0, r1, c0, c1 = R.zone(w, h)
    one = (r1 - r0) * (c1 - c0) == 1
    return [a for a in ALTERATIONS if not (one and a in ("R+", "B+"))]


def edge_frame(w, h, ll, layout, what):
    """Colours A (0) and P (1): A has one pixel more than P in the true zone
    and holds its last pixel; every pixel outside the zone is P and every
    pixel that narrowing `what` removes is A, so the altered zone's winner is
    P (or nothing), the true zone's A."""
    zn = R.zone(w, h)
    rr, cc = _zone_index(w, h)
    n = rr.size
    r0, r1, c0, c1 = R.alter(zn, what)
    forced = ~((rr >= r0) & (rr < r1) & (cc >= c0) & (cc < c1))  # removed by a narrowing
    seq = np.ones(n, np.int64)
    seq[forced] = 0
    need = (n + 1) // 2 - int(forced.sum())
    assert need >= 0
    free = np.flatnonzero(~forced)
    if need:
        seq[free[-need:]] = 0
    assert seq[-1] == 0 and 2 * int((seq == 0).sum()) == n + 1
    return seq_frame(w, h, ll, layout, seq, 1)


# ---------------------------------------------------------------------------
# B. ties
# ---------------------------------------------------------------------------
# mask (bit 0 H, 1 S, 2 V) -> (U, V, Ya, Yb, Yc): the colours (Ya, U, V) and
# (Yb, U, V) differ in exactly the mask's channels, as do their scaled outputs,
# and (Yc, U, V) differs from both in all three.  Found by a search over the oracle's table;
# test_hsv_detect_cpu.py asserts each property on the table.
TIE_COLOURS = {
    1: (255, 2, 20, 21, 8),
    2: (253, 108, 20, 46, 248),
    3: (253, 104, 20, 51, 248),
    4: (1, 0, 20, 21, 225),
    5: (131, 0, 20, 21, 197),
    6: (129, 126, 20, 21, 128),
    7: (126, 126, 20, 21, 237),
}
TIE_HEIGHTS = (32, 56, 104)  # zones of 81, 289, 1089 pixels: one full pass of 64, 256, 1024 lanes plus 17, 33, 65
TIE_WIDTH = 64


def tie_positions(n, variant, k=2):
    """Zone positions (scan order) of the k tied colours' last occurrences.
    'final': the zone's last pixels, in the final, partially active pass of
    the 64-, 256- and 1024-lane walks.  'waves': the last lanes of
    neighbouring waves in the last full pass (81 pixels: lane 63 of wave 0 and
    the last active lane of wave 1), everything after them the rarer colour."""
    if variant == "final":
        return list(range(n - k, n))
    lanes = max(v for v in (64, 256, 1024) if v < n)
    if lanes == 64:
        return [63 - 16 * i for i in range(k - 2, -1, -1)] + [n - 1]
    return [lanes - 1 - 64 * i for i in range(k - 1, -1, -1)]


def tie_sequence(n, pos, order):
    """n zone pixels of len(pos) colours with equal counts, colour order[i]
    with its last occurrence at pos[i] (ascending), and a rarer colour
    len(pos): a colour index per pixel."""
    k = len(pos)
    assert list(pos) == sorted(pos) and pos[-1] < n
    tail = n - 1 - pos[-1]
    a = (n - tail - 1) // k
    lead = n - k * a - tail
    seq = np.full(n, -1, np.int64)
    seq[:lead] = k
    seq[pos[-1] + 1:] = k
    left = [a] * k
    for i, p in enumerate(pos):
        seq[p] = i
        left[i] -= 1
    for x in range(pos[-1], lead - 1, -1):
        if seq[x] >= 0:
            continue
        allowed = [i for i in range(k) if pos[i] > x and left[i] > 0]
        assert allowed, (n, pos, x)
        i = max(allowed, key=lambda c: (left[c], c))
        seq[x] = i
        left[i] -= 1
    assert not any(left) and (seq >= 0).all() and n - k * a < a
    remap = np.asarray(list(order) + [k])
    return remap[seq]


def tie_cases(h):
    """(name, lumas, uv, seq, outside, tied mask) of every tie frame of height
    h.  `outside` is the winner's colour in the 'final' variants -- a later
    occurrence of it beside or below the zone must not count as its last --
    and the loser's in the 'waves' ones."""
    rr, _ = _zone_index(TIE_WIDTH, h)
    n = rr.size
    out = []
    for mask, (u, v, ya, yb, yc) in sorted(TIE_COLOURS.items()):
        for first in (0, 1):
            for variant in ("final", "waves"):
                seq = tie_sequence(n, tie_positions(n, variant), (first, 1 - first))
                outside = first if variant == "final" else 1 - first
                out.append((f"mask{mask}-first{first}-{variant}", (ya, yb, yc), (u, v), seq, outside, mask))
    for first in range(3):  # three-way: colours 2, 0, 1 of LUMA (Y 60, 100, 180) and the fourth as the rarer one
        order = [(first + i) % 3 for i in range(3)]
        seq = tie_sequence(n, tie_positions(n, "waves", 3), order)
        out.append((f"three-first{first}", (LUMA[2], LUMA[0], LUMA[1], LUMA[3]), UV, seq, order[0], 7))
    return out


def tie_frames(h, layout):
    ll = min_ll(TIE_WIDTH, layout)
    return np.stack([seq_frame(TIE_WIDTH, h, ll, layout, seq, outside, lumas, uv)
                     for _, lumas, uv, seq, outside, _ in tie_cases(h)])


# ---------------------------------------------------------------------------
# C. more than one load batch of chunks
# ---------------------------------------------------------------------------
def big_geometry(layout):
    """The geometry with the fewest pixels (then the smallest width) whose
    zone has more chunks than one load batch of a workgroup."""
    best = None
    for w in range(32, 288, 32):
        for h in range(4, 640, 4):
            f = form(w, h, min_ll(w, layout), layout, 1)
            if f.kernel == "vec" and f.total > VEC_BATCH_CHUNKS:
                if best is None or (w * h, w) < (best[0] * best[1], best[0]):
                    best = (w, h)
                break
    return best


BIG = {LAYOUT_YUYV: (96, 264), LAYOUT_OV7670: (160, 392)}


def chunk_index(w, h, layout, rr, cc):
    """The chunked kernel's chunk number of zone pixels (rows rr, columns cc)."""
    f = form(w, h, min_ll(w, layout), layout, 1)
    pxc = 8 if layout == LAYOUT_YUYV else 16
    return (rr - R.zone(w, h)[0]) * f.per_row + cc // pxc - f.k0


def big_frame(layout):
    """Long single-colour runs: A (0) on even zone rows and P (1) on odd ones,
    every fourth chunk column colour 2, up to the first load batch's last
    chunk; in the second batch P on four chunks, then colours 2 and 3 by turns.  Counts of A
    and P are then levelled by turning the earliest pixels of the more
    frequent one into colour 3.  A's last occurrence lies in the first batch,
    P's in the second: a tie in every channel that A wins, and A fills the
    frame outside the zone."""
    w, h = BIG[layout]
    rr, cc = _zone_index(w, h)
    j = chunk_index(w, h, layout, rr, cc)
    pxc = 8 if layout == LAYOUT_YUYV else 16
    seq = np.where((rr - rr[0]) % 2 == 0, 0, 1)
    seq[(cc // pxc) % 4 == 3] = 2
    late = j >= VEC_BATCH_CHUNKS
    seq[late] = np.where(j[late] < VEC_BATCH_CHUNKS + 4, 1, 2 + j[late] % 2)
    na, nb = int((seq == 0).sum()), int((seq == 1).sum())
    more = 0 if na > nb else 1
    seq[np.flatnonzero(seq == more)[: abs(na - nb)]] = 3
    cnt = np.bincount(seq, minlength=4)
    assert cnt[0] == cnt[1] and cnt[2] < cnt[0] and cnt[3] < cnt[0]
    return seq_frame(w, h, min_ll(w, layout), layout, seq, 0)


# ---------------------------------------------------------------------------
# D, E. every (Y, U, V), frames built on the device
# ---------------------------------------------------------------------------
SLICE = 1 << 20
N_SLICES = (1 << 24) // SLICE
# D: (w, h, majority pixel of a pair): a 3x3 zone at columns 15..17 (odd
# columns hold 6 of 9 pixels), a 5x5 zone at columns 14..18 (even: 15 of 25)
D_GEOMS = {"32x12": (32, 12, 1), "32x20": (32, 20, 0)}


def other_luma(y):
    return (167 * y + 13) & 255  # never y: 166 y is even, -13 odd


def _i32(x):
    import torch

    return torch.where(x >= 1 << 31, x - (1 << 32), x).to(torch.int32)


def pair_word(y0, u, y1, v):
    return y0 | (u << 8) | (y1 << 16) | (v << 24)


def to_layout(words, layout):
    """YUYV words (torch int32 [N, h, pairs per line]) -> frames uint8 [N, frame bytes]."""
    import torch

    n = words.shape[0]
    if layout == LAYOUT_YUYV:
        return words.contiguous().view(torch.uint8).reshape(n, -1)
    b = words.contiguous().view(torch.uint8).reshape(n, words.shape[1], words.shape[2], 4)
    luma, chroma = b[..., [0, 2]].reshape(n, -1), b[..., [3, 1]].reshape(n, -1)  # chroma: V even, U odd
    return torch.cat([luma, chroma], 1)


def d_words(tr, geom):
    """D frames of the triples `tr` (torch int64 [N], Y | U << 8 | V << 16):
    every pair holds the triple in its majority pixel and other_luma(Y) in
    the other."""
    w, h, major = D_GEOMS[geom]
    y, u, v = tr & 255, (tr >> 8) & 255, tr >> 16
    o = other_luma(y)
    word = _i32(pair_word(o, u, y, v) if major else pair_word(y, u, o, v))
    return word.view(-1, 1, 1).expand(-1, h, w // 2)


# E: 32x12, zone rows 5..7, columns 15 (the second pixel of pair 7) and
# 16, 17 (pair 8).  Zone pixels in scan order: Z Z Z / Q X X / Q W W.  In the
# channel under test X's value has count 4 (X twice, its probe Q twice), the
# rival Z's 3 and the filler W's 2.  Were the kernel's value of X off in both
# pixels of the pair, X's value would keep Q's count 2; were it off in one, 3,
# a tie that Z wins: its last occurrence comes first.
E_ZONE = ("z", "z", "z", "q", "x", "x", "q", "w", "w")
# (Y, U, V) that are the only triple with their S or with their V value, and so have no probe: none
E_SINGLE_TRIPLES = []


def e_tables(table, ch):
    """For channel ch (1 S, 2 V) and each of its values v: two triples with
    that value (q1, q2: X's probe is the one that is not X), a rival triple z
    whose value is 128 away (it scales differently) and a filler w whose value
    is 64 away (not v, v - 1, v + 1 or z's).  int64 [4, 256]; -1 where a
    value has no triple."""
    vals = ((table & 0xFFFFFFFF) >> (8 * ch)).astype(np.uint8)
    first = np.full(256, -1, np.int64)
    last = np.full(256, -1, np.int64)
    u, i = np.unique(vals, return_index=True)
    first[u] = i
    u, i = np.unique(vals[::-1], return_index=True)
    last[u] = vals.size - 1 - i
    v = np.arange(256)
    return np.stack([last, first, first[(v + 128) & 255], first[(v + 64) & 255]])


def e_triples(tr, tabs, table_dev, ch):
    """{'x', 'q', 'z', 'w'} -> triples (torch int64 [N]) of the E frames for
    the triples under test `tr`."""
    import torch

    xv = (table_dev[tr] >> (8 * ch)) & 255
    q = torch.where(tabs[0][xv] == tr, tabs[1][xv], tabs[0][xv])
    return {"x": tr, "q": q, "z": tabs[2][xv], "w": tabs[3][xv]}


def e_words(t):
    """The 32x12 frames of e_triples' output as YUYV words [N, 12, 16]: the
    rival's pair everywhere outside the zone."""
    def pair(tr, end=False):
        y, u, v = tr & 255, (tr >> 8) & 255, tr >> 16
        return _i32(pair_word(other_luma(y) if end else y, u, y, v))

    words = pair(t["z"]).view(-1, 1, 1).repeat(1, 12, 16)
    for row, (end, whole) in zip((5, 6, 7), (("z", "z"), ("q", "x"), ("q", "w"))):
        words[:, row, 7] = pair(t[end], end=True)  # (column 14, outside the zone: another luma)
        words[:, row, 8] = pair(t[whole])
    return words


def scaled(wins):
    """The six outputs [N, 6] of the winners (three torch int64 [N])."""
    import torch

    hue = torch.from_numpy(R.HUE_OUT).to(wins[0].device)
    sv = torch.from_numpy(R.SV_OUT).to(wins[0].device)
    tol = torch.full_like(wins[0], 15)
    return torch.stack([hue[wins[0]], tol, sv[wins[1]], 2 * tol, sv[wins[2]], 2 * tol], 1)


def d_expected(tr, table_dev):
    """The winners of a D frame are its triple's own H, S, V."""
    e = table_dev[tr].long()
    return scaled([(e >> (8 * k)) & 255 for k in range(3)])


def e_expected(t, table_dev):
    """The restatement (small_zone_winners) over an E frame's nine zone pixels."""
    import torch

    e = table_dev[torch.stack([t[k] for k in E_ZONE], 1)].long()
    return scaled([R.small_zone_winners((e >> (8 * k)) & 255) for k in range(3)])
