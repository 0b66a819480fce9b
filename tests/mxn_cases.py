"""The inputs of the MxN colour-grid sensor's shape tests and a restatement of
its launcher, shared by tests/test_mxn_shapes_cpu.py (which asserts on the
restatement and on the reference's output what every input reaches),
tests/test_reference_cpu.py (which runs the frames through the reference's own
class) and tests/test_gpu_mxn_shapes.py (which runs them on the GPU).

form() restates launch_mxn and mxn_hist_kernel's walk (trik-media-sensors-dsp_amd/
csrc/trik_hsv_mxn.hip): a cell row is walked in aligned 4-pixel groups, one
more than ceil(col_step / 4) for a cell that starts inside a group; a wave
takes 64 consecutive groups, the four waves 256, and a cell of more groups
takes several trips of the loop.  A wave handles its lanes' pixel j in slot j:
the first two distinct bins of a slot (by leading lane) are added with one LDS
update each and take the position of their highest lane, the others add lane
by lane.  partials() is the per-wave histograms and last positions this
placement implies, and winner() combines them as the kernel does -- or as a
wrong kernel would (the alterations the cases name).

Every pixel's bin is set on its own: the chroma bytes of all pairs are
(U, V) = CHROMA, under which the luma byte alone reaches 23 bins.
"""
import numpy as np

import mxn_ref

N_BINS = mxn_ref.N_BINS
BLOCK, WAVE, PEEL = 256, 64, 2
WAVES = BLOCK // WAVE
CHROMA = (127, 129)  # (U, V)
GREY = (128, 128)
PAD = 0x77           # the line padding of both planes


# ------------------------------------------------------------ pixel builder

def bins_of_luma(table, u, v):
    """int [256]: the bin of (Y, u, v) for every Y, on the oracle's table."""
    word = table[np.arange(256) | (u << 8) | (v << 16)]
    hsv = (word & np.uint64(0xFFFFFFFF)).astype(np.int64)
    return (((hsv & 255) >> 3) << 4) | ((((hsv >> 8) & 255) >> 6) << 2) | (((hsv >> 16) & 255) >> 6)


class Palette:
    """The bins the luma byte reaches under CHROMA (bin 0, an empty cell's
    winner, left out) and a luma for each.  The sensor's output is a bin's
    colour, and the reference's own class gives nothing else, so a winner
    shows there only by its colour: the palette's bins have four (black and
    three greys), the contenders A, B, C take one grey each (B < A < C by
    index, so neither a lower nor a higher index wins by luck), and every
    noise bin is black."""

    def __init__(self, table):
        b = bins_of_luma(table, *CHROMA)
        uniq, first = np.unique(b, return_index=True)
        self.luma = np.zeros(N_BINS, np.uint8)
        self.luma[uniq] = first
        self.bins = [int(k) for k in uniq if k != 0]
        by_color = {}
        for k in self.bins:
            by_color.setdefault(mxn_ref.bin_color(k), []).append(k)
        greys = sorted(c for c in by_color if c != 0)
        assert len(greys) >= 3
        mid = by_color[greys[1]]
        self.B, self.A, self.C = by_color[greys[0]][0], mid[len(mid) // 2], by_color[greys[2]][-1]
        self.noise = by_color[0]

    def frame(self, bins, ll=None):
        """The ov7670 frame (Y plane, then the V U V U plane) whose pixel (r, c) falls into bins[r, c]."""
        bins = np.asarray(bins)
        h, w = bins.shape
        ll = w if ll is None else ll
        fr = np.full((2, h, ll), PAD, np.uint8)
        fr[0, :, :w] = self.luma[bins]
        fr[1, :, 0:w:2] = CHROMA[1]
        fr[1, :, 1:w:2] = CHROMA[0]
        return fr.reshape(-1)


# ------------------------------------------------- the launcher's decision

class Form:
    """launch_mxn's geometry for a w x h frame at m x n cells, and where the
    kernel's walk puts a cell's pixels."""

    def __init__(self, w, h, m, n):
        self.w, self.h, self.m, self.n = w, h, m, n
        self.row_step, self.col_step = h // m, w // n
        self.per_row = (self.col_step + 3) // 4 + 1 if self.col_step > 0 else 1
        self.total = self.per_row * self.row_step if self.col_step > 0 else 0
        self.trips = -(-self.total // BLOCK)

    def origin(self, cell):
        return cell[0] * self.row_step, cell[1] * self.col_step

    def group(self, cell, r, c):
        """The group number q of cell pixel (r, c) (both inside the cell)."""
        c0 = cell[1] * self.col_step
        return r * self.per_row + ((c0 + c) >> 2) - (c0 >> 2)

    def place(self, cell, r, c):
        """(trip, wave, lane, slot j) of cell pixel (r, c)."""
        q = self.group(cell, r, c)
        return q // BLOCK, (q % BLOCK) // WAVE, q % WAVE, (cell[1] * self.col_step + c) & 3

    def pixel(self, cell, trip, wave, lane, j):
        """The cell pixel (r, c) at a placement, or None where the lane's pixel
        j lies outside the cell (or the lane past the last group)."""
        q = trip * BLOCK + wave * WAVE + lane
        if q >= self.total:
            return None
        c0 = cell[1] * self.col_step
        r, g = divmod(q, self.per_row)
        c = 4 * ((c0 >> 2) + g) + j - c0
        return (r, c) if 0 <= c < self.col_step else None

    def groups_spanned(self, cell):
        """Groups a row of the cell touches; per_row when the extra group is needed."""
        c0 = cell[1] * self.col_step
        return ((c0 + self.col_step - 1) >> 2) - (c0 >> 2) + 1


def form(w, h, m, n):
    return Form(w, h, m, n)


def partials(f, cell, cell_bins, lead=False, peel_only=False, pos_mask=0xFFFFFFFF):
    """The per-wave LDS histograms of one cell: {"cnt", "lst": int64 [trips,
    WAVES, N_BINS] (last raster position + 1, 0: no pixel), "store": int64
    [WAVES, N_BINS], "distinct": {(trip, wave, j): distinct bins of the slot}}.

    lead       the peeled bins take their leading lane's position (first
               instead of last lane);
    peel_only  the lanes left after the PEEL rounds are lost;
    pos_mask   positions are cut to these bits before they are combined;
    "store"    is the position a wave would hold had each update overwritten
               the last one instead of taking the maximum: slots run in the
               order (trip, j), which is not the raster order."""
    cell_bins = np.asarray(cell_bins, np.int64)
    rs, cs = cell_bins.shape
    assert (rs, cs) == (f.row_step, f.col_step)
    c0 = cell[1] * f.col_step
    r, c = np.divmod(np.arange(rs * cs, dtype=np.int64), cs)
    q = r * f.per_row + ((c0 + c) >> 2) - (c0 >> 2)
    trip, wave, j = q // BLOCK, (q % BLOCK) // WAVE, (c0 + c) & 3
    pos1 = (np.arange(rs * cs, dtype=np.int64) + 1) & pos_mask
    slot = (trip * WAVES + wave) * 4 + j
    key, inv = np.unique(slot * N_BINS + cell_bins.reshape(-1), return_inverse=True)
    inv = inv.reshape(-1)
    n = np.bincount(inv, minlength=key.size)
    pmax = np.zeros(key.size, np.int64)
    np.maximum.at(pmax, inv, pos1)
    first = np.full(key.size, rs * cs + 1, np.int64)  # by raster order, whatever pos_mask does
    np.minimum.at(first, inv, np.arange(rs * cs, dtype=np.int64))
    pmin = pos1[first]
    gslot, gbin = key // N_BINS, key % N_BINS
    order = np.lexsort((first, gslot))
    start = np.flatnonzero(np.r_[True, gslot[order][1:] != gslot[order][:-1]])
    sizes = np.diff(np.r_[start, key.size])
    rank = np.empty(key.size, np.int64)
    rank[order] = np.arange(key.size) - np.repeat(start, sizes)
    peeled = rank < PEEL
    add = np.where(peeled | (not peel_only), n, 0)
    pos = np.where(peeled & lead, pmin, pmax)
    pos = np.where(add > 0, pos, 0)
    gt, gw, gj = gslot // (4 * WAVES), (gslot // 4) % WAVES, gslot % 4
    cnt = np.zeros((max(f.trips, 1), WAVES, N_BINS), np.int64)
    lst = np.zeros_like(cnt)
    np.add.at(cnt, (gt, gw, gbin), add)
    np.maximum.at(lst, (gt, gw, gbin), pos)
    store = np.zeros((WAVES, N_BINS), np.int64)
    seq = np.zeros((WAVES, N_BINS), np.int64)
    for i in np.argsort(gt * 4 + gj, kind="stable"):
        if add[i] and gt[i] * 4 + gj[i] + 1 >= seq[gw[i], gbin[i]]:
            seq[gw[i], gbin[i]] = gt[i] * 4 + gj[i] + 1
            store[gw[i], gbin[i]] = pos[i]
    distinct = {(int(s) // (4 * WAVES), (int(s) // 4) % WAVES, int(s) % 4): int(k)
                for s, k in zip(gslot[order][start], sizes)}
    return {"cnt": cnt, "lst": lst, "store": store, "distinct": distinct}


def winner(p, counts="sum", pos="max", bits=32):
    """The cell's winning bin from partials(): counts added and positions
    maximised over the waves, the smallest last position among the bins at the
    largest count (the kernel), or an alteration of it:

    counts="max"  the waves' counts combined by maximum;
    pos="wave"    a later wave taken as a later position: the highest wave
                  that holds a bin gives its last position;
    pos="store"   last update instead of maximum within a wave;
    bits=16       counts and positions held in 16 bits."""
    per_wave = p["cnt"].sum(0)
    c = per_wave.sum(0) if counts == "sum" else per_wave.max(0)
    lw = p["lst"].max(0)
    if pos == "max":
        last = lw.max(0)
    elif pos == "store":
        last = p["store"].max(0)
    else:
        top = (WAVES - 1) - np.argmax((per_wave > 0)[::-1], axis=0)
        last = lw[top, np.arange(N_BINS)]
    mask = (1 << bits) - 1
    c, last = c & mask, last & mask
    at = np.flatnonzero(c == c.max())
    return int(at[np.argmin(last[at] * N_BINS + at)])


# ------------------------------------------------------------------- edges

# (w, h, m, n): every (c0 % 4, col_step % 4) a grid can produce, each with a
# row step of 1 (a column is one pixel) and with a larger one; leftover
# columns (32 // 6, 32 // 10, 32 // 5, 64 // 9, 64 // 7, 64 // 3) and rows
EDGE_GEOMS = [
    (32, 4, 4, 6), (32, 8, 3, 6),       # col_step 5
    (32, 4, 4, 10), (32, 16, 3, 10),    # 3
    (32, 8, 5, 5), (32, 12, 2, 5),      # 6
    (64, 4, 4, 9), (64, 16, 3, 9),      # 7
    (32, 8, 4, 16),                     # 2 (cells of fewer than three pixels cannot make every
    (32, 12, 3, 32),                    # 1  pixel decisive: two bins of one pixel each already tie)
    (32, 4, 4, 8), (32, 8, 2, 8),       # 4
    (64, 8, 8, 7),                      # 9
    (64, 8, 2, 3),                      # 21
]
EMPTY_GEOM = (32, 4, 5, 1)  # row_step == 0: every cell empty


def cell_class(f, cell):
    return (cell[1] * f.col_step) % 4, f.col_step % 4


def reachable_classes(widths=range(32, 641, 32), cells=100):
    """Every (c0 % 4, col_step % 4) of a cell of some grid: the entry point
    takes widths that are multiples of 32, and m * n <= 100 bounds n."""
    out = set()
    for w in widths:
        for n in range(1, cells + 1):
            cs = w // n
            if cs > 0:
                out |= {((j * cs) % 4, cs % 4) for j in range(n)}
    return out


def edge_targets(f):
    """The cells of a grid that get frames of their own: the first five
    columns (every c0 % 4 of an odd step, each with a left neighbour) and the
    last, in the first and the last row of cells."""
    cols = sorted(set(range(min(f.n, 5))) | {f.n - 1})
    return [(ci, cj) for ci in sorted({0, f.m - 1}) for cj in cols]


class EdgeCase:
    """One frame made for one cell.  The cell's pixels alternate between two
    bins in raster order (odd: X, even: Y), but for one pixel:

      lead  X has one pixel more than Y and its last two pixels come after
            Y's last: X wins, and without any one X pixel Y wins the tie;
      tie   equal counts, Y's last pixel first: Y wins the tie, loses it
            without any one Y pixel, and loses to one more X pixel, wherever
            it is counted -- the rest of the frame holds X.

    So every pixel of the cell is decisive in one of the two frames (the one
    pixel of the third bin of a frame is X or Y in the other), and every pixel
    outside it is in the tie frame."""

    def __init__(self, pal, geom, cell, kind):
        self.geom, self.cell, self.kind = geom, cell, kind
        self.name = "%dx%d_%dx%d_cell%d_%d_%s" % (geom + cell + (kind,))
        f = self.form = Form(*geom)
        X, Y = (pal.A, pal.B) if (cell[0] + cell[1]) % 2 == 0 else (pal.B, pal.A)
        N = f.row_step * f.col_step
        assert N >= 3
        seq = np.where(np.arange(N) % 2 == 1, X, Y)
        if N % 2 == 1:
            seq[N - 1] = X if kind == "lead" else pal.C
        elif kind == "lead":
            seq[N - 2] = pal.C
        self.X, self.Y = X, Y
        self.bins = np.full((f.h, f.w), X if kind == "tie" else Y, np.int64)
        r0, c0 = f.origin(cell)
        self.bins[r0:r0 + f.row_step, c0:c0 + f.col_step] = seq.reshape(f.row_step, f.col_step)

    def region(self):
        f = self.form
        r0, c0 = f.origin(self.cell)
        return r0, c0, f.row_step, f.col_step

    def border(self):
        """The pixels (r, c) of the cell's first and last row and column."""
        r0, c0, rs, cs = self.region()
        return [(r, c) for r in range(r0, r0 + rs) for c in range(c0, c0 + cs)
                if r in (r0, r0 + rs - 1) or c in (c0, c0 + cs - 1)]

    def ring(self):
        """The frame's pixels adjacent to the cell: the column left and right
        of it (a neighbour's, or leftover), the row above and below."""
        f = self.form
        r0, c0, rs, cs = self.region()
        out = [(r, c) for r in range(r0, r0 + rs) for c in (c0 - 1, c0 + cs) if 0 <= c < f.w]
        out += [(r, c) for r in (r0 - 1, r0 + rs) for c in range(c0, c0 + cs) if 0 <= r < f.h]
        return out

    def winner_of(self, pixels):
        """winner_sequential over the given frame pixels in raster order."""
        return mxn_ref.winner_sequential([int(self.bins[r, c]) for r, c in sorted(pixels)])

    def cell_pixels(self):
        r0, c0, rs, cs = self.region()
        return [(r, c) for r in range(r0, r0 + rs) for c in range(c0, c0 + cs)]

    def columns(self, lo, hi):
        """The pixels of the cell's rows in frame columns c0 + lo .. c0 + cs - 1 + hi."""
        f = self.form
        r0, c0, rs, cs = self.region()
        return [(r, c) for r in range(r0, r0 + rs) for c in range(max(c0 + lo, 0), min(c0 + cs + hi, f.w))]

    def __repr__(self):
        return self.name


def edge_cases(pal):
    return [EdgeCase(pal, g, cell, kind) for g in EDGE_GEOMS for cell in edge_targets(Form(*g))
            for kind in ("lead", "tie")]


def by_geometry(cases):
    """[(geom, [cases])] in first-seen order: one batch per geometry."""
    out = {}
    for c in cases:
        out.setdefault(c.geom, []).append(c)
    return list(out.items())


# ------------------------------------------------------------------- split

SPLIT_GEOM = (64, 32, 1, 1)   # 17 groups per row, 544 per cell: trips 0 and 1 whole, wave 0 half of trip 2
SPLIT_GEOM2 = (96, 20, 1, 1)  # 25 groups per row, 500 per cell: two trips
PREFIX_ROWS = 8               # rows that only level the contenders' counts


class SplitCase:
    """One single-cell frame.  `slots` gives whole slots {(trip, wave, j):
    bins of lanes 0..63}; the contenders' counts are levelled to `count` in
    the first PREFIX_ROWS rows (which the slots lie after), and every other
    pixel takes the noise bins in turn.  `where` names the placement of each
    contender's last pixel, `alter` the winner() alteration that must change
    the winner, `says` what is placed."""

    def __init__(self, pal, name, slots, contenders, count, where, alter, says, geom=SPLIT_GEOM):
        self.name, self.geom, self.cell, self.where, self.alter, self.says = name, geom, (0, 0), where, alter, says
        self.contenders = contenders
        f = self.form = Form(*geom)
        n_noise = len(pal.noise)
        bins = np.array(pal.noise, np.int64)[np.arange(f.h * f.w) % n_noise].reshape(f.h, f.w)
        for (t, w, j), lanes in slots.items():
            assert len(lanes) == WAVE
            for lane, b in enumerate(lanes):
                px = f.pixel(self.cell, t, w, lane, j)
                if px is not None:
                    assert px[0] >= PREFIX_ROWS, (name, t, w, lane)
                    bins[px] = b
        self.bins = bins
        if count is None:
            return
        # level the contenders in the prefix, interleaved; the rest of it is noise
        need = {b: count - int((bins[PREFIX_ROWS:] == b).sum()) for b in contenders}
        assert all(v >= 0 for v in need.values()) and sum(need.values()) <= PREFIX_ROWS * f.w, (name, need)
        order = [b for i in range(max(need.values())) for b in contenders if need[b] > i]
        pre = bins[:PREFIX_ROWS].reshape(-1)
        pre[:len(order)] = order

    def cell_bins(self):
        return self.bins

    def __repr__(self):
        return self.name


def _lanes(*runs):
    out = [b for b, k in runs for _ in range(k)]
    assert len(out) == WAVE
    return out


def split_cases(pal):
    A, B, C = pal.A, pal.B, pal.C
    N1, N2, N3 = pal.noise[:3]
    out = []

    # (a) the winner is second in every wave of every trip: wave k's own bin
    # holds 3 pixels of 5 there, the winner 2 of 5 everywhere
    own = [B, C, N1, N2]
    c = SplitCase(pal, "sum_over_waves", {}, [A], None, {}, {"counts": "max"},
                  "the winner leads in no wave's histogram of any trip")
    for r in range(c.form.h):
        for col in range(c.form.w):
            t, w, lane, j = c.form.place((0, 0), r, col)
            c.bins[r, col] = A if (4 * lane + j) % 5 < 2 else own[w]
    out.append(c)

    # (b) ties between A and B, the two last pixels ...
    # ... in one slot, the first occurrences in the other order
    out.append(SplitCase(pal, "tie_same_slot", {(1, 1, 2): _lanes((A, 16), (B, 32), (A, 16))}, [A, B], 230,
                         {A: (1, 1, 2), B: (1, 1, 2)}, {"lead": True},
                         "A B A in one slot: B ends first, A begins first"))
    # ... in slots j of one wave: B's last pixel in slot 0 at a high lane, A's in slot 1 at a lower
    # lane and so earlier in raster order, and a B pixel in slot 3 at a low lane is the last B update
    out.append(SplitCase(pal, "tie_slots_of_a_wave",
                         {(1, 2, 0): _lanes((N1, 52), (B, 4), (N1, 8)),
                          (1, 2, 1): _lanes((N2, 40), (A, 4), (N2, 20)),
                          (1, 2, 3): _lanes((N3, 10), (B, 4), (N3, 50))}, [A, B], 230,
                         {A: (1, 2, 1), B: (1, 2, 0)}, {"pos": "store"},
                         "A ends at lane 43 of slot 1, B at lane 55 of slot 0 after a B at lane 13 of slot 3"))
    # ... in two waves of one trip; only A lies in wave 3 (of trip 0)
    out.append(SplitCase(pal, "tie_waves_of_a_trip",
                         {(0, 3, 1): _lanes((A, 8), (N1, 56)),
                          (1, 1, 0): _lanes((B, 8), (N2, 56)), (1, 1, 2): _lanes((B, 24), (N2, 40)),
                          (1, 2, 0): _lanes((A, 24), (N3, 40))}, [A, B], 230,
                         {A: (1, 2, 0), B: (1, 1, 2)}, {"pos": "wave"},
                         "B ends in wave 1 and A in wave 2 of trip 1, A alone is in wave 3"))
    # ... in wave 3 of trip 0 and wave 0 of trip 1
    out.append(SplitCase(pal, "tie_across_trips",
                         {(0, 3, 3): _lanes((N1, 30), (A, 20), (N1, 14)),
                          (1, 0, 0): _lanes((B, 20), (N2, 44))}, [A, B], 230,
                         {A: (0, 3, 3), B: (1, 0, 0)}, {"pos": "wave"},
                         "A ends in wave 3 of trip 0, B in wave 0 of trip 1"))
    out.append(SplitCase(pal, "tie_last_trip",
                         {(1, 3, 2): _lanes((B, 40), (N1, 24)),
                          (2, 0, 1): _lanes((A, 12), (N2, 52))}, [A, B], 230,
                         {A: (2, 0, 1), B: (1, 3, 2)}, {"pos": "wave"},
                         "B ends in wave 3 of trip 1, A in the half-filled wave 0 of trip 2"))

    # (c) slots of 1, 2, 3 and 5 distinct bins
    # ... both contenders after the two peeled bins, A with more pixels there and the earlier end
    out.append(SplitCase(pal, "tie_two_remainder_bins",
                         {(1, 0, 1): _lanes((N1, 6), (N2, 6), (A, 20), (B, 4), (A, 6), (B, 6), (N3, 16))}, [A, B], 230,
                         {A: (1, 0, 1), B: (1, 0, 1)}, {"peel_only": True},
                         "five bins in a slot, A and B third and fourth to appear"))
    # ... A peeled, B one by one
    out.append(SplitCase(pal, "tie_peeled_and_remainder",
                         {(1, 3, 3): _lanes((A, 10), (N1, 10), (B, 20), (A, 10), (N1, 14))}, [A, B], 230,
                         {A: (1, 3, 3), B: (1, 3, 3)}, {"lead": True},
                         "A N B A N in one slot: A is peeled, B adds lane by lane and ends first"))
    # ... three at one count: C ends first, one by one; whole slots of one bin before it
    out.append(SplitCase(pal, "tie_three_way",
                         {(1, 0, 0): _lanes((A, 64)), (1, 0, 2): _lanes((B, 64)), (1, 0, 3): _lanes((C, 64)),
                          (1, 2, 1): _lanes((A, 12), (B, 12), (C, 12), (B, 12), (A, 16))}, [A, B, C], 200,
                         {A: (1, 2, 1), B: (1, 2, 1), C: (1, 2, 1)}, {"lead": True},
                         "A B C B A in one slot: three bins at one count, C ends first"))
    out.append(SplitCase(pal, "tie_three_way_96x20",
                         {(1, 1, 2): _lanes((B, 12), (C, 12), (A, 12), (C, 12), (B, 16))}, [A, B, C], 150,
                         {A: (1, 1, 2), B: (1, 1, 2), C: (1, 1, 2)}, {"lead": True},
                         "B C A C B in one slot of the 96 x 20 cell", geom=SPLIT_GEOM2))
    return out


# --------------------------------------------------------------------- big

BIG_GEOM = (640, 480, 1, 1)
BIG_COUNT = 70000             # of each of the two tied bins: above 2^16
BIG_LAST = (196606, 196613)   # their last positions + 1: above 2^17, the earlier one larger modulo 2^16


class BigCase:
    def __init__(self, name, bins):
        self.name, self.geom, self.cell, self.bins = name, BIG_GEOM, (0, 0), bins
        self.form = Form(*BIG_GEOM)

    def __repr__(self):
        return self.name


def big_cases(pal):
    """The whole-frame cell: A and B alternate over the first positions to
    BIG_COUNT - 1 pixels each, end at BIG_LAST, and three noise bins share the
    rest (about 55,733 pixels each, the last 110,587 positions theirs alone); and
    the same cell in one colour."""
    w, h = BIG_GEOM[:2]
    i = np.arange(w * h, dtype=np.int64)
    bins = np.array(pal.noise[:3], np.int64)[i % 3]
    ab = 2 * (BIG_COUNT - 1)
    bins[:ab] = np.where(i[:ab] % 2 == 0, pal.A, pal.B)  # position + 1 odd: A
    bins[BIG_LAST[0] - 1] = pal.A
    bins[BIG_LAST[1] - 1] = pal.B
    return [BigCase("big_tie", bins.reshape(h, w)), BigCase("big_single", np.full((h, w), pal.C, np.int64))]


# ----------------------------------------------------------------- preview

# (w, h, ll, m, n, ow, oh, oll): squares with gaps (steps 24 and 32); squares
# that overlap (steps 6 and 7) and clamp at the right and bottom edges, 1
# leftover column and 2 leftover rows, an odd output line; an output larger
# than the input both ways (x 2.5), overlapping squares with unwritten pixels
# inside; the same at x 4.5 with an output line above 512 bytes (two blocks a row)
PREVIEW_GEOMS = [
    (96, 48, 96, 2, 3, 48, 24, 96),
    (64, 20, 64, 3, 9, 32, 10, 67),
    (32, 8, 32, 2, 3, 80, 20, 161),
    (64, 8, 66, 2, 5, 288, 36, 580),
]
PREVIEW_FRAMES = 2


def preview_body(pal, w, h, f):
    """A frame whose pixels walk through the palette, shifted per frame."""
    i = np.arange(w * h).reshape(h, w)
    return np.array(pal.bins, np.int64)[(i + i // w + 5 * f) % len(pal.bins)]


def rgb_of_565(v):
    """A 0x00RRGGBB colour that write_px565 turns into v (R in the low bits)."""
    return ((v & 0x1F) << 19) | (((v >> 5) & 0x3F) << 10) | ((v >> 11) << 3)


def preview_colors(body565, n_frames, cells):
    """int32 [n_frames, cells]: one colour per cell and frame, all different
    as RGB565 and none a body pixel's."""
    taken = set(int(v) for v in np.unique(body565))
    out, v = [], 0x0821
    while len(out) < n_frames * cells:
        v = (v * 5 + 0x2F1) & 0xFFFF
        if v not in taken and v != 0:
            taken.add(v)
            out.append(rgb_of_565(v))
    return np.array(out, np.int32).reshape(n_frames, cells)


def square_cell(o, n_cells, step, size, smap, upward=False):
    """mxn_square_cell: the highest cell along one axis whose clamped square
    maps onto output coordinate o, or -1 (upward: the lowest instead)."""
    order = range(n_cells) if upward else range(n_cells - 1, -1, -1)
    for i in order:
        lo, hi = min(i * step, size - 1), min(i * step + 19, size - 1)
        if smap[lo] <= o <= smap[hi]:
            return i
    return -1


def preview_model(rgb, w, h, m, n, colors, ow, oh, oll, upward=False, guard=True):
    """mxn_preview_kernel restated on the frame's RGB values [h, w]."""
    wi2wo, hi2ho = mxn_ref.scale_maps(w, h, ow, oh)
    last_row, last_col = [-1] * oh, [-1] * ow
    for r, ro in enumerate(hi2ho):
        if ro < oh:
            last_row[ro] = r
    for c, co in enumerate(wi2wo):
        if co < ow:
            last_col[co] = c
    out = np.zeros((oh, ow), np.uint16)
    for ro in range(oh):
        ci = square_cell(ro, m, h // m, h, hi2ho, upward)
        for x in range(ow):
            sr, sc = last_row[ro], last_col[x]
            written = sr >= 0 and sc >= 0
            if guard and not written:
                continue
            v = rgb[sr, sc] if written else 0
            cj = square_cell(x, n, w // n, w, wi2wo, upward) if ci >= 0 else -1
            if cj >= 0:
                v = colors[ci * n + cj]
            out[ro, x] = mxn_ref.px565(v)
    buf = np.zeros((oh, oll), np.uint8)
    buf[:, 0:2 * ow:2] = (out & 0xFF).astype(np.uint8)
    buf[:, 1:2 * ow:2] = (out >> 8).astype(np.uint8)
    return buf
