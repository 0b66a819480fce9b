"""What the inputs of tests/test_gpu_mxn_shapes.py reach, asserted on the
reference restatement (tests/mxn_ref.py) and on the restated launcher
(tests/mxn_cases.py) alone -- no GPU.  Every claim the GPU file relies on for
its coverage is an assertion here: which pixels decide a cell, where the
kernel's walk puts the contenders of a tie, and which alteration of the kernel
each case tells from the kernel."""
import numpy as np
import pytest

import mxn_cases as mc
import mxn_ref


@pytest.fixture(scope="module")
def pal(table):
    return mc.Palette(table)


@pytest.fixture(scope="module")
def edges(pal):
    return mc.edge_cases(pal)


def _cell(case):
    f = case.form
    r0, c0 = f.origin(case.cell)
    return case.bins[r0:r0 + f.row_step, c0:c0 + f.col_step]


def _kernel_winner(case, **kw):
    alter = {k: kw.pop(k) for k in ("lead", "peel_only", "pos_mask") if k in kw}
    return mc.winner(mc.partials(case.form, case.cell, _cell(case), **alter), **kw)


def test_pixel_builder(table, pal):
    """The luma byte alone sets a pixel's bin: 8 bins at grey chroma, 23 at
    CHROMA; the frame builder's pixels fall into the bins asked for."""
    grey = set(mc.bins_of_luma(table, *mc.GREY).tolist())
    assert grey == {160, 161, 162, 163, 256, 257, 258, 259}
    assert len(set(mc.bins_of_luma(table, *mc.CHROMA).tolist())) == 23
    assert len(pal.bins) >= 22 and 0 not in pal.bins and len({pal.A, pal.B, pal.C}) == 3
    assert pal.B < pal.A < pal.C
    # a winner shows in the sensor's output by its colour alone: the contenders' colours differ from
    # each other and from every noise bin's
    colors = [mxn_ref.bin_color(b) for b in (pal.A, pal.B, pal.C)]
    assert len(set(colors)) == 3 and {mxn_ref.bin_color(b) for b in pal.noise} == {0} and 0 not in colors
    assert len(pal.noise) >= 10 and not set(pal.noise) & {pal.A, pal.B, pal.C}
    want = np.array(pal.bins, np.int64)[np.arange(8 * 32).reshape(8, 32) % len(pal.bins)]
    for ll in (32, 34, 40):
        _, got = mxn_ref.frame_pixels(table, pal.frame(want, ll), 32, 8, ll)
        assert np.array_equal(got, want)


def test_form_against_the_walk():
    """place() and pixel() against a literal walk of the kernel's loop: every
    cell pixel is met once, at the placement place() gives, in raster order
    within a slot; lanes past the cell's columns hold nothing."""
    for w, h, m, n in mc.EDGE_GEOMS + [mc.SPLIT_GEOM, mc.SPLIT_GEOM2, (640, 480, 3, 3), (320, 240, 10, 10)]:
        f = mc.form(w, h, m, n)
        assert f.row_step == h // m and f.col_step == w // n
        assert f.per_row == (f.col_step + 3) // 4 + 1 and f.total == f.per_row * f.row_step
        assert f.trips == -(-f.total // 256)
        for cell in ((0, 0), (m - 1, n - 1), (0, min(1, n - 1))):
            c0 = cell[1] * f.col_step
            seen = {}
            for q0 in range(0, f.total, 256):           # a trip
                for wave in range(4):
                    for lane in range(64):
                        q = q0 + wave * 64 + lane
                        if q >= f.total:
                            continue
                        rr, col4 = q // f.per_row, 4 * (c0 // 4 + q % f.per_row)
                        for j in range(4):
                            inside = col4 < c0 + f.col_step and c0 <= col4 + j < c0 + f.col_step
                            px = f.pixel(cell, q0 // 256, wave, lane, j)
                            assert (px is not None) == inside
                            if inside:
                                assert px == (rr, col4 + j - c0) and px not in seen
                                seen[px] = (q0 // 256, wave, lane, j)
            assert len(seen) == f.row_step * f.col_step
            assert all(f.place(cell, r, c) == at for (r, c), at in seen.items())
            assert f.groups_spanned(cell) <= f.per_row


def test_reachable_classes_complete(edges):
    """Even column steps give even cell starts only: 11 of the 16 classes
    (c0 % 4, col_step % 4) exist, and the edge cases hold each of them both
    with a row step of 1 and with a larger one."""
    want = {(a, b) for a in range(4) for b in range(4) if b % 2 == 1 or (b == 0 and a == 0) or (b == 2 and a % 2 == 0)}
    assert len(want) == 11 and mc.reachable_classes() == want
    # any width and any number of cell columns, not only the entry point's
    assert mc.reachable_classes(widths=range(1, 200), cells=200) - {(0, 0)} <= want
    one_row = {mc.cell_class(c.form, c.cell) for c in edges if c.form.row_step == 1}
    rows = {mc.cell_class(c.form, c.cell) for c in edges if c.form.row_step > 1}
    assert one_row == want and rows == want
    # cells that need the extra group of a row, and cells that do not
    spans = {c.form.groups_spanned(c.cell) == c.form.per_row for c in edges}
    assert spans == {True, False}
    assert mc.form(*mc.EMPTY_GEOM).row_step == 0 and mc.form(*mc.EMPTY_GEOM).total == 0


def test_edge_every_border_pixel_decides(edges):
    """Per cell, over its two frames: every pixel of the cell is decisive
    (the winner changes without it), the border included, and every adjacent
    pixel outside is decisive as an intruder.  The share left out is 0."""
    cells = {}
    for c in edges:
        cells.setdefault((c.geom, c.cell), []).append(c)
    assert all(sorted(k.kind for k in v) == ["lead", "tie"] for v in cells.values())
    n_border = n_ring = 0
    sides = set()
    for (geom, cell), pair in cells.items():
        inside = pair[0].cell_pixels()
        border, ring = pair[0].border(), pair[0].ring()
        r0, c0, rs, cs = pair[0].region()
        assert set(border) <= set(inside) and not set(ring) & set(inside)
        f = pair[0].form
        # the ring is complete: whatever of the four sides lies inside the frame
        want = rs * ((c0 > 0) + (c0 + cs < f.w)) + cs * ((r0 > 0) + (r0 + rs < f.h))
        assert len(ring) == want and len(border) == len(set(border)) == rs * cs - max(rs - 2, 0) * max(cs - 2, 0)
        sides |= {"left" for r, c in ring if c < c0} | {"right" for r, c in ring if c >= c0 + cs}
        sides |= {"above" for r, c in ring if r < r0} | {"below" for r, c in ring if r >= r0 + rs}
        if c0 + cs < f.w and cell[1] == f.n - 1:
            sides.add("leftover columns")
        if r0 + rs < f.h and cell[0] == f.m - 1:
            sides.add("leftover rows")
        decided, intruded = set(), set()
        for c in pair:
            base = c.winner_of(inside)
            assert base == (c.X if c.kind == "lead" else c.Y)
            assert base == mxn_ref.winner_order_free(_cell(c)) == _kernel_winner(c)
            tied = len(mxn_ref.tied_bins(_cell(c))) >= 2
            assert tied == (c.kind == "tie") or rs * cs == 3  # three pixels: 1 : 1 : 1
            decided |= {p for p in inside if c.winner_of([x for x in inside if x != p]) != base}
            intruded |= {p for p in ring if c.winner_of(inside + [p]) != base}
        assert decided == set(inside), (geom, cell, sorted(set(inside) - decided))
        assert intruded == set(ring), (geom, cell, sorted(set(ring) - intruded))
        n_border += len(border)
        n_ring += len(ring)
    assert sides == {"left", "right", "above", "below", "leftover columns", "leftover rows"}
    assert n_border > 1000 and n_ring > 1000


def test_edge_column_clipping_alterations(edges):
    """The kernel edits the clipping invites, as whole columns: the cell's
    first or last column dropped, the column left or right of it counted, and
    the extra group of a row dropped.  Each changes the winner of some frame
    of every class it can touch."""
    hit = {k: set() for k in ("drop_first", "drop_last", "admit_left", "admit_right", "no_extra_group")}
    can = {k: set() for k in hit}
    for c in edges:
        f = c.form
        cls = mc.cell_class(f, c.cell)
        r0, c0, rs, cs = c.region()
        base = c.winner_of(c.cell_pixels())
        regions = {"drop_first": c.columns(1, 0), "drop_last": c.columns(0, -1)}
        if c0 > 0:
            regions["admit_left"] = c.columns(-1, 0)
        if c0 + cs < f.w:
            regions["admit_right"] = c.columns(0, 1)
        if f.groups_spanned(c.cell) == f.per_row:  # without the extra group: ceil(col_step / 4) groups from c0's
            end = 4 * (c0 // 4 + f.per_row - 1)
            regions["no_extra_group"] = [(r, col) for r, col in c.cell_pixels() if col < end]
        for k, px in regions.items():
            can[k].add(cls)
            if c.winner_of(px) != base:
                hit[k].add(cls)
    assert all(hit[k] == can[k] for k in hit), {k: sorted(can[k] - hit[k]) for k in hit}
    assert len(can["drop_first"]) == len(can["admit_left"]) == len(can["admit_right"]) == 11
    # a row reaches into one group more than ceil(col_step / 4) where c0 % 4 + col_step passes the next
    # multiple of 4: steps of 3 mod 4 that start at 2 or 3 mod 4
    assert can["no_extra_group"] == {(2, 3), (3, 3)}


def test_split_cases(pal):
    """The placement puts the contenders where each case says, and the
    alteration the case names changes the winner."""
    cases = mc.split_cases(pal)
    distinct = set()
    altered = set()
    where = set()
    for c in cases:
        f, cell = c.form, _cell(c)
        assert f.trips >= 2
        seq = cell.reshape(-1).tolist()
        base = mxn_ref.winner_sequential(seq)
        assert base == mxn_ref.winner_order_free(cell) == _kernel_winner(c), c
        assert base in c.contenders
        if c.name == "sum_over_waves":
            p = mc.partials(f, c.cell, cell)
            assert mxn_ref.tied_bins(cell) == [base]
            lead = p["cnt"].argmax(2)  # [trip, wave]
            live = p["cnt"].sum(2) > 0
            assert live.sum() == 9 and not (lead[live] == base).any()
            assert not (p["cnt"].sum(0).argmax(1) == base).any()
            assert (p["cnt"].sum(0)[:, base] > 0).all()
        else:
            assert sorted(mxn_ref.tied_bins(cell)) == sorted(c.contenders), c
            lasts = {}
            for b in c.contenders:
                r, col = divmod(int(np.flatnonzero(cell.reshape(-1) == b)[-1]), f.col_step)
                t, w, lane, j = f.place(c.cell, r, col)
                assert (t, w, j) == c.where[b], (c, b, (t, w, lane, j))
                lasts[b] = (r, col)
                where.add((t, w))
            assert min(lasts, key=lasts.get) == base
        got = _kernel_winner(c, **c.alter)
        assert got != base and mxn_ref.bin_color(got) != mxn_ref.bin_color(base), (c, c.alter)
        altered |= set(c.alter.items())
        distinct |= set(mc.partials(f, c.cell, cell)["distinct"].values())
        if c.name == "tie_same_slot":
            sl = [cell[f.pixel(c.cell, 1, 1, lane, 2)] for lane in range(64) if f.pixel(c.cell, 1, 1, lane, 2)]
            assert sl.index(pal.A) < sl.index(pal.B) and base == pal.B
            assert len(sl) - 1 - sl[::-1].index(pal.B) < len(sl) - 1 - sl[::-1].index(pal.A)
    assert {1, 2, 3} <= distinct and max(distinct) >= 5
    assert altered == {("counts", "max"), ("lead", True), ("pos", "store"), ("pos", "wave"), ("peel_only", True)}
    assert {(0, 3), (1, 0), (2, 0)} <= where
    by = {c.name: c for c in cases}
    # the remainder ties: both contenders past the peel rounds / one of each kind
    for name, n_peeled in (("tie_two_remainder_bins", 0), ("tie_peeled_and_remainder", 1), ("tie_three_way", 2)):
        c = by[name]
        t, w, j = next(iter(c.where.values()))
        sl = [int(_cell(c)[c.form.pixel(c.cell, t, w, lane, j)]) for lane in range(64)
              if c.form.pixel(c.cell, t, w, lane, j)]
        firsts = sorted(set(sl), key=sl.index)
        assert sum(firsts.index(b) < mc.PEEL for b in c.contenders) == n_peeled, (name, firsts)
    assert len(by["tie_three_way"].contenders) == 3 and by["tie_three_way_96x20"].geom == mc.SPLIT_GEOM2


def test_big_cases(pal):
    """Counts above 2^16, last positions above 2^17 with another bin's pixels
    after them; 16-bit counts or positions change the winner."""
    tie, single = mc.big_cases(pal)
    seq = tie.bins.reshape(-1)
    counts = np.bincount(seq, minlength=mc.N_BINS)
    assert counts[pal.A] == counts[pal.B] == mc.BIG_COUNT > 1 << 16 and counts.max() == mc.BIG_COUNT
    last = {b: int(np.flatnonzero(seq == b)[-1]) + 1 for b in (pal.A, pal.B)}
    assert (last[pal.A], last[pal.B]) == mc.BIG_LAST and min(mc.BIG_LAST) > 1 << 17
    assert set(seq[max(mc.BIG_LAST):].tolist()) == set(pal.noise[:3])
    base = mxn_ref.winner_sequential(seq.tolist())
    assert base == pal.A == mxn_ref.winner_order_free(seq) == _kernel_winner(tie)
    assert tie.form.trips == 302 and tie.form.total == 161 * 480
    p = mc.partials(tie.form, tie.cell, tie.bins)
    # counts modulo 2^16 (positions whole), positions modulo 2^16 when combined, or when stored
    c16 = p["cnt"].sum((0, 1)) & 0xFFFF
    assert int(np.argmax(c16)) in pal.noise[:3]
    assert mc.winner(p, bits=16) not in (pal.A, pal.B)
    assert len({mxn_ref.bin_color(b) for b in (pal.A, pal.B, mc.winner(p, bits=16))}) == 3
    l16 = p["lst"].max((0, 1)) & 0xFFFF
    assert l16[pal.B] < l16[pal.A]
    assert _kernel_winner(tie, pos_mask=0xFFFF) == pal.B
    assert (single.bins == pal.C).all() and single.bins.size == 307200
    assert _kernel_winner(single) == pal.C and mc.winner(mc.partials(single.form, (0, 0), single.bins), bits=16) == pal.C
    assert (mc.partials(single.form, (0, 0), single.bins)["cnt"].sum((0, 1))[pal.C] & 0xFFFF) != 307200


def test_preview_cases(table, pal):
    """The caller's colours differ from each other and from every body pixel
    as RGB565, so a square pixel names its cell; the geometries hold gaps,
    overlaps, clamped squares, leftover columns and rows, unwritten pixels
    inside squares and a second block per row; the restated kernel equals the
    reference, and scanning the cells upward or dropping the written-pixel
    guard does not."""
    seen = set()
    for w, h, ll, m, n, ow, oh, oll in mc.PREVIEW_GEOMS:
        bodies = [mc.preview_body(pal, w, h, i) for i in range(mc.PREVIEW_FRAMES)]
        frames = [pal.frame(b, ll) for b in bodies]
        rgb = [mxn_ref.frame_pixels(table, fr, w, h, ll)[0] for fr in frames]
        body565 = np.concatenate([mxn_ref.px565(x).reshape(-1) for x in rgb])
        colors = mc.preview_colors(body565, mc.PREVIEW_FRAMES, m * n)
        c565 = mxn_ref.px565(colors.reshape(-1).astype(np.uint32))
        assert len(set(c565.tolist())) == c565.size and not set(c565.tolist()) & set(body565.tolist())
        assert 0 not in c565.tolist()
        rs, cs = h // m, w // n
        wi2wo, hi2ho = mxn_ref.scale_maps(w, h, ow, oh)
        if rs > 20 and cs > 20:
            seen.add("gaps")
        if rs < 20 and cs < 20:
            seen.add("overlap")
        if (n - 1) * cs + 19 > w - 1 and (m - 1) * rs + 19 > h - 1:
            seen.add("clamped")
        if w % n and h % m:
            seen.add("leftover")
        if oll % 2:
            seen.add("odd line")
        if oll > 512:
            seen.add("two blocks")
        if ow > w and oh > h:
            seen.add("upscaled")
        for i in range(mc.PREVIEW_FRAMES):
            want = mxn_ref.preview(table, frames[i], w, h, ll, m, n, colors[i].tolist(), ow, oh, oll)
            assert np.array_equal(mc.preview_model(rgb[i], w, h, m, n, colors[i], ow, oh, oll), want)
            px = want[:, 0:2 * ow:2].astype(np.uint16) | (want[:, 1:2 * ow:2].astype(np.uint16) << 8)
            assert set(c565[i * m * n:(i + 1) * m * n].tolist()) <= set(px.reshape(-1).tolist()) or rs < 20 or cs < 20
            up = mc.preview_model(rgb[i], w, h, m, n, colors[i], ow, oh, oll, upward=True)
            if rs < 20 or cs < 20:
                assert not np.array_equal(up, want)
            if ow > w and oh > h:
                # unwritten output pixels inside a square stay 0
                written = np.zeros((oh, ow), bool)
                written[np.ix_(sorted(set(hi2ho)), sorted(set(wi2wo)))] = True
                in_sq = np.array([[mc.square_cell(r, m, rs, h, hi2ho) >= 0 and mc.square_cell(x, n, cs, w, wi2wo) >= 0
                                   for x in range(ow)] for r in range(oh)])
                assert (in_sq & ~written).sum() > 0 and not px[~written].any()
                seen.add("unwritten in a square")
                assert not np.array_equal(mc.preview_model(rgb[i], w, h, m, n, colors[i], ow, oh, oll, guard=False), want)
    assert seen == {"gaps", "overlap", "clamped", "leftover", "odd line", "two blocks", "upscaled",
                    "unwritten in a square"}
