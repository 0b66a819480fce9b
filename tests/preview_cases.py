"""The inputs of the object-sensor preview's shape tests and the launcher's
decision for each, shared by tests/test_preview_cpu.py (which asserts on the
restated decision and on the reference's output what every input reaches) and
tests/test_gpu_preview_shapes.py (which runs them on the GPU).

forms() restates ensure_maps (trik-media-sensors-dsp_amd/csrc/trik_hsv_sensors.cpp)
and launch_preview, launch_rows2 and launch_gather (trik_hsv_operator.hip beside
it) for one trik_hsv_batch_preview call, as tests/test_gpu_blob_shapes.py restates
launch_blob.  What the restatement shows: the rows kernel's WIN form together
with GUIDES is unreachable from trik_hsv_batch_preview.  An unwritten output
column under 2:1 row maps needs out_h / h < out_w / w, so out_w > w / 2, and
then 2 * out_w > w makes launch_rows2 refuse (test_preview_cpu.py sweeps
geometries for it); the instantiations stay, the line sensors use WIN.  It
shows the same of launch_rows2's out_w % 8 test alone: the entry point takes
widths that are multiples of 32 only, 2:1 maps with every column written need
out_w == w / 2, a multiple of 16; any other out_w under 2:1 row maps is larger,
and the 2 * out_w > w test refuses it as well (the same sweep).

Every case list is a function of the CU count, so the GPU tests build theirs
from the device and the CPU test checks the claims for several counts.
"""
import numpy as np

import preview_ref
from preview_ref import LAYOUT_OV7670, LAYOUT_YUYV

T0 = (0, 30, 50, 100, 30, 100)        # a hue-bounded range
V_BAND = (0, 359, 0, 100, 30, 70)     # every hue: the rows kernel's HUEFREE form
SV_BAND = (0, 359, 40, 90, 30, 70)    # every hue, saturation bounded too: HUEFREE's own read of that axis
TAGS = {T0: "t0", V_BAND: "v", SV_BAND: "sv"}
STRIPE_TABLES = 256 * 260 + 256 * 4 * (8 + 4)  # sizeof(StripeTables)


def frame_bytes(w, h, ll, layout):
    return h * ll * (2 if layout == LAYOUT_OV7670 else 1)


def line_length(w, layout):
    return 2 * w if layout == LAYOUT_YUYV else w


# ------------------------------------------------------------------ ranges

def pack_scale(v, full):
    return min(max(v * 255 // full, 0), 255)


def packed(rng):
    """WSEQ:425-445: ((hue, sat, val) from, (hue, sat, val) to, expect)."""
    hf, ht = pack_scale(rng[0], 359), pack_scale(rng[1], 359)
    sv = [pack_scale(v, 100) for v in rng[2:6]]
    if hf <= ht:
        return (hf, sv[0], sv[2]), (ht, sv[1], sv[3]), 0
    return ((ht + 1) & 255, sv[0], sv[2]), ((hf - 1) & 255, sv[1], sv[3]), 1


def hue_free(rng):
    """preview_tables' rule: the single-range table set's detect[0] is not
    kDetectFull, i.e. the range accepts all 256 hue values (detect_mode)."""
    lo, hi, expect = packed(rng)
    return all((1 if (x < lo[0] or x > hi[0]) else 0) == expect for x in range(256))


def detect_table(table, rng):
    """detectHsvPixel (WSEQ:171-179) on the table's HSV words: bool [2^24].
    Only used to find colours; what a frame's pixels detect is the oracle's
    word (oracle.frame)."""
    lo, hi, expect = packed(rng)
    hsv = (table & np.uint64(0xFFFFFFFF)).astype(np.int64)
    H, S, V = hsv & 255, (hsv >> 8) & 255, (hsv >> 16) & 255
    return ((((H < lo[0]) | (H > hi[0])) == bool(expect)) & (S >= lo[1]) & (S <= hi[1]) & (V >= lo[2]) & (V <= hi[2]))


# ------------------------------------------------- the launcher's decision

def rows2_maps(w, h, ow, oh):
    """ensure_maps: (first source row of the 2:1 row maps or -1, written
    column window [c0, c1), guide bits built)."""
    last_row, last_col = preview_ref.last_writers(w, h, ow, oh)
    rows2 = oh > 0 and ow > 0 and last_row[0] >= 0 and all(last_row[r] == last_row[0] + 2 * r for r in range(oh))
    c0, c1 = 0, ow
    while c0 < ow and last_col[c0] < 0:
        c0 += 1
    while c1 > c0 and last_col[c1 - 1] < 0:
        c1 -= 1
    rows2 = rows2 and all((last_col[c] == 2 * c + 1) if c0 <= c < c1 else last_col[c] < 0 for c in range(ow))
    return (last_row[0] if rows2 else -1), c0, c1, bool(rows2 and ow % 8 == 0)


def rows2_plan(n, ow, oh, cus):
    """launch_rows2's grid for n previews of ow x oh: (grid, step_f, step_r,
    step_q), the fewest and the most units a lane takes, and whether the last
    round is partial."""
    gpr = ow // 8
    pf = oh * gpr
    total = n * pf
    grid = min((total + 1023) // 1024, 2 * cus)
    T = grid * 1024
    return {"grid": grid, "steps": (T // pf, (T % pf) // gpr, T % gpr), "total": total, "lanes": T,
            "min_units": total // T, "max_units": -(-total // T), "partial": total % T != 0}


def advance_outcomes(n, ow, oh, cus):
    """The (q carries, r carries) outcomes of every advance() that leads to a
    stored unit, over all lanes of the grid: preview_rows2_kernel's loop walked
    with the host's steps, and checked against the unit number it stands for."""
    gpr = ow // 8
    p = rows2_plan(n, ow, oh, cus)
    sf, sr, sq = p["steps"]
    i0 = np.arange(p["lanes"], dtype=np.int64)
    f, rem = i0 // (oh * gpr), i0 % (oh * gpr)
    r, q = rem // gpr, rem % gpr
    seen, k = set(), 0
    while True:
        q2 = q + sq
        cq = q2 >= gpr
        q2 = np.where(cq, q2 - gpr, q2)
        r2 = r + sr + cq
        cr = r2 >= oh
        r2 = np.where(cr, r2 - oh, r2)
        f2 = f + sf + cr
        k += 1
        live = f2 < n
        assert np.array_equal(((f2 * oh + r2) * gpr + q2)[live], (i0 + k * p["lanes"])[live])
        if not live.any():
            return seen
        seen |= set(zip(cq[live].tolist(), cr[live].tolist()))
        f, r, q = f2, r2, q2


def gather_plan(n, oh, oll, cus):
    """launch_gather's grid: the fewest and the most 128-group chunks a wave takes."""
    total = n * oh * ((oll + 3) // 4)
    grid = min((total + 2047) // 2048, 2 * cus)
    chunks = (total + 127) // 128
    return {"grid": grid, "chunks": chunks, "min_chunks": chunks // (grid * 16), "max_chunks": -(-chunks // (grid * 16))}


def forms(w, h, ll, layout, ow, oh, oll, n, frames_offset, frame_stride, previews_offset, preview_stride,
          hue_free, cus):
    """What one trik_hsv_batch_preview call runs.  frames_offset and
    previews_offset: the pointers' distance from a 16-byte boundary."""
    first, c0, c1, guide_bits = rows2_maps(w, h, ow, oh)
    fb = frame_bytes(w, h, ll, layout)
    total = n * oh * (ow // 8)
    # launch_rows2's conditions by name: those that fail
    checks = [("maps", first >= 0), ("out_w", ow % 8 == 0), ("out_ll", oll == 2 * ow), ("width", 2 * ow <= w),
              ("frames", frames_offset % 16 == 0), ("line_length", ll % 16 == 0),
              ("frame_stride", n <= 1 or frame_stride % 16 == 0), ("previews", previews_offset % 8 == 0),
              ("preview_stride", n <= 1 or preview_stride % 8 == 0),
              ("size", total < 1 << 31 and frame_stride < 1 << 32 and preview_stride < 1 << 32 and fb < 1 << 32
               and oh * oll < 1 << 32 and ll < 1 << 24 and oll < 1 << 24 and h < 1 << 24)]
    refused = [name for name, ok in checks if not ok]
    rows2 = not refused
    out = {"hue_free": bool(hue_free), "layout": layout, "overlay_lds": 4 * (w + h) <= 32 * 1024, "refused": refused}
    if rows2:
        # launch_preview tries the rows kernel with guides wherever the guide bits
        # exist, and they exist wherever it can run (out_w % 8 == 0)
        assert guide_bits
        p = rows2_plan(n, ow, oh, cus)
        out.update(kernel="rows2", guides=True, win=c0 > 0 or c1 < ow, grid=p["grid"], steps=p["steps"],
                   min_units=p["min_units"], max_units=p["max_units"], partial=p["partial"])
        return out
    aligned4 = (frames_offset % 4 == 0 and (n <= 1 or frame_stride % 4 == 0) and ll % 4 == 0
                and previews_offset % 4 == 0 and (n <= 1 or preview_stride % 4 == 0) and oll % 4 == 0)
    p = gather_plan(n, oh, oll, cus)
    out.update(kernel="gather", guides=False, win=False, grid=p["grid"], steps=None, loads="aligned" if aligned4 else "byte",
               gather_lds=w < 65535 and h < 65535 and STRIPE_TABLES + 2 * (ow + oh) <= 80 * 1024,
               min_units=p["min_chunks"], max_units=p["max_chunks"], partial=p["chunks"] % (p["grid"] * 16) != 0)
    return out


class Case:
    """One preview call: geometry, batch placement and range."""

    def __init__(self, name, w, h, layout, ow, oh, n=1, rng=T0, ll=None, oll=None, frames_offset=0,
                 frame_pad=0, previews_offset=0, preview_pad=0, entry="batch"):
        self.name, self.w, self.h, self.layout, self.ow, self.oh, self.n, self.rng = name, w, h, layout, ow, oh, n, rng
        self.ll = line_length(w, layout) if ll is None else ll
        self.oll = 2 * ow if oll is None else oll
        self.frames_offset, self.previews_offset, self.entry = frames_offset, previews_offset, entry
        self.fb = frame_bytes(w, h, self.ll, layout)
        self.pb = oh * self.oll
        self.frame_stride, self.preview_stride = self.fb + frame_pad, self.pb + preview_pad

    def forms(self, cus):
        return forms(self.w, self.h, self.ll, self.layout, self.ow, self.oh, self.oll, self.n, self.frames_offset,
                     self.frame_stride, self.previews_offset, self.preview_stride, hue_free(self.rng), cus)

    def __repr__(self):
        return self.name


def _lay(layout):
    return "yuyv" if layout == LAYOUT_YUYV else "ov7670"


# --------------------------------------------------------- A. grid passes

GRID_SHAPE = (320, 8, 160, 4)     # 20 units per row: the grid's lanes are no multiple of a row
GRID_POW2 = (256, 8, 128, 4)      # 16 units per row: step_q == step_r == 0, the contrast
GRID_GATHER = (320, 8, 200, 5)    # not 2:1: preview_gather_kernel
ROUNDS = 3.25                     # every lane takes 3 units, some a 4th


def grid_frames(ow, oh, cus):
    """Frames that give every lane of launch_rows2's full grid ROUNDS units."""
    T, pf = 2 * cus * 1024, oh * (ow // 8)
    n = int(-(-ROUNDS * T // pf))
    return n + (1 if (n * pf) % T == 0 else 0)


def gather_frames(oh, oll, cus):
    """Frames that give every wave of launch_gather's full grid ROUNDS chunks."""
    waves, per = 2 * cus * 16, oh * ((oll + 3) // 4)
    return int(-(-ROUNDS * waves * 128 // per)) + 1


def grid_cases(cus):
    w, h, ow, oh = GRID_SHAPE
    n = grid_frames(ow, oh, cus)
    out = [Case("grid_%s_%s" % (_lay(lay), TAGS[rng]), w, h, lay, ow, oh, n, rng)
           for lay in (LAYOUT_YUYV, LAYOUT_OV7670) for rng in (T0, V_BAND)]
    pw, ph, pow_, poh = GRID_POW2
    out.append(Case("grid_pow2_yuyv_t0", pw, ph, LAYOUT_YUYV, pow_, poh, grid_frames(pow_, poh, cus), T0))
    out.append(Case("grid_line", w, h, LAYOUT_OV7670, ow, oh, n, entry="line"))
    out.append(Case("grid_blob", w, h, LAYOUT_OV7670, ow, oh, n, entry="blob"))
    gw, gh, gow, goh = GRID_GATHER
    out.append(Case("grid_gather_yuyv_t0", gw, gh, LAYOUT_YUYV, gow, goh, gather_frames(goh, 2 * gow, cus), T0))
    return out


# ------------------------------------ B. every (Y, U, V) through the preview

SAMPLED = (8192, 512, 4096, 256, 16)  # w, h, ow, oh, frames: 2^24 sampled pixels


def sampled_triples():
    """(Y, U, V) uint8 [16, 256, 4096] of the sampled-exhaustive batch: frame
    f, output pixel (r', c') holds triple number t = f << 20 | r' << 12 | c',
    scrambled so that neighbouring pixels differ in all three bytes: Y = t's
    low byte, U = its middle byte + 37 Y, V = its high byte + 91 Y + 53 U
    (mod 256), a bijection of the 2^24 triples."""
    t = np.arange(1 << 24, dtype=np.uint32).reshape(16, 256, 4096)
    Y = t & 255
    U = ((t >> 8) + 37 * Y) & 255
    V = ((t >> 16) + 91 * Y + 53 * U) & 255
    return Y.astype(np.uint8), U.astype(np.uint8), V.astype(np.uint8)


def sampled_batch(layout):
    """16 frames of 8192 x 512: triple (f, r', c') at source pixel (2 r' + 1,
    2 c' + 1), the pixel the 2:1 maps sample; the even pixel of each pair holds
    the complement luma, and every even row the complement of the odd row
    below it, so a tap on a wrong pixel or row shows."""
    w, h, ow, oh, n = SAMPLED
    Y, U, V = sampled_triples()
    if layout == LAYOUT_YUYV:
        fr = np.empty((n, oh, 2, ow, 4), np.uint8)  # frame, row pair, row, pixel pair, byte
        odd, even = fr[:, :, 1], fr[:, :, 0]
        odd[..., 0], odd[..., 1], odd[..., 2], odd[..., 3] = ~Y, U, Y, V
    else:
        fr = np.empty((n, 2, oh, 2, ow, 2), np.uint8)  # frame, plane, row pair, row, pixel pair, byte
        odd, even = fr[:, :, :, 1], fr[:, :, :, 0]
        odd[:, 0, ..., 0], odd[:, 0, ..., 1] = ~Y, Y
        odd[:, 1, ..., 0], odd[:, 1, ..., 1] = V, U
    even[...] = ~odd
    return fr.reshape(-1)


def exhaustive_cases():
    """The gather on the exhaustive frame at identity scale, the rows kernel on
    the sampled batch; in an order that builds each layout's frames once."""
    w, h, ow, oh, n = SAMPLED
    out = []
    for lay in (LAYOUT_YUYV, LAYOUT_OV7670):
        out += [Case("all_gather_%s_%s" % (_lay(lay), TAGS[rng]), 8192, 2048, lay, 8192, 2048, 1, rng)
                for rng in (T0, V_BAND)]  # (the gather has one form for every range)
        out += [Case("all_rows2_%s_%s" % (_lay(lay), TAGS[rng]), w, h, lay, ow, oh, n, rng)
                for rng in (T0, V_BAND, SV_BAND)]
    return out


def exhaustive_frame(layout):
    """gpu_util.exhaustive_yuyv_frame(), or the same pixels as ov7670 planes."""
    from gpu_util import exhaustive_yuyv_frame

    fr, w, h, ll = exhaustive_yuyv_frame()
    if layout == LAYOUT_YUYV:
        return fr
    px = fr.reshape(h, w // 2, 4)
    out = np.empty((2, h, w // 2, 2), np.uint8)
    out[0, :, :, 0], out[0, :, :, 1] = px[..., 0], px[..., 2]
    out[1, :, :, 0], out[1, :, :, 1] = px[..., 3], px[..., 1]  # V the even chroma byte, U the odd one
    return out.reshape(-1)


# ------------------------------------------------- corner-block frames

PLACES = ("tl", "tr", "bl", "br", "top", "bottom", "left", "right", "centre", "full", "one", "two")
CORNERS = ("tl", "tr", "bl", "br")


# 9 points, radius 2 around the middle pixel: a small radius, rounded up, is what lets a corner's
# circle lose output pixels to the clamp (a large rectangle's circle barely leaves the frame)
BLOCK = (3, 3)


def place(name, w, h, size=None):
    """(x0, y0, block width, block height) of a placement; `size` replaces BLOCK."""
    bw, bh = BLOCK if size is None else size
    xs = {"l": 0, "c": (w - bw) // 2 & ~1, "r": w - bw}
    ys = {"t": 0, "c": (h - bh) // 2, "b": h - bh}
    at = {"tl": "lt", "tr": "rt", "bl": "lb", "br": "rb", "top": "ct", "bottom": "cb", "left": "lc", "right": "rc",
          "centre": "cc"}
    if name in at:
        return xs[at[name][0]], ys[at[name][1]], bw, bh
    if name == "full":
        return 0, 0, w, h
    if name == "one":
        return (w // 3) | 1, h // 3, 1, 1
    assert name == "two"
    return (2 * w // 3) & ~1, 2 * h // 3, 2, 2


def _colours(table, rng):
    det = detect_table(table, rng).reshape(256, 256, 256)  # [V, U, Y]
    # a chroma pair under which some luma is detected and some is not: the
    # pixel that shares a block pixel's chroma can then stay undetected
    some, every = det.any(axis=2), det.all(axis=2)
    vv, uu = np.nonzero(some & ~every)
    k = len(vv) // 2
    V, U = int(vv[k]), int(uu[k])
    ys = np.flatnonzero(det[V, U])
    Y = int(ys[len(ys) // 2])
    Yn = int(np.flatnonzero(~det[V, U])[0])
    grey = next(y for y in (120, 20, 240, 0, 255) if not det[128, 128, y])
    return (Y, U, V), Yn, grey


_COLOURS = {}


def colours(table, rng):
    """((Y, U, V) detected under rng, a luma that is not detected with that
    chroma, a grey luma that is not detected), searched in the oracle's table
    (once per range)."""
    if rng not in _COLOURS:
        _COLOURS[rng] = _colours(table, rng)
    return _COLOURS[rng]


def pack(Y, U, V, ll, layout):
    """Luma [h, w] and per-pair chroma [h, w / 2] -> frame bytes."""
    h, w = Y.shape
    if layout == LAYOUT_YUYV:
        fr = np.zeros((h, ll), np.uint8)
        fr[:, 0:2 * w:2] = Y
        fr[:, 1:2 * w:4] = U
        fr[:, 3:2 * w:4] = V
    else:
        fr = np.zeros((2, h, ll), np.uint8)
        fr[0, :, :w] = Y
        fr[1, :, 0:w:2] = V
        fr[1, :, 1:w:2] = U
    return fr.reshape(-1)


def corner_block(table, rng, w, h, ll, layout, name, size=None):
    """A grey, undetected frame with one rectangle of a detected colour at
    placement `name`."""
    (Yc, Uc, Vc), Yn, grey = colours(table, rng)
    x0, y0, bw, bh = place(name, w, h, size)
    Y = np.full((h, w), grey, np.uint8)
    U = np.full((h, w // 2), 128, np.uint8)
    V = np.full((h, w // 2), 128, np.uint8)
    p0, p1 = x0 // 2, (x0 + bw + 1) // 2
    Y[y0:y0 + bh, 2 * p0:2 * p1] = Yn
    Y[y0:y0 + bh, x0:x0 + bw] = Yc
    U[y0:y0 + bh, p0:p1] = Uc
    V[y0:y0 + bh, p0:p1] = Vc
    return pack(Y, U, V, ll, layout)


# --------------------------------- C. the circle from the caller's sums

# (w, h, ow, oh): 2:1 with a width that is a multiple of 8 (rows kernel and its
# guides, the overlay draws the circle alone); not 2:1 (gather, the overlay
# draws both); upscaled (output pixels nobody writes)
CIRCLE_GEOMS = [(96, 64, 48, 32), (96, 64, 60, 40), (32, 16, 64, 32)]


def circle_sums(w, h):
    """[(name, (points, sum_x, sum_y))], one preview each."""
    out = []
    centres = {"tl": (0, 0), "tr": (w - 1, 0), "bl": (0, h - 1), "br": (w - 1, h - 1),
               "top": (w // 2, 0), "bottom": (w // 2, h - 1), "left": (0, h // 2), "right": (w - 1, h // 2),
               "in_tl": (1, 1), "in_tr": (w - 2, 1), "in_bl": (1, h - 2), "in_br": (w - 2, h - 2),
               "centre": (w // 2, h // 2)}
    for name, (cx, cy) in centres.items():
        out.append((name + "_r2", (4, 4 * cx, 4 * cy)))
    for name in ("tl", "centre"):
        cx, cy = centres[name]
        out.append((name + "_n1", (1, cx, cy)))
        out.append((name + "_n3", (3, 3 * cx, 3 * cy)))
    n = 3 * (h // 4) ** 2  # radius about h / 4 around a point h / 8 in from a corner: crosses two edges
    out.append(("two_edges", (n, n * (w - 1 - h // 8), n * (h // 8))))
    n = 4 * w * h
    out.append(("huge", (n, n * (w // 2), n * (h // 2))))
    out.append(("no_points", (0, 5, 5)))
    cx, cy = centres["centre"]
    out.append(("low_word_x", (4, (1 << 32) + 4 * cx, 4 * cy)))
    out.append(("low_word_y", (4, 4 * cx, (3 << 32) + 4 * cy)))
    # low words of 2^31 or more: the unsigned quotient (2^32 - 8) / 3 lies far
    # right of / below the frame, a signed one (-8 / 3) left of / above it
    out.append(("unsigned_x", (3, (1 << 32) - 8, 3 * cy)))
    out.append(("unsigned_y", (3, 3 * cx, -8)))
    return out


def circle_cases():
    return [Case("circle_%dx%d_%dx%d" % g, g[0], g[1], LAYOUT_YUYV, g[2], g[3], len(circle_sums(g[0], g[1])))
            for g in CIRCLE_GEOMS]


def process_cases():
    """(w, h, layout, ow, oh) x placement through ObjectSensor.process."""
    return [(w, h, lay, ow, oh, name) for w, h, ow, oh in CIRCLE_GEOMS for lay in (LAYOUT_YUYV, LAYOUT_OV7670)
            for name in PLACES]


# ------------------------------------------------- D. launcher branches

def overlay_memory_cases():
    """Frames with w + h > 8192 (overlay_kernel<false>), each with a 2:1 and
    another output."""
    return [Case("ovl_mem_yuyv_2to1", 8192, 32, LAYOUT_YUYV, 4096, 16, 2),
            Case("ovl_mem_yuyv_other", 8192, 32, LAYOUT_YUYV, 5120, 20, 2),
            Case("ovl_mem_ov7670_2to1", 8192, 128, LAYOUT_OV7670, 4096, 64, 2),
            Case("ovl_mem_ov7670_other", 8192, 128, LAYOUT_OV7670, 2048, 32, 2)]


def refusal_cases():
    """[(aligned twin, [one refusing condition each])] on 2:1 maps, per layout;
    a case's name ends in the name forms() gives the condition.  Six conditions
    are broken alone; out_w % 8 cannot be, and comes with the width test."""
    out = []
    for lay in (LAYOUT_YUYV, LAYOUT_OV7670):
        def c(name, ow=48, **kw):
            return Case("refuse_%s_%s" % (_lay(lay), name), 96, 64, lay, ow, 32, 3, **kw)

        ll = line_length(96, lay)
        out.append((c("twin"), [
            c("frames", frames_offset=4),
            c("line_length", ll=ll + 8),
            c("frame_stride", frame_pad=4),
            c("previews", previews_offset=4),
            c("preview_stride", preview_pad=4),
            c("out_ll", oll=2 * 48 + 4),
            # 2:1 maps (the height binds) with columns 48..51 unwritten: 52 % 8 != 0.  Never alone:
            # on a width the entry point takes, such an out_w is past w / 2 (the module docstring)
            c("out_w", ow=52),
        ]))
    return out


def byte_path_cases():
    """The gather's byte loads and stores (aligned4 == 0), one cause each."""
    out = []
    for lay in (LAYOUT_YUYV, LAYOUT_OV7670):
        for ow, oh in ((48, 32), (60, 40)):
            def c(name, **kw):
                return Case("bytes_%s_%dx%d_%s" % (_lay(lay), ow, oh, name), 96, 64, lay, ow, oh, 3, **kw)

            out += [c("frames_odd", frames_offset=1), c("previews_odd", previews_offset=1),
                    c("out_ll_odd", oll=2 * ow + 1), c("preview_stride_odd", preview_pad=1)]
    return out


def all_cases(cus):
    """Every batch_preview case of the GPU tests (the line and multi-blob twins aside)."""
    out = [c for c in grid_cases(cus) if c.entry == "batch"] + exhaustive_cases() + circle_cases()
    out += overlay_memory_cases() + byte_path_cases()
    for twin, refused in refusal_cases():
        out += [twin] + refused
    return out
