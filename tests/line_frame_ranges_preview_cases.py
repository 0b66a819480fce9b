"""The inputs of the line sensors' per-frame-range preview tests and the
launcher's decision for each, shared by
tests/test_line_frame_ranges_preview_cpu.py (which asserts every coverage claim
on the restated decision and on the reference's own output) and
tests/test_gpu_line_frame_ranges_preview.py (which runs the inputs through
trik_hsv_line_frame_ranges_preview on the GPU).

forms() restates line_frame_ranges_preview_core and
launch_line_frame_ranges_preview
(trik-media-sensors-dsp_amd/csrc/trik_hsv_frame_ranges_preview.hip):
ensure_maps with the layout's column window (ov7670: source columns 5..W-5),
then the 2:1 kernel where the windowed maps are the 2:1 ones, the overlay maps
are monotone (ovl_ok) and preview_rows2_ok's conditions hold -- its WIN form
when the window leaves output columns unwritten -- and the gather otherwise.
In both a wave takes tasks of 64 lanes of ONE frame, round robin over the
grid's waves (frame_ranges_preview_cases.plan's numbers).

The expectation everywhere is line_preview_ref.previews: frame f under
pairs[f] = (val_from, val_to) with the target line of sums[f].
"""
import numpy as np

import frame_ranges_preview_cases as FP
import line_frame_ranges_cases as LC
import line_preview_ref as LR
import preview_cases as pc
import preview_ref
from preview_ref import LAYOUT_OV7670, LAYOUT_YUYV

BLOCK, WAVES, BLOCKS_PER_CU, GATHER_Q, MAP_LDS_BYTES = FP.BLOCK, FP.WAVES, FP.BLOCKS_PER_CU, FP.GATHER_Q, FP.MAP_LDS_BYTES
ROUNDS = pc.ROUNDS
LAYOUTS = (LAYOUT_YUYV, LAYOUT_OV7670)
Case = pc.Case


# ------------------------------------------------- the launcher's decision

def rows2_maps(w, h, ow, oh, layout):
    """ensure_maps on the windowed maps: (first source row of the 2:1 row maps
    or -1, written column window [c0, c1))."""
    last_row, last_col = LR.last_writers(w, h, ow, oh, layout)
    rows2 = oh > 0 and ow > 0 and last_row[0] >= 0 and all(last_row[r] == last_row[0] + 2 * r for r in range(oh))
    c0, c1 = 0, ow
    while c0 < ow and last_col[c0] < 0:
        c0 += 1
    while c1 > c0 and last_col[c1 - 1] < 0:
        c1 -= 1
    rows2 = rows2 and all((last_col[c] == 2 * c + 1) if c0 <= c < c1 else last_col[c] < 0 for c in range(ow))
    return (last_row[0] if rows2 else -1), c0, c1


def ovl_ok(w, h, ow, oh):
    """ensure_maps' maps_ovl_ok: the column map rises in steps of 0 or 1."""
    if w <= 0 or h <= 0:
        return False
    wi2wo, _ = preview_ref.maps(w, h, ow, oh)
    return all(0 <= wi2wo[c] - wi2wo[c - 1] <= 1 for c in range(1, w))


def forms(w, h, ll, layout, ow, oh, oll, n, frames_offset, frame_stride, previews_offset, preview_stride, cus):
    """What one trik_hsv_line_frame_ranges_preview call runs.  frames_offset and
    previews_offset: the pointers' distance from a 16-byte boundary."""
    first, c0, c1 = rows2_maps(w, h, ow, oh, layout)
    fb = pc.frame_bytes(w, h, ll, layout)
    total = n * oh * (ow // 8)
    # preview_rows2_ok's conditions by name (preview_cases.forms), and ovl_ok: those that fail
    checks = [("ovl", ovl_ok(w, h, ow, oh)), ("maps", first >= 0), ("out_w", ow % 8 == 0), ("out_ll", oll == 2 * ow),
              ("width", 2 * ow <= w), ("frames", frames_offset % 16 == 0), ("line_length", ll % 16 == 0),
              ("frame_stride", n <= 1 or frame_stride % 16 == 0), ("previews", previews_offset % 8 == 0),
              ("preview_stride", n <= 1 or preview_stride % 8 == 0),
              ("size", total < 1 << 31 and frame_stride < 1 << 32 and preview_stride < 1 << 32 and fb < 1 << 32
               and oh * oll < 1 << 32 and ll < 1 << 24 and oll < 1 << 24 and h < 1 << 24)]
    refused = [name for name, ok in checks if not ok]
    rows2 = not refused
    per_row = ow // 8 if rows2 else (oll + 3) // 4
    per_task = 64 if rows2 else 64 * GATHER_Q
    per_frame = oh * per_row
    segs = -(-per_frame // per_task)
    tasks = n * segs
    grid = min(-(-tasks // WAVES), BLOCKS_PER_CU * cus)
    waves = grid * WAVES
    out = {"kernel": "rows2" if rows2 else "gather", "layout": layout, "refused": refused, "grid": grid, "waves": waves,
           "segs": segs, "tasks": tasks, "idle": segs * per_task - per_frame, "min_tasks": tasks // waves,
           "max_tasks": -(-tasks // waves), "partial": tasks % waves != 0}
    if rows2:
        out.update(win=c0 > 0 or c1 < ow, window=(c0, c1))
    else:
        aligned4 = (frames_offset % 4 == 0 and (n <= 1 or frame_stride % 4 == 0) and ll % 4 == 0
                    and previews_offset % 4 == 0 and (n <= 1 or preview_stride % 4 == 0) and oll % 4 == 0)
        out.update(loads="aligned" if aligned4 else "byte",
                   maps_lds=w < 65535 and h < 65535 and 2 * (ow + oh) <= MAP_LDS_BYTES)
    return out


def forms_of(c, cus):
    return forms(c.w, c.h, c.ll, c.layout, c.ow, c.oh, c.oll, c.n, c.frames_offset, c.frame_stride, c.previews_offset,
                 c.preview_stride, cus)


# ------------------------------------------------------------------ inputs

def frames2d(host, c):
    """uint8 [n, frame bytes]: the frames of a batch laid out as the case says."""
    host = np.asarray(host, np.uint8)
    return np.lib.stride_tricks.as_strided(host, (c.n, c.fb), (c.frame_stride, 1), writeable=False)


def noise_frames(c, seed):
    """c.n frames of uniform luma and near-grey chroma (so V spreads over the
    whole byte), random bytes in the line padding and between frames."""
    rng = np.random.default_rng(seed)
    host = rng.integers(0, 256, (c.n - 1) * c.frame_stride + c.fb, dtype=np.uint8)
    Y = rng.integers(0, 256, (c.n, c.h, c.w), dtype=np.uint8)
    U, V = (rng.integers(100, 156, (c.n, c.h, c.w // 2), dtype=np.uint8) for _ in range(2))
    fr = rng.integers(0, 256, (c.n, c.fb), dtype=np.uint8)
    if c.layout == LAYOUT_YUYV:
        img = fr.reshape(c.n, c.h, c.ll)
        img[:, :, 0:2 * c.w:2], img[:, :, 1:2 * c.w:4], img[:, :, 3:2 * c.w:4] = Y, U, V
    else:
        img = fr.reshape(c.n, 2, c.h, c.ll)
        img[:, 0, :, :c.w], img[:, 1, :, 0:c.w:2], img[:, 1, :, 1:c.w:2] = Y, V, U
    for f in range(c.n):
        host[f * c.frame_stride:f * c.frame_stride + c.fb] = fr[f]
    return host


def scene_frames(oracle_mod, c, seed=70):
    """c.n line scenes of the layout's sensor (a dark slanted line on a bright
    floor), each with its own position and slope."""
    scene = oracle_mod.line_scene if c.layout == LAYOUT_OV7670 else oracle_mod.wline_scene
    host = np.zeros((c.n - 1) * c.frame_stride + c.fb, np.uint8)
    for f in range(c.n):
        host[f * c.frame_stride:f * c.frame_stride + c.fb] = scene(
            c.w, c.h, c.ll, seed + f, x0=c.w // 5 + (c.w // 2) * f // max(1, c.n - 1), slope=0.1 * (f - 1))
    return host


def own_sums(oracle_mod, table, host, c, pairs):
    """int64 [n, 3]: the sums trik_hsv_line_frame_ranges_batch gives frame f
    under pairs[f] (line_ref / oracle.frame, line_frame_ranges_cases)."""
    frames = list(frames2d(host, c))
    if c.layout == LAYOUT_OV7670:
        s, _ = LC.expected_ov7670(table, frames, c.w, c.h, c.ll, pairs)
    else:
        s, _ = LC.expected_yuyv(oracle_mod, frames, c.w, c.h, c.ll, [tuple(min(v, 255) for v in p) for p in pairs])
    return np.asarray(s, np.int64).reshape(c.n, 3)


def expected(table, host, c, pairs, sums, smp=None):
    """uint8 [n, oh * oll] (line_preview_ref.previews)."""
    return LR.previews(table, frames2d(host, c), c.w, c.h, c.ll, c.layout, c.ow, c.oh, c.oll, pairs, sums, smp)


def six(pairs):
    """[n, 6] uint16: entries 4 and 5 from the pairs; entries 0..3 hold numbers
    that would matter if they were read (a hue wrap, a narrow saturation)."""
    a = LC.six(pairs)
    a[:, 0:4] = (300, 20, 90, 95)
    return a


# ------------------------------------------ a. the range follows the frame

EMPTY = LC.EMPTY
ABOVE_100 = (45, 300)  # scaled 114..255
# neighbours differ in every rotation; one empty range, one with a bound above 100
PAIRS = [(0, 35), (30, 65), (60, 100), EMPTY, ABOVE_100, (10, 55), (50, 90)]


def follow_pairs(n, shift=0):
    return [PAIRS[(f + shift) % len(PAIRS)] for f in range(n)]


def follow_cases():
    """Small frames, many of them: with fewer than 64 units a frame a wave walks
    frame after frame and must change its bounds and its target line with each."""
    out = []
    for lay in LAYOUTS:
        out += [Case("follow_rows2_%s_32x8" % pc._lay(lay), 32, 8, lay, 16, 4, 130),
                Case("follow_rows2_%s_96x12" % pc._lay(lay), 96, 12, lay, 48, 6, 23),
                Case("follow_gather_%s_32x8" % pc._lay(lay), 32, 8, lay, 10, 3, 130, oll=2 * 10 + 4),
                Case("follow_gather_%s_64x16" % pc._lay(lay), 64, 16, lay, 24, 5, 23, oll=2 * 24 + 12)]
    return out


# ------------------------------------------------------- b. grid passes

GRID_ROWS2 = (32, 8, 16, 4)
GRID_GATHER = (32, 8, 10, 3)


def grid_frames(w, h, ow, oh, layout, cus):
    """Frames that give every wave of the full grid ROUNDS tasks: at least
    three rounds each, a fourth for some."""
    ll = pc.line_length(w, layout)
    fb, pb = pc.frame_bytes(w, h, ll, layout), oh * 2 * ow
    segs = forms(w, h, ll, layout, ow, oh, 2 * ow, 1, 0, fb, 0, pb, cus)["segs"]
    waves = BLOCKS_PER_CU * cus * WAVES
    n = int(-(-ROUNDS * waves // segs))
    return n + (1 if (n * segs) % waves == 0 else 0)


def grid_cases(cus):
    out = []
    for kind, (w, h, ow, oh) in (("rows2", GRID_ROWS2), ("gather", GRID_GATHER)):
        for lay in LAYOUTS:
            out.append(Case("grid_%s_%s" % (kind, pc._lay(lay)), w, h, lay, ow, oh, grid_frames(w, h, ow, oh, lay, cus)))
    return out


# ------------------------------------------------ c. every (Y, U, V)

# 64 V ranges, 16 a pass over the 16 frames: line_frame_ranges_cases' 64 (0..100,
# from == to at 0, 50 and 100, an empty one) with the narrowest empty range and
# a bound above 100 in place of its last two.  A scaled from of exactly to + 1
# does not exist: consecutive percent values lie 2 or 3 bytes apart and all
# values past 100 give 255 (the CPU test checks every uint16), so the narrowest
# empty range is from = to + 1 in percent.
NARROWEST_EMPTY = (51, 50)  # bytes 130 > 127
EXHAUSTIVE_PAIRS = LC.EXHAUSTIVE_PAIRS[:62] + [NARROWEST_EMPTY, ABOVE_100]
PASSES = 4


def exhaustive_pairs(p):
    return EXHAUSTIVE_PAIRS[16 * p:16 * p + 16]


def exhaustive_cases():
    """The sampled batch through the 2:1 kernel, the exhaustive frame as 16
    frames of 8192 x 128 at identity scale through the gather."""
    w, h, ow, oh, n = pc.SAMPLED
    out = []
    for lay in LAYOUTS:
        out.append(Case("all_rows2_%s" % pc._lay(lay), w, h, lay, ow, oh, n))
        out.append(Case("all_gather_%s" % pc._lay(lay), 8192, 128, lay, 8192, 128, 16))
    return out


def exhaustive_host(c):
    return FP.exhaustive_batch(c.layout) if "gather" in c.name else pc.sampled_batch(c.layout)


# ------------------------------- d. the target line from the caller's sums

# (w, h, ow, oh): at 32 wide the four thin lines (W/2 -+ 40, -+ 80) clamp to the edges
TARGET_GEOMS = [(32, 8, 16, 4), (32, 8, 10, 3), (320, 240, 160, 120), (320, 240, 100, 75)]


def target_sums(w):
    """[(name, (points, sum_x, sum_y))], one preview each."""
    out = [("cx_%d" % cx, (11, 11 * cx, 5)) for cx in (0, 1, w // 2, w - 2, w - 1)]
    out += [("points_10", (10, 10 * (w // 4), 0)), ("points_11", (11, 11 * (w // 4), 0)), ("no_points", (0, 77, 0)),
            # the high words must not count: points 11 (not 5 * 2^32 + 11), cx = w / 4 + 3
            ("high_words", ((5 << 32) + 11, (3 << 32) + 11 * (w // 4 + 3), 9 << 32)),
            ("high_points_only", ((1 << 32) + 3, 3 * (w // 2), 0)),      # low word 3: no line
            ("past_the_frame", (11, 11 * (w + 50), 0)),                   # cx - 1 .. cx + 1 all clamp to W - 1
            ("unsigned_x", (11, (1 << 32) - 8, 0))]                       # the low word read unsigned: far right
    return out


def target_cases():
    out = []
    for w, h, ow, oh in TARGET_GEOMS:
        for lay in LAYOUTS:
            out.append(Case("target_%s_%dx%d_%dx%d" % (pc._lay(lay), w, h, ow, oh), w, h, lay, ow, oh,
                            len(target_sums(w))))
    return out


# ------------------------------------- e. against the existing calls

def equal_cases():
    """Scene frames: ov7670 against single-frame trik_hsv_line_preview calls,
    YUYV against WebcamLineSensor.process (240 x 320: the webcam glue's default
    output, not 2:1)."""
    return [Case("equal_ov7670_320x240", 320, 240, LAYOUT_OV7670, 160, 120, 4),
            Case("equal_ov7670_640x480", 640, 480, LAYOUT_OV7670, 320, 240, 3),
            Case("equal_yuyv_320x240", 320, 240, LAYOUT_YUYV, 160, 120, 4),
            Case("equal_yuyv_640x480", 640, 480, LAYOUT_YUYV, 240, 320, 3)]


EQUAL_PAIRS = [(0, 30), (0, 45), EMPTY, (20, 100)]


# ---------------------------------------------------------- f. placement

def placement_cases():
    """preview_cases' refusals of the 2:1 form one condition at a time (with
    their aligned twins) and its byte paths, and what they leave out: an odd
    frame_stride, previews misaligned by 2, a gap between the 2:1 kernel's
    previews."""
    out = []
    for twin, refused in pc.refusal_cases():
        out += [twin] + refused
    out += pc.byte_path_cases()
    for lay in LAYOUTS:
        def c(name, **kw):
            return Case("extra_%s_%s" % (pc._lay(lay), name), 96, 64, lay, 48, 32, 3, **kw)

        out += [c("frame_stride_odd", frame_pad=3), c("previews_2", previews_offset=2), c("gap", preview_pad=24)]
    return out


def all_cases(cus):
    return follow_cases() + grid_cases(cus) + exhaustive_cases() + target_cases() + equal_cases() + placement_cases()
