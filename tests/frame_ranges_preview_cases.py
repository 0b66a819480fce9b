"""The inputs of the per-frame-range preview tests and the launcher's decision
for each, shared by tests/test_frame_ranges_preview_cpu.py (which asserts every
coverage claim on the restated decision and on the reference's own output) and
tests/test_gpu_frame_ranges_preview.py (which runs the inputs through
trik_hsv_frame_ranges_preview on the GPU).

plan() restates launch_frame_ranges_preview
(trik-media-sensors-dsp_amd/csrc/trik_hsv_frame_ranges_preview.hip): the 2:1
kernel under preview_cases.forms()'s conditions (the predicate it shares with
launch_rows2), the gather otherwise (the line sensors' launcher in the same
file: line_frame_ranges_preview_cases.forms()).  In both a wave takes tasks of 64 lanes
of ONE frame -- 64 units of 8 output pixels, or 128 four-byte output groups --
round robin over the grid's waves; a frame is ceil(per_frame / per task) tasks,
the last of them with idle lanes.

The expectation everywhere is expected(): preview_ref.body over
oracle.frame(frame f, range f)'s mask (a bound above 255 enters the oracle's
byte fields as 255), then preview_ref.preview with the slot's sums.  Where the
sums are the frame's own and the range fits the reference's InArgs, that is
oracle.run(frame f, range f)'s preview (the CPU test holds the two together);
the grid-pass and closed-loop tests use oracle.run for their thousands of
frames.
"""
import functools
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import frame_ranges_cases as FC
import preview_cases as pc
import preview_ref
from preview_ref import LAYOUT_OV7670, LAYOUT_YUYV

POOL = FC.POOL
# disjoint hue sectors: a colour one of them detects, the others do not (the
# pool's fourth range wraps through hue 0 into the first one's sector, so the
# fourth sector here is another)
SECTORS = POOL[:3] + [(290, 340, 30, 100, 30, 100)]
# the pool and four more: a sector between the pool's, a saturation band, a dark
# sector, a band of every hue
SIXTEEN = POOL + [(40, 80, 0, 100, 0, 100), (150, 200, 10, 60, 40, 90), (270, 330, 50, 100, 10, 100),
                  (0, 359, 30, 70, 30, 70)]
BLOCK, WAVES, BLOCKS_PER_CU, GATHER_Q = 256, 4, 8, 2
MAP_LDS_BYTES = 32 * 1024
ROUNDS = pc.ROUNDS
WORKERS = 16


# ------------------------------------------------- the launcher's decision

def plan(w, h, ll, layout, ow, oh, oll, n, frames_offset, frame_stride, previews_offset, preview_stride, cus):
    """What one trik_hsv_frame_ranges_preview call runs: kernel, grid (in
    workgroups of 4 waves), tasks per frame, lanes of a frame's last task that
    hold no unit, and the fewest and the most tasks a wave takes."""
    f = pc.forms(w, h, ll, layout, ow, oh, oll, n, frames_offset, frame_stride, previews_offset, preview_stride,
                 False, cus)
    rows2 = f["kernel"] == "rows2"
    assert not (rows2 and (f["win"] or not f["guides"]))  # launch_frame_ranges_preview would take the gather
    per_row = ow // 8 if rows2 else (oll + 3) // 4
    per_task = 64 if rows2 else 64 * GATHER_Q
    per_frame = oh * per_row
    segs = -(-per_frame // per_task)
    tasks = n * segs
    grid = min(-(-tasks // WAVES), BLOCKS_PER_CU * cus)
    waves = grid * WAVES
    out = {"kernel": f["kernel"], "layout": layout, "refused": f["refused"], "overlay_lds": f["overlay_lds"],
           "guides": rows2, "grid": grid, "waves": waves, "segs": segs, "tasks": tasks,
           "idle": segs * per_task - per_frame, "min_tasks": tasks // waves, "max_tasks": -(-tasks // waves),
           "partial": tasks % waves != 0, "frames_per_wave": -(-tasks // waves) / segs}
    if not rows2:
        out.update(loads=f["loads"], maps_lds=w < 65535 and h < 65535 and 2 * (ow + oh) <= MAP_LDS_BYTES)
    return out


def plan_of(c, cus):
    return plan(c.w, c.h, c.ll, c.layout, c.ow, c.oh, c.oll, c.n, c.frames_offset, c.frame_stride, c.previews_offset,
                c.preview_stride, cus)


# ------------------------------------------------------------ expectation

def clamp255(rng):
    """The six numbers as the oracle's Range takes them: saturation and value
    above 255 behave as 255 (pack_scale clamps after the scaling); a hue fits
    its uint16 field as it is."""
    return (int(rng[0]) & 0xFFFF, int(rng[1]) & 0xFFFF) + tuple(min(int(v) & 0xFFFF, 255) for v in rng[2:6])


def threaded(fn, n):
    """[fn(f) for f in range(n)], the frames split among threads (the oracle's
    calls and numpy's indexing release the GIL)."""
    if n < 8:
        return [fn(f) for f in range(n)]
    parts = [range(i * n // WORKERS, (i + 1) * n // WORKERS) for i in range(WORKERS)]
    with ThreadPoolExecutor(WORKERS) as ex:
        return [r for part in ex.map(lambda rg: [fn(f) for f in rg], parts) for r in part]


def frame_of(host, c, f):
    return host[f * c.frame_stride:f * c.frame_stride + c.fb]


def own_sums(oracle_mod, host, c, ranges):
    """int64 [n, 3]: oracle.frame's sums of frame f under ranges[f]."""
    return np.stack(threaded(lambda f: oracle_mod.frame(frame_of(host, c, f), c.w, c.h, c.ll, c.layout,
                                                        [clamp255(ranges[f])])[0][0], c.n))


def expected(oracle_mod, table, host, c, ranges, sums):
    """uint8 [n, oh * oll]: preview f is the body of frame f under ranges[f]
    (oracle.frame's mask), the guide lines, and the circle of sums[f]."""
    def one(f):
        fr = frame_of(host, c, f)
        _, mask = oracle_mod.frame(fr, c.w, c.h, c.ll, c.layout, [clamp255(ranges[f])], want_mask=True)
        body = preview_ref.body(table, mask, fr, c.w, c.h, c.ll, c.layout, c.ow, c.oh, c.oll)
        return preview_ref.preview(body, c.w, c.h, c.ow, c.oh, c.oll, sums[f]).reshape(-1)

    return np.stack(threaded(one, c.n))


def oracle_previews(oracle_mod, host, c, ranges):
    """uint8 [n, oh * oll]: oracle.run(frame f, ranges[f])'s preview (its own sums)."""
    def one(f):
        rc, _, pv = oracle_mod.run(frame_of(host, c, f), c.w, c.h, c.ll, c.layout, ranges[f], out_width=c.ow,
                                   out_height=c.oh, out_line_length=c.oll)
        assert rc == 0
        return pv

    return np.stack(threaded(one, c.n))


# ------------------------------------------ a. the range follows the frame

def follow_cases():
    """Small frames, many of them: a frame is one task of few live lanes, so a
    wave walks frame after frame and must change its range with each."""
    return [pc.Case("follow_yuyv_32x4", 32, 4, LAYOUT_YUYV, 16, 2, 300),
            pc.Case("follow_ov7670_96x8", 96, 8, LAYOUT_OV7670, 48, 4, 64),
            pc.Case("follow_gather_32x4", 32, 4, LAYOUT_YUYV, 20, 3, 300),
            pc.Case("follow_gather_ov7670_96x8", 96, 8, LAYOUT_OV7670, 60, 5, 64)]


def follow_ranges(n):
    return [SECTORS[f % len(SECTORS)] for f in range(n)]


def follow_frames(table, c):
    """Frame f: pixel pair p of row r holds the colour sector (p + r + f) % 4
    detects (both pixels), so every sampled row holds all four colours; its
    own range paints one of them, a neighbour's range another."""
    cols = [pc.colours(table, rng)[0] for rng in SECTORS]
    Yc, Uc, Vc = (np.array([col[k] for col in cols], np.uint8) for k in range(3))
    p, r = np.arange(c.w // 2)[None, :], np.arange(c.h)[:, None]
    out = np.zeros(c.n * c.fb, np.uint8)
    for f in range(c.n):
        k = (p + r + f) % len(SECTORS)
        out[f * c.fb:(f + 1) * c.fb] = pc.pack(np.repeat(Yc[k], 2, axis=1), Uc[k], Vc[k], c.ll, c.layout)
    return out


# ------------------------------------------------------- b. grid passes

def grid_frames(w, h, ow, oh, layout, cus):
    """Frames that give every wave of the full grid ROUNDS tasks: at least
    three rounds each, a fourth for some."""
    ll = pc.line_length(w, layout)
    fb, pb = pc.frame_bytes(w, h, ll, layout), oh * 2 * ow
    segs = plan(w, h, ll, layout, ow, oh, 2 * ow, 1, 0, fb, 0, pb, cus)["segs"]
    waves = BLOCKS_PER_CU * cus * WAVES
    n = int(-(-ROUNDS * waves // segs))
    return n + (1 if (n * segs) % waves == 0 else 0)


def grid_cases(cus):
    out = []
    for kind, (w, h, ow, oh) in (("rows2", pc.GRID_SHAPE), ("gather", pc.GRID_GATHER)):
        for lay in (LAYOUT_YUYV, LAYOUT_OV7670):
            out.append(pc.Case("grid_%s_%s" % (kind, pc._lay(lay)), w, h, lay, ow, oh, grid_frames(w, h, ow, oh, lay, cus)))
    return out


def pool_ranges(n, shift=0):
    return [POOL[(f + shift) % len(POOL)] for f in range(n)]


# ------------------------------------------------ c. every (Y, U, V)

def exhaustive_cases():
    """The sampled batch through the 2:1 kernel, the exhaustive frame as 16
    frames of 8192 x 128 at identity scale through the gather."""
    w, h, ow, oh, n = pc.SAMPLED
    out = []
    for lay in (LAYOUT_YUYV, LAYOUT_OV7670):
        out.append(pc.Case("all_rows2_%s" % pc._lay(lay), w, h, lay, ow, oh, n))
        out.append(pc.Case("all_gather_%s" % pc._lay(lay), 8192, 128, lay, 8192, 128, 16))
    return out


def exhaustive_batch(layout):
    """preview_cases.exhaustive_frame cut into 16 frames of 128 rows (ov7670:
    each frame its own luma rows, then its own chroma rows)."""
    fr = pc.exhaustive_frame(layout)
    if layout == LAYOUT_YUYV:
        return fr
    return np.ascontiguousarray(fr.reshape(2, 16, -1).transpose(1, 0, 2)).reshape(-1)


def sixteen_ranges(shift):
    return [SIXTEEN[(f + shift) % 16] for f in range(16)]


# ------------------------------------------------------- d. the slot

SLOT_T, SLOT_t = 3, 1
SLOT_OTHERS = (POOL[4], POOL[10])  # entries 0 and 2: every pixel, the dark ones
OTHER_SUMS = (9, 9 * 3, 9 * 3)     # a circle of radius 2 around (3, 3)


# ------------------------------------- e. against the shared-range call

def equal_cases():
    """12 scene frames, 12 ranges: the 2:1 kernel with a gap between previews,
    the gather with line padding and a gap."""
    return [pc.Case("equal_rows2_yuyv", 96, 64, LAYOUT_YUYV, 48, 32, 12, preview_pad=16),
            pc.Case("equal_rows2_ov7670", 96, 64, LAYOUT_OV7670, 48, 32, 12, preview_pad=16),
            pc.Case("equal_pad_yuyv", 96, 64, LAYOUT_YUYV, 48, 32, 12, oll=2 * 48 + 12, preview_pad=20),
            pc.Case("equal_pad_ov7670", 96, 64, LAYOUT_OV7670, 60, 40, 12, oll=2 * 60 + 8, preview_pad=8)]


# ---------------------------------------------------------- f. placement

def placement_cases():
    """preview_cases' refusals (with their aligned twins) and byte paths, and a
    gather whose maps are too large for LDS."""
    out = []
    for twin, refused in pc.refusal_cases():
        out += [twin] + refused
    out += pc.byte_path_cases()
    out += [pc.Case("maps_mem_yuyv", 16416, 4, LAYOUT_YUYV, 16416, 4, 2),
            pc.Case("maps_mem_ov7670", 16416, 4, LAYOUT_OV7670, 16416, 4, 2)]
    return out


SEED = 0x51A9


def scene_frames(oracle_mod, c, first_frame=5):
    return oracle_mod.synth(c.n, c.w, c.h, c.ll, c.layout, 1, SEED, first_frame=first_frame, frame_stride=c.frame_stride)


# ---------------------------------------------------------- h. closed loop

def loop_case():
    v = FC.LOOP
    return pc.Case("loop", v["w"], v["h"], LAYOUT_YUYV, v["w"] // 2, v["h"] // 2, v["n"])


@functools.lru_cache(maxsize=None)
def loop_ranges(oracle_mod):
    return [FC.blob_range_of(d) for d in FC.loop_detect(oracle_mod)]


def all_cases(cus):
    return follow_cases() + grid_cases(cus) + exhaustive_cases() + pc.circle_cases() + equal_cases() + \
        placement_cases() + [loop_case()]
