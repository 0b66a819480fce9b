"""The inputs of the detection-mask tests, shared by tests/test_mask_cpu.py
(which checks on the reference output that each input reaches what it is meant
to reach) and tests/test_gpu_mask.py (which compares trik_hsv_mask_batch with
tests/mask_ref.py on the same inputs, byte for byte, padding included).

Ranges carry a label (label()): 'full' and 'empty' planes are deliberately
constant; a 'mixed' plane must hold both bit values in every row, at every bit
position 0..7 and in each of the four byte lanes of a 32-bit word, so that a
reversed bit order, a swapped lane or a dropped row shows; the narrow ranges of
the frame_ranges pool ('pool': a few percent of uniform pixels or less) make
no per-plane claim -- they are there for the packing's edges."""
import functools
from collections import namedtuple

import numpy as np

import mask_ref as MR
from convert_cases import GUARD, In, in_ll, in_size, in_stride, uniform_input  # noqa: F401
from frame_ranges_cases import (LOOP, POOL, T_COUNTS, drawn, exhaustive_yuyv, loop_frames, ov7670_twin,  # noqa: F401
                                rotated, uniform_batch)

LAYOUT_YUYV, LAYOUT_OV7670 = MR.LAYOUT_YUYV, MR.LAYOUT_OV7670
BITS, BYTES = MR.BITS, MR.BYTES
FORMS = (BITS, BYTES)
FORM_NAMES = {BITS: "bits", BYTES: "bytes"}
LAYOUT_NAMES = {LAYOUT_YUYV: "yuyv", LAYOUT_OV7670: "ov7670"}
MAX_RANGES = 64

# ---- ranges -------------------------------------------------------------------
FULL = POOL[4]
FULL_WRAP = POOL[6]                  # From == To + 1 after the scaling: the wrapped form of "every hue"
FULL_CLAMPED = (0, 360, 0, 255, 0, 255)
EMPTY_V = (0, 359, 0, 100, 60, 40)   # from > to in V
POINT = (180, 180, 50, 50, 50, 50)
HALF = (0, 180, 0, 100, 0, 100)
WRAP_HALF = (270, 90, 0, 100, 0, 100)   # hue wrap
SV_ABOVE_100 = (0, 359, 50, 200, 50, 150)  # To bounds above 100: 510 and 382 after the scaling, clamped to 255
V_ABOVE_255 = (0, 359, 0, 100, 50, 300)   # a value no InArgs byte holds: behaves as 255
FROM_EQ_TO = POOL[11]                # From == To in hue (H == 85: 8 % of uniform pixels)
WRAP_NARROW = (300, 60, 10, 90, 10, 90)


def window(k):
    """Half the hue circle from 30 k degrees on (wrapped from k = 6 on)."""
    return ((30 * k) % 360, (30 * k + 180) % 360, 0, 100, 0, 100)


_FULLS = {FULL, FULL_WRAP, FULL_CLAMPED}
_EMPTIES = {EMPTY_V}
_MIXED = {HALF, WRAP_HALF, SV_ABOVE_100, V_ABOVE_255} | {window(k) for k in range(12)}


def label(r):
    r = tuple(r)
    return "full" if r in _FULLS else "empty" if r in _EMPTIES else "mixed" if r in _MIXED else "pool"


# the exhaustive test's 16: the pool plus wrap, point, full and empty ranges
EXH_RANGES = list(POOL) + [WRAP_NARROW, POINT, FULL_CLAMPED, EMPTY_V]
# the small geometries' and the placements' five
SMALL_RANGES = [HALF, WRAP_HALF, window(3), FULL, EMPTY_V]
# range edges, one at a time (T = 1) and all together
EDGE_RANGES = [FULL, POINT, WRAP_HALF, WRAP_NARROW, FROM_EQ_TO, FULL_WRAP, SV_ABOVE_100, V_ABOVE_255, EMPTY_V,
               (65535, 65535, 65535, 65535, 65535, 65535), (0, 0, 0, 65535, 0, 65535)]
COLUMN_RANGE = (0, 359, 0, 100, 0, 30)  # the dark column of a bright floor


def t_sets(n_frames, t):
    """t ranges per frame, another rotation per frame.  t < 3: hue windows
    (frame f: window(f), window(f + 1)).  Otherwise the rotation by f of one
    mixed window, the empty range, the full one, then the pool cycled with the
    value bound shifted per cycle (frame_ranges_cases.t_ranges' rule), so that
    no two of a frame's ranges are equal."""
    if t < 3:
        return [[window((f + k) % 12) for k in range(t)] for f in range(n_frames)]
    base = [HALF, EMPTY_V, FULL]
    for k in range(t - 3):
        hf, ht, sf, st, vf, vt = POOL[k % len(POOL)]
        base.append((hf, ht, sf, st, vf + 3 * (k // len(POOL) + 1), vt))
    assert len(set(base)) == t
    return [[base[(f + k) % t] for k in range(t)] for f in range(n_frames)]


T_VALUES = (1, 3, 4, 5, 8, 9, 64)
assert set(T_COUNTS) <= set(T_VALUES)  # the sums call's group boundaries, and 3
T_IN = {LAYOUT_YUYV: In(LAYOUT_YUYV, 96, 8, 5), LAYOUT_OV7670: In(LAYOUT_OV7670, 96, 8, 5)}
PAD_RANGE = FULL  # what the tuples between two frames' sets hold: read by mistake, it fills a plane


# ---- output placement -----------------------------------------------------------
# Out: row_pitch = the row's bytes + row_pad, plane_stride = a plane + plane_pad,
# frame_stride = T planes + frame_pad, `out` at byte GUARD + off of a 16-byte
# aligned buffer that ends GUARD bytes after frame n - 1's stride.
Out = namedtuple("Out", "form row_pad plane_pad frame_pad off", defaults=(0, 0, 0, 0))


def row_bytes(form, w):
    return w // 8 if form == BITS else w


def out_geometry(o, w, h, n, t):
    """(offset of `out`, frame_stride, plane_stride, row_pitch, buffer bytes)"""
    row_pitch = row_bytes(o.form, w) + o.row_pad
    plane_stride = h * row_pitch + o.plane_pad
    frame_stride = t * plane_stride + o.frame_pad
    return GUARD + o.off, frame_stride, plane_stride, row_pitch, GUARD + o.off + n * frame_stride + GUARD


def form(i, o, t):
    """'vec' or 'generic': the launcher's predicate (mask_vec_ok) restated.  The
    vector kernel takes a call whose every 16-byte load address is 16-byte
    aligned (the base, line_length, and frame_stride when there is more than
    one frame) and whose every store address is a multiple of the store's
    width, 4 bytes for the bits and 8 for the bytes: `out`, row_pitch,
    plane_stride when there is more than one range and frame_stride when there
    is more than one frame."""
    _, frame_stride, plane_stride, row_pitch, _ = out_geometry(o, i.w, i.h, i.n, t)
    load = i.off | in_ll(i) | (in_stride(i) if i.n > 1 else 0)
    store = o.off | row_pitch | (plane_stride if t > 1 else 0) | (frame_stride if i.n > 1 else 0)
    return "vec" if load % 16 == 0 and store % (4 if o.form == BITS else 8) == 0 else "generic"


def sentinel(size):
    """The pattern an output buffer holds before the call (convert_cases.sentinel's:
    period 251, so no alignment of the output repeats it; never 0x00 or 0xFF)."""
    return np.resize((np.arange(251) + 3).astype(np.uint8), size)


def expected(oracle_mod, table, buf, i, ranges, o):
    """(the whole output buffer after the call, offset of `out`, frame_stride,
    plane_stride, row_pitch, the planes bool [n, T, h, w]): sentinel() with the
    mask's bytes laid over it; frame f under ranges[f]."""
    t = len(ranges[0])
    off, frame_stride, plane_stride, row_pitch, size = out_geometry(o, i.w, i.h, i.n, t)
    det = MR.planes(oracle_mod, table, buf[i.off:], in_stride(i), i.n, i.w, i.h, in_ll(i), i.layout, ranges)
    want = MR.lay_out(det, o.form, sentinel(size), off, frame_stride, plane_stride, row_pitch)
    return want, off, frame_stride, plane_stride, row_pitch, det


def ranges_buffer(ranges, stride=None, pad=PAD_RANGE):
    """int16 (uint16 bits) [n * stride] with frame f's tuples at f * stride;
    the elements between two sets hold `pad` repeated.  stride None: 6 T."""
    n, t = len(ranges), len(ranges[0])
    stride = 6 * t if stride is None else stride
    assert stride >= 6 * t
    fill = np.resize(np.array(pad, np.int64), stride)
    buf = np.tile(fill, n).reshape(n, stride)
    buf[:, :6 * t] = np.array(ranges, np.int64).reshape(n, 6 * t)
    return (buf.reshape(-1) & 0xFFFF).astype(np.uint16).view(np.int16)


def check_plane(det, lab, what):
    """The label's claim on one plane (bool [h, w])."""
    if lab == "full":
        assert det.all(), what
    elif lab == "empty":
        assert not det.any(), what
    elif lab == "mixed":
        h, w = det.shape
        assert det.any(axis=1).all() and not det.all(axis=1).any(), (what, "a constant row")
        for p in range(8):
            col = det[:, p::8]
            assert col.any() and not col.all(), (what, "bit position", p)
        lanes = det.reshape(h, w // 32, 4, 8)
        for k in range(4):
            lane = lanes[:, :, k, :]
            assert lane.any() and not lane.all(), (what, "byte lane", k)


def check_planes(det, ranges, what):
    for f in range(det.shape[0]):
        for t, r in enumerate(ranges[f]):
            check_plane(det[f, t], label(r), (what, f, t, r))


def case_id(i, o):
    return (f"{LAYOUT_NAMES[i.layout]}-{i.w}x{i.h}x{i.n}-p{i.pad}s{i.stride_pad}o{i.off}-"
            f"{FORM_NAMES[o.form]}-r{o.row_pad}p{o.plane_pad}f{o.frame_pad}o{o.off}")


# ---- 1. all 2^24 (Y, U, V): 64 frames of 8192 x 32 -------------------------------
EXH = dict(w=8192, h=32, n=64)


@functools.lru_cache(maxsize=None)
def exhaustive_frames(layout):
    w, h, n = EXH["w"], EXH["h"], EXH["n"]
    host = exhaustive_yuyv()
    if layout == LAYOUT_OV7670:
        fb = h * 2 * w
        host = np.concatenate([ov7670_twin(host[f * fb:(f + 1) * fb], w, h) for f in range(n)])
    host.setflags(write=False)
    return host


def exhaustive_ranges():
    """Frame f: the 16 ranges rotated by f, so every triple meets every range
    and every plane index holds every range."""
    return [[EXH_RANGES[(f + k) % len(EXH_RANGES)] for k in range(len(EXH_RANGES))] for f in range(EXH["n"])]


# (layout, form, input base offset, row_pad): the vector kernel, then the
# generic one reached by the input's base and by the output's pitch
EXHAUSTIVE = [(layout, f, in_off, row_pad) for layout in (LAYOUT_YUYV, LAYOUT_OV7670) for f in FORMS
              for in_off, row_pad in ((0, 0), (1, 0) if (layout == LAYOUT_YUYV) == (f == BITS) else (0, 1))]


def exhaustive_case(layout, f, in_off, row_pad):
    return In(layout, EXH["w"], EXH["h"], EXH["n"], off=in_off), Out(f, row_pad=row_pad)


# ---- 2. smallest geometries ---------------------------------------------------------
def small_inputs(layout):
    return [
        In(layout, 32, 4, 1), In(layout, 32, 4, 3), In(layout, 32, 4, 300),  # one word per row, one quad; 16 units per frame
        In(layout, 64, 4, 2), In(layout, 32, 8, 2),
        In(layout, 96, 8, 3),      # 12 units per row: no power of two, a wave spans rows
        In(layout, 544, 4, 2),     # 68 units per row: no multiple of a wave's 64
        In(layout, 2080, 4, 2),    # 1040 units per frame: a second run of 16 units
        In(layout, 64, 8, 3, pad=16), In(layout, 64, 8, 3, pad=4),
        In(layout, 64, 8, 3, stride_pad=33),  # frame_stride larger than a frame and odd
        In(layout, 64, 8, 1, stride_pad=33),  # (a single frame's stride is no address)
        In(layout, 64, 8, 2, off=1), In(layout, 64, 8, 2, off=4),
        In(layout, 640, 52, 1),    # 4160 units: more than one run of the frame (4 x 1024, then 64)
    ]


def small_ranges(i):
    """Every frame the same five, rotated by the frame."""
    return [[SMALL_RANGES[(f + k) % 5] for k in range(5)] for f in range(i.n)]


# ---- 5. output placement --------------------------------------------------------------
def pitch_outs(f):
    """Padding in rows, planes and frames, each alone and together, aligned to
    the store (multiples of 8) and not; then a misaligned `out` alone."""
    return [Out(f), Out(f, row_pad=4), Out(f, row_pad=8), Out(f, row_pad=1), Out(f, plane_pad=8), Out(f, plane_pad=4),
            Out(f, plane_pad=3), Out(f, frame_pad=16), Out(f, frame_pad=4), Out(f, frame_pad=5),
            Out(f, row_pad=8, plane_pad=16, frame_pad=24), Out(f, row_pad=3, plane_pad=7, frame_pad=9, off=5),
            Out(f, off=1), Out(f, off=4), Out(f, off=8)]


PITCH_IN = {LAYOUT_YUYV: In(LAYOUT_YUYV, 96, 8, 3), LAYOUT_OV7670: In(LAYOUT_OV7670, 96, 8, 3)}


# ---- 6. one-hot columns ------------------------------------------------------------------
COLUMN_WIDTHS = (32, 64, 544)
COLUMN_H = 4


def one_hot_columns(width, layout):
    """width frames of width x 4 (tests/line_cases.py's construction): frame c
    is the bright floor (Y 200, grey chroma) with column c dark (Y 20) in all
    rows."""
    from line_cases import floor

    h = COLUMN_H
    buf = np.tile(floor(width, h), width).reshape(width, 2 * h, width)
    for c in range(width):
        buf[c, :h, c] = 20
    if layout == LAYOUT_OV7670:
        return buf.reshape(-1)
    yuyv = np.full((width, h, width // 2, 4), 128, np.uint8)
    yuyv[..., 0] = buf[:, :h, 0::2]
    yuyv[..., 2] = buf[:, :h, 1::2]
    return yuyv.reshape(-1)


def one_hot_planes(width):
    """bool [width, 1, 4, width]: plane c holds column c alone."""
    det = np.zeros((width, 1, COLUMN_H, width), bool)
    for c in range(width):
        det[c, 0, :, c] = True
    return det
