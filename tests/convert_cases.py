"""The inputs of the colour-conversion tests, shared by
tests/test_convert_cpu.py (which checks on the reference output that each
input reaches what it is meant to reach) and tests/test_gpu_convert.py (which
compares trik_hsv_convert_batch with tests/convert_ref.py on the same inputs,
byte for byte, padding included)."""
import functools
from collections import namedtuple

import numpy as np

import convert_ref as CR
from frame_ranges_cases import exhaustive_yuyv, ov7670_twin

LAYOUT_YUYV, LAYOUT_OV7670 = CR.LAYOUT_YUYV, CR.LAYOUT_OV7670
RGB888HSV, HSV_PLANES, RGB_PLANES = CR.RGB888HSV, CR.HSV_PLANES, CR.RGB_PLANES
FORMS = (RGB888HSV, HSV_PLANES, RGB_PLANES)
FORM_NAMES = {RGB888HSV: "rgb888hsv", HSV_PLANES: "hsv-planes", RGB_PLANES: "rgb-planes"}
LAYOUT_NAMES = {LAYOUT_YUYV: "yuyv", LAYOUT_OV7670: "ov7670"}

GUARD = 64  # sentinel bytes kept before `out` and after the last frame


def row_bytes(w, layout):
    return 2 * w if layout == LAYOUT_YUYV else w


def frame_bytes(w, h, ll, layout):
    return h * ll * (2 if layout == LAYOUT_OV7670 else 1)


# ---- input and output placement ---------------------------------------------
# In: n frames of w x h; line_length = row bytes + pad, frame_stride = frame
# bytes + stride_pad, frame 0 at byte `off` of a 16-byte aligned buffer.
In = namedtuple("In", "layout w h n pad stride_pad off", defaults=(0, 0, 0))


def in_ll(i):
    return row_bytes(i.w, i.layout) + i.pad


def in_stride(i):
    return frame_bytes(i.w, i.h, in_ll(i), i.layout) + i.stride_pad


def in_size(i):
    return i.off + i.n * in_stride(i)


# Out: row_pitch = the row's bytes + row_pad, plane_stride = a plane + plane_pad,
# frame_stride = a frame's output + frame_pad, `out` at byte GUARD + off of a
# 16-byte aligned buffer (GUARD is a multiple of 16) that ends GUARD bytes after
# frame n - 1's stride.
Out = namedtuple("Out", "form row_pad plane_pad frame_pad off", defaults=(0, 0, 0, 0))


def out_geometry(o, w, h, n):
    """(offset of `out`, frame_stride, plane_stride, row_pitch, buffer bytes)"""
    row_pitch = (8 * w if o.form == RGB888HSV else w) + o.row_pad
    image = h * row_pitch
    plane_stride = 0 if o.form == RGB888HSV else image + o.plane_pad
    frame_stride = 2 * plane_stride + image + o.frame_pad
    return GUARD + o.off, frame_stride, plane_stride, row_pitch, GUARD + o.off + n * frame_stride + GUARD


def form(i, o):
    """'vec' or 'generic': the launcher's predicate (convert_vec_ok) restated.
    The vector kernel takes a call whose every load and store address is
    16-byte aligned: the bases, line_length, row_pitch, plane_stride for the
    planes, and both frame strides when there is more than one frame."""
    _, frame_stride, plane_stride, row_pitch, _ = out_geometry(o, i.w, i.h, i.n)
    bits = i.off | in_ll(i) | o.off | row_pitch
    if i.n > 1:
        bits |= in_stride(i) | frame_stride
    if o.form != RGB888HSV:
        bits |= plane_stride
    return "vec" if bits % 16 == 0 else "generic"


def sentinel(size):
    """The pattern an output buffer holds before the call (period 251: no
    alignment of the output repeats it)."""
    return (np.arange(size, dtype=np.uint32) % 251 + 3).astype(np.uint8)


def uniform_input(i, seed):
    """The input buffer: uniform random bytes, padding included."""
    return np.random.default_rng(seed).integers(0, 256, in_size(i), dtype=np.uint8)


def expected(table, buf, i, o):
    """(the whole output buffer after the call, offset of `out`, frame_stride,
    plane_stride, row_pitch): sentinel() with the pixels' bytes laid over it."""
    off, frame_stride, plane_stride, row_pitch, size = out_geometry(o, i.w, i.h, i.n)
    ent = CR.entries(table, buf[i.off:], in_stride(i), i.n, i.w, i.h, in_ll(i), i.layout)
    want = CR.lay_out(ent, o.form, sentinel(size), off, frame_stride, plane_stride, row_pitch)
    return want, off, frame_stride, plane_stride, row_pitch


# ---- 1. all 2^24 (Y, U, V): 64 frames of 8192 x 32 ---------------------------
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


# (layout, form, input base offset, row_pad): the vector kernel on each form,
# then form 0 and HSV_PLANES through the generic kernel, reached by the input's
# base or by the output's pitch
EXHAUSTIVE = [(layout, f, 0, 0) for layout in (LAYOUT_YUYV, LAYOUT_OV7670) for f in FORMS] + [
    (LAYOUT_YUYV, RGB888HSV, 1, 0), (LAYOUT_OV7670, RGB888HSV, 0, 8),
    (LAYOUT_YUYV, HSV_PLANES, 0, 4), (LAYOUT_OV7670, HSV_PLANES, 1, 0)]


def exhaustive_case(layout, f, in_off, row_pad):
    return In(layout, EXH["w"], EXH["h"], EXH["n"], off=in_off), Out(f, row_pad=row_pad)


# ---- 2. smallest geometries -------------------------------------------------
# (w, h, n, pad, stride_pad, off) per layout; pads in bytes on top of the row
def small_inputs(layout):
    big, small = 16, 4  # line_length 2W+16 / 2W+4 (W+16 / W+4 for ov7670)
    return [
        In(layout, 32, 4, 1), In(layout, 32, 4, 2), In(layout, 32, 4, 3),  # fewer than one wave's units
        In(layout, 64, 4, 2), In(layout, 32, 8, 2),
        In(layout, 96, 20, 3),       # 240 / 120 units per frame: no multiple of a workgroup, waves cross rows
        In(layout, 640, 8, 2),       # 80 units per row: a wave's 64 cross a row end mid-wave
        In(layout, 64, 8, 3, pad=big), In(layout, 64, 8, 3, pad=small),
        In(layout, 64, 8, 3, stride_pad=33),  # frame_stride larger than a frame and odd
        In(layout, 64, 8, 1, stride_pad=33),  # (a single frame's stride is no address)
        In(layout, 64, 8, 2, off=1), In(layout, 64, 8, 2, off=8),
    ]


# ---- 3. output layout ---------------------------------------------------------
def pitch_outs(f):
    """Padding in rows, planes and frames, each alone and together, aligned
    (multiples of 16) and not; then a misaligned `out` alone."""
    outs = [Out(f, row_pad=16), Out(f, frame_pad=48), Out(f, row_pad=32, frame_pad=16),
            Out(f, row_pad=8), Out(f, frame_pad=8), Out(f, row_pad=3, frame_pad=5, off=1), Out(f, off=8), Out(f, off=3)]
    if f != RGB888HSV:
        outs += [Out(f, plane_pad=32), Out(f, row_pad=16, plane_pad=16, frame_pad=16), Out(f, plane_pad=8),
                 Out(f, row_pad=1, plane_pad=7, frame_pad=9, off=5)]
    return outs


PITCH_IN = {LAYOUT_YUYV: In(LAYOUT_YUYV, 96, 8, 3), LAYOUT_OV7670: In(LAYOUT_OV7670, 96, 8, 3)}


def case_id(i, o):
    return (f"{LAYOUT_NAMES[i.layout]}-{i.w}x{i.h}x{i.n}-p{i.pad}s{i.stride_pad}o{i.off}-"
            f"{FORM_NAMES[o.form]}-r{o.row_pad}p{o.plane_pad}f{o.frame_pad}o{o.off}")
