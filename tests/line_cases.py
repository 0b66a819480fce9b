"""The inputs of the line sensor's shape tests, shared by
tests/test_line_cpu.py (which checks on tests/line_ref.py that each input
reaches what it is meant to reach) and tests/test_gpu_line_shapes.py (which
compares the GPU with tests/line_ref.py on the same inputs).  Every coverage
condition is a function of the reference's own output."""
import functools

import numpy as np

import line_ref

# the two V ranges of the noise frames: uniform bytes detect 28 % of the pixels
# in the first and 85 % in the second
RANGES = ((0, 70), (50, 100))

# (w, h, frames) of the shape tests, line_length = w, with line_geom's
# (cu, rpi, block, segs x seg_rows) for each (csrc/trik_hsv_line.hip)
# (trik_hsv_line_batch takes what the reference's setup() takes: w % 32 == 0
# and h % 4 == 0.  So 68 units, 544 columns, is the narrowest frame whose
# workgroup has idle lanes: below it some rpi <= 16 makes rpi x cu a multiple
# of 64.)
SHAPES = [
    (64, 36, 1),      # 8, 8, 64, 1 x 40: 5 iterations (one unrolled group + one tail row), the last
                      #   taken by the row offsets 0..3 only
    (64, 100, 1),     # 8, 8, 64, 2 x 56: the second segment holds 44 rows
    (64, 100, 7),     # the same
    (64, 100, 1024),  # 8, 8, 64, 1 x 104: frames >= 1024 force one segment, 13 iterations
    (544, 36, 1),     # 68, 15, 1024, 1 x 45: 1020 of 1024 lanes, seg_rows > height, 3 iterations, the
                      #   last taken by the row offsets 0..5
    (544, 52, 2),     # 68, 15, 1024, 1 x 60: 15 does not divide 52, 4 iterations
    (1088, 20, 1),    # 136, 7, 960, 1 x 21: 952 of 960 lanes
    (8224, 40, 3),    # 1024 (2 chunks, the second of 4 units), 1, 1024, 5 x 8
    (64, 4, 1),       # 8, 8, 64, 1 x 8: the row offsets 4..7 start past the last row
    (32, 4, 1),       # 4, 16, 64, 1 x 16: the offsets 4..15 do
    (32, 8, 1),       # 4, 16, 64, 1 x 16: the offsets 8..15 do
]

# the one-hot column batches: w frames of w x 8
#   32: 4, 16, 64, 1 x 16;  64: 8, 8, 64, 1 x 8;  544: 68, 15, 1024, 1 x 15
COLUMN_WIDTHS = (32, 64, 544)
COLUMN_RANGE = (0, 30)

# the generic kernel (line_sums_kernel), h = 20: three row groups of 8, the
# last of 4 rows.  (w, ll, frames, frame stride - frame bytes, base offset)
# (A width that is no multiple of 8 never reaches it: the entry point refuses
# it.)
GENERIC = [
    (64, 64, 1, 0, 1),    # base pointer 1 past a 16-byte boundary
    (64, 64, 1, 0, 4),    # base pointer 4 past a 16-byte boundary
    (64, 64, 3, 3, 0),    # frame_stride = 2 h ll + 3
    (64, 68, 2, 0, 0),    # line_length = w + 4
    (32, 36, 2, 0, 0),
    (96, 100, 2, 0, 0),
]
GENERIC_H = 20


def bands(height):
    """The bands run on every shape: the default (None), the first row, the
    last row, the last row with the largest stop, a start of 0xFFFFFFFF (empty),
    a stop of 0xFFFFFFFF (rows 3 to the end), start > stop (empty)."""
    h = height
    return [None, (0, 0), (h - 1, h - 1), (h - 1, 2**31 - 1), (-1, 5), (3, -1), (5, 2)]


def _salt(y, c, width, height, shift):
    """Plants black (Y 16) and white (Y 235) pixels with grey chroma, which the
    two RANGES detect in opposite ways (black: V = 0, white: V = 253): one of
    each in every row and in every column of the window.  Position i is row
    i % h, window column (i + shift) % n for black and the next one for white."""
    n = width - 9  # window columns 5 .. width - 5
    assert n >= 2 and height >= 2
    i = np.arange(max(height, n))
    rows = i % height
    cb, cw = 5 + (i + shift) % n, 5 + (i + shift + 1) % n
    assert not np.intersect1d(rows * width + cb, rows * width + cw).size
    for col, lum in ((cb, 16), (cw, 235)):
        y[rows, col] = lum
        c[rows, col & ~1] = 128
        c[rows, col | 1] = 128


def noise(width, height, line_length, n_frames, seed, frame_stride=None):
    """n_frames frames of uniform random bytes, the row and frame padding
    included, with _salt's few planted pixels.  Pure noise cannot hold the
    condition check_noise() asserts at every shape: at 85 % detections some of
    the 8215 window columns of 40 rows are detected throughout."""
    fb = 2 * height * line_length
    stride = fb if frame_stride is None else frame_stride
    rng = np.random.default_rng(seed)
    buf = rng.integers(0, 256, n_frames * stride, dtype=np.uint8)
    for f in range(n_frames):
        fr = buf[f * stride:f * stride + fb]
        _salt(fr[:fb // 2].reshape(height, line_length), fr[fb // 2:].reshape(height, line_length),
              width, height, 3 * f)
    return buf


def check_noise(table, buf, width, height, line_length, n_frames, frame_stride=None):
    """At both RANGES, inside the window: every row of every frame holds a
    detection and a non-detection, and so does every column.  No two frames
    are equal."""
    fb = 2 * height * line_length
    stride = fb if frame_stride is None else frame_stride
    frames = [buf[f * stride:f * stride + fb] for f in range(n_frames)]
    assert len({fr.tobytes() for fr in frames}) == n_frames
    for vf, vt in RANGES:
        for f, fr in enumerate(frames):
            win = line_ref.detect(table, fr, width, height, line_length, vf, vt)[:, 5:width - 4]
            for axis in (0, 1):
                assert win.any(axis=axis).all() and (~win).any(axis=axis).all(), (width, height, f, vf, vt, axis)


@functools.lru_cache(maxsize=None)
def _shape_noise(width, height):
    n = max(n for w, h, n in SHAPES if (w, h) == (width, height))
    buf = noise(width, height, width, n, 1000 * width + height)
    buf.setflags(write=False)
    return buf


def shape_noise(width, height, n_frames):
    """The first n_frames frames of the shape's noise batch (one batch per
    (w, h): the 1024-frame call reads the frames the 7-frame call reads)."""
    return _shape_noise(width, height)[:n_frames * 2 * height * width]


def generic_noise(case):
    """(buffer, offset of frame 0 in it, frame stride) of a GENERIC case; the
    caller places the buffer on a 16-byte boundary."""
    w, ll, n, pad, off = case
    stride = 2 * GENERIC_H * ll + pad
    buf = np.random.default_rng(77 * w + ll + pad + off).integers(0, 256, off + n * stride, dtype=np.uint8)
    buf[off:] = noise(w, GENERIC_H, ll, n, 5 * w + ll + pad + off, frame_stride=stride)
    return buf, off, stride


def floor(width, height, line_length=None):
    """A bright floor (Y 200, grey chroma): no detection below V = 212."""
    ll = width if line_length is None else line_length
    fr = np.full(2 * height * ll, 128, np.uint8)
    fr[:height * ll] = 200
    return fr


def one_hot_columns(width):
    """width frames of width x 8: frame c is the floor with column c dark
    (Y 20) in all rows."""
    h = 8
    buf = np.tile(floor(width, h), width).reshape(width, 2 * h, width)
    for c in range(width):
        buf[c, :h, c] = 20
    return buf.reshape(-1)


def one_hot_expected(width):
    """[points, sum_x, cross] of each frame at COLUMN_RANGE and the default
    band (rows 4..7 of 8): column c's 8 pixels if it lies in the window."""
    return [[8, 8 * c, 4] if 5 <= c <= width - 5 else [0, 0, 0] for c in range(width)]


def dark_pixels(width, height, count, line_length=None):
    """The floor with `count` dark pixels (Y 20) inside the window, spread over
    the rows and columns."""
    ll = width if line_length is None else line_length
    fr = floor(width, height, ll)
    y = fr[:ll * height].reshape(height, ll)
    n = width - 9
    for i in range(count):
        y[(3 * i) % height, 5 + (7 * i) % n] = 20
    return fr
