"""A plain reference of the ov7670 line sensor's sums and OutArgs (LSEQ =
trik/ov7670/line_sensor/include/internal/cv_line_detector_seqpass.hpp), in
numpy over the oracle's per-pixel table (oracle.yuv_table: index
Y | U<<8 | V<<16, the HSV word in the low half, its V byte in bits 16-23).
It keeps the detection map, so a test forms the sums of many bands from one
pass and can ask what a frame reaches (tests/line_cases.py); it keeps sum_x
exact where the reference's int32 wraps; and it has no restriction on the
geometry.  Test code: tests/test_line_cpu.py holds it to oracle.line_run."""
import numpy as np

M32 = 0xFFFFFFFF


def scale_val(v):
    """A percent bound as the byte LSEQ:397-414 compares V with."""
    return min(255, max(0, (int(v) * 255) // 100))


def default_band(height):
    """The band the detector leaves behind for its next run (LSEQ:449-450)."""
    return (height // 2, height // 2 + 80)


def detect(table, frame, width, height, line_length, val_from, val_to):
    """bool [height, 2 * (width // 2)]: the pixels whose V lies in the scaled
    range and whose column lies in the window 5 <= col <= width - 5 (LSEQ:288).
    Planes: luma, then chroma with V at even and U at odd bytes (LSEQ:211-234);
    a trailing odd column belongs to no pixel pair and is never read."""
    fr = np.asarray(frame, np.uint8)
    pairs = width // 2
    y = fr[:height * line_length].reshape(height, line_length)[:, :2 * pairs].astype(np.int64)
    c = fr[height * line_length:2 * height * line_length].reshape(height, line_length)[:, :2 * pairs]
    v = np.repeat(c[:, 0::2].astype(np.int64), 2, axis=1)
    u = np.repeat(c[:, 1::2].astype(np.int64), 2, axis=1)
    val = (table[y | (u << 8) | (v << 16)] >> np.uint64(16)).astype(np.int64) & 255
    cols = np.arange(2 * pairs)
    win = (cols >= 5) & (cols <= width - 5)
    return (val >= scale_val(val_from)) & (val <= scale_val(val_to)) & win[None, :]


def band_rows(height, band):
    """bool [height]: (uint32)row in [(uint32)band[0], (uint32)band[1]] (LSEQ:298)."""
    rows = np.arange(height, dtype=np.int64)
    return (rows >= (int(band[0]) & M32)) & (rows <= (int(band[1]) & M32))


def sums_of(det, band):
    """[points, sum_x, cross] of a detect() map, exact Python ints."""
    row_n = det.sum(axis=1, dtype=np.int64)
    col_n = det.sum(axis=0, dtype=np.int64)  # (the column sum stays far below 2^63 at any testable size)
    sum_x = int((col_n * np.arange(det.shape[1], dtype=np.int64)).sum())
    return [int(row_n.sum()), sum_x, int(row_n[band_rows(det.shape[0], band)].sum())]


def sums(table, frame, width, height, line_length, val_from, val_to, band=None):
    """[points, sum_x, cross points] of one frame as exact Python ints (the
    reference keeps sum_x in an int32; targets() takes its low word)."""
    det = detect(table, frame, width, height, line_length, val_from, val_to)
    return sums_of(det, default_band(height) if band is None else band)


def _s8(v):
    return ((v & 0xFF) ^ 0x80) - 0x80


def _s32(v):
    return ((v & M32) ^ 0x80000000) - 0x80000000


def _cdiv(a, b):
    """C's integer division (towards zero), b > 0."""
    return -((-a) // b) if a < 0 else a // b


def center(points, sum_x):
    """The target line's column (LSEQ:464): the uint32 quotient as an int32."""
    return _s32((sum_x & M32) // (points & M32))


def targets(points, sum_x, cross, width, height):
    """(targetX, targetY, targetSize) with the reference's widths
    (LSEQ:455-474): uint32 points and cross points, an int32 column sum, int8
    targetX and targetY, uint8 targetSize; all 0 unless points > 10."""
    n = points & M32
    if n <= 10:
        return (0, 0, 0)
    cx = center(points, sum_x)
    x = _s8(_cdiv(_s32((cx - width // 2) * 100 * 2), width))
    y = _s8((((cross & M32) * 100) & M32) // (width * 2 * 40))
    size = (((n * 100) & M32) // (height * width)) & 0xFF
    return (x, y, size)
