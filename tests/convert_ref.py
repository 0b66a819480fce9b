"""The expected output of trik_hsv_convert_batch in numpy (test code, not
product): gather (Y, U, V) of every pixel of a frame of either layout, index
oracle.yuv_table(False) -- (rgb << 32) | hsv for every triple, pinned to the
reference's own compiled code by tests/test_reference_cpu.py -- and lay the
entries out in each of the call's forms with any pitches."""
import numpy as np

LAYOUT_YUYV, LAYOUT_OV7670 = 0, 1
RGB888HSV, HSV_PLANES, RGB_PLANES = 0, 1, 2


def _rows(buf, h, nbytes, ll):
    """[h, nbytes]: the first nbytes of h rows ll apart."""
    if h == 0 or nbytes == 0:
        return np.zeros((h, nbytes), np.uint8)
    assert buf.size >= (h - 1) * ll + nbytes
    return np.lib.stride_tricks.as_strided(buf, (h, nbytes), (ll, 1), writeable=False)


def gather(frame, w, h, ll, layout):
    """uint32 [h, w]: Y | U << 8 | V << 16 of every pixel (the table's index).
    Packed YUYV: chroma per word.  ov7670: the Y plane's rows, then the chroma
    plane's; V is the even chroma byte of a pair, U the odd one."""
    frame = np.ascontiguousarray(frame, dtype=np.uint8)
    if layout == LAYOUT_YUYV:
        px = _rows(frame, h, 2 * w, ll).reshape(h, w // 2, 4).astype(np.uint32)
        y = px[..., [0, 2]].reshape(h, w)
        u = np.repeat(px[..., 1], 2, axis=1)
        v = np.repeat(px[..., 3], 2, axis=1)
    else:
        y = _rows(frame, h, w, ll).astype(np.uint32)
        c = _rows(frame[h * ll:], h, w, ll).reshape(h, w // 2, 2).astype(np.uint32)
        v = np.repeat(c[..., 0], 2, axis=1)
        u = np.repeat(c[..., 1], 2, axis=1)
    return y | (u << 8) | (v << 16)


def entries(table, frames, stride, n, w, h, ll, layout):
    """uint64 [n, h, w]: the s_rgb888hsv entry of every pixel of n frames at
    frames[f * stride:]."""
    out = np.zeros((n, h, w), np.uint64)
    for f in range(n):
        out[f] = table[gather(frames[f * stride:], w, h, ll, layout)]
    return out


def planes(ent, form):
    """uint8 [n, 3, h, w] of uint64 [n, h, w]: H, S, V or R, G, B."""
    shifts = (0, 8, 16) if form == HSV_PLANES else (48, 40, 32)
    return np.stack([((ent >> np.uint64(s)) & np.uint64(0xFF)).astype(np.uint8) for s in shifts], axis=1)


def dense(ent, form):
    """The dense result: int64 [n, h, w] (the top byte is 0) or uint8 [n, 3, h, w]."""
    return ent.view(np.int64) if form == RGB888HSV else planes(ent, form)


def lay_out(ent, form, buf, offset, frame_stride, plane_stride, row_pitch):
    """Writes the entries' bytes into buf (uint8, 1-D) where the call puts
    them -- pixel (f, r, c) of form 0 at offset + f frame_stride + r row_pitch +
    8 c, little-endian; byte (f, p, r, c) of the planes at offset + f
    frame_stride + p plane_stride + r row_pitch + c -- and no other byte."""
    n, h, w = ent.shape
    if n == 0 or h == 0 or w == 0:
        return buf
    tail = buf[offset:]
    if form == RGB888HSV:
        assert tail.size >= (n - 1) * frame_stride + (h - 1) * row_pitch + 8 * w
        view = np.lib.stride_tricks.as_strided(tail, (n, h, w, 8), (frame_stride, row_pitch, 8, 1))
        view[...] = np.ascontiguousarray(ent).astype("<u8").view(np.uint8).reshape(n, h, w, 8)
    else:
        assert tail.size >= (n - 1) * frame_stride + 2 * plane_stride + (h - 1) * row_pitch + w
        view = np.lib.stride_tricks.as_strided(tail, (n, 3, h, w), (frame_stride, plane_stride, row_pitch, 1))
        view[...] = planes(ent, form)
    return buf
