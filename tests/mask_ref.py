"""The expected output of trik_hsv_mask_batch in numpy (test code, not
product): H, S, V of every pixel from oracle.yuv_table(False) -- pinned to the
reference's own compiled code by tests/test_reference_cpu.py -- computed once
per pixel, then per range the reference's detectHsvPixel (WSEQ:171-179) under
oracle.pack_range's packed form, laid out as bit planes or byte planes at any
strides.  tests/test_mask_cpu.py holds it to oracle.frame(..., want_mask=True)
bit for bit."""
import numpy as np

import convert_ref as CR

LAYOUT_YUYV, LAYOUT_OV7670 = CR.LAYOUT_YUYV, CR.LAYOUT_OV7670
BITS, BYTES = 0, 1


def as_inargs(r):
    """The six numbers as InArgs bytes hold them for oracle.pack_range: a
    saturation or value above 255 behaves as 255 (every bound is clamped to 255
    after the scaling, and 255 already scales past it)."""
    return (r[0], r[1]) + tuple(min(int(v), 255) for v in r[2:6])


def hsv_of(table, frames, stride, n, w, h, ll, layout):
    """(H, S, V), each uint8 [n, h, w], of n frames at frames[f * stride:]."""
    hsv = np.zeros((n, h, w), np.uint32)
    for f in range(n):
        hsv[f] = table[CR.gather(frames[f * stride:], w, h, ll, layout)] & np.uint64(0xFFFFFF)
    return (hsv & 0xFF).astype(np.uint8), ((hsv >> 8) & 0xFF).astype(np.uint8), (hsv >> 16).astype(np.uint8)


def detect(oracle_mod, H, S, V, r):
    """detectHsvPixel on arrays: bit k of `out` is set where byte k of the pixel
    lies outside byte k of the packed bounds; detected where out == expect."""
    lo, hi, expect = oracle_mod.pack_range(as_inargs(r))
    out = ((H < (lo & 0xFF)) | (H > (hi & 0xFF))).astype(np.uint8)
    out |= ((S < ((lo >> 8) & 0xFF)) | (S > ((hi >> 8) & 0xFF))).astype(np.uint8) << 1
    out |= ((V < ((lo >> 16) & 0xFF)) | (V > ((hi >> 16) & 0xFF))).astype(np.uint8) << 2
    return out == expect


def planes(oracle_mod, table, frames, stride, n, w, h, ll, layout, ranges):
    """bool [n, T, h, w]: plane (f, t) is frame f under ranges[f][t]."""
    H, S, V = hsv_of(table, frames, stride, n, w, h, ll, layout)
    T = len(ranges[0]) if n else 0
    det = np.zeros((n, T, h, w), bool)
    for f in range(n):
        assert len(ranges[f]) == T
        for t, r in enumerate(ranges[f]):
            det[f, t] = detect(oracle_mod, H[f], S[f], V[f], r)
    return det


def dense(det, form):
    """uint8 [n, T, h, w // 8] (pixel c = bit c & 7 of byte c >> 3, least
    significant first) or [n, T, h, w] (0xFF / 0x00)."""
    if form == BITS:
        return np.packbits(det, axis=-1, bitorder="little")
    return det.astype(np.uint8) * np.uint8(0xFF)


def lay_out(det, form, buf, offset, frame_stride, plane_stride, row_pitch):
    """Writes the mask's bytes into buf (uint8, 1-D) where the call puts them
    -- byte b of row r of plane t of frame f at offset + f frame_stride + t
    plane_stride + r row_pitch + b -- and no other byte."""
    n, T, h, w = det.shape
    if n == 0 or T == 0 or h == 0 or w == 0:
        return buf
    img = dense(det, form)
    rb = img.shape[-1]
    tail = buf[offset:]
    assert tail.size >= (n - 1) * frame_stride + (T - 1) * plane_stride + (h - 1) * row_pitch + rb
    view = np.lib.stride_tricks.as_strided(tail, (n, T, h, rb), (frame_stride, plane_stride, row_pitch, 1))
    view[...] = img
    return buf
