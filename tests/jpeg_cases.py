"""The input matrix of the JPEG encoder's tests, shared by tests/test_jpeg_cpu.py
(which checks that the inputs reach every path of the coder) and
tests/test_gpu_jpeg.py (which compares the GPU's bytes with tests/jpeg_ref.py on
the same inputs).  Reference results are computed once per case."""
import math

import numpy as np

import jpeg_ref

LAYOUT_OV7670 = 1

# (width, height, line_length)
SMALL = [(32, 8, 32), (64, 16, 64), (96, 24, 128), (64, 64, 64)]
MID = (320, 240, 320)
VGA = (640, 480, 640)
QUALITIES_SMALL = (0, 1, 10, 49, 50, 75, 100, 255)
QUALITIES_MID = (1, 50, 100)
# (content, quality, black and white) on VGA
VGA_CASES = (("uniform", 100, False), ("scene", 50, True))


def planes(w, h, ll, luma, chroma):
    """A frame from a luma and a chroma plane [h, w] (padding bytes zero)."""
    fr = np.zeros((2 * h, ll), np.uint8)
    fr[:h, :w] = luma
    fr[h:, :w] = chroma
    return fr.reshape(-1)


def basis_frame():
    """64 x 64: block k holds the DCT basis function whose coefficient sits at
    zigzag position k, so every zigzag position is the only non-zero AC of
    some block: runs 0..62, one to three ZRL codes, and coefficient 63."""
    nat_of_zz = [0] * 64
    for nat, z in enumerate(jpeg_ref.ZZ):
        nat_of_zz[z] = nat
    luma = np.zeros((64, 64), np.float64)
    for k in range(64):
        v, u = divmod(nat_of_zz[k], 8)
        by, bx = divmod(k, 8)
        for y in range(8):
            for x in range(8):
                luma[8 * by + y, 8 * bx + x] = 128 + 100 * math.cos((2 * x + 1) * u * math.pi / 16) * \
                    math.cos((2 * y + 1) * v * math.pi / 16)
    return planes(64, 64, 64, np.rint(luma).astype(np.uint8), np.full((64, 64), 128, np.uint8))


def contents(oracle_mod, w, h, ll):
    """name -> frame: uniform random bytes, a scene, a flat frame, all-0 and
    all-255 planes, a full-scale 1-pixel checkerboard; the basis frame at 64 x 64."""
    yy, xx = np.mgrid[0:h, 0:w]
    checker = (((xx + yy) & 1) * 255).astype(np.uint8)
    out = {
        "uniform": oracle_mod.synth(1, w, h, ll, LAYOUT_OV7670, 0, 0x51DE + w),
        "scene": oracle_mod.synth(1, w, h, ll, LAYOUT_OV7670, 1, 0x7A1C, first_frame=3),
        "flat": planes(w, h, ll, np.full((h, w), 77, np.uint8), np.full((h, w), 140, np.uint8)),
        "zeros": planes(w, h, ll, np.zeros((h, w), np.uint8), np.zeros((h, w), np.uint8)),
        "full": planes(w, h, ll, np.full((h, w), 255, np.uint8), np.full((h, w), 255, np.uint8)),
        "checker": planes(w, h, ll, checker, 255 - checker),
    }
    if (w, h, ll) == (64, 64, 64):
        out["basis"] = basis_frame()
    return {k: np.ascontiguousarray(v.reshape(-1)) for k, v in out.items()}


_FRAMES = {}
_REF = {}


def frames_of(oracle_mod, geom):
    if geom not in _FRAMES:
        _FRAMES[geom] = contents(oracle_mod, *geom)
    return _FRAMES[geom]


def ref(oracle_mod, geom, name, quality, bw):
    """jpeg_ref.encode of one case: (bytes, coeffs, entropy bits), cached."""
    key = (geom, name, quality, bool(bw))
    if key not in _REF:
        w, h, ll = geom
        _REF[key] = jpeg_ref.encode(frames_of(oracle_mod, geom)[name], w, h, ll, quality, bw)
    return _REF[key]


def small_cases():
    """Every (geometry, content, quality, bw) of the small geometries."""
    for geom in SMALL:
        names = ["uniform", "scene", "flat", "zeros", "full", "checker"] + (["basis"] if geom == (64, 64, 64) else [])
        for q in QUALITIES_SMALL:
            for bw in (False, True):
                for name in names:
                    yield geom, name, q, bw


MID_NAMES = ("uniform", "scene", "flat", "checker")


def mid_cases():
    for q in QUALITIES_MID:
        for bw in (False, True):
            for name in MID_NAMES:
                yield MID, name, q, bw
