"""A restatement of the ov7670 JPEG encoder (trik/ov7670/jpeg_encoder, JENC =
include/internal/jpeg_encoder_reference.hpp) as the GPU tests' reference.

The transform runs over all data units at once in numpy float64 (numpy neither
fuses nor reorders: every multiply and add is rounded on its own, as on the
C674x); the symbol loop and the bit writer are the sequential loops they are in
the reference.  The four Huffman tables and the two quantiser tables are
retyped from ITU-T T.81 Annex K.
"""
import numpy as np

# T.81 Annex K.1: luminance and chrominance quantisers, natural order
Q_LUM = [16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55,
         14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
         18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
         49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99]
Q_CHR = [17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99,
         24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32


def _zigzag_of_natural():
    """zz[natural index] = position in the zigzag scan (T.81 figure A.6)."""
    zz = [0] * 64
    r = c = 0
    for k in range(64):
        zz[8 * r + c] = k
        if (r + c) % 2 == 0:  # moving up-right
            if c == 7:
                r += 1
            elif r == 0:
                c += 1
            else:
                r -= 1
                c += 1
        else:  # moving down-left
            if r == 7:
                c += 1
            elif c == 0:
                r += 1
            else:
                r += 1
                c -= 1
    return zz


ZZ = _zigzag_of_natural()


def _span(lo, hi):
    return list(range(lo, hi + 1))


# T.81 Annex K.3: BITS (codes of each length 1..16) and HUFFVAL
DC_LUM_BITS = [0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0]
DC_CHR_BITS = [0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0]
DC_VALS = list(range(12))
AC_LUM_BITS = [0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7D]
AC_LUM_VALS = ([0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07,
                0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xA1, 0x08, 0x23, 0x42, 0xB1, 0xC1, 0x15, 0x52, 0xD1, 0xF0,
                0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0A, 0x16, 0x17, 0x18, 0x19, 0x1A]
               + _span(0x25, 0x2A) + _span(0x34, 0x3A) + _span(0x43, 0x4A) + _span(0x53, 0x5A)
               + _span(0x63, 0x6A) + _span(0x73, 0x7A) + _span(0x83, 0x8A) + _span(0x92, 0x9A)
               + _span(0xA2, 0xAA) + _span(0xB2, 0xBA) + _span(0xC2, 0xCA) + _span(0xD2, 0xDA)
               + _span(0xE1, 0xEA) + _span(0xF1, 0xFA))
AC_CHR_BITS = [0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77]
AC_CHR_VALS = ([0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71,
                0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xA1, 0xB1, 0xC1, 0x09, 0x23, 0x33, 0x52, 0xF0,
                0x15, 0x62, 0x72, 0xD1, 0x0A, 0x16, 0x24, 0x34, 0xE1, 0x25, 0xF1, 0x17, 0x18, 0x19, 0x1A]
               + _span(0x26, 0x2A) + _span(0x35, 0x3A) + _span(0x43, 0x4A) + _span(0x53, 0x5A)
               + _span(0x63, 0x6A) + _span(0x73, 0x7A) + _span(0x82, 0x8A) + _span(0x92, 0x9A)
               + _span(0xA2, 0xAA) + _span(0xB2, 0xBA) + _span(0xC2, 0xCA) + _span(0xD2, 0xDA)
               + _span(0xE2, 0xEA) + _span(0xF2, 0xFA))
assert len(AC_LUM_VALS) == 162 == sum(AC_LUM_BITS) and len(AC_CHR_VALS) == 162 == sum(AC_CHR_BITS)

# the eight AAN scale factors as the reference's decimal literals (JENC:207-210)
AASF = [1.0, 1.387039845, 1.306562965, 1.175875602, 1.0, 0.785694958, 0.541196100, 0.275899379]


def _huff(bits, vals, size):
    """(code, length) per symbol; an undefined symbol has length 0 (JENC:286-307)."""
    code = [0] * size
    length = [0] * size
    v = 0
    p = 0
    for k in range(1, 17):
        for _ in range(bits[k - 1]):
            code[vals[p]] = v
            length[vals[p]] = k
            p += 1
            v += 1
        v *= 2
    return code, length


HT_DC = (_huff(DC_LUM_BITS, DC_VALS, 12), _huff(DC_CHR_BITS, DC_VALS, 12))
HT_AC = (_huff(AC_LUM_BITS, AC_LUM_VALS, 256), _huff(AC_CHR_BITS, AC_CHR_VALS, 256))


def quant_tables(quality):
    """(luminance, chrominance) quantisers in natural order (JENC:244-267, 771-791)."""
    q = min(max(int(quality), 1), 100)
    sf = 5000 // q if q < 50 else 200 - 2 * q
    return tuple([min(max((v * sf + 50) // 100, 1), 255) for v in t] for t in (Q_LUM, Q_CHR))


def divisors(qt):
    """fdtbl of JENC:268-278: 1 / (q * aasf[row] * aasf[col] * 8), left to right."""
    return np.array([1.0 / (float(qt[8 * r + c]) * AASF[r] * AASF[c] * 8.0) for r in range(8) for c in range(8)],
                    dtype=np.float64)


def header(quality, bw, width, height):
    """SOI, APP0, DQT, SOF0, DHT, SOS (JENC:517-647, 811-817)."""
    ql, qc = quant_tables(quality)
    o = bytearray()

    def word(v):
        o.extend(((v >> 8) & 0xFF, v & 0xFF))

    def in_zigzag(t):
        z = [0] * 64
        for i in range(64):
            z[ZZ[i]] = t[i]
        return z

    word(0xFFD8)
    word(0xFFE0); word(16); o.extend(b"JFIF\0"); o.extend((1, 1, 0)); word(1); word(1); o.extend((0, 0))
    word(0xFFDB); word(67 if bw else 132)
    o.append(0); o.extend(in_zigzag(ql))
    if not bw:
        o.append(1); o.extend(in_zigzag(qc))
    word(0xFFC0); word(11 if bw else 17); o.append(8); word(height); word(width)
    o.append(1 if bw else 3)
    o.extend((1, 0x11, 0))
    if not bw:
        o.extend((2, 0x11, 1, 3, 0x11, 1))
    word(0xFFC4); word(0xD2 if bw else 0x01A2)
    o.append(0x00); o.extend(DC_LUM_BITS); o.extend(DC_VALS)
    o.append(0x10); o.extend(AC_LUM_BITS); o.extend(AC_LUM_VALS)
    if not bw:
        o.append(0x01); o.extend(DC_CHR_BITS); o.extend(DC_VALS)
        o.append(0x11); o.extend(AC_CHR_BITS); o.extend(AC_CHR_VALS)
    word(0xFFDA)
    if bw:
        word(8); o.extend((1, 1, 0))
    else:
        word(12); o.extend((3, 1, 0, 2, 0x11, 3, 0x11))
    o.extend((0, 0x3F, 0))
    return bytes(o)


def _pass(d):
    """One AAN pass along the last axis of an int64 array (JENC:411-454):
    integer sums, one double multiply or add per rotated term, every store
    truncated toward zero."""
    f = np.float64
    x = [d[..., i] for i in range(8)]
    t0, t7 = x[0] + x[7], x[0] - x[7]
    t1, t6 = x[1] + x[6], x[1] - x[6]
    t2, t5 = x[2] + x[5], x[2] - x[5]
    t3, t4 = x[3] + x[4], x[3] - x[4]
    t10, t13 = t0 + t3, t0 - t3
    t11, t12 = t1 + t2, t1 - t2
    out = [None] * 8
    out[0] = t10 + t11
    out[4] = t10 - t11
    z1 = (t12 + t13).astype(f) * 0.707106781
    out[2] = (t13.astype(f) + z1).astype(np.int64)
    out[6] = (t13.astype(f) - z1).astype(np.int64)
    t10 = t4 + t5
    t11 = t5 + t6
    t12 = t6 + t7
    z5 = (t10 - t12).astype(f) * 0.382683433
    z2 = 0.541196100 * t10.astype(f) + z5
    z4 = 1.306562965 * t12.astype(f) + z5
    z3 = t11.astype(f) * 0.707106781
    z11 = t7.astype(f) + z3
    z13 = t7.astype(f) - z3
    out[5] = (z13 + z2).astype(np.int64)
    out[3] = (z13 - z2).astype(np.int64)
    out[1] = (z11 + z4).astype(np.int64)
    out[7] = (z11 - z4).astype(np.int64)
    return np.stack(out, axis=-1)


def transform(blocks, fdtbl):
    """fDCTQuant (JENC:402-513) of int blocks [..., 8, 8]: quantised
    coefficients in natural order, int64 [..., 64]."""
    d = _pass(blocks.astype(np.int64))  # rows
    d = np.swapaxes(_pass(np.swapaxes(d, -1, -2)), -1, -2)  # columns
    d = d.reshape(d.shape[:-2] + (64,))
    return np.rint(d.astype(np.float64) * fdtbl).astype(np.int64)  # double2int: to nearest even


def data_units(frame, width, height, line_length, bw):
    """getBlock (JENC:734-752): int [blocks, components, 8, 8], Y then U then V,
    blocks in raster order.  `frame` holds the luma plane, then the chroma
    plane (V at even bytes, U at odd bytes, one pair per two pixels)."""
    fr = np.asarray(frame, dtype=np.uint8).reshape(-1)
    ll = line_length
    y = fr[: height * ll].reshape(height, ll)[:, :width].astype(np.int64) - 128
    planes = [y]
    if not bw:
        c = fr[height * ll: 2 * height * ll].reshape(height, ll)[:, :width].astype(np.int64) - 128
        planes.append(np.repeat(c[:, 1::2], 2, axis=1))  # U: the odd byte of pair x / 2
        planes.append(np.repeat(c[:, 0::2], 2, axis=1))  # V: the even byte
    bh, bwid = height // 8, width // 8
    du = np.stack([p.reshape(bh, 8, bwid, 8).transpose(0, 2, 1, 3).reshape(bh * bwid, 8, 8) for p in planes], axis=1)
    return du


def coefficients(frame, width, height, line_length, quality, bw):
    """Quantised coefficients in zigzag order: int16 [blocks, components, 64]."""
    ql, qc = quant_tables(quality)
    du = data_units(frame, width, height, line_length, bw)
    ncomp = du.shape[1]
    fd = np.stack([divisors(ql)] + [divisors(qc)] * (ncomp - 1))  # [components, 64]
    nat = transform(du, fd[None, :, :])
    zz = np.empty_like(nat)
    zz[..., ZZ] = nat
    return zz.astype(np.int16)


def encode(frame, width, height, line_length, quality, bw):
    """JPGEncoder::encode (JENC:802-852).  Returns (stream bytes, quantised
    zigzag coefficients int16 [blocks, components, 64], entropy-coded bits
    before the fill bits)."""
    assert width % 8 == 0 and height % 8 == 0
    coeffs = coefficients(frame, width, height, line_length, quality, bw)
    out = bytearray(header(quality, bw, width, height))
    acc = 0  # the bits not yet written as a byte, and their count (< 8)
    n = 0
    total = 0
    ncomp = coeffs.shape[1]
    dc_prev = [0] * ncomp
    rows = coeffs.reshape(-1, 64).tolist()
    for k, du in enumerate(rows):
        comp = k % ncomp
        t = 0 if comp == 0 else 1
        dcc, dcl = HT_DC[t]
        acc_c, acc_l = HT_AC[t]
        syms = []  # (value, length) pairs of this data unit, in order (JENC:653-711)
        diff = du[0] - dc_prev[comp]
        dc_prev[comp] = du[0]
        if diff == 0:
            syms.append((dcc[0], dcl[0]))
        else:
            cat = abs(diff).bit_length()
            syms.append((dcc[cat], dcl[cat]))
            syms.append((diff if diff > 0 else (1 << cat) - 1 + diff, cat))
        end0 = 63
        while end0 > 0 and du[end0] == 0:
            end0 -= 1
        if end0 == 0:
            syms.append((acc_c[0x00], acc_l[0x00]))
        else:
            i = 1
            while i <= end0:
                start = i
                while du[i] == 0 and i <= end0:
                    i += 1
                run = i - start
                if run >= 16:
                    syms.extend([(acc_c[0xF0], acc_l[0xF0])] * (run // 16))
                    run &= 0xF
                v = du[i]
                cat = abs(v).bit_length()
                syms.append((acc_c[run * 16 + cat], acc_l[run * 16 + cat]))
                syms.append((v if v > 0 else (1 << cat) - 1 + v, cat))
                i += 1
            if end0 != 63:
                syms.append((acc_c[0x00], acc_l[0x00]))
        for val, ln in syms:  # writeBits (JENC:358-387): MSB first, 0x00 after every 0xFF
            acc = (acc << ln) | val
            n += ln
            total += ln
            while n >= 8:
                n -= 8
                b = (acc >> n) & 0xFF
                out.append(b)
                if b == 0xFF:
                    out.append(0)
            acc &= (1 << n) - 1
    fill = 8 - n  # the free bits of the current byte: 8, not 0, when aligned (JENC:838-847)
    b = ((acc << fill) | ((1 << fill) - 1)) & 0xFF
    out.append(b)
    if b == 0xFF:
        out.append(0)
    out.extend((0xFF, 0xD9))
    return bytes(out), coeffs, total
