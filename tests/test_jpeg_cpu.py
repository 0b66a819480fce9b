"""tests/jpeg_ref.py, the restatement of the ov7670 JPEG encoder (JENC =
trik/ov7670/jpeg_encoder/include/internal/jpeg_encoder_reference.hpp) that the
GPU tests compare against, checked on its own: the header and its tables, that
an independent decoder reads its streams, and that the inputs of the GPU tests
(tests/jpeg_cases.py) reach every path of the coder -- every bit alignment of
the end, byte stuffing, ZRL codes, a non-zero last coefficient -- so that the
GPU tests cannot pass by never getting there.  No GPU."""
import io

import numpy as np
import pytest

import jpeg_cases
import jpeg_ref


@pytest.mark.parametrize("bw", [False, True])
def test_header_and_quantisers(bw):
    """324 / 607 bytes; the DQT carries clamp((Q sf + 50) / 100, 1, 255) in
    zigzag order, sf = 5000 / q below 50, else 200 - 2 q, q clamped to 1..100."""
    for q in (0, 1, 49, 50, 100, 255):
        hd = jpeg_ref.header(q, bw, 640, 480)
        assert len(hd) == (324 if bw else 607)
        assert hd[:4] == b"\xff\xd8\xff\xe0" and hd[20:22] == b"\xff\xdb"
        qq = min(max(q, 1), 100)
        sf = 5000 // qq if qq < 50 else 200 - 2 * qq
        for t, table in enumerate((jpeg_ref.Q_LUM, jpeg_ref.Q_CHR)[: 1 if bw else 2]):
            at = 24 + 65 * t  # SOI 2, APP0 18, marker 2, length 2; then (id, 64 bytes) per table
            assert hd[at] == t
            want = [0] * 64
            for i, v in enumerate(table):
                want[jpeg_ref.ZZ[i]] = min(max((v * sf + 50) // 100, 1), 255)
            assert list(hd[at + 1: at + 65]) == want, (q, t)
    assert jpeg_ref.header(0, bw, 64, 8) == jpeg_ref.header(1, bw, 64, 8)
    assert jpeg_ref.header(255, bw, 64, 8) == jpeg_ref.header(100, bw, 64, 8)
    assert jpeg_ref.header(49, bw, 64, 8) != jpeg_ref.header(50, bw, 64, 8)


def test_zigzag_and_huffman_tables():
    assert sorted(jpeg_ref.ZZ) == list(range(64))
    assert jpeg_ref.ZZ[:9] == [0, 1, 5, 6, 14, 15, 27, 28, 2] and jpeg_ref.ZZ[63] == 63
    for (code, length), n in ((jpeg_ref.HT_DC[0], 12), (jpeg_ref.HT_DC[1], 12), (jpeg_ref.HT_AC[0], 162),
                              (jpeg_ref.HT_AC[1], 162)):
        defined = [(length[s], code[s]) for s in range(len(code)) if length[s]]
        assert len(defined) == n
        # prefix-free: no code is the head of another
        strings = sorted(format(c, "0%db" % ln) for ln, c in defined)
        assert all(not b.startswith(a) for a, b in zip(strings, strings[1:]))
    # an undefined symbol writes no bits (run 0, category 11 has no code)
    assert jpeg_ref.HT_AC[0][1][0x0B] == 0 and jpeg_ref.HT_AC[1][1][0x0B] == 0


def smooth(w, h, ll):
    yy, xx = np.mgrid[0:h, 0:w]
    luma = (128 + 90 * np.sin(xx / 9.0) * np.cos(yy / 7.0)).astype(np.uint8)
    chroma = (128 + 60 * np.cos(xx / 11.0 + yy / 13.0)).astype(np.uint8)
    return jpeg_cases.planes(w, h, ll, luma, chroma)


def test_streams_decode(oracle_mod):
    Image = pytest.importorskip("PIL.Image")
    for w, h, ll in ((32, 8, 32), (64, 16, 64), (96, 24, 128)):
        frames = {"uniform": oracle_mod.synth(1, w, h, ll, jpeg_cases.LAYOUT_OV7670, 0, 5),
                  "smooth": smooth(w, h, ll),
                  "flat": jpeg_cases.planes(w, h, ll, np.full((h, w), 200, np.uint8), np.full((h, w), 90, np.uint8))}
        for name, fr in frames.items():
            for q in (1, 50, 100):
                for bw in (False, True):
                    data, _, _ = jpeg_ref.encode(fr, w, h, ll, q, bw)
                    im = Image.open(io.BytesIO(data))
                    im.load()
                    assert im.size == (w, h) and im.mode == ("L" if bw else "RGB"), (w, h, name, q, bw)
            # black and white at quality 100 gives the luma back
            data, _, _ = jpeg_ref.encode(fr, w, h, ll, 100, True)
            got = np.asarray(Image.open(io.BytesIO(data)), dtype=np.int64)
            src = fr[: h * ll].reshape(h, ll)[:, :w].astype(np.int64)
            mae = float(np.abs(got - src).mean())
            print("mean absolute error", (w, h, name), mae)
            assert mae < 1.0, (w, h, name, mae)


def scan_of(data, bw):
    """The entropy-coded segment with its fill bits: between the header and EOI."""
    assert data[-2:] == b"\xff\xd9"
    return data[324 if bw else 607: -2]


def test_gpu_inputs_reach_every_path(oracle_mod):
    """Over the small and 320 x 240 cases of the GPU tests: all eight residues
    mod 8 of the entropy bit count (the aligned end included, which appends
    FF 00), a stuffed FF 00 inside the scan, a ZRL code, a non-zero coefficient 63."""
    residues = set()
    stuffed = zrl = last = aligned_tail = 0
    for geom, name, q, bw in list(jpeg_cases.small_cases()) + list(jpeg_cases.mid_cases()):
        data, coeffs, bits = jpeg_cases.ref(oracle_mod, geom, name, q, bw)
        residues.add(bits % 8)
        scan = scan_of(data, bw)
        assert b"\xff" not in scan.replace(b"\xff\x00", b""), "an unstuffed 0xFF in the scan"
        if bits % 8 == 0:
            assert scan[-2:] == b"\xff\x00"  # eight fill bits, stuffed
            aligned_tail += 1
        stuffed += scan[:-2].count(b"\xff\x00") > 0
        c = coeffs.reshape(-1, 64).astype(np.int64)
        last += int((c[:, 63] != 0).any())
        # a run of 16 or more zeros before a non-zero AC coefficient
        nz = c[:, 1:] != 0
        for row in nz[nz.any(axis=1)]:
            idx = np.flatnonzero(row)
            gaps = np.diff(np.concatenate(([-1], idx))) - 1
            if (gaps >= 16).any():
                zrl += 1
                break
    assert residues == set(range(8)), residues
    assert aligned_tail > 0 and stuffed > 0 and zrl > 0 and last > 0


def test_basis_frame_puts_one_coefficient_everywhere(oracle_mod):
    """At quality 50 block k of the basis frame has its only non-zero AC at
    zigzag position k: runs 0..62, one to three ZRL codes, coefficient 63."""
    _, coeffs, _ = jpeg_cases.ref(oracle_mod, (64, 64, 64), "basis", 50, True)
    c = coeffs.reshape(64, 64)
    for k in range(1, 64):
        assert np.flatnonzero(c[k, 1:]).tolist() == [k - 1], k
