"""tests/golden/reference_golden.json, the vectors recorded from the reference's
own code, checked on the CPU: always against the generators and our
restatements (oracle, mxn_ref, jpeg_ref), and against the reference's host
build when there is one -- so a stale fixture fails here, and
tests/test_gpu_reference.py can rely on it where there is no reference."""
import json
import os

import numpy as np
import pytest

import jpeg_cases
import ref_lib
from golden import make_reference_golden as mk

CODECS = sorted(mk.CODECS)


@pytest.fixture(scope="module")
def ref_golden():
    with open(mk.OUT_PATH) as f:
        return json.load(f)


def test_fixture_lists_the_generators_cases(ref_golden):
    """The same cases in the same order, about eight per codec, hashes only,
    smaller than oracle_golden.json."""
    n = 0
    for codec in CODECS:
        assert [r["name"] for r in ref_golden[codec]] == [c[0] for c in mk.CODECS[codec]], codec
        assert 6 <= len(ref_golden[codec]) <= 10
        for r in ref_golden[codec]:
            assert set(r) == {"name", "frame_sha256", "out", "stream_len", "stream_sha256"}
            assert sum(len(v) for v in r["out"].values()) <= 100
            n += 1
    assert n == 48
    assert os.path.getsize(mk.OUT_PATH) < os.path.getsize(os.path.join(os.path.dirname(mk.OUT_PATH),
                                                                       "oracle_golden.json"))


def test_case_lists_hold_the_required_geometries():
    """Each codec: its smallest geometry, a ragged lineLength, a 320 x 240 frame."""
    smallest = {"object": (32, 4), "line": (64, 8), "wline": (64, 8), "blob": (32, 4), "mxn": (64, 8), "jpeg": (32, 8)}
    n = 0
    for codec in CODECS:
        geoms = []
        for c in mk.CODECS[codec]:
            w, h, ll = c[1] if codec == "jpeg" else (c[2:5] if codec == "blob" else c[1:4])
            geoms.append((w, h, ll, ll != (2 * w if codec in ("object", "wline") else w)))
            n += 1
        assert any((w, h) == smallest[codec] for w, h, _, _ in geoms), codec
        assert any(ragged for _, _, _, ragged in geoms), codec
        assert any((w, h) == (320, 240) for w, h, _, _ in geoms), codec
    assert n == 48


@pytest.mark.parametrize("codec", CODECS)
def test_fixture_equals_the_restatements(ref_golden, oracle_mod, codec):
    """Input hashes (the generators), OutArgs and stream hashes by the oracle
    and the Python references."""
    n = 0
    for case, row in zip(mk.CODECS[codec], ref_golden[codec]):
        fr = mk.frame(codec, case)
        assert mk.record(case, fr, *mk.restated(codec, case, fr)) == row, case[0]
        n += 1
    assert n == 8


@pytest.mark.parametrize("codec", CODECS)
def test_fixture_equals_the_reference(ref_golden, oracle_mod, codec):
    """The same by the reference's own classes (skips without a host build)."""
    ref_lib.require()
    n = 0
    for case, row in zip(mk.CODECS[codec], ref_golden[codec]):
        fr = mk.frame(codec, case)
        assert mk.record(case, fr, *mk.referenced(codec, case, fr)) == row, case[0]
        n += 1
    assert n == 8


def test_jpeg_cases_hold_the_bitstream_shapes(oracle_mod):
    """Among the JPEG cases: an aligned tail (eight fill bits, FF 00), stuffed
    bytes inside the scan, a ZRL code, a non-zero coefficient 63."""
    aligned = stuffed = zrl = last = 0
    for name, geom, content, q, bw in mk.JPEG:
        data, coeffs, bits = jpeg_cases.ref(oracle_mod, geom, content, q, bw)
        scan = data[324 if bw else 607:-2]
        if bits % 8 == 0:
            assert scan[-2:] == b"\xff\x00"
            aligned += 1
        stuffed += scan[:-2].count(b"\xff\x00") > 0
        c = coeffs.reshape(-1, 64).astype(np.int64)
        last += int((c[:, 63] != 0).any())
        for row in c[:, 1:]:
            idx = np.flatnonzero(row)
            if idx.size and (np.diff(np.concatenate(([-1], idx))) - 1 >= 16).any():
                zrl += 1
                break
    assert aligned >= 1 and stuffed >= 1 and zrl >= 1 and last >= 1, (aligned, stuffed, zrl, last)
