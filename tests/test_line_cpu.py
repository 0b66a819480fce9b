"""CPU-only checks of the line sensor's shape tests: the test reference
(tests/line_ref.py) against the oracle's restatement of LineDetector::run
(oracle.line_run, which tests/test_reference_cpu.py holds to the reference's
own code) wherever the oracle takes the geometry, and the inputs of the GPU
tests (tests/line_cases.py): that each reaches what it is meant to reach,
stated on the reference's output."""
import numpy as np
import pytest

import line_cases
import line_ref


def _oracle(oracle_mod, fr, w, h, ll, vf, vt, band):
    rc, oa, _, sums, _ = oracle_mod.line_run(fr, w, h, ll, vf, vt, band=band, preview=False)
    assert rc == 0
    return sums.tolist(), (oa["target_x"], oa["target_y"], oa["target_size"])


def _as_oracle(sums):
    """The oracle reports its int32 column sum sign-extended."""
    return [sums[0], line_ref._s32(sums[1]), sums[2]]


# (w, h, ll): w % 32 == 0 and h % 4 == 0, with and without row padding
ORACLE_GEOMS = [(32, 4, 32), (64, 36, 64), (64, 36, 72), (96, 100, 100), (160, 8, 161), (320, 240, 320)]


@pytest.mark.parametrize("geom", ORACLE_GEOMS)
def test_line_ref_equals_oracle(oracle_mod, table, geom):
    w, h, ll = geom
    frames = [line_cases.noise(w, h, ll, 1, 31 * w + h + ll),
              oracle_mod.line_scene(w, h, ll, 5, slope=0.25),
              oracle_mod.line_scene(w, h, ll, 6, x0=-20),       # the line mostly outside: few points
              line_cases.dark_pixels(w, h, 10, ll), line_cases.dark_pixels(w, h, 11, ll)]
    bands = line_cases.bands(h) + [(3, 17), (h // 3, h // 2), (-5, -2), (-2**31, 2), (1, -2**31)]
    seen = set()
    for fr in frames:
        for vf, vt in line_cases.RANGES + ((0, 30), (0, 100), (80, 20), (0, 0), (100, 100)):
            for band in bands:
                got = line_ref.sums(table, fr, w, h, ll, vf, vt, band)
                want, want_t = _oracle(oracle_mod, fr, w, h, ll, vf, vt, band)
                assert _as_oracle(got) == want, (geom, vf, vt, band)
                assert line_ref.targets(*got, w, h) == want_t, (geom, vf, vt, band)
                seen.add((got[0] > 10, got[2] > 0))
    # both sides of the points threshold, with and without cross points
    assert seen >= {(False, False), (True, False), (True, True)}


def test_line_ref_uniform_bytes_figures(table):
    """Uniform bytes detect about 28 % at (0, 70) and 85 % at (50, 100)."""
    w, h = 64, 1024
    fr = np.random.default_rng(1).integers(0, 256, 2 * w * h, dtype=np.uint8)
    for (vf, vt), share in zip(line_cases.RANGES, (0.28, 0.85)):
        n = line_ref.sums(table, fr, w, h, w, vf, vt)[0]
        assert abs(n / (h * (w - 9)) - share) < 0.02, (vf, vt, n)


def test_line_ref_column_sum_wraps(oracle_mod, table):
    """4096 x 600 with every window pixel detected: the column sum passes 2^32,
    the reference's int32 keeps its low word and targetX comes from that."""
    w, h = 4096, 600
    fr = line_cases.noise(w, h, w, 1, 4096)
    got = line_ref.sums(table, fr, w, h, w, 0, 100)
    assert got[:2] == [h * (w - 9), h * sum(range(5, w - 4))] and got[1] > 2**32
    want, want_t = _oracle(oracle_mod, fr, w, h, w, 0, 100, None)
    assert _as_oracle(got) == want
    assert line_ref.targets(*got, w, h) == want_t
    assert line_ref.center(*got[:2]) != got[1] // got[0]  # the wrap moves the target line


def test_line_ref_targets_widths():
    """The OutArgs' integer widths, on sums no small frame reaches."""
    t = line_ref.targets
    assert t(10, 10 * 50, 10, 64, 8) == (0, 0, 0) and t(11, 11 * 50, 0, 64, 8)[0] == (18 * 200) // 64
    assert t(11, 11 * 5, 0, 64, 8)[0] == -((27 * 200) // 64)         # C division, towards zero
    assert t(2**32 + 5, 0, 0, 64, 8) == (0, 0, 0)                    # uint32 points
    assert t(11, 2**32 + 11 * 40, 0, 64, 8) == t(11, 11 * 40, 0, 64, 8)
    assert t(100, 100 * 600, 0, 640, 480)[0] == ((600 - 320) * 200) // 640
    assert t(11, 11 * 639, 0, 640, 8)[0] == 99
    assert t(20000, 0, 20000, 640, 480) == (-100, 20000 * 100 // 51200, 20000 * 100 // (640 * 480))
    assert t(300000, 0, 300000, 640, 480) == (-100, 585 - 512, 97)   # int8 truncation of targetY
    # uint32 products: 5 10^9 - 2^32 = 705032704 = 51200 * 13770 + 8704 = 307200 * 2295 + 8704
    assert t(50000000, 0, 50000000, 640, 480) == (-100, 13770 % 256 - 256, 2295 % 256)


@pytest.mark.parametrize("shape", sorted({s[:2] for s in line_cases.SHAPES}))
def test_shape_noise_reaches_every_row_and_column(table, shape):
    w, h = shape
    n = max(n for sw, sh, n in line_cases.SHAPES if (sw, sh) == shape)
    line_cases.check_noise(table, line_cases.shape_noise(w, h, n), w, h, w, n)


@pytest.mark.parametrize("case", line_cases.GENERIC)
def test_generic_noise_reaches_every_row_and_column(table, case):
    w, ll, n, pad, off = case
    buf, off, stride = line_cases.generic_noise(case)
    line_cases.check_noise(table, buf[off:], w, line_cases.GENERIC_H, ll, n, stride)
    # none of these may take the fast kernel: a misaligned base, frame stride,
    # line length or width
    assert off % 8 or (n > 1 and stride % 8) or ll % 8 or w % 8


def test_shape_bands_differ(table):
    """The bands of the shape tests select different rows (so a band the
    kernel ignored would show), on the 64 x 36 frame."""
    w, h = 64, 36
    det = line_ref.detect(table, line_cases.shape_noise(w, h, 1), w, h, w, 0, 70)
    rows = det.sum(axis=1)
    got = [line_ref.sums_of(det, line_ref.default_band(h) if b is None else b)[2] for b in line_cases.bands(h)]
    assert got == [rows[18:].sum(), rows[0], rows[35], rows[35], 0, rows[3:].sum(), 0]
    assert len(set(got)) == 5


@pytest.mark.parametrize("width", line_cases.COLUMN_WIDTHS)
def test_one_hot_columns(table, width):
    h = 8
    buf = line_cases.one_hot_columns(width)
    fb = 2 * h * width
    got = [line_ref.sums(table, buf[c * fb:(c + 1) * fb], width, h, width, *line_cases.COLUMN_RANGE)
           for c in range(width)]
    assert got == line_cases.one_hot_expected(width)


def test_dark_pixel_counts(table):
    for count in (10, 11):
        fr = line_cases.dark_pixels(64, 8, count)
        s = line_ref.sums(table, fr, 64, 8, 64, *line_cases.COLUMN_RANGE)
        assert s[0] == count
        assert (line_ref.targets(*s, 64, 8) != (0, 0, 0)) == (count == 11)
    assert line_ref.sums(table, line_cases.floor(64, 8), 64, 8, 64, *line_cases.COLUMN_RANGE) == [0, 0, 0]
