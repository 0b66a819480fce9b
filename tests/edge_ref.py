"""CPU restatement of the ov7670 edge-line sensor (test code, not product),
ESEQ = trik/ov7670/edge_line_sensor/include/internal/cv_ball_detector_seqpass.hpp.

The sensor calls three TI IMGLIB functions that exist on no machine we have,
so nothing here is pinned to executed reference code: the formulas are TI's
documented natural-C semantics of those functions, and together with what
ESEQ:154-268, 365-420 builds on them they are the contract.

  * IMG_sobel_3x3_8(in, out, w, h) (ESEQ:179): the image is one linear array;
    for i in 0 .. w*(h-2)-3
        H = -in[i] - 2in[i+1] - in[i+2] + in[i+2w] + 2in[i+2w+1] + in[i+2w+2]
        V = -in[i] + in[i+2] - 2in[i+w] + 2in[i+w+2] - in[i+2w] + in[i+2w+2]
        out[i+1] = min(|H| + |V|, 255)
    so out (r, c) is the window whose top-left is (r, c-1), columns 0 and w-1
    mix adjacent rows, and out[0], out[w*(h-2)-1] and the last two rows are
    never written: they are 0 here (the reference's zero-initialised static).
  * IMG_thr_gt2max_8 (ESEQ:181): out = out > thr ? 255 : out; a pixel is
    detected iff the result is 255.
  * sums (ESEQ:189-205): per row, count and column sum over columns
    16 <= c <= w-16 in uint16_t accumulators (they wrap mod 65536), added to
    the frame's int32 / uint32 totals; the row sum (m_targetY) stays 0.
  * OutArgs (ESEQ:397-417).
  * preview (ESEQ:163-173, 226-249, 405): IMG_ycbcr422pl_to_rgb565 with the
    thresholded map as luma and cb = chroma byte 2k, cr = chroma byte 2k+1 of
    pixel pair k, native uint16 RGB565; zero fill, every source pixel through
    the truncated scale maps (last writer in raster order wins), then the
    target line.

`edge_map`, `sums` and `preview` are vectorised; `edge_map_scalar`,
`sums_scalar` and `preview_scalar` are the literal loops, and
tests/test_edge_cpu.py holds the two equal."""
import numpy as np

COEFF = (0x2000, 0x2BDD, -0x0AC5, -0x1658, 0x3770)
LINE_PIXEL = 0x001F  # writeOutputPixel(0xff0000), ESEQ:91-95


def luma(frame, width, height):
    return np.asarray(frame, np.uint8)[:width * height]


def edge_map_scalar(frame, width, height, thr=50):
    """The literal loops: uint8 [height, width]."""
    a = [int(v) for v in luma(frame, width, height)]
    w = width
    out = [0] * (width * height)
    for i in range(w * (height - 2) - 2):
        H = -a[i] - 2 * a[i + 1] - a[i + 2] + a[i + 2 * w] + 2 * a[i + 2 * w + 1] + a[i + 2 * w + 2]
        V = -a[i] + a[i + 2] - 2 * a[i + w] + 2 * a[i + w + 2] - a[i + 2 * w] + a[i + 2 * w + 2]
        out[i + 1] = min(abs(H) + abs(V), 255)
    out = [255 if o > thr else o for o in out]
    return np.array(out, np.uint8).reshape(height, width)


def hv(frame, width, height):
    """The signed H and V of IMG_sobel_3x3_8: two int32 [height * width],
    element i + 1 = window i, 0 where the loop never writes."""
    a = luma(frame, width, height).astype(np.int32)
    w, n = width, width * (height - 2) - 2
    H = np.zeros(width * height, np.int32)
    V = np.zeros(width * height, np.int32)
    H[1:n + 1] = -a[0:n] - 2 * a[1:n + 1] - a[2:n + 2] + a[2 * w:2 * w + n] + 2 * a[2 * w + 1:2 * w + 1 + n] + \
        a[2 * w + 2:2 * w + 2 + n]
    V[1:n + 1] = -a[0:n] + a[2:n + 2] - 2 * a[w:w + n] + 2 * a[w + 2:w + 2 + n] - a[2 * w:2 * w + n] + \
        a[2 * w + 2:2 * w + 2 + n]
    return H, V


def sobel(frame, width, height):
    """IMG_sobel_3x3_8 before the threshold: int32 [height * width]."""
    H, V = hv(frame, width, height)
    return np.minimum(np.abs(H) + np.abs(V), 255)


def threshold(o, width, height, thr=50):
    """IMG_thr_gt2max_8 of sobel()'s output: uint8 [height, width]."""
    return np.where(o > thr, 255, o).astype(np.uint8).reshape(height, width)


def edge_map(frame, width, height, thr=50):
    """The thresholded map: uint8 [height, width]."""
    return threshold(sobel(frame, width, height), width, height, thr)


def sums_scalar(emap, wrap=True):
    """(points, sum_x) of ESEQ:189-205, the literal loops; wrap=False: without
    the uint16 wraps."""
    height, width = emap.shape
    points = sum_x = 0
    for r in range(height):
        cols = [c for c in range(16, width - 15) if emap[r, c] == 0xFF]
        n, sx = len(cols), sum(cols)
        if wrap:
            n, sx = n & 0xFFFF, sx & 0xFFFF
        points += n
        sum_x += sx
    return points, sum_x


def sums(emap, wrap=True):
    """sums_scalar, vectorised: the rows' counts and column sums, each cut to
    uint16 before the rows are added."""
    height, width = emap.shape
    det = emap[:, 16:width - 15] == 0xFF
    n = det.sum(axis=1, dtype=np.int64)
    sx = (det * np.arange(16, width - 15, dtype=np.int64)).sum(axis=1)
    if wrap:
        n, sx = n & 0xFFFF, sx & 0xFFFF
    return int(n.sum()), int(sx.sum())


def _cdiv(a, b):
    """C's truncating signed division."""
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def _s8(v):
    return ((v + 128) & 255) - 128


def targets(points, sum_x, width, height):
    """(targetX, targetY, targetSize) of ESEQ:397-417, cut to int8, int8, uint8."""
    points &= 0xFFFFFFFF
    if points == 0:
        return 0, 0, 0
    tx = (sum_x & 0xFFFFFFFF) // points
    tx = tx - (1 << 32) if tx >= 1 << 31 else tx
    radius = int(np.ceil(np.sqrt(np.float32(points) / np.float32(3.1415927))))
    x = _cdiv((tx - width // 2) * 200, width)
    y = _cdiv((0 - height // 2) * 200, height)
    size = ((radius * 400) & 0xFFFFFFFF) // (width + height)
    return _s8(x), _s8(y), size & 255


def rgb565(y, cb, cr):
    """IMG_ycbcr422pl_to_rgb565 of one pixel with the codec's coefficients."""
    yt = COEFF[0] * (y - 16)
    cb, cr = cb - 128, cr - 128
    r = min(max((yt + COEFF[1] * cr) >> 13, 0), 255)
    g = min(max((yt + COEFF[2] * cb + COEFF[3] * cr) >> 13, 0), 255)
    b = min(max((yt + COEFF[4] * cb) >> 13, 0), 255)
    return ((r >> 3) << 11) | ((g >> 2) << 5) | (b >> 3)


def scale_maps(width, height, out_w, out_h):
    """wi2wo, hi2ho of ESEQ:327-340."""
    shift = min(out_w / width, out_h / height)
    wi2wo = [int(i * shift) for i in range(width)]
    hi2ho = [int(i * shift) for i in range(height)]
    return wi2wo, hi2ho


def _line(out16, wi2wo, hi2ho, points, sum_x, width, height):
    points &= 0xFFFFFFFF
    if points == 0:
        return
    tx = (sum_x & 0xFFFFFFFF) // points
    tx = tx - (1 << 32) if tx >= 1 << 31 else tx  # targetX is an int32_t (ESEQ:399)
    col = min(max(tx, 0), width - 1)
    for adj in range(100):
        for row in (height // 2 - adj, height // 2 + adj):
            out16[hi2ho[min(max(row, 0), height - 1)], wi2wo[col]] = LINE_PIXEL


def _bytes(out16, out_w, out_h, out_ll):
    out = np.zeros((out_h, out_ll), np.uint8)
    out[:, :2 * out_w] = out16.astype("<u2").view(np.uint8).reshape(out_h, 2 * out_w)
    return out


def preview_scalar(frame, width, height, emap, points, sum_x, out_w, out_h, out_ll):
    """The literal loops of ESEQ:163-173, 226-249, 405: uint8 [out_h, out_ll]."""
    fr = np.asarray(frame, np.uint8)
    chroma = fr[width * height:2 * width * height]
    y = emap.reshape(-1)
    wi2wo, hi2ho = scale_maps(width, height, out_w, out_h)
    out16 = np.zeros((out_h, out_w), np.uint16)
    for r in range(height):
        for c in range(width):
            i = r * width + c
            k = i >> 1
            out16[hi2ho[r], wi2wo[c]] = rgb565(int(y[i]), int(chroma[2 * k]), int(chroma[2 * k + 1]))
    _line(out16, wi2wo, hi2ho, points, sum_x, width, height)
    return _bytes(out16, out_w, out_h, out_ll)


def preview(frame, width, height, emap, points, sum_x, out_w, out_h, out_ll):
    """preview_scalar, vectorised: the maps are separable, so the last writer
    of output (ro, co) is (last row onto ro, last column onto co)."""
    fr = np.asarray(frame, np.uint8)
    chroma = fr[width * height:2 * width * height].astype(np.int64)
    y = emap.reshape(-1).astype(np.int64)
    cb = np.repeat(chroma[0::2], 2) - 128
    cr = np.repeat(chroma[1::2], 2) - 128
    yt = COEFF[0] * (y - 16)
    r = np.clip((yt + COEFF[1] * cr) >> 13, 0, 255)
    g = np.clip((yt + COEFF[2] * cb + COEFF[3] * cr) >> 13, 0, 255)
    b = np.clip((yt + COEFF[4] * cb) >> 13, 0, 255)
    pix = (((r >> 3) << 11) | ((g >> 2) << 5) | (b >> 3)).astype(np.uint16).reshape(height, width)
    wi2wo, hi2ho = scale_maps(width, height, out_w, out_h)
    assert max(wi2wo) < out_w and max(hi2ho) < out_h
    last_row = {ro: sr for sr, ro in enumerate(hi2ho)}
    last_col = {co: sc for sc, co in enumerate(wi2wo)}
    out16 = np.zeros((out_h, out_w), np.uint16)
    ros, srs = zip(*sorted(last_row.items()))
    cos, scs = zip(*sorted(last_col.items()))
    out16[np.ix_(ros, cos)] = pix[np.ix_(srs, scs)]
    _line(out16, wi2wo, hi2ho, points, sum_x, width, height)
    return _bytes(out16, out_w, out_h, out_ll)


def run(frame, width, height, thr=50):
    """(emap, (points, sum_x), (targetX, targetY, targetSize)) of one frame."""
    emap = edge_map(frame, width, height, thr)
    p, sx = sums(emap)
    return emap, (p, sx), targets(p, sx, width, height)


def single_pixel(width, height, row, col, base=100, value=255):
    """A flat ov7670 frame with one pixel set (chroma 128)."""
    fr = np.full(2 * width * height, 128, np.uint8)
    fr[:width * height] = base
    fr[row * width + col] = value
    return fr


def level_frame(width, height, level, chroma=128):
    """Rows 0, 0, x, x, ... with x = level // 4 in even and level // 2 -
    level // 4 in odd columns: s = a[c-1] + 2a[c] + a[c+1] = 2 (level // 2) on
    the x rows, so for an even level H = +-level and V = 0, and the Sobel
    magnitude is exactly `level` on columns 1 .. width-2 of map rows
    0 .. height-3."""
    fr = np.full(2 * width * height, chroma, np.uint8)
    y = fr[:width * height].reshape(height, width)
    y[:] = 0
    rows = np.arange(height) % 4 >= 2
    y[rows, 0::2] = level // 4
    y[rows, 1::2] = level // 2 - level // 4
    return fr
