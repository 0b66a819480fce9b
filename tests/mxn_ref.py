"""CPU restatement of the ov7670 MxN colour-grid sensor (test code, not
product), MSEQ = trik/ov7670/mxn_sensor/include/internal/
cv_ball_detector_seqpass.hpp.  Per-pixel (rgb, hsv) come from the oracle's
2^24-entry table (index Y | U << 8 | V << 16; U = odd chroma byte, V = even);
everything after the pixel is written here from the reference's rules:

  * cells: m rows x n columns (InArgs widthM = m, heightN = n), steps H // m
    and W // n, visited rows outer, columns inner (MSEQ:585-618);
  * a cell's winner: every pixel in raster order increments its
    (H >> 3, S >> 6, V >> 6) bin, which becomes the winner when its count is
    strictly greater than the running maximum (MSEQ:411-452) -- the literal
    sequential loop, winner_sequential; winner_order_free is the form the
    kernel implements, and the tests hold the two equal;
  * colour: HSVtoRGB(8 h, 64 s, 64 v) (MSEQ:480-517), float divisions widened
    to double;
  * preview: zero fill, every source pixel through the truncated scale maps
    (last writer wins), then a clamped 20 x 20 square per cell, in cell order
    (MSEQ:328-366, 536-551, 609-618).
"""
import numpy as np

N_BINS = 32 * 4 * 4


def hsv_to_rgb(H, S, V):
    """HSVtoRGB, MSEQ:480-517: X / 255.0f is a float division widened to double."""
    h = float(np.float32(H) / np.float32(255))
    s = float(np.float32(S) / np.float32(255))
    v = float(np.float32(V) / np.float32(255))
    v = 0.0 if v < 0.2 else v
    s = 0.0 if s < 0.2 else 1.0
    i = int(h * 6)
    f = h * 6 - i
    p = v * (1 - s)
    q = v * (1 - f * s)
    t = v * (1 - (1 - f) * s)
    r, g, b = [(v, t, p), (q, v, p), (p, v, t), (p, q, v), (t, p, v), (v, p, q)][i % 6]
    return (int(r * 255) << 16) + (int(g * 255) << 8) + int(b * 255)


def bin_color(b):
    """The colour of bin b = h << 4 | s << 2 | v."""
    return hsv_to_rgb(8 * (b >> 4), 64 * ((b >> 2) & 3), 64 * (b & 3))


def frame_pixels(table, frame, width, height, line_length):
    """(rgb uint32 [H, W], bins int32 [H, W]) of one ov7670 frame (MSEQ:252-296)."""
    fr = np.asarray(frame, np.uint8)
    y = fr[:height * line_length].reshape(height, line_length)[:, :width].astype(np.int64)
    c = fr[height * line_length:2 * height * line_length].reshape(height, line_length)[:, :width].astype(np.int64)
    v = np.repeat(c[:, 0::2], 2, axis=1)
    u = np.repeat(c[:, 1::2], 2, axis=1)
    word = table[y | (u << 8) | (v << 16)]
    rgb = (word >> np.uint64(32)).astype(np.uint32)
    hsv = (word & np.uint64(0xFFFFFFFF)).astype(np.int64)  # 0x00VVSSHH
    bins = (((hsv & 255) >> 3) << 4) | ((((hsv >> 8) & 255) >> 6) << 2) | (((hsv >> 16) & 255) >> 6)
    return rgb, bins.astype(np.int32)


def winner_sequential(cell_bins):
    """GetImgColor2's loop (MSEQ:426-443) over a cell's bins in raster order."""
    counts = [0] * N_BINS
    best, best_n = 0, 0
    for b in cell_bins:
        counts[b] += 1
        if counts[b] > best_n:
            best_n = counts[b]
            best = b
    return best


def winner_order_free(cell_bins):
    """Among the bins with the largest final count, the one whose last pixel
    comes earliest in raster order; bin 0 for an empty cell."""
    a = np.asarray(cell_bins, np.int64).reshape(-1)
    if a.size == 0:
        return 0
    counts = np.bincount(a, minlength=N_BINS)
    last = np.full(N_BINS, -1, np.int64)
    np.maximum.at(last, a, np.arange(a.size))
    top = np.flatnonzero(counts == counts.max())
    return int(top[np.argmin(last[top])])


def tied_bins(cell_bins):
    """The bins at the largest final count of a cell."""
    a = np.asarray(cell_bins, np.int64).reshape(-1)
    if a.size == 0:
        return []
    counts = np.bincount(a, minlength=N_BINS)
    return np.flatnonzero(counts == counts.max()).tolist()


def cells(width, height, m, n):
    """(k, row_start, col_start, row_step, col_step) in visiting order."""
    row_step, col_step = height // m, width // n
    return [(i * n + j, i * row_step, j * col_step, row_step, col_step) for i in range(m) for j in range(n)]


def run(table, frame, width, height, line_length, m, n):
    """(colors [m * n], bins [m * n], tie flags [m * n]) of one frame, by the sequential loop."""
    _, bins = frame_pixels(table, frame, width, height, line_length)
    colors, winners, ties = [], [], []
    for _, r0, c0, rs, cs in cells(width, height, m, n):
        cell = bins[r0:r0 + rs, c0:c0 + cs].reshape(-1)
        w = winner_sequential(cell.tolist())
        winners.append(w)
        colors.append(bin_color(w))
        ties.append(len(tied_bins(cell)) >= 2)
    return colors, winners, ties


def scale_maps(width, height, out_w, out_h):
    """wi2wo, hi2ho of MSEQ:536-551: i * min(out / in) truncated."""
    shift = min(out_w / width, out_h / height)
    return [int(i * shift) for i in range(width)], [int(i * shift) for i in range(height)]


def px565(rgb):
    """writeOutputPixel: 0x00RRGGBB -> B5 G6 R5, R in the low bits."""
    rgb = np.asarray(rgb, np.uint32)
    return (((rgb >> 19) & 0x1F) | ((rgb >> 5) & 0x07E0) | ((rgb << 8) & 0xF800)).astype(np.uint16)


def preview(table, frame, width, height, line_length, m, n, colors, out_w, out_h, out_ll):
    """The out_h x out_ll preview bytes.  The maps are monotone, so the last
    writer of an output pixel is the largest source row and column that map
    onto it; the squares are the literal loops of MSEQ:355-366."""
    rgb, _ = frame_pixels(table, frame, width, height, line_length)
    wi2wo, hi2ho = scale_maps(width, height, out_w, out_h)
    out = np.zeros((out_h, out_w), np.uint16)
    last_row = {}
    for r, ro in enumerate(hi2ho):
        last_row[ro] = r
    last_col = {}
    for c, co in enumerate(wi2wo):
        last_col[co] = c
    rows = sorted(ro for ro in last_row if ro < out_h)
    cols = sorted(co for co in last_col if co < out_w)
    if rows and cols:
        src = px565(rgb[np.array([last_row[ro] for ro in rows])][:, np.array([last_col[co] for co in cols])])
        out[np.ix_(rows, cols)] = src
    for k, r0, c0, _, _ in cells(width, height, m, n):
        v = px565(colors[k])
        for row in range(r0, r0 + 20):
            for col in range(c0, c0 + 20):
                sr = min(max(row, 0), height - 1)
                sc = min(max(col, 0), width - 1)
                out[hi2ho[sr], wi2wo[sc]] = v
    buf = np.zeros((out_h, out_ll), np.uint8)
    buf[:, 0:2 * out_w:2] = (out & 0xFF).astype(np.uint8)
    buf[:, 1:2 * out_w:2] = (out >> 8).astype(np.uint8)
    return buf
