"""Measure the operator outputs of SURVEY 8(f) rows 1-2 on the C3 batch.

  preview     trik_hsv_batch_preview: 4096 x 640x480 YUYV -> 320x240 RGB565X
              previews for one range.  Algorithmic bytes per frame: the source
              rows the 2:1 preview samples (H/2 rows of lineLength bytes) plus
              the preview written (outH * outLineLength), read/written once.
  auto_range  trik_hsv_batch_auto_range: the central zone of each frame
              (159 x 159 px at 640x480, 2 B/px) -- small, launch/latency-bound.
  line        trik_hsv_line_batch: 4096 x 640x480 ov7670 (YUV422P) frames, the
              line sensor's sums + OutArgs; algorithmic bytes = both planes
              (2 B/px) once.  line_preview: its 320x240 previews.
  autorange_exact  trik_hsv_batch_auto_range_exact (and trik_hsv_auto_scores):
              the exact autoDetectHsv of the ov7670 object sensor, the ov7670
              line sensor and the webcam line sensor over 4096 frames of 320x240
              and of 640x480, scene and uniform random bytes, the line sensor on
              the same geometry beside them; algorithmic bytes = 2 B/px once.
  blob        trik_hsv_blob_batch: 4096 x 640x480 ov7670 frames through the
              multi-blob sensor (metapixel bitmap + clusterer + 8 targets).
  edge        trik_hsv_edge_batch: the edge-line sensor's sums + OutArgs over
              the same ov7670 frames and over 4096 x 320x240 ones (with the line
              sensor on those beside it); algorithmic bytes = the Y plane once
              (1 B/px).  sums_preview: + trik_hsv_edge_preview's 320x240 previews.
  mxn         trik_hsv_mxn_batch: the MxN colour-grid sensor over the same
              ov7670 frames at 3x3 and 10x10 cells, scene and uniform random
              bytes; algorithmic bytes = both planes once, as the line row.
  jpeg        trik_hsv_jpeg_batch: the JPEG encoder over the same ov7670 frames,
              scene and uniform random bytes, quality 50 and 100, colour and
              black-and-white; algorithmic bytes = both planes once plus the
              stream bytes written.
  process     one host frame through the XDAIS quartet (H2D + kernels + D2H,
              PCIe-inclusive latency per frame), with preview and auto range.
  blob_ranges (--blob-ranges, a run of its own) trik_hsv_blob_batch_ranges: the
              four SURVEY 8(d) ranges over 4096 x 640x480 ov7670 scene frames in
              one call, against four trik_hsv_blob_batch calls, alternating; and
              the one call on the packed-YUYV twins of the same frames.
  frame_ranges (--frame-ranges, a run of its own) trik_hsv_frame_ranges_batch:
              4096 x 640x480 YUYV scene frames, each under its own ranges read
              from device memory, T = 4 and T = 1, beside trik_hsv_process_batch
              with one shared set; and at N = 256 against a loop of 256
              single-frame trik_hsv_process_batch calls with 256 range sets.
  blob_frame_ranges (--blob-frame-ranges, a run of its own)
              trik_hsv_blob_frame_ranges_batch: 4096 x 640x480 ov7670 scene
              frames and their packed-YUYV twins, each frame under its own
              ranges read from device memory, T = 1 and T = 4, beside
              trik_hsv_blob_batch_ranges with one shared set; and at N = 256
              against a loop of 256 single-frame trik_hsv_blob_batch_ranges
              calls with 256 range sets.
  line_frame_ranges (--line-frame-ranges, a run of its own)
              trik_hsv_line_frame_ranges_batch: 4096 x 640x480 ov7670 scene
              frames and their packed-YUYV twins, each frame under its own V
              range read from device memory, beside trik_hsv_line_batch with one
              shared range, trik_hsv_frame_ranges_batch at T = 1 with hue and
              saturation open and the shared-range object step; and at N = 256
              against a loop of 256 single-frame trik_hsv_line_batch calls.
  frame_ranges_preview (--frame-ranges-preview, a run of its own)
              trik_hsv_frame_ranges_preview: 4096 x 640x480 scene frames ->
              320x240 previews, each frame under its own range read from device
              memory, beside trik_hsv_batch_preview with one shared range, on
              the YUYV frames and their ov7670 twins; a 400x300 output through
              both gathers; at N = 256 against a loop of 256 single-frame
              trik_hsv_batch_preview calls; and the whole device loop
              (autoDetectHsv, ranges_of_detect, sums, preview) per step.
  line_frame_ranges_preview (--line-frame-ranges-preview, a run of its own)
              trik_hsv_line_frame_ranges_preview: 4096 x 640x480 ov7670 scene
              frames -> 320x240 previews, each frame under its own V range read
              from device memory, beside trik_hsv_line_preview with one shared
              range; the same on the packed-YUYV twins (the webcam line
              sensor); a 400x300 output through both gathers; at N = 256
              against a loop of 256 single-frame trik_hsv_line_preview calls;
              and the whole device loop of the ov7670 line kind per step.
  convert (--convert, a run of its own)
              trik_hsv_convert_batch: 4096 x 640x480 ov7670 scene frames and
              their packed-YUYV twins to each of the three forms, beside (a)
              trik_hsv_frame_ranges_batch at T = 1 on the same frames (the same
              per-pixel arithmetic, no image written) and (b) a device-to-device
              Tensor.copy_ that moves as many bytes as the form reads plus
              writes; the bound is each form <= 1.1 x ((a) + (b)).
  mask (--mask, a run of its own)
              trik_hsv_mask_batch with a range set per frame: 4096 x 640x480
              ov7670 scene frames and their packed-YUYV twins to bit planes at
              T = 1 and T = 4 and to a byte plane at T = 1, beside (a)
              trik_hsv_frame_ranges_batch at the same T (the same arithmetic, no
              image written), (b) a device-to-device Tensor.copy_ of the mask's
              byte count and, for information, trik_hsv_batch_masks with one
              shared range; the aim is each form <= 1.1 x ((a) + (b)).  And at
              N = 256 against a loop of 256 single-frame calls.

Prints one JSON object.  usage: python scripts/bench_operator.py [--frames N]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# TRIK_HSV_PKG_DIR: a directory holding another build's trik_hsv package (A/B)
sys.path.insert(0, os.environ.get("TRIK_HSV_PKG_DIR", os.path.join(ROOT, "trik-media-sensors-dsp_amd")))
HBM_PEAK_GBS = 8000.0


def timed(fn, stream, iters):
    """Average GPU time per call of `iters` back-to-back calls (asynchronous
    launches, so host-side call overhead overlaps the previous call's kernels),
    after `iters` untimed calls of the same operation (the first calls after
    another operation's batches run up to 25 % slower: the auto-range launches
    right after the previews' 1.9 GB of stores took 198 -> 161 us in
    profiles/r06/r06x_operator_kernel_trace_auto_range.txt)."""
    import torch

    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    for _ in range(iters):
        fn()
    b.record(stream)
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def scene_frames_and_twins(F, W, H):
    """F ov7670 scene frames (line length W) and their packed-YUYV twins (Y0 U
    Y1 V; U = odd, V = even chroma byte), on the device."""
    import torch

    import trik_hsv

    fb = 2 * H * W
    ov = torch.empty(F * fb, dtype=torch.uint8, device="cuda")
    trik_hsv.synth(ov, W, H, W, trik_hsv.LAYOUT_OV7670, 1, 0x7A1C)
    yuyv = torch.empty(F * fb, dtype=torch.uint8, device="cuda")
    for f0 in range(0, F, 256):
        src = ov[f0 * fb:(f0 + 256) * fb].view(-1, 2, H, W)
        dst = yuyv[f0 * fb:(f0 + 256) * fb].view(-1, H, 2 * W)
        dst[:, :, 0::2] = src[:, 0]
        dst[:, :, 1::4] = src[:, 1, :, 1::2]
        dst[:, :, 3::4] = src[:, 1, :, 0::2]
    return ov, yuyv


def blob_ranges(args):
    """The multi-blob sensor for the four SURVEY 8(d) ranges on 640x480 scene
    frames: one trik_hsv_blob_batch_ranges call against four single-range
    trik_hsv_blob_batch calls (alternating, in this process), and the same call
    on the packed-YUYV twins of the frames."""
    import torch

    import trik_hsv

    W, H, F = 640, 480, args.frames
    ranges = [(0, 30, 50, 100, 30, 100), (90, 150, 40, 100, 20, 100), (200, 260, 40, 100, 20, 100),
              (330, 20, 30, 100, 30, 100)]  # T0-T3
    centres = [(15, 15, 75, 25, 65, 35), (120, 30, 70, 30, 60, 40), (230, 30, 70, 30, 60, 40),
               (355, 25, 65, 35, 65, 35)]
    assert [trik_hsv.blob_range_of(c) for c in centres] == ranges
    ov, yuyv = scene_frames_and_twins(F, W, H)
    stream = torch.cuda.current_stream()
    det = trik_hsv.Detector()

    def four_calls():
        return [det.blob_batch(ov, W, H, W, c) for c in centres]

    def one_call():
        return det.blob_batch_ranges(ov, W, H, W, ranges)

    def one_call_yuyv():
        return det.blob_batch_ranges(yuyv, W, H, 2 * W, ranges, layout=trik_hsv.LAYOUT_YUYV)

    singles, one, twin = four_calls(), one_call(), one_call_yuyv()
    det.blob_batch(ov, W, H, W, centres[0])
    single_kernel = det.last_hot_kernel()
    same = all(torch.equal(one[k][:, t], singles[t][k]) and torch.equal(twin[k], one[k])
               for k in ("targets", "top", "n_labels") for t in range(4))
    runs = {"four_calls": [], "one_call": [], "one_call_yuyv": []}
    for _ in range(args.rounds):
        for name, fn in (("four_calls", four_calls), ("one_call", one_call), ("one_call_yuyv", one_call_yuyv)):
            runs[name].append(timed(fn, stream, args.iters))
    det.close()
    med = {k: sorted(v)[len(v) // 2] for k, v in runs.items()}
    return {"blob_ranges": {
        "frames": F, "ranges": 4, "geometry": [W, H], "iters": args.iters, "rounds": args.rounds,
        "results_identical": bool(same), "single_call_bitmap_kernel": int(single_kernel),
        "ms": {k: round(v, 4) for k, v in med.items()},
        "ms_runs": {k: [round(x, 4) for x in v] for k, v in runs.items()},
        "one_call_over_four_calls": round(med["one_call"] / med["four_calls"], 3),
        "yuyv_over_ov7670": round(med["one_call_yuyv"] / med["one_call"], 3),
        "Mslots_per_s": round(4 * F / med["one_call"] / 1e3, 3),
        "note": "four_calls: 4 x trik_hsv_blob_batch (unchanged code; bitmap kernel as reported, 2 = chroma-run); "
                "one_call: blob_meta_ranges_kernel (stripe arithmetic, one read of the frames) + blob_ccl_kernel "
                "per chunk of 4096 slots; medians of alternating rounds"}}


def frame_ranges(args):
    """trik_hsv_frame_ranges_batch (HSV ranges per frame, read on the device)
    on 640x480 YUYV scene frames, alternating in this process with
      (a) trik_hsv_process_batch with ONE shared set at the same N and T, and
      (b) at N = 256, a loop of 256 single-frame trik_hsv_process_batch calls
          with 256 different range sets (each call builds its tables) -- the
          only way to per-frame ranges without the new call.
    Algorithmic bytes = the frames once (2 B/px)."""
    import torch

    import trik_hsv

    W, H, LL, F, FB = 640, 480, 1280, args.frames, 256
    base = [(0, 30, 50, 100, 30, 100), (90, 150, 40, 100, 20, 100), (200, 260, 40, 100, 20, 100),
            (330, 20, 30, 100, 30, 100)]  # T0-T3

    def sets(n, t):  # frame f: the base ranges with every hue bound shifted by f degrees
        return [[((hf + f) % 360, (ht + f) % 360, sf, st, vf, vt) for hf, ht, sf, st, vf, vt in base[:t]]
                for f in range(n)]

    fb = H * LL
    dev = torch.empty(F * fb, dtype=torch.uint8, device="cuda")
    trik_hsv.synth(dev, W, H, LL, trik_hsv.LAYOUT_YUYV, 1, 0x7A1C)
    stream = torch.cuda.current_stream()
    det = trik_hsv.Detector()
    dev_sets = {t: torch.tensor(sets(F, t), dtype=torch.int16, device="cuda") for t in (4, 1)}
    small_sets = sets(FB, 4)
    small_dev = torch.tensor(small_sets, dtype=torch.int16, device="cuda")
    assert len({tuple(s) for s in small_sets}) == FB

    def loop256():
        return [det.process_batch(dev[f * fb:(f + 1) * fb], W, H, LL, trik_hsv.LAYOUT_YUYV, small_sets[f])
                for f in range(FB)]

    fns = {
        "frame_ranges_T4": lambda: trik_hsv.frame_ranges_batch(dev, W, H, LL, trik_hsv.LAYOUT_YUYV, dev_sets[4]),
        "shared_T4": lambda: det.process_batch(dev, W, H, LL, trik_hsv.LAYOUT_YUYV, base),
        "frame_ranges_T1": lambda: trik_hsv.frame_ranges_batch(dev, W, H, LL, trik_hsv.LAYOUT_YUYV, dev_sets[1]),
        "shared_T1": lambda: det.process_batch(dev, W, H, LL, trik_hsv.LAYOUT_YUYV, base[:1]),
        "frame_ranges_256_T4": lambda: trik_hsv.frame_ranges_batch(dev, W, H, LL, trik_hsv.LAYOUT_YUYV, small_dev,
                                                                   n_frames=FB),
        "loop_256_T4": loop256,
    }
    one, singles = fns["frame_ranges_256_T4"](), loop256()
    same = all(torch.equal(one[0][f], singles[f][0][0]) and torch.equal(one[1][f], singles[f][1][0])
               for f in range(FB))
    # frame 0's set is the shared set: its slots must agree with the shared-range step
    same0 = torch.equal(fns["frame_ranges_T4"]()[0][0], fns["shared_T4"]()[0][0])
    runs = {k: [] for k in fns}
    for _ in range(args.rounds):
        for name, fn in fns.items():
            runs[name].append(timed(fn, stream, 2 if name == "loop_256_T4" else args.iters))
    det.close()
    med = {k: sorted(v)[len(v) // 2] for k, v in runs.items()}

    def row(name, n):
        nb = n * fb
        return {"frames": n, "ms": round(med[name], 4), "ms_runs": [round(x, 4) for x in runs[name]],
                "Mframes_per_s": round(n / med[name] / 1e3, 3), "bytes_algorithmic": nb,
                "achieved_GBs": round(nb / (med[name] / 1e3) / 1e9, 1),
                "hbm_frac": round(nb / (med[name] / 1e3) / 1e9 / HBM_PEAK_GBS, 4)}

    out = {k: row(k, FB if "256" in k else F) for k in fns}
    for t in (4, 1):
        out[f"frame_ranges_T{t}"]["over_shared"] = round(med[f"frame_ranges_T{t}"] / med[f"shared_T{t}"], 2)
    out["frame_ranges_256_T4"]["over_loop"] = round(med["frame_ranges_256_T4"] / med["loop_256_T4"], 4)
    out["loop_256_T4"]["ms_per_call"] = round(med["loop_256_T4"] / FB, 4)
    return {"frame_ranges": {
        "geometry": [W, H], "layout": "YUYV", "scene_frames": True, "iters": args.iters, "rounds": args.rounds,
        "results_identical_256": bool(same), "frame0_equals_shared": bool(same0), **out,
        "note": "frame_ranges_*: memset + frame_ranges_kernel (exact per-pixel HSV, ranges read from device memory, "
                "frame f under the base ranges shifted by f degrees of hue) + targets_kernel; shared_*: "
                "trik_hsv_process_batch, one set for the batch (warm tables); loop_256_T4: 256 single-frame "
                "trik_hsv_process_batch calls, 256 different sets (2 timed iterations per round); medians of "
                "alternating rounds, all in one process"}}


def blob_frame_ranges(args):
    """trik_hsv_blob_frame_ranges_batch (the multi-blob sensor with HSV ranges
    per frame, read on the device) on 640x480 ov7670 scene frames and their
    packed-YUYV twins, alternating in this process with
      (a) trik_hsv_blob_batch_ranges with ONE shared set at the same N and T, and
      (b) at N = 256, a loop of 256 single-frame trik_hsv_blob_batch_ranges
          calls with 256 different range sets (each call builds its tables) --
          the only way to per-frame ranges without the new call.
    Both calls run blob_ccl_kernel over the same slots; what differs is the
    bitmap pass (a kernel trace of this mode splits the two)."""
    import torch

    import trik_hsv

    W, H, F, FB = 640, 480, args.frames, 256
    OV, YUYV = trik_hsv.LAYOUT_OV7670, trik_hsv.LAYOUT_YUYV
    base = [(0, 30, 50, 100, 30, 100), (90, 150, 40, 100, 20, 100), (200, 260, 40, 100, 20, 100),
            (330, 20, 30, 100, 30, 100)]  # T0-T3

    def sets(n, t):  # frame f: the base ranges with every hue bound shifted by f degrees
        return [[((hf + f) % 360, (ht + f) % 360, sf, st, vf, vt) for hf, ht, sf, st, vf, vt in base[:t]]
                for f in range(n)]

    ov, yuyv = scene_frames_and_twins(F, W, H)
    fb = 2 * H * W
    stream = torch.cuda.current_stream()
    det = trik_hsv.Detector()
    dev_sets = {t: torch.tensor(sets(F, t), dtype=torch.int16, device="cuda") for t in (4, 1)}
    small_sets = {t: sets(FB, t) for t in (4, 1)}
    small_dev = {t: torch.tensor(small_sets[t], dtype=torch.int16, device="cuda") for t in (4, 1)}
    assert all(len({tuple(s) for s in small_sets[t]}) == FB for t in (4, 1))
    frames = {"ov7670": (ov, W, OV), "yuyv": (yuyv, 2 * W, YUYV)}

    def ours(lay, rng, n=None):
        buf, ll, layout = frames[lay]
        return lambda: det.blob_frame_ranges_batch(buf, W, H, ll, rng, layout=layout, n_frames=n, top=True)

    def shared(lay, t):
        buf, ll, layout = frames[lay]
        return lambda: det.blob_batch_ranges(buf, W, H, ll, base[:t], layout=layout)

    def loop256(t):
        return lambda: [det.blob_batch_ranges(ov[f * fb:(f + 1) * fb], W, H, W, small_sets[t][f]) for f in range(FB)]

    fns = {}
    for lay in frames:
        for t in (1, 4):
            fns[f"frame_ranges_T{t}_{lay}"] = ours(lay, dev_sets[t])
            fns[f"shared_T{t}_{lay}"] = shared(lay, t)
    for t in (1, 4):
        fns[f"frame_ranges_256_T{t}"] = ours("ov7670", small_dev[t], FB)
        fns[f"loop_256_T{t}"] = loop256(t)
    if args.only:  # a kernel trace of one pair: the timed calls of the rows whose name holds the text
        for name in [k for k in fns if args.only in k]:
            timed(fns[name], stream, args.iters)
        det.close()
        return {"blob_frame_ranges": {"only": args.only, "iters": args.iters}}
    keys = ("targets", "top", "n_labels")
    same = True
    for t in (1, 4):
        one, singles = fns[f"frame_ranges_256_T{t}"](), fns[f"loop_256_T{t}"]()
        same = same and all(torch.equal(one[k][f], singles[f][k][0]) for k in keys for f in range(FB))
    # frame 0's set is the shared set: its slots must agree with the shared-range call, in both layouts
    same0 = all(torch.equal(fns[f"frame_ranges_T4_{lay}"]()[k][0], fns[f"shared_T4_{lay}"]()[k][0])
                for k in keys for lay in frames)
    runs = {k: [] for k in fns}
    for _ in range(args.rounds):
        for name, fn in fns.items():
            runs[name].append(timed(fn, stream, 2 if name.startswith("loop_256") else args.iters))
    det.close()
    med = {k: sorted(v)[len(v) // 2] for k, v in runs.items()}

    def row(name):
        n = FB if "256" in name else F
        t = 4 if "T4" in name else 1
        return {"frames": n, "ranges": t, "ms": round(med[name], 4), "ms_runs": [round(x, 4) for x in runs[name]],
                "Mslots_per_s": round(n * t / med[name] / 1e3, 3),
                "achieved_GBs": round(n * fb / (med[name] / 1e3) / 1e9, 1)}

    out = {k: row(k) for k in fns}
    for lay in frames:
        for t in (1, 4):
            out[f"frame_ranges_T{t}_{lay}"]["over_shared"] = round(
                med[f"frame_ranges_T{t}_{lay}"] / med[f"shared_T{t}_{lay}"], 3)
    for t in (1, 4):
        out[f"frame_ranges_256_T{t}"]["over_loop"] = round(med[f"frame_ranges_256_T{t}"] / med[f"loop_256_T{t}"], 4)
        out[f"loop_256_T{t}"]["ms_per_call"] = round(med[f"loop_256_T{t}"] / FB, 4)
    return {"blob_frame_ranges": {
        "geometry": [W, H], "scene_frames": True, "iters": args.iters, "rounds": args.rounds,
        "results_identical_256": bool(same), "frame0_equals_shared": bool(same0), **out,
        "note": "frame_ranges_*: blob_meta_frame_ranges_kernel (exact per-pixel HSV once per pixel, ranges read from "
                "device memory, frame f under the base ranges shifted by f degrees of hue) + blob_ccl_kernel per "
                "chunk of 4096 slots; shared_*: trik_hsv_blob_batch_ranges, one set for the batch (warm tables; "
                "blob_meta_ranges_kernel + blob_ccl_kernel); loop_256_*: 256 single-frame "
                "trik_hsv_blob_batch_ranges calls, 256 different sets (2 timed iterations per round); achieved_GBs "
                "counts the frames once (2 B/px); medians of alternating rounds, all in one process"}}


def line_frame_ranges(args):
    """trik_hsv_line_frame_ranges_batch (the line sensors with a V range per
    frame, read on the device) on 640x480 scene frames and their packed-YUYV
    twins, alternating in this process:
      a  trik_hsv_line_batch, one shared range (0, 30) -- the unchanged path;
      b  the new call on ov7670, every frame given that same range;
      c  the new call on ov7670, a distinct range per frame;
      d  the new call on the YUYV twins (the webcam line sensor);
      e  trik_hsv_frame_ranges_batch at T = 1 with (0, 359, 0, 100, vf, vt) on
         the same YUYV frames -- the only per-frame route before;
      f  the shared-range object step at T = 1 on them;
    and at N = 256: the new call against 256 single-frame trik_hsv_line_batch
    calls with 256 different ranges.  Algorithmic bytes = the frames once
    (2 B/px in both layouts).  --only a runs row a alone (also against another
    build's package, TRIK_HSV_PKG_DIR)."""
    import torch

    import trik_hsv

    W, H, F, FB = 640, 480, args.frames, 256
    fb = 2 * H * W
    ov, yuyv = scene_frames_and_twins(F, W, H)
    stream = torch.cuda.current_stream()

    def six(pairs):
        t = torch.zeros((len(pairs), 6), dtype=torch.int16)
        t[:, 4:] = torch.tensor(pairs, dtype=torch.int16)
        return t.cuda()

    distinct = [((7 * f) % 41, 45 + (11 * f) % 56) for f in range(F)]  # lo <= 40 < 45 <= hi
    fns = {"a_line_batch_shared": lambda: trik_hsv.line_batch(ov, W, H, W, 0, 30)}
    if not args.only:
        same_dev, distinct_dev, small_dev = six([(0, 30)] * F), six(distinct), six(distinct[:FB])
        full = torch.tensor([[(0, 359, 0, 100, lo, hi)] for lo, hi in distinct], dtype=torch.int16, device="cuda")
        det = trik_hsv.Detector()
        YUYV, OV = trik_hsv.LAYOUT_YUYV, trik_hsv.LAYOUT_OV7670

        def loop256():
            return [trik_hsv.line_batch(ov[f * fb:(f + 1) * fb], W, H, W, *distinct[f]) for f in range(FB)]

        fns.update({
            "b_ov7670_same_range": lambda: trik_hsv.line_frame_ranges_batch(ov, W, H, W, OV, same_dev),
            "c_ov7670_distinct": lambda: trik_hsv.line_frame_ranges_batch(ov, W, H, W, OV, distinct_dev),
            "d_yuyv_distinct": lambda: trik_hsv.line_frame_ranges_batch(yuyv, W, H, 2 * W, YUYV, distinct_dev),
            "e_frame_ranges_T1_open": lambda: trik_hsv.frame_ranges_batch(yuyv, W, H, 2 * W, YUYV, full),
            "f_shared_object_T1": lambda: det.process_batch(yuyv, W, H, 2 * W, YUYV, [(0, 359, 0, 100, 0, 30)]),
            "line_frame_ranges_256": lambda: trik_hsv.line_frame_ranges_batch(ov, W, H, W, OV, small_dev,
                                                                              n_frames=FB),
            "loop_256_line_batch": loop256,
        })
        a, b = fns["a_line_batch_shared"](), fns["b_ov7670_same_range"]()
        same_ab = torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        d, e = fns["d_yuyv_distinct"](), fns["e_frame_ranges_T1_open"]()
        same_de = torch.equal(d[0], e[0][:, 0])
        one, singles = fns["line_frame_ranges_256"](), loop256()
        same_256 = all(torch.equal(one[0][f], singles[f][0][0]) and torch.equal(one[1][f], singles[f][1][0])
                       for f in range(FB))
    # the host-bound loop first and the slow row e after it: the rows compared
    # with each other (a, b, c, d) then follow a busy GPU, not the loop's idle one
    order = sorted(fns, key=lambda k: (k != "loop_256_line_batch", k[0] != "e", k))
    runs = {k: [] for k in fns}
    for _ in range(args.rounds):
        for name in order:
            runs[name].append(timed(fns[name], stream, 2 if name == "loop_256_line_batch" else args.iters))
    med = {k: sorted(v)[len(v) // 2] for k, v in runs.items()}

    def row(name):
        n = FB if "256" in name else F
        nb = n * fb
        return {"frames": n, "ms": round(med[name], 4), "ms_runs": [round(x, 4) for x in runs[name]],
                "Mframes_per_s": round(n / med[name] / 1e3, 3), "bytes_algorithmic": nb,
                "achieved_GBs": round(nb / (med[name] / 1e3) / 1e9, 1),
                "hbm_frac": round(nb / (med[name] / 1e3) / 1e9 / HBM_PEAK_GBS, 4)}

    out = {k: row(k) for k in fns}
    if not args.only:
        det.close()
        out["b_ov7670_same_range"]["over_a"] = round(med["b_ov7670_same_range"] / med["a_line_batch_shared"], 4)
        out["c_ov7670_distinct"]["over_a"] = round(med["c_ov7670_distinct"] / med["a_line_batch_shared"], 4)
        out["d_yuyv_distinct"]["over_e"] = round(med["d_yuyv_distinct"] / med["e_frame_ranges_T1_open"], 4)
        out["line_frame_ranges_256"]["over_loop"] = round(med["line_frame_ranges_256"] / med["loop_256_line_batch"], 4)
        out["loop_256_line_batch"]["ms_per_call"] = round(med["loop_256_line_batch"] / FB, 4)
        out.update({"b_equals_a": bool(same_ab), "d_equals_e": bool(same_de), "results_identical_256": bool(same_256)})
    return {"line_frame_ranges": {
        "geometry": [W, H], "scene_frames": True, "iters": args.iters, "rounds": args.rounds, **out,
        "note": "a: memset + line_vec_kernel<ov7670, shared> + line_targets_kernel; b, c: the same with the range "
                "read per frame by the kernel; d: line_vec_kernel<YUYV, per frame> (V-only packed 16-bit arithmetic, "
                "sum_y by rows); e: frame_ranges_kernel (exact H, S, V per pixel); f: trik_hsv_process_batch, warm "
                "tables; loop_256_line_batch: 256 single-frame trik_hsv_line_batch calls (2 timed iterations per "
                "round); medians of alternating rounds, all in one process"}}


def frame_ranges_preview(args):
    """trik_hsv_frame_ranges_preview (the object sensor's preview with an HSV
    range per frame, read on the device) on 640x480 scene frames -> 320x240,
    alternating in this process:
      a  trik_hsv_batch_preview, one shared range -- the unchanged path;
      b  the new call, every frame given that same range (bytes compared with a);
      c  the new call, a distinct range per frame;
      d  (c) on the ov7670 twins of the frames;
      e  a 400x300 output (not 2:1) through the shared-range gather and the new one;
      f  at N = 256: the new call with 256 ranges against the loop of 256
         single-frame trik_hsv_batch_preview calls it replaces (each builds a
         table set);
      g  the whole device loop per step: trik_hsv_batch_auto_range,
         trik_hsv_ranges_of_detect, trik_hsv_frame_ranges_batch, the new call.
    Algorithmic bytes of a preview row = the source rows the maps sample
    (out_height rows of line_length bytes, both planes on ov7670) plus the
    previews written; row g adds the frames read once by the sums pass."""
    import torch

    import trik_hsv

    W, H, F, FB = 640, 480, args.frames, 256
    OW, OH, GW, GH = 320, 240, 400, 300
    YUYV, OV = trik_hsv.LAYOUT_YUYV, trik_hsv.LAYOUT_OV7670
    T0 = (0, 30, 50, 100, 30, 100)
    fb = 2 * H * W
    ov, yuyv = scene_frames_and_twins(F, W, H)
    stream = torch.cuda.current_stream()
    det = trik_hsv.Detector()
    distinct = [((T0[0] + f) % 360, (T0[1] + f) % 360) + T0[2:] for f in range(F)]  # T0's hue sector turned by f degrees
    assert len(set(distinct[:FB])) == FB
    same_dev = torch.tensor([[T0]] * F, dtype=torch.int16, device="cuda")
    distinct_dev = torch.tensor([[r] for r in distinct], dtype=torch.int16, device="cuda")
    small_dev = distinct_dev[:FB].contiguous()
    sums_a, _ = det.process_batch(yuyv, W, H, 2 * W, YUYV, [T0])
    sums_c, _ = trik_hsv.frame_ranges_batch(yuyv, W, H, 2 * W, YUYV, distinct_dev)
    sums_small = sums_c[:FB].contiguous()

    def ours(buf, ll, lay, rng, sums, ow=OW, oh=OH, n=None):
        return lambda: det.frame_ranges_preview(buf, W, H, ll, lay, rng, sums, out_width=ow, out_height=oh, n_frames=n)

    def shared(ow=OW, oh=OH):
        return lambda: det.batch_preview(yuyv, W, H, 2 * W, YUYV, T0, sums_a, out_width=ow, out_height=oh)

    def loop256():
        return [det.batch_preview(yuyv[f * fb:(f + 1) * fb], W, H, 2 * W, YUYV, distinct[f], sums_small[f],
                                  out_width=OW, out_height=OH) for f in range(FB)]

    def device_loop():
        d = trik_hsv.batch_auto_range(yuyv, W, H, 2 * W, YUYV)
        r = trik_hsv.ranges_of_detect(d)
        s, _ = trik_hsv.frame_ranges_batch(yuyv, W, H, 2 * W, YUYV, r)
        return det.frame_ranges_preview(yuyv, W, H, 2 * W, YUYV, r, s, out_width=OW, out_height=OH)

    fns = {
        "a_batch_preview_shared": shared(),
        "b_same_range": ours(yuyv, 2 * W, YUYV, same_dev, sums_a),
        "c_distinct": ours(yuyv, 2 * W, YUYV, distinct_dev, sums_c),
        "d_distinct_ov7670": ours(ov, W, OV, distinct_dev, sums_c),
        "e_gather_shared": shared(GW, GH),
        "e_gather_distinct": ours(yuyv, 2 * W, YUYV, distinct_dev, sums_c, GW, GH),
        "f_256_ranges": ours(yuyv, 2 * W, YUYV, small_dev, sums_small, n=FB),
        "f_loop_256_batch_preview": loop256,
        "g_device_loop": device_loop,
    }
    same_ab = torch.equal(fns["a_batch_preview_shared"](), fns["b_same_range"]())
    same_cd = torch.equal(fns["c_distinct"](), fns["d_distinct_ov7670"]())
    one, singles = fns["f_256_ranges"](), loop256()
    same_256 = all(torch.equal(one[f], singles[f][0]) for f in range(FB))
    del one, singles
    # the host-bound loop first: the rows compared with each other then follow a busy GPU
    order = sorted(fns, key=lambda k: (k != "f_loop_256_batch_preview", k))
    runs = {k: [] for k in fns}
    for _ in range(args.rounds):
        for name in order:
            runs[name].append(timed(fns[name], stream, 2 if name == "f_loop_256_batch_preview" else args.iters))
    det.close()
    med = {k: sorted(v)[len(v) // 2] for k, v in runs.items()}

    def row(name):
        n = FB if "256" in name else F
        ow, oh = (GW, GH) if name.startswith("e_") else (OW, OH)
        nb = n * (oh * 2 * W + oh * 2 * ow) + (n * fb if name == "g_device_loop" else 0)
        return {"frames": n, "out": [ow, oh], "ms": round(med[name], 4), "ms_runs": [round(x, 4) for x in runs[name]],
                "Mframes_per_s": round(n / med[name] / 1e3, 3), "bytes_algorithmic": nb,
                "achieved_GBs": round(nb / (med[name] / 1e3) / 1e9, 1),
                "hbm_frac": round(nb / (med[name] / 1e3) / 1e9 / HBM_PEAK_GBS, 4)}

    out = {k: row(k) for k in fns}
    for k in ("b_same_range", "c_distinct", "d_distinct_ov7670"):
        out[k]["over_a"] = round(med[k] / med["a_batch_preview_shared"], 4)
    out["e_gather_distinct"]["over_shared"] = round(med["e_gather_distinct"] / med["e_gather_shared"], 4)
    out["f_256_ranges"]["over_loop"] = round(med["f_256_ranges"] / med["f_loop_256_batch_preview"], 4)
    out["f_loop_256_batch_preview"]["ms_per_call"] = round(med["f_loop_256_batch_preview"] / FB, 4)
    return {"frame_ranges_preview": {
        "geometry": [W, H], "scene_frames": True, "iters": args.iters, "rounds": args.rounds,
        "b_equals_a": bool(same_ab), "d_equals_c": bool(same_cd), "results_identical_256": bool(same_256), **out,
        "note": "a, e_gather_shared: preview_rows2_kernel / preview_gather_kernel on a warm table set + overlay_kernel; "
                "b, c, d, f_256_ranges: fr_preview_rows2_kernel (exact H, S, V per sampled pixel, the range read per "
                "frame by the kernel) + overlay_kernel; e_gather_distinct: fr_preview_gather_kernel; "
                "f_loop_256_batch_preview: 256 single-frame trik_hsv_batch_preview calls with 256 ranges (2 timed "
                "iterations per round); g: auto_range_vec_kernel, ranges_of_detect_kernel, memset + frame_ranges_kernel "
                "+ targets_kernel, then the preview; each call allocates its previews from torch's cache; medians of "
                "alternating rounds, all in one process"}}


def line_frame_ranges_preview(args):
    """trik_hsv_line_frame_ranges_preview (the line sensors' previews with a V
    range per frame, read on the device) on 640x480 scene frames -> 320x240,
    alternating in this process:
      a  trik_hsv_line_preview, one shared range -- the unchanged path;
      b  the new call on the ov7670 frames, every frame given that same range
         (bytes compared with a);
      c  the new call, a distinct V range per frame, ov7670;
      d  (c) on the packed-YUYV twins (the webcam line sensor's preview);
      e  a 400x300 output (not 2:1) through the shared-range gather and the new one;
      f  at N = 256: the new call with 256 ranges against the loop of 256
         single-frame trik_hsv_line_preview calls it replaces (each builds or
         looks up a table set);
      g  the whole device loop per step for the ov7670 line kind:
         trik_hsv_batch_auto_range_exact, trik_hsv_ranges_of_detect,
         trik_hsv_line_frame_ranges_batch, the new call.
    The yardstick of b and c is a in the same run; the margin is the spread of
    a's own per-round values.  Algorithmic bytes of a preview row = the source
    rows the maps sample (out_height rows of line_length bytes, both planes on
    ov7670) plus the previews written; row g adds the frames read once each by
    the auto-range pass and by the sums pass."""
    import torch

    import trik_hsv

    W, H, F, FB = 640, 480, args.frames, 256
    OW, OH, GW, GH = 320, 240, 400, 300
    YUYV, OV = trik_hsv.LAYOUT_YUYV, trik_hsv.LAYOUT_OV7670
    SHARED = (0, 30)
    fb = 2 * H * W
    ov, yuyv = scene_frames_and_twins(F, W, H)
    stream = torch.cuda.current_stream()
    det = trik_hsv.Detector()
    valid = [(lo, hi) for lo in range(101) for hi in range(lo, 101)]
    distinct = [valid[(1009 * f + 17) % len(valid)] for f in range(F)]  # a stride coprime to the 5151 pairs
    assert len(set(distinct)) == min(F, len(valid))

    def six(pairs):
        return torch.tensor([(0, 0, 0, 0) + tuple(p) for p in pairs], dtype=torch.int16, device="cuda")

    same_dev, distinct_dev = six([SHARED] * F), six(distinct)
    small_dev = distinct_dev[:FB].contiguous()
    sums_a, _ = trik_hsv.line_batch(ov, W, H, W, *SHARED)
    sums_c, _ = trik_hsv.line_frame_ranges_batch(ov, W, H, W, OV, distinct_dev)
    sums_d, _ = trik_hsv.line_frame_ranges_batch(yuyv, W, H, 2 * W, YUYV, distinct_dev)
    sums_small = sums_c[:FB].contiguous()

    def ours(buf, ll, lay, rng, sums, ow=OW, oh=OH, n=None):
        return lambda: det.line_frame_ranges_preview(buf, W, H, ll, lay, rng, sums, out_width=ow, out_height=oh,
                                                     n_frames=n)

    def shared(ow=OW, oh=OH):
        return lambda: det.line_preview(ov, W, H, W, *SHARED, sums_a, out_width=ow, out_height=oh)

    def loop256():
        return [det.line_preview(ov[f * fb:(f + 1) * fb], W, H, W, *distinct[f], sums_small[f], out_width=OW,
                                 out_height=OH) for f in range(FB)]

    def device_loop():
        d, _ = trik_hsv.batch_auto_range_exact(ov, W, H, W, trik_hsv.AUTO_OV7670_LINE)
        r = trik_hsv.ranges_of_detect(d, n_ranges=1)
        s, _ = trik_hsv.line_frame_ranges_batch(ov, W, H, W, OV, r)
        return det.line_frame_ranges_preview(ov, W, H, W, OV, r, s, out_width=OW, out_height=OH)

    fns = {
        "a_line_preview_shared": shared(),
        "b_same_range": ours(ov, W, OV, same_dev, sums_a),
        "c_distinct": ours(ov, W, OV, distinct_dev, sums_c),
        "d_distinct_yuyv": ours(yuyv, 2 * W, YUYV, distinct_dev, sums_d),
        "e_gather_shared": shared(GW, GH),
        "e_gather_distinct": ours(ov, W, OV, distinct_dev, sums_c, GW, GH),
        "f_256_ranges": ours(ov, W, OV, small_dev, sums_small, n=FB),
        "f_loop_256_line_preview": loop256,
        "g_device_loop": device_loop,
    }
    same_ab = torch.equal(fns["a_line_preview_shared"](), fns["b_same_range"]())
    one, singles = fns["f_256_ranges"](), loop256()
    same_256 = all(torch.equal(one[f], singles[f][0]) for f in range(FB))
    del one, singles
    # the host-bound loop first: the rows compared with each other then follow a busy GPU
    order = sorted(fns, key=lambda k: (k != "f_loop_256_line_preview", k))
    runs = {k: [] for k in fns}
    for _ in range(args.rounds):
        for name in order:
            runs[name].append(timed(fns[name], stream, 2 if name == "f_loop_256_line_preview" else args.iters))
    det.close()
    med = {k: sorted(v)[len(v) // 2] for k, v in runs.items()}

    def row(name):
        n = FB if "256" in name else F
        ow, oh = (GW, GH) if name.startswith("e_") else (OW, OH)
        nb = n * (oh * 2 * W + oh * 2 * ow) + (2 * n * fb if name == "g_device_loop" else 0)
        return {"frames": n, "out": [ow, oh], "ms": round(med[name], 4), "ms_runs": [round(x, 4) for x in runs[name]],
                "Mframes_per_s": round(n / med[name] / 1e3, 3), "bytes_algorithmic": nb,
                "achieved_GBs": round(nb / (med[name] / 1e3) / 1e9, 1),
                "hbm_frac": round(nb / (med[name] / 1e3) / 1e9 / HBM_PEAK_GBS, 4)}

    out = {k: row(k) for k in fns}
    a_runs = runs["a_line_preview_shared"]
    spread = (max(a_runs) - min(a_runs)) / med["a_line_preview_shared"]
    out["a_line_preview_shared"]["spread_of_rounds"] = round(spread, 4)
    for k in ("b_same_range", "c_distinct", "d_distinct_yuyv"):
        out[k]["over_a"] = round(med[k] / med["a_line_preview_shared"], 4)
        out[k]["within_a_spread"] = bool(med[k] <= med["a_line_preview_shared"] * (1 + spread))
    out["e_gather_distinct"]["over_shared"] = round(med["e_gather_distinct"] / med["e_gather_shared"], 4)
    out["f_256_ranges"]["over_loop"] = round(med["f_256_ranges"] / med["f_loop_256_line_preview"], 4)
    out["f_loop_256_line_preview"]["ms_per_call"] = round(med["f_loop_256_line_preview"] / FB, 4)
    return {"line_frame_ranges_preview": {
        "geometry": [W, H], "scene_frames": True, "iters": args.iters, "rounds": args.rounds,
        "b_equals_a": bool(same_ab), "results_identical_256": bool(same_256), **out,
        "note": "a, e_gather_shared: preview_rows2_kernel<WIN, HUEFREE, OVL> / preview_gather_kernel + "
                "line_overlay_kernel on a warm table set; b, c, d, f_256_ranges: lfr_preview_rows2_kernel (V = max of "
                "the clamped colour, the bounds and the target line read per frame by the kernel, no LDS); "
                "e_gather_distinct: lfr_preview_gather_kernel + line_overlay_kernel; f_loop_256_line_preview: 256 "
                "single-frame trik_hsv_line_preview calls with 256 ranges (2 timed iterations per round); g: the "
                "exact auto-range kernels, ranges_of_detect_kernel, memset + line_vec_kernel + line_targets_kernel, "
                "then the preview; each call allocates its previews from torch's cache; medians of alternating "
                "rounds, all in one process"}}


def convert(args):
    """trik_hsv_convert_batch on 640x480 scene frames of both layouts, each
    form, alternating in this process with
      (a) trik_hsv_frame_ranges_batch at T = 1 on the same frames: the same
          per-pixel arithmetic and the same bytes read, no image written, and
      (b) a device-to-device Tensor.copy_ whose bytes read plus bytes written
          equal the form's (a copy of 5 B/px for the 64-bit form, which reads 2
          and writes 8; of 2.5 B/px for the planes, which read 2 and write 3).
    Algorithmic bytes = the frames once plus the image once.  The bound: a form's
    time <= 1.1 x ((a) + (b)) of the same run -- converting and writing in one
    pass is no slower than doing them one after the other."""
    import torch

    import trik_hsv

    W, H, F = 640, 480, args.frames
    px = F * W * H
    ov, yuyv = scene_frames_and_twins(F, W, H)
    stream = torch.cuda.current_stream()
    forms = {"rgb888hsv": trik_hsv.CONVERT_RGB888HSV, "hsv_planes": trik_hsv.CONVERT_HSV_PLANES,
             "rgb_planes": trik_hsv.CONVERT_RGB_PLANES}
    layouts = {"ov7670": (ov, W, trik_hsv.LAYOUT_OV7670), "yuyv": (yuyv, 2 * W, trik_hsv.LAYOUT_YUYV)}
    outs = {"rgb888hsv": torch.empty((F, H, W), dtype=torch.int64, device="cuda"),
            "planes": torch.empty((F, 3, H, W), dtype=torch.uint8, device="cuda")}
    one_range = torch.tensor([[(0, 30, 50, 100, 30, 100)]] * F, dtype=torch.int16, device="cuda")
    copy_bytes = {"rgb888hsv": 5 * px, "planes": 5 * px // 2}
    src = torch.empty(copy_bytes["rgb888hsv"], dtype=torch.uint8, device="cuda").fill_(7)
    dst = torch.empty_like(src)
    fns = {}
    for lname, (frames, ll, layout) in layouts.items():
        fns[f"frame_ranges_T1_{lname}"] = (lambda fr=frames, ll=ll, lay=layout:
                                           trik_hsv.frame_ranges_batch(fr, W, H, ll, lay, one_range))
        for fname, form in forms.items():
            o = outs["rgb888hsv" if fname == "rgb888hsv" else "planes"]
            fns[f"{fname}_{lname}"] = (lambda fr=frames, ll=ll, lay=layout, form=form, o=o:
                                       trik_hsv.convert_batch(fr, W, H, ll, lay, form, out=o))
    for cname, nb in copy_bytes.items():
        fns[f"copy_{cname}"] = lambda nb=nb: dst[:nb].copy_(src[:nb])
    # both layouts hold the same (Y, U, V) at every pixel: the same image
    same = all(torch.equal(trik_hsv.convert_batch(ov[:8 * 2 * H * W], W, H, W, trik_hsv.LAYOUT_OV7670, f),
                           trik_hsv.convert_batch(yuyv[:8 * 2 * H * W], W, H, 2 * W, trik_hsv.LAYOUT_YUYV, f))
               for f in forms.values())
    runs = {k: [] for k in fns}
    for _ in range(args.rounds):
        for name, fn in fns.items():
            runs[name].append(timed(fn, stream, args.iters))
    med = {k: sorted(v)[len(v) // 2] for k, v in runs.items()}

    def row(name, nb):
        return {"ms": round(med[name], 4), "ms_runs": [round(x, 4) for x in runs[name]], "bytes_algorithmic": nb,
                "achieved_GBs": round(nb / (med[name] / 1e3) / 1e9, 1),
                "hbm_frac": round(nb / (med[name] / 1e3) / 1e9 / HBM_PEAK_GBS, 4)}

    out = {}
    for lname in layouts:
        out[f"frame_ranges_T1_{lname}"] = row(f"frame_ranges_T1_{lname}", 2 * px)
    for cname, nb in copy_bytes.items():
        out[f"copy_{cname}"] = row(f"copy_{cname}", 2 * nb)
    ok = True
    for lname in layouts:
        for fname in forms:
            cname = "rgb888hsv" if fname == "rgb888hsv" else "planes"
            name = f"{fname}_{lname}"
            r = row(name, 2 * copy_bytes[cname])
            r["Mframes_per_s"] = round(F / med[name] / 1e3, 3)
            bound = 1.1 * (med[f"frame_ranges_T1_{lname}"] + med[f"copy_{cname}"])
            r["bound_ms"] = round(bound, 4)
            r["over_bound"] = round(med[name] / bound, 3)
            r["within_bound"] = bool(med[name] <= bound)
            ok = ok and r["within_bound"]
            out[name] = r
    return {"convert": {
        "frames": F, "geometry": [W, H], "scene_frames": True, "iters": args.iters, "rounds": args.rounds,
        "layouts_give_the_same_image": bool(same), "all_within_bound": bool(ok), **out,
        "note": "<form>_<layout>: trik_hsv_convert_batch into a dense tensor (convert_vec_kernel); bytes = frames read "
                "(2 B/px) + image written (8 or 3 B/px); frame_ranges_T1_*: memset + frame_ranges_kernel + "
                "targets_kernel; copy_*: Tensor.copy_ of half the form's bytes (read + written = the form's); "
                "bound_ms = 1.1 x (frame_ranges_T1 + copy); medians of alternating rounds, all in one process"}}


def mask(args):
    """trik_hsv_mask_batch on 640x480 scene frames of both layouts with a range
    set per frame (the four bench ranges, rotated by the frame): bit planes at
    T = 1 and T = 4, a byte plane at T = 1, alternating in this process with
      (a) trik_hsv_frame_ranges_batch at the same T on the same frames and
          ranges: the same per-pixel arithmetic and bytes read, no image written,
      (b) a device-to-device Tensor.copy_ of the mask's byte count, and
      (c) for information, trik_hsv_batch_masks with one shared range (a handle,
          its tables, a byte per pixel with the ranges in its bits).
    Algorithmic bytes = the frames once plus the mask once.  The aim: a form's
    time <= 1.1 x ((a) + (b)) of the same run.  At N = 256 the T = 4 bit planes
    with 256 range sets against 256 single-frame calls of the same entry point."""
    import torch

    import trik_hsv

    W, H, F, FB = 640, 480, args.frames, 256
    px = F * W * H
    ov, yuyv = scene_frames_and_twins(F, W, H)
    stream = torch.cuda.current_stream()
    R4 = [(0, 30, 50, 100, 30, 100), (90, 150, 40, 100, 20, 100), (200, 260, 40, 100, 20, 100),
          (330, 20, 30, 100, 30, 100)]
    ranges = {t: torch.tensor([[R4[(f + k) % 4] for k in range(t)] for f in range(F)], dtype=torch.int16, device="cuda")
              for t in (1, 4)}
    layouts = {"ov7670": (ov, W, trik_hsv.LAYOUT_OV7670), "yuyv": (yuyv, 2 * W, trik_hsv.LAYOUT_YUYV)}
    forms = {"bits_T1": (trik_hsv.MASK_BITS, 1), "bits_T4": (trik_hsv.MASK_BITS, 4), "bytes_T1": (trik_hsv.MASK_BYTES, 1)}
    mask_bytes = {"bits_T1": px // 8, "bits_T4": px // 2, "bytes_T1": px}
    outs = {k: torch.empty((F, t, H, W // 8 if form == trik_hsv.MASK_BITS else W), dtype=torch.uint8, device="cuda")
            for k, (form, t) in forms.items()}
    src = torch.empty(px, dtype=torch.uint8, device="cuda").fill_(7)
    dst = torch.empty_like(src)
    det = trik_hsv.Detector()
    fns = {}
    for lname, (frames, ll, layout) in layouts.items():
        for t in (1, 4):
            fns[f"frame_ranges_T{t}_{lname}"] = (lambda fr=frames, ll=ll, lay=layout, t=t:
                                                 trik_hsv.frame_ranges_batch(fr, W, H, ll, lay, ranges[t]))
        for fname, (form, t) in forms.items():
            fns[f"mask_{fname}_{lname}"] = (lambda fr=frames, ll=ll, lay=layout, form=form, t=t, o=outs[fname]:
                                            trik_hsv.mask_batch(fr, W, H, ll, lay, ranges[t], form, out=o))
        fns[f"batch_masks_shared_T1_{lname}"] = (lambda fr=frames, ll=ll, lay=layout:
                                                 det.batch_masks(fr, W, H, ll, lay, R4[:1]))
    for fname, nb in mask_bytes.items():
        fns[f"copy_{fname}"] = lambda nb=nb: dst[:nb].copy_(src[:nb])
    small = ranges[4][:FB].contiguous()

    def loop256():
        return [trik_hsv.mask_batch(yuyv[f * 2 * H * W:], W, H, 2 * W, trik_hsv.LAYOUT_YUYV, small[f], n_frames=1)
                for f in range(FB)]

    fns["mask_bits_256_T4_yuyv"] = lambda: trik_hsv.mask_batch(yuyv, W, H, 2 * W, trik_hsv.LAYOUT_YUYV, small,
                                                               n_frames=FB)
    fns["loop_256_T4_yuyv"] = loop256
    # both layouts hold the same (Y, U, V) at every pixel: the same mask; the loop gives the one call's planes;
    # bit 0 of batch_masks' byte is the byte plane of the same range
    n8 = 8 * 2 * H * W
    same = all(torch.equal(trik_hsv.mask_batch(ov[:n8], W, H, W, trik_hsv.LAYOUT_OV7670, ranges[t][:8], form),
                           trik_hsv.mask_batch(yuyv[:n8], W, H, 2 * W, trik_hsv.LAYOUT_YUYV, ranges[t][:8], form))
               for form, t in forms.values())
    one, singles = fns["mask_bits_256_T4_yuyv"](), loop256()
    same_256 = all(torch.equal(one[f], singles[f][0]) for f in range(FB))
    old = det.batch_masks(yuyv[:n8], W, H, 2 * W, trik_hsv.LAYOUT_YUYV, R4[:1])[0]
    new = trik_hsv.mask_batch(yuyv[:n8], W, H, 2 * W, trik_hsv.LAYOUT_YUYV, [R4[0]], trik_hsv.MASK_BYTES)
    same_old = torch.equal((old & 1) * 255, new[:, 0])
    runs = {k: [] for k in fns}
    for _ in range(args.rounds):
        for name, fn in fns.items():
            runs[name].append(timed(fn, stream, 2 if name.startswith("loop_256") else args.iters))
    det.close()
    med = {k: sorted(v)[len(v) // 2] for k, v in runs.items()}

    def row(name, nb):
        return {"ms": round(med[name], 4), "ms_runs": [round(x, 4) for x in runs[name]], "bytes_algorithmic": nb,
                "achieved_GBs": round(nb / (med[name] / 1e3) / 1e9, 1),
                "hbm_frac": round(nb / (med[name] / 1e3) / 1e9 / HBM_PEAK_GBS, 4)}

    out = {}
    for lname in layouts:
        for t in (1, 4):
            out[f"frame_ranges_T{t}_{lname}"] = row(f"frame_ranges_T{t}_{lname}", 2 * px)
        out[f"batch_masks_shared_T1_{lname}"] = row(f"batch_masks_shared_T1_{lname}", 3 * px)
    for fname, nb in mask_bytes.items():
        out[f"copy_{fname}"] = row(f"copy_{fname}", 2 * nb)
    ok = True
    for lname in layouts:
        for fname, (form, t) in forms.items():
            name = f"mask_{fname}_{lname}"
            r = row(name, 2 * px + mask_bytes[fname])
            r["Mframes_per_s"] = round(F / med[name] / 1e3, 3)
            bound = 1.1 * (med[f"frame_ranges_T{t}_{lname}"] + med[f"copy_{fname}"])
            r["bound_ms"] = round(bound, 4)
            r["over_bound"] = round(med[name] / bound, 3)
            r["within_bound"] = bool(med[name] <= bound)
            ok = ok and r["within_bound"]
            out[name] = r
    px256 = FB * W * H
    for name in ("mask_bits_256_T4_yuyv", "loop_256_T4_yuyv"):
        out[name] = row(name, 2 * px256 + px256 // 2)
    out["mask_bits_256_T4_yuyv"]["over_loop"] = round(med["mask_bits_256_T4_yuyv"] / med["loop_256_T4_yuyv"], 4)
    out["loop_256_T4_yuyv"]["ms_per_call"] = round(med["loop_256_T4_yuyv"] / FB, 4)
    return {"mask": {
        "frames": F, "geometry": [W, H], "scene_frames": True, "iters": args.iters, "rounds": args.rounds,
        "layouts_give_the_same_mask": bool(same), "results_identical_256": bool(same_256),
        "byte_plane_equals_batch_masks_bit0": bool(same_old), "all_within_bound": bool(ok), **out,
        "note": "mask_<form>_T<t>_<layout>: trik_hsv_mask_batch into a dense tensor, a range set per frame "
                "(mask_vec_kernel); bytes = frames read (2 B/px) + mask written (T/8 or T B/px); frame_ranges_T<t>_*: "
                "memset + frame_ranges_kernel + targets_kernel on the same ranges; copy_*: Tensor.copy_ of the mask's "
                "byte count; bound_ms = 1.1 x (frame_ranges + copy); batch_masks_shared_T1_*: trik_hsv_batch_masks, one "
                "shared range, information only; loop_256_T4_yuyv: 256 single-frame trik_hsv_mask_batch calls (2 timed "
                "iterations per round); medians of alternating rounds, all in one process"}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5, help="alternating rounds of the blob_ranges mode")
    ap.add_argument("--no-cpu", action="store_true", help="skip the oracle CPU baselines")
    ap.add_argument("--only-autorange", action="store_true",
                    help="stop after the preview, auto_range, line and autorange_exact rows")
    ap.add_argument("--blob-ranges", action="store_true",
                    help="the blob_ranges mode alone: one 4-range multi-blob call against four single-range calls")
    ap.add_argument("--frame-ranges", action="store_true",
                    help="the frame_ranges mode alone: per-frame ranges against the shared-range step and against a "
                         "loop of single-frame calls")
    ap.add_argument("--blob-frame-ranges", action="store_true",
                    help="the blob_frame_ranges mode alone: the multi-blob sensor with per-frame ranges against the "
                         "shared-range call and against a loop of single-frame calls")
    ap.add_argument("--only", default="",
                    help="with --blob-frame-ranges: run only the rows whose name holds this text, once, for a kernel "
                         "trace (e.g. T4_ov7670: the per-frame and the shared call at T = 4 on ov7670 frames)")
    ap.add_argument("--line-frame-ranges", action="store_true",
                    help="the line_frame_ranges mode alone: the line sensors with a V range per frame against the "
                         "shared-range call, the object sensor's per-frame call and a loop of single-frame calls "
                         "(--only a: the shared-range row alone)")
    ap.add_argument("--frame-ranges-preview", action="store_true",
                    help="the frame_ranges_preview mode alone: the object sensor's preview with a range per frame "
                         "against the shared-range preview, a loop of single-frame calls and the whole device loop")
    ap.add_argument("--line-frame-ranges-preview", action="store_true",
                    help="the line_frame_ranges_preview mode alone: the line sensors' previews with a V range per "
                         "frame against the shared-range preview, a loop of single-frame calls and the whole device "
                         "loop")
    ap.add_argument("--convert", action="store_true",
                    help="the convert mode alone: trik_hsv_convert_batch, each form and layout, against the per-frame "
                         "sums at T = 1 plus a device-to-device copy of the same bytes")
    ap.add_argument("--mask", action="store_true",
                    help="the mask mode alone: trik_hsv_mask_batch, bit and byte planes with a range set per frame, "
                         "against the per-frame sums at the same T plus a device-to-device copy of the mask's bytes")
    args = ap.parse_args()
    if args.mask:
        print(json.dumps(mask(args)))
        return
    if args.convert:
        print(json.dumps(convert(args)))
        return
    if args.line_frame_ranges_preview:
        print(json.dumps(line_frame_ranges_preview(args)))
        return
    if args.frame_ranges_preview:
        print(json.dumps(frame_ranges_preview(args)))
        return
    if args.line_frame_ranges:
        print(json.dumps(line_frame_ranges(args)))
        return
    if args.blob_frame_ranges:
        print(json.dumps(blob_frame_ranges(args)))
        return
    if args.blob_ranges:
        print(json.dumps(blob_ranges(args)))
        return
    if args.frame_ranges:
        print(json.dumps(frame_ranges(args)))
        return
    import numpy as np
    import torch

    import trik_hsv

    W, H, LL, F = 640, 480, 1280, args.frames
    OW, OH, OLL = 320, 240, 640
    T0 = (0, 30, 50, 100, 30, 100)
    dev = torch.empty(F * H * LL, dtype=torch.uint8, device="cuda")
    trik_hsv.synth(dev, W, H, LL, trik_hsv.LAYOUT_YUYV, 1, 0x7A1C)
    stream = torch.cuda.current_stream()
    det = trik_hsv.Detector()
    sums, _ = det.process_batch(dev, W, H, LL, trik_hsv.LAYOUT_YUYV, [T0])
    out = {}

    pv_ms = timed(lambda: det.batch_preview(dev, W, H, LL, trik_hsv.LAYOUT_YUYV, T0, sums,
                                            out_width=OW, out_height=OH, out_line_length=OLL),
                  stream, args.iters)
    pv_bytes = F * ((H // 2) * LL + OH * OLL)
    out["preview"] = {"frames": F, "ms": round(pv_ms, 4), "Mframes_per_s": round(F / pv_ms / 1e3, 3),
                      "bytes_algorithmic": pv_bytes,
                      "achieved_GBs": round(pv_bytes / (pv_ms / 1e3) / 1e9, 1),
                      "hbm_frac": round(pv_bytes / (pv_ms / 1e3) / 1e9 / HBM_PEAK_GBS, 4),
                      "note": "preview_rows2_kernel (the 2:1 map: writes every preview byte, guide lines included) + overlay_kernel (the target circle)"}

    ar_ms = timed(lambda: trik_hsv.batch_auto_range(dev, W, H, LL, trik_hsv.LAYOUT_YUYV), stream,
                  args.iters)
    zone = 159 * 159
    out["auto_range"] = {"frames": F, "ms": round(ar_ms, 4), "Mframes_per_s": round(F / ar_ms / 1e3, 3),
                         "zone_px_per_frame": zone,
                         "achieved_GBs": round(F * zone * 2 / (ar_ms / 1e3) / 1e9, 1)}

    lf = min(F, 4096)
    lfb = 2 * H * W
    ldev = torch.empty(lf * lfb, dtype=torch.uint8, device="cuda")
    trik_hsv.synth(ldev, W, H, W, trik_hsv.LAYOUT_OV7670, 1, 0x7A1C)
    ln_ms = timed(lambda: trik_hsv.line_batch(ldev, W, H, W, 0, 30), stream, args.iters)
    out["line"] = {"frames": lf, "ms": round(ln_ms, 4), "Mframes_per_s": round(lf / ln_ms / 1e3, 3),
                   "bytes_algorithmic": lf * lfb,
                   "achieved_GBs": round(lf * lfb / (ln_ms / 1e3) / 1e9, 1),
                   "hbm_frac": round(lf * lfb / (ln_ms / 1e3) / 1e9 / HBM_PEAK_GBS, 4),
                   "note": "line_vec_kernel + line_targets_kernel"}
    # the exact autoDetectHsv of the ov7670 object sensor and the two line
    # sensors, beside the webcam object sensor's auto_range row and the line
    # row above: one workgroup per frame, a barrier pair per row of the
    # positive band (every row for the line kinds)
    out["autorange_exact"] = {"frames": lf,
                              "note": "auto_exact_kernel (histogram + start cell + exact search + scaling, one launch); "
                                      "bytes_algorithmic = 2 B/px once: both planes (ov7670 kinds) or the YUYV frame "
                                      "(webcam line); over_line: against trik_hsv_line_batch on the same geometry"}
    kinds = (("ov7670_object", trik_hsv.AUTO_OV7670_OBJECT), ("ov7670_line", trik_hsv.AUTO_OV7670_LINE),
             ("webcam_line", trik_hsv.AUTO_WEBCAM_LINE))
    for aw, ah in ((320, 240), (W, H)):
        adev = torch.empty(lf * 2 * ah * aw, dtype=torch.uint8, device="cuda")
        aln_ms = None
        for fill, name in ((1, "scene"), (0, "uniform")):
            for kname, kind in kinds:
                lay = trik_hsv.LAYOUT_YUYV if kind == trik_hsv.AUTO_WEBCAM_LINE else trik_hsv.LAYOUT_OV7670
                all_ = 2 * aw if lay == trik_hsv.LAYOUT_YUYV else aw
                trik_hsv.synth(adev, aw, ah, all_, lay, fill, 0x7A1C)
                if aln_ms is None:  # (the first pass: ov7670 scene frames)
                    aln_ms = timed(lambda: trik_hsv.line_batch(adev, aw, ah, aw, 0, 30), stream, args.iters)
                ms = timed(lambda: trik_hsv.batch_auto_range_exact(adev, aw, ah, all_, kind), stream, args.iters)
                sc_ms = timed(lambda: trik_hsv.auto_scores(adev, aw, ah, all_, kind), stream, args.iters)
                nb = lf * 2 * aw * ah
                out["autorange_exact"][f"{aw}x{ah}_{name}_{kname}"] = {
                    "ms": round(ms, 4), "scores_only_ms": round(sc_ms, 4), "Mframes_per_s": round(lf / ms / 1e3, 3),
                    "bytes_algorithmic": nb, "achieved_GBs": round(nb / (ms / 1e3) / 1e9, 1),
                    "hbm_frac": round(nb / (ms / 1e3) / 1e9 / HBM_PEAK_GBS, 4), "line_ms": round(aln_ms, 4),
                    "over_line": round(ms / aln_ms, 2)}
        del adev
    if args.only_autorange:
        det.close()
        print(json.dumps(out))
        return

    lsums, _ = trik_hsv.line_batch(ldev, W, H, W, 0, 30)
    lp_ms = timed(lambda: det.line_preview(ldev, W, H, W, 0, 30, lsums, out_width=OW, out_height=OH,
                                           out_line_length=OLL), stream, args.iters)
    lp_bytes = lf * (H // 2 * 2 * W + OH * OLL)
    out["line_preview"] = {"frames": lf, "ms": round(lp_ms, 4),
                           "achieved_GBs": round(lp_bytes / (lp_ms / 1e3) / 1e9, 1),
                           "hbm_frac": round(lp_bytes / (lp_ms / 1e3) / 1e9 / HBM_PEAK_GBS, 4)}
    RED = (0, 20, 80, 20, 50, 50)
    bl_ms = timed(lambda: det.blob_batch(ldev, W, H, W, RED), stream, args.iters)
    out["blob"] = {"frames": lf, "ms": round(bl_ms, 4), "Mframes_per_s": round(lf / bl_ms / 1e3, 3),
                   "achieved_GBs": round(lf * lfb / (bl_ms / 1e3) / 1e9, 1),
                   "hbm_frac": round(lf * lfb / (bl_ms / 1e3) / 1e9 / HBM_PEAK_GBS, 4),
                   "note": "bitmap (blob_chroma_meta_kernel for large batches, else blob_meta_kernel) + blob_ccl_kernel (one wave per frame)"}
    # the edge-line sensor on the line row's frames (640x480) and on 320x240
    # scene frames with the line sensor beside it: the sums read the Y plane only
    out["edge"] = {"frames": lf,
                   "note": "edge_vec_kernel + edge_targets_kernel; bytes_algorithmic = the Y plane once (1 B/px); "
                           "line_ms: trik_hsv_line_batch on the same frames (both planes); sums_preview: + "
                           "edge_preview_kernel into 320x240 previews"}
    for ew, eh in ((W, H), (320, 240)):
        edev = ldev
        if (ew, eh) != (W, H):
            edev = torch.empty(lf * 2 * eh * ew, dtype=torch.uint8, device="cuda")
            trik_hsv.synth(edev, ew, eh, ew, trik_hsv.LAYOUT_OV7670, 1, 0x7A1C)
        eln_ms = ln_ms if edev is ldev else timed(lambda: trik_hsv.line_batch(edev, ew, eh, ew, 0, 30), stream,
                                                   args.iters)
        ed_ms = timed(lambda: trik_hsv.edge_batch(edev, ew, eh, ew), stream, args.iters)
        esums, _ = trik_hsv.edge_batch(edev, ew, eh, ew)

        def edge_both():
            s, _ = trik_hsv.edge_batch(edev, ew, eh, ew)
            det.edge_preview(edev, ew, eh, ew, s, out_width=OW, out_height=OH, out_line_length=OLL)

        ep_ms = timed(edge_both, stream, args.iters)
        yb = lf * ew * eh
        out["edge"][f"{ew}x{eh}"] = {"ms": round(ed_ms, 4), "Mframes_per_s": round(lf / ed_ms / 1e3, 3),
                                     "bytes_algorithmic": yb, "achieved_GBs": round(yb / (ed_ms / 1e3) / 1e9, 1),
                                     "hbm_frac": round(yb / (ed_ms / 1e3) / 1e9 / HBM_PEAK_GBS, 4),
                                     "line_ms": round(eln_ms, 4),
                                     "line_hbm_frac": round(2 * yb / (eln_ms / 1e3) / 1e9 / HBM_PEAK_GBS, 4),
                                     "over_line": round(ed_ms / eln_ms, 2),
                                     "sums_preview_ms": round(ep_ms, 4),
                                     "points_frame0": int(esums[0, 0])}
        del edev
    # the MxN colour-grid sensor over the same bytes as the line row (scene
    # frames), then over uniform random bytes; colours only, no preview
    out["mxn"] = {"frames": lf, "bytes_algorithmic": lf * lfb,
                  "note": "mxn_hist_kernel, one workgroup per (frame, cell); beside the line row's pass over the "
                          "same planes"}
    ldev_host = ldev[: 8 * lfb].cpu().numpy()
    for kind, name in ((1, "scene"), (0, "uniform")):
        if kind == 0:
            trik_hsv.synth(ldev, W, H, W, trik_hsv.LAYOUT_OV7670, 0, 0x7A1C)
        for m, n in ((3, 3), (10, 10)):
            ms = timed(lambda: det.mxn_batch(ldev, W, H, W, m, n), stream, args.iters)
            out["mxn"][f"{name}_{m}x{n}"] = {"ms": round(ms, 4), "Mframes_per_s": round(lf / ms / 1e3, 3),
                                             "achieved_GBs": round(lf * lfb / (ms / 1e3) / 1e9, 1),
                                             "hbm_frac": round(lf * lfb / (ms / 1e3) / 1e9 / HBM_PEAK_GBS, 4),
                                             "over_line": round(ms / ln_ms, 2)}
    # the JPEG encoder over the same frames: scene, then uniform random bytes;
    # each stream written whole (the capacity is the batch's longest stream)
    out["jpeg"] = {"frames": lf,
                   "note": "jpeg_block / scan / zero / emit / count / sizes / stuff kernels per chunk of frames; "
                           "bytes_algorithmic = both planes + the streams written"}
    jbuf = None
    for kind, name in ((1, "scene"), (0, "uniform")):
        trik_hsv.synth(ldev, W, H, W, trik_hsv.LAYOUT_OV7670, kind, 0x7A1C)
        for q in (100, 50):
            for bw in (False, True):
                _, sizes = det.jpeg_batch(ldev, W, H, W, q, bw, sizes_only=True)
                cap, written = int(sizes.max()), int(sizes.sum(dtype=torch.int64))
                if jbuf is None or jbuf.numel() < lf * cap:
                    jbuf = None
                    jbuf = torch.empty(lf * cap, dtype=torch.uint8, device="cuda")
                view = jbuf[: lf * cap].view(lf, cap)
                ms = timed(lambda: det.jpeg_batch(ldev, W, H, W, q, bw, capacity=cap, out=view), stream, args.iters)
                nbytes = lf * lfb + written
                out["jpeg"][f"{name}_q{q}_{'bw' if bw else 'colour'}"] = {
                    "ms": round(ms, 4), "Mframes_per_s": round(lf / ms / 1e3, 4), "stream_bytes_per_frame": written // lf,
                    "bytes_algorithmic": nbytes, "achieved_GBs": round(nbytes / (ms / 1e3) / 1e9, 1),
                    "hbm_frac": round(nbytes / (ms / 1e3) / 1e9 / HBM_PEAK_GBS, 4), "over_line": round(ms / ln_ms, 2)}
    del jbuf
    del ldev

    s = trik_hsv.ObjectSensor()
    assert s.set_params(W, H, LL) == 0
    host = dev[: H * LL].cpu().numpy()
    prev = np.zeros(OH * OLL, np.uint8)
    for _ in range(3):
        s.process(host, T0, out_buffer=prev, auto_detect=True)
    n = 50
    t0 = time.perf_counter()
    for _ in range(n):
        rc, _ = s.process(host, T0, out_buffer=prev, auto_detect=True)
        assert rc == 0
    dt = (time.perf_counter() - t0) / n
    out["process_single_frame"] = {"ms_per_frame": round(dt * 1e3, 4),
                                   "note": "host frame in, preview + targets + detect* out; "
                                           "PCIe-inclusive, one synchronous call per frame"}
    s.close()
    det.close()
    if not args.no_cpu:
        cpu_baselines(out, dev, ldev_host, W, H, LL, OW, OH, OLL, T0)
    print(json.dumps(out))


def cpu_baselines(out, dev, ldev_host, W, H, LL, OW, OH, OLL, T0):
    """The oracle (C restatement of the reference, one thread) on a few of the
    same frames, per row: ms per frame, beside the GPU's ms per frame."""
    import numpy as np

    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import oracle

    oracle.build()
    n = 8
    fb = H * LL
    frames = dev[: n * fb].cpu().numpy()
    lfb = 2 * H * W
    lframes = ldev_host[: n * lfb]

    def per_frame(fn):
        t0 = time.perf_counter()
        for i in range(n):
            fn(i)
        return (time.perf_counter() - t0) / n * 1e3

    rows = {
        "preview": lambda i: oracle.run(frames[i * fb:(i + 1) * fb], W, H, LL, 0, T0, out_width=OW,
                                        out_height=OH, out_line_length=OLL),
        "auto_range": lambda i: oracle.run(frames[i * fb:(i + 1) * fb], W, H, LL, 0, T0, auto_detect=True,
                                           preview=False),
        "line": lambda i: oracle.line_run(lframes[i * lfb:(i + 1) * lfb], W, H, W, 0, 30, preview=False),
        "blob": lambda i: oracle.blob_run(lframes[i * lfb:(i + 1) * lfb], W, H, W, hsv=(0, 20, 80, 20, 50, 50),
                                          preview=False),
    }
    for k, fn in rows.items():
        ms = per_frame(fn)
        gpu_ms = out[k]["ms"] / out[k]["frames"]
        out[k]["cpu_baseline"] = {"kind": "port", "cores": 1, "ms_per_frame": round(ms, 3),
                                  "sample": f"{n} frames of the same batch, oracle (whole run incl. its "
                                            "per-pixel HSV pass), single thread",
                                  "gpu_ms_per_frame": round(gpu_ms, 6),
                                  "gpu_over_cpu": round(ms / gpu_ms, 1)}


if __name__ == "__main__":
    main()
