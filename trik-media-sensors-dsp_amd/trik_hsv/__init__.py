"""trik_hsv -- host-side mirror of the TRIK object-sensor operator, MI355X-native.

Everything computes in libtrik_hsv.so (HIP kernels for gfx950 + the C++
XDAIS-shaped layer) through its C ABI (include/trik_hsv.h).  PyTorch is used
only to own device memory and streams.  There is no CPU fallback.

Two surfaces, mirroring the reference (paths relative to the reference checkout):
  * ObjectSensor -- the codec instance: create / control / process / delete of
    trik/webcam/object_sensor/src/vidtranscode_cv_fxns.c, one host frame per
    process() call, OutArgs.targetX/targetY/targetSize out.
  * Detector -- the batched device path: N frames resident in HBM, T HSV
    ranges, per-frame per-range {points, sumX, sumY} and targets.
"""
from __future__ import annotations

import ctypes as C
from typing import Iterable, Sequence, Tuple

from . import _abi
from ._abi import (MASK_BITS, MASK_BYTES, CONVERT_HSV_PLANES, CONVERT_RGB888HSV, CONVERT_RGB_PLANES, FORMAT_RGB565X, FORMAT_UNKNOWN, FORMAT_YUV422, FORMAT_YUV422P,  # noqa: F401
                   IALG_EFAIL, IALG_EOK, IVIDTRANSCODE_EFAIL, IVIDTRANSCODE_EOK,
                   IVIDTRANSCODE_EUNSUPPORTED, LAYOUT_OV7670, LAYOUT_YUYV, XDM_FLUSH,
                   XDM_GETBUFINFO, XDM_GETSTATUS, XDM_GETVERSION, XDM_RESET, XDM_SETDEFAULT,
                   XDM_SETPARAMS)

_lib = _abi.load()  # fails loudly when the native library is missing

Range = Tuple[int, int, int, int, int, int]  # hue_from, hue_to, sat_from, sat_to, val_from, val_to


class TrikHsvError(RuntimeError):
    def __init__(self, rc: int, what: str):
        super().__init__(f"{what} failed (rc={rc}): {_abi.last_error()}")
        self.rc = rc


def version() -> str:
    return _lib.trik_hsv_version().decode()


def _ranges(ranges: Iterable[Sequence[int]]):
    rs = [tuple(int(v) for v in r) for r in ranges]
    arr = (_abi.InArgsAlg * max(1, len(rs)))()
    for i, r in enumerate(rs):
        arr[i] = _abi.InArgsAlg(*r[:6], 0)
    return arr, len(rs)


def frame_bytes(width: int, height: int, line_length: int, layout: int) -> int:
    return height * line_length * (2 if layout == LAYOUT_OV7670 else 1)


def _stream_ptr(stream, tensor) -> C.c_void_p:
    """`stream`, or torch's current stream of the device `tensor` lives on."""
    import torch

    s = stream if stream is not None else torch.cuda.current_stream(tensor.device)
    return C.c_void_p(s.cuda_stream)


def _batch(frames, width, height, line_length, layout, n_frames=None, frame_stride=None):
    fb = frame_bytes(width, height, line_length, layout)
    if frame_stride is None:
        frame_stride = fb
    if n_frames is None:
        n_frames = frames.numel() // frame_stride if frame_stride else 0
    if frames.dtype.itemsize != 1 or not frames.is_cuda:
        raise ValueError("frames must be a uint8 CUDA (HIP) tensor")
    if n_frames > 0 and (n_frames - 1) * frame_stride + fb > frames.numel():
        raise ValueError("frames tensor too small for the batch geometry")
    return _abi.FrameBatch(frames.data_ptr(), frame_stride, n_frames, width, height, line_length,
                           layout)


def _ptr(t) -> C.c_void_p:
    """The tensor's device pointer, or NULL for None."""
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _preview_dims(b, out_width, out_height, out_line_length):
    """(out_width, out_height, out_line_length) with their defaults: half the
    frame, two bytes per pixel."""
    ow = b.width // 2 if out_width is None else out_width
    oh = b.height // 2 if out_height is None else out_height
    return ow, oh, 2 * ow if out_line_length is None else out_line_length


def _preview_out(b, frames, out_width, out_height, out_line_length):
    """A preview call's output: (out_width, out_height, out_line_length) with
    their defaults (half the frame, two bytes per pixel) and the previews
    tensor uint8 [N, out_height, out_line_length]; its stride is oh * oll."""
    import torch

    ow, oh, oll = _preview_dims(b, out_width, out_height, out_line_length)
    return ow, oh, oll, torch.empty((b.n_frames, oh, oll), dtype=torch.uint8, device=frames.device)


def _blob_out(frames, lead, width, height, meta, labels):
    """The multi-blob calls' output dict; `lead` = the leading axes, (N,) or (N, T)."""
    import torch

    def new(shape, dtype):
        return torch.empty(lead + shape, dtype=dtype, device=frames.device)

    cells = (height // 4, width // 4)
    return {"targets": new((8, 4), torch.int8), "top": new((8, 3), torch.int32), "n_labels": new((), torch.int32),
            "meta": new(cells, torch.uint8) if meta else None, "labels": new(cells, torch.int16) if labels else None}


HOT_AUTO, HOT_STRIPE, HOT_CHROMA, HOT_GENERIC = 0, 1, 2, 3
HOT_MIXED = 4  # last_hot_kernel(): the call's groups of 4 ranges ran different kernels


class _HotKernel:
    """Hot-kernel selection of one handle (trik_hsv_set_hot_kernel)."""

    def set_hot_kernel(self, kind: int) -> int:
        """HOT_AUTO (the chroma-run kernel for large batches), HOT_STRIPE,
        HOT_CHROMA or HOT_GENERIC for this handle's batched sums.  Returns the
        previous setting.  Results are identical."""
        prev = _lib.trik_hsv_set_hot_kernel(self._h, int(kind))
        if prev < 0:
            raise ValueError(f"unknown hot kernel {kind}")
        return prev

    def last_hot_kernel(self) -> int:
        """The kernel this handle's last hot launch ran."""
        return _lib.trik_hsv_last_hot_kernel(self._h)

    def set_reserved_cus(self, n: int) -> int:
        """CUs the chroma-run kernel leaves free for kernels on other streams
        (trik_hsv_set_reserved_cus).  Returns the previous setting."""
        prev = _lib.trik_hsv_set_reserved_cus(self._h, int(n))
        if prev < 0:
            raise ValueError(f"reserved CUs out of range: {n}")
        return prev


class Detector(_HotKernel):
    """Batched HSV-threshold + centroid over frames resident in device memory.

    Owns one library handle, bound to `device` (default: the current device;
    device tables are compiled per range set and cached).  Methods enqueue on
    `stream` (default: torch's current stream of the frames' device) and do
    not synchronise.
    """

    def __init__(self, device=None, hot: int = HOT_AUTO):
        import torch

        h = C.c_void_p()
        p = _default_params(0)
        with torch.cuda.device(device if device is not None else torch.cuda.current_device()):
            rc = _lib.TRIK_VIDTRANSCODE_CV_create(C.byref(p), C.byref(h))
        if rc != IALG_EOK:
            raise TrikHsvError(rc, "TRIK_VIDTRANSCODE_CV_create")
        self._h = h
        if hot != HOT_AUTO:
            self.set_hot_kernel(hot)

    def close(self):
        if getattr(self, "_h", None):
            _lib.TRIK_VIDTRANSCODE_CV_delete(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def process_batch(self, frames, width, height, line_length, layout, ranges, *, n_frames=None,
                      frame_stride=None, stream=None, sums=None, targets=None):
        """Returns (sums int64 [N,T,3] = points/sumX/sumY, targets int8 [N,T,4] = x/y/size/0)."""
        import torch

        b = _batch(frames, width, height, line_length, layout, n_frames, frame_stride)
        arr, T = _ranges(ranges)
        if sums is None:
            sums = torch.empty((b.n_frames, T, 3), dtype=torch.int64, device=frames.device)
        if targets is None:
            targets = torch.empty((b.n_frames, T, 4), dtype=torch.int8, device=frames.device)
        rc = _lib.trik_hsv_process_batch(self._h, C.byref(b), arr, T, C.c_void_p(sums.data_ptr()),
                                         C.c_void_p(targets.data_ptr()), _stream_ptr(stream, frames))
        if rc:
            raise TrikHsvError(rc, "trik_hsv_process_batch")
        return sums, targets

    def process_batch_totals(self, frames, width, height, line_length, layout, ranges, *, n_frames=None,
                             frame_stride=None, stream=None, sums=None, targets=None, totals=None):
        """The full step (trik_hsv_process_batch_totals): sums, targets and the
        per-target batch totals; one launch per group of 4 ranges where the
        chroma-run kernel runs on >= 4 frames per CU.  Returns (sums, targets,
        totals int64 [T,3])."""
        import torch

        b = _batch(frames, width, height, line_length, layout, n_frames, frame_stride)
        arr, T = _ranges(ranges)
        if sums is None:
            sums = torch.empty((b.n_frames, T, 3), dtype=torch.int64, device=frames.device)
        if targets is None:
            targets = torch.empty((b.n_frames, T, 4), dtype=torch.int8, device=frames.device)
        if totals is None:
            totals = torch.empty((T, 3), dtype=torch.int64, device=frames.device)
        rc = _lib.trik_hsv_process_batch_totals(self._h, C.byref(b), arr, T, C.c_void_p(sums.data_ptr()),
                                                C.c_void_p(targets.data_ptr()), C.c_void_p(totals.data_ptr()),
                                                _stream_ptr(stream, frames))
        if rc:
            raise TrikHsvError(rc, "trik_hsv_process_batch_totals")
        return sums, targets, totals

    def batch_sums(self, frames, width, height, line_length, layout, ranges, sums, *,
                   n_frames=None, frame_stride=None, stream=None):
        """Hot kernel only; ADDS into `sums` (int64 [N,T,3], caller zeroes it)."""
        b = _batch(frames, width, height, line_length, layout, n_frames, frame_stride)
        arr, T = _ranges(ranges)
        rc = _lib.trik_hsv_batch_sums(self._h, C.byref(b), arr, T, C.c_void_p(sums.data_ptr()),
                                      _stream_ptr(stream, frames))
        if rc:
            raise TrikHsvError(rc, "trik_hsv_batch_sums")
        return sums

    def chroma_flagged_share(self) -> float:
        """The chroma-run kernel's expected exact-path word share for the
        current batched-sums range set (-1 before its tables are built)."""
        v = C.c_double()
        rc = _lib.trik_hsv_chroma_share(self._h, C.byref(v))
        if rc:
            raise TrikHsvError(rc, "trik_hsv_chroma_share")
        return v.value

    def chroma_measured_share(self) -> float:
        """The exact-path word share the chroma-run kernel measured on this
        handle's recent AUTO batches of the current range set (-1 unknown)."""
        v = C.c_double()
        rc = _lib.trik_hsv_chroma_measured_share(self._h, C.byref(v))
        if rc:
            raise TrikHsvError(rc, "trik_hsv_chroma_measured_share")
        return v.value

    def batch_masks(self, frames, width, height, line_length, layout, ranges, *, n_frames=None,
                    frame_stride=None, stream=None):
        """Verification mode: returns (masks uint8 [N,H,W], sums int64 [N,T,3])."""
        import torch

        b = _batch(frames, width, height, line_length, layout, n_frames, frame_stride)
        arr, T = _ranges(ranges)
        masks = torch.zeros((b.n_frames, height, width), dtype=torch.uint8, device=frames.device)
        sums = torch.zeros((b.n_frames, T, 3), dtype=torch.int64, device=frames.device)
        rc = _lib.trik_hsv_batch_masks(self._h, C.byref(b), arr, T, C.c_void_p(masks.data_ptr()),
                                       C.c_void_p(sums.data_ptr()), _stream_ptr(stream, frames))
        if rc:
            raise TrikHsvError(rc, "trik_hsv_batch_masks")
        return masks, sums

    def batch_preview(self, frames, width, height, line_length, layout, hsv_range, sums, *,
                      out_width=None, out_height=None, out_line_length=None, n_frames=None,
                      frame_stride=None, sums_pitch=1, stream=None):
        """RGB565X previews (uint8 [N, out_height, out_line_length]) for one range;
        `sums` holds that range's per-frame sums (every `sums_pitch` entries)."""
        b = _batch(frames, width, height, line_length, layout, n_frames, frame_stride)
        ow, oh, oll, previews = _preview_out(b, frames, out_width, out_height, out_line_length)
        arr, _ = _ranges([hsv_range])
        rc = _lib.trik_hsv_batch_preview(self._h, C.byref(b), arr, C.c_void_p(sums.data_ptr()),
                                         sums_pitch, ow, oh, oll, C.c_void_p(previews.data_ptr()),
                                         oh * oll, _stream_ptr(stream, frames))
        if rc:
            raise TrikHsvError(rc, "trik_hsv_batch_preview")
        return previews

    def frame_ranges_preview(self, frames, width, height, line_length, layout, ranges, sums, *, t=0,
                             sums_pitch=None, out_width=None, out_height=None, out_line_length=None,
                             n_frames=None, frame_stride=None, stream=None):
        """RGB565X previews (uint8 [N, out_height, out_line_length]) with an HSV
        range per frame (trik_hsv_frame_ranges_preview): frame f under
        ranges[f, t], a CUDA tensor [N, T, 6] of int16 / uint16 as
        frame_ranges_batch takes it, read by the kernels in stream order.  The
        circle of preview f comes from sums[f * sums_pitch]; `sums` is the sums
        call's tensor [N, T, 3] (entry t is taken, the pitch is T), one row
        per frame [N, 3], or any tensor that starts at frame 0's sums, with
        `sums_pitch` given."""
        import torch

        b = _batch(frames, width, height, line_length, layout, n_frames, frame_stride)
        if (not isinstance(ranges, torch.Tensor) or not ranges.is_cuda or ranges.dtype.itemsize != 2
                or ranges.dtype.is_floating_point or ranges.dim() != 3 or ranges.shape[0] != b.n_frames
                or ranges.shape[2] != 6 or not ranges.is_contiguous()):
            raise ValueError("ranges must be a contiguous CUDA (HIP) tensor [n_frames, T, 6] of int16 or uint16")
        T = ranges.shape[1]
        sums_ptr = sums.data_ptr()
        if sums_pitch is None and tuple(sums.shape) == (b.n_frames, 3) and sums.is_contiguous():
            sums_pitch = 1  # one sums row per frame
        if sums_pitch is None:
            if sums.dim() != 3 or tuple(sums.shape) != (b.n_frames, T, 3) or not sums.is_contiguous():
                raise ValueError("sums must be the contiguous [n_frames, T, 3] tensor of the sums call, or sums_pitch given")
            sums_pitch = T
            if 0 <= t < T:
                sums_ptr += 24 * int(t)
        ow, oh, oll, previews = _preview_out(b, frames, out_width, out_height, out_line_length)
        rc = _lib.trik_hsv_frame_ranges_preview(self._h, C.byref(b), C.c_void_p(ranges.data_ptr()), T, int(t),
                                                C.c_void_p(sums_ptr), sums_pitch, ow, oh, oll,
                                                C.c_void_p(previews.data_ptr()), oh * oll, _stream_ptr(stream, frames))
        if rc:
            raise TrikHsvError(rc, "trik_hsv_frame_ranges_preview")
        return previews

    def blob_batch(self, frames, width, height, line_length, hsv, *, n_frames=None, frame_stride=None,
                   meta=False, labels=False, stream=None):
        """The ov7670 multi-blob sensor over N frames (OSEQ:516-602) for the range
        hsv = (hue, hueTol, sat, satTol, val, valTol).  Returns a dict of device
        tensors: targets int8 [N, 8, 4] (x, y, size, 0), top int32 [N, 8, 3]
        (size, sum_x, sum_y), n_labels int32 [N], and meta uint8 / labels int16
        [N, H/4, W/4] when asked (else meta is the handle's scratch, None here)."""
        b = _batch(frames, width, height, line_length, LAYOUT_OV7670, n_frames, frame_stride)
        out = _blob_out(frames, (b.n_frames,), width, height, meta, labels)
        alg = _abi.OV7670InArgsAlg(1, *[int(v) for v in hsv], 0)
        rc = _lib.trik_hsv_blob_batch(self._h, C.byref(b), C.byref(alg), _ptr(out["targets"]), _ptr(out["top"]),
                                      _ptr(out["meta"]), _ptr(out["labels"]), _ptr(out["n_labels"]),
                                      _stream_ptr(stream, frames))
        if rc:
            raise TrikHsvError(rc, "trik_hsv_blob_batch")
        return out

    def blob_batch_ranges(self, frames, width, height, line_length, ranges, *, layout=LAYOUT_OV7670,
                          n_frames=None, frame_stride=None, meta=False, labels=False, stream=None):
        """The multi-blob sensor over N frames of either layout for T from/to
        ranges per frame (trik_hsv_blob_batch_ranges; blob_range_of converts a
        centre/tolerance range).  Returns blob_batch's dict with a range axis:
        targets int8 [N, T, 8, 4], top int32 [N, T, 8, 3], n_labels int32
        [N, T], and meta uint8 / labels int16 [N, T, H/4, W/4] when asked."""
        b = _batch(frames, width, height, line_length, layout, n_frames, frame_stride)
        arr, T = _ranges(ranges)
        out = _blob_out(frames, (b.n_frames, T), width, height, meta, labels)
        rc = _lib.trik_hsv_blob_batch_ranges(self._h, C.byref(b), arr, T, _ptr(out["targets"]), _ptr(out["top"]),
                                             _ptr(out["meta"]), _ptr(out["labels"]), _ptr(out["n_labels"]),
                                             _stream_ptr(stream, frames))
        if rc:
            raise TrikHsvError(rc, "trik_hsv_blob_batch_ranges")
        return out

    def blob_frame_ranges_batch(self, frames, width, height, line_length, ranges, *, layout=LAYOUT_OV7670,
                                n_frames=None, frame_stride=None, top=False, meta=False, labels=False,
                                stream=None):
        """The multi-blob sensor over N frames of either layout with T from/to
        ranges PER FRAME (trik_hsv_blob_frame_ranges_batch).  `ranges` is a
        contiguous CUDA tensor [N, T, 6] of int16 / uint16 (hue_from, hue_to,
        sat_from, sat_to, val_from, val_to), read by the kernel in stream
        order: what ranges_of_detect writes is taken as it is.  Returns
        blob_batch_ranges' dict, slot (f, t) being frame f under ranges[f, t]:
        targets int8 [N, T, 8, 4], and when asked top int32 [N, T, 8, 3] with
        n_labels int32 [N, T], meta uint8 and labels int16 [N, T, H/4, W/4]
        (None otherwise: the call then gets NULL for them)."""
        b = _batch(frames, width, height, line_length, layout, n_frames, frame_stride)
        if (not ranges.is_cuda or ranges.dtype.itemsize != 2 or ranges.dtype.is_floating_point or ranges.dim() != 3
                or ranges.shape[0] != b.n_frames or ranges.shape[2] != 6 or not ranges.is_contiguous()):
            raise ValueError("ranges must be a contiguous CUDA (HIP) tensor [n_frames, T, 6] of int16 or uint16")
        T = ranges.shape[1]
        out = _blob_out(frames, (b.n_frames, T), width, height, meta, labels)
        if not top:
            out["top"] = out["n_labels"] = None
        rc = _lib.trik_hsv_blob_frame_ranges_batch(self._h, C.byref(b), _ptr(ranges), T, _ptr(out["targets"]),
                                                   _ptr(out["top"]), _ptr(out["meta"]), _ptr(out["labels"]),
                                                   _ptr(out["n_labels"]), _stream_ptr(stream, frames))
        if rc:
            raise TrikHsvError(rc, "trik_hsv_blob_frame_ranges_batch")
        return out

    def blob_preview(self, frames, width, height, line_length, meta, top, *, out_width=None,
                     out_height=None, out_line_length=None, n_frames=None, frame_stride=None, stream=None):
        """Multi-blob previews (uint8 [N, out_height, out_line_length]) from blob_batch's meta and top."""
        b = _batch(frames, width, height, line_length, LAYOUT_OV7670, n_frames, frame_stride)
        ow, oh, oll, previews = _preview_out(b, frames, out_width, out_height, out_line_length)
        rc = _lib.trik_hsv_blob_preview(self._h, C.byref(b), C.c_void_p(meta.data_ptr()),
                                        C.c_void_p(top.data_ptr()), ow, oh, oll,
                                        C.c_void_p(previews.data_ptr()), oh * oll, _stream_ptr(stream, frames))
        if rc:
            raise TrikHsvError(rc, "trik_hsv_blob_preview")
        return previews

    def mxn_batch(self, frames, width, height, line_length, m, n, *, n_frames=None, frame_stride=None,
                  bins=False, stream=None):
        """The ov7670 MxN colour-grid sensor over N frames (MSEQ:576-621): m
        cell rows (InArgs widthM) x n cell columns (heightN).  Returns colors
        int32 [N, m * n] (outColor of each frame), or (colors, bins int16
        [N, m * n] = h << 4 | s << 2 | v of the winning bins) when asked."""
        import torch

        b = _batch(frames, width, height, line_length, LAYOUT_OV7670, n_frames, frame_stride)
        cells = max(int(m) * int(n), 0)
        colors = torch.empty((b.n_frames, cells), dtype=torch.int32, device=frames.device)
        bn = torch.empty((b.n_frames, cells), dtype=torch.int16, device=frames.device) if bins else None
        rc = _lib.trik_hsv_mxn_batch(self._h, C.byref(b), int(m), int(n), C.c_void_p(colors.data_ptr()),
                                     C.c_void_p(bn.data_ptr()) if bins else None, _stream_ptr(stream, frames))
        if rc:
            raise TrikHsvError(rc, "trik_hsv_mxn_batch")
        return (colors, bn) if bins else colors

    def mxn_preview(self, frames, width, height, line_length, m, n, colors, *, out_width=None,
                    out_height=None, out_line_length=None, n_frames=None, frame_stride=None, stream=None):
        """MxN previews (uint8 [N, out_height, out_line_length]) from mxn_batch's colors."""
        b = _batch(frames, width, height, line_length, LAYOUT_OV7670, n_frames, frame_stride)
        ow, oh, oll, previews = _preview_out(b, frames, out_width, out_height, out_line_length)
        rc = _lib.trik_hsv_mxn_preview(self._h, C.byref(b), int(m), int(n), C.c_void_p(colors.data_ptr()),
                                       ow, oh, oll, C.c_void_p(previews.data_ptr()), oh * oll,
                                       _stream_ptr(stream, frames))
        if rc:
            raise TrikHsvError(rc, "trik_hsv_mxn_preview")
        return previews

    def jpeg_batch(self, frames, width, height, line_length, quality, black_and_white=False, *, capacity=None,
                   out_stride=None, n_frames=None, frame_stride=None, coeffs=False, sizes_only=False,
                   out=None, stream=None):
        """The ov7670 JPEG encoder over N frames (JENC:802-852).  Returns
        (streams, sizes[, coeffs]): streams uint8 [N, out_stride] (frame i's
        stream is streams[i, :sizes[i]]; a stream longer than `capacity` is not
        written; None with sizes_only), sizes int32 [N] (always the full
        lengths), coeffs int16 [N, blocks, components, 64] (quantised, zigzag
        order) when asked.  `capacity` defaults to the worst case of the
        geometry; `out` is a caller's uint8 tensor to write into instead of a
        fresh one (its rows are then `out_stride` apart)."""
        import torch

        b = _batch(frames, width, height, line_length, LAYOUT_OV7670, n_frames, frame_stride)
        ncomp = 1 if black_and_white else 3
        blocks = (width // 8) * (height // 8)
        if capacity is None:  # header + every data unit at its longest, every byte stuffed + EOI
            capacity = 608 + 2 * (blocks * ncomp * 208 + 1) + 2
        stride = int(capacity) if out_stride is None else int(out_stride)
        streams = None
        if not sizes_only:
            streams = out if out is not None else torch.empty((b.n_frames, stride), dtype=torch.uint8,
                                                              device=frames.device)
        sizes = torch.empty((b.n_frames,), dtype=torch.int32, device=frames.device)
        co = torch.empty((b.n_frames, blocks, ncomp, 64), dtype=torch.int16, device=frames.device) if coeffs else None
        rc = _lib.trik_hsv_jpeg_batch(self._h, C.byref(b), int(quality), int(bool(black_and_white)),
                                      C.c_void_p(streams.data_ptr()) if streams is not None else None, stride,
                                      int(capacity), C.c_void_p(sizes.data_ptr()),
                                      C.c_void_p(co.data_ptr()) if coeffs else None, _stream_ptr(stream, frames))
        if rc:
            raise TrikHsvError(rc, "trik_hsv_jpeg_batch")
        return (streams, sizes, co) if coeffs else (streams, sizes)

    def line_preview(self, frames, width, height, line_length, val_from, val_to, sums, *,
                     out_width=None, out_height=None, out_line_length=None, n_frames=None,
                     frame_stride=None, stream=None):
        """Line-sensor previews (uint8 [N, out_height, out_line_length]) from the
        per-frame sums of line_batch (LSEQ:283-291, 433-467)."""
        b = _batch(frames, width, height, line_length, LAYOUT_OV7670, n_frames, frame_stride)
        ow, oh, oll, previews = _preview_out(b, frames, out_width, out_height, out_line_length)
        rc = _lib.trik_hsv_line_preview(self._h, C.byref(b), int(val_from), int(val_to),
                                        C.c_void_p(sums.data_ptr()), ow, oh, oll,
                                        C.c_void_p(previews.data_ptr()), oh * oll, _stream_ptr(stream, frames))
        if rc:
            raise TrikHsvError(rc, "trik_hsv_line_preview")
        return previews

    def line_frame_ranges_preview(self, frames, width, height, line_length, layout, ranges, sums, *,
                                  out_width=None, out_height=None, out_line_length=None, n_frames=None,
                                  frame_stride=None, previews=None, preview_stride=None, stream=None):
        """Line-sensor previews (uint8 [N, out_height, out_line_length]) with a V
        range per frame (trik_hsv_line_frame_ranges_preview): LAYOUT_OV7670 is
        the ov7670 line sensor's picture, LAYOUT_YUYV the webcam line sensor's.
        `ranges` is line_frame_ranges_batch's CUDA tensor [N, 6] (or [N, 1, 6])
        of int16 / uint16, entries 4 and 5 read by the kernels in stream order;
        `sums` its sums [N, 3] (int64), whose frame f gives the target line.
        `previews`: a uint8 CUDA tensor to write into instead of a new one,
        preview f at byte f * preview_stride (default out_height *
        out_line_length); it is returned as it is."""
        import torch

        b = _batch(frames, width, height, line_length, layout, n_frames, frame_stride)
        if (not isinstance(ranges, torch.Tensor) or not ranges.is_cuda or ranges.dtype.itemsize != 2
                or ranges.dtype.is_floating_point or not ranges.is_contiguous()
                or tuple(ranges.shape) not in ((b.n_frames, 6), (b.n_frames, 1, 6))):
            raise ValueError("ranges must be a contiguous CUDA (HIP) tensor [n_frames, 6] of int16 or uint16")
        if (not isinstance(sums, torch.Tensor) or not sums.is_cuda or sums.dtype != torch.int64
                or not sums.is_contiguous() or sums.numel() != 3 * b.n_frames):
            raise ValueError("sums must be a contiguous CUDA (HIP) int64 tensor [n_frames, 3]")
        ow, oh, oll = _preview_dims(b, out_width, out_height, out_line_length)
        stride = oh * oll if preview_stride is None else int(preview_stride)
        if previews is None:
            if stride != oh * oll:
                raise ValueError("preview_stride needs the previews tensor it strides over")
            previews = torch.empty((b.n_frames, oh, oll), dtype=torch.uint8, device=frames.device)
        else:
            need = (b.n_frames - 1) * stride + oh * oll if b.n_frames > 0 else 0
            if (not isinstance(previews, torch.Tensor) or not previews.is_cuda or previews.dtype != torch.uint8
                    or not previews.is_contiguous() or stride < oh * oll or previews.numel() < need):
                raise ValueError("previews must be a contiguous CUDA (HIP) uint8 tensor of at least "
                                 "(n_frames - 1) * preview_stride + out_height * out_line_length bytes")
        rc = _lib.trik_hsv_line_frame_ranges_preview(self._h, C.byref(b), C.c_void_p(ranges.data_ptr()),
                                                     C.c_void_p(sums.data_ptr()), ow, oh, oll,
                                                     C.c_void_p(previews.data_ptr()), stride,
                                                     _stream_ptr(stream, frames))
        if rc:
            raise TrikHsvError(rc, "trik_hsv_line_frame_ranges_preview")
        return previews


    def edge_preview(self, frames, width, height, line_length, sums, threshold=50, *, out_width=None,
                     out_height=None, out_line_length=None, n_frames=None, frame_stride=None, stream=None):
        """Edge-line previews (uint8 [N, out_height, out_line_length], native
        uint16 RGB565 pixels) from edge_batch's sums and the same threshold."""
        b = _batch(frames, width, height, line_length, LAYOUT_OV7670, n_frames, frame_stride)
        ow, oh, oll, previews = _preview_out(b, frames, out_width, out_height, out_line_length)
        rc = _lib.trik_hsv_edge_preview(self._h, C.byref(b), int(threshold), C.c_void_p(sums.data_ptr()), ow, oh,
                                        oll, C.c_void_p(previews.data_ptr()), oh * oll,
                                        _stream_ptr(stream, frames))
        if rc:
            raise TrikHsvError(rc, "trik_hsv_edge_preview")
        return previews


def line_batch(frames, width, height, line_length, val_from, val_to, *, band=None, n_frames=None,
               frame_stride=None, stream=None):
    """The ov7670 line sensor over N frames (LSEQ:376-476): sums int64 [N, 3] =
    {points, sum_x, cross points} and targets int8 [N, 4] (targetX, targetY =
    cross size, targetSize).  `band` = the cross-point rows (default: the
    reference's steady state H/2 .. H/2+80)."""
    import torch

    b = _batch(frames, width, height, line_length, LAYOUT_OV7670, n_frames, frame_stride)
    band = (height // 2, height // 2 + 80) if band is None else band
    sums = torch.empty((b.n_frames, 3), dtype=torch.int64, device=frames.device)
    targets = torch.empty((b.n_frames, 4), dtype=torch.int8, device=frames.device)
    rc = _lib.trik_hsv_line_batch(C.byref(b), int(val_from), int(val_to), int(band[0]), int(band[1]),
                                  C.c_void_p(sums.data_ptr()), C.c_void_p(targets.data_ptr()),
                                  _stream_ptr(stream, frames))
    if rc:
        raise TrikHsvError(rc, "trik_hsv_line_batch")
    return sums, targets


def line_scale_val(percent: int) -> int:
    """The byte a line sensor compares V with for a percent bound
    (trik_hsv_line_scale_val, host code): clamp(percent * 255 / 100, 0, 255)."""
    return int(_lib.trik_hsv_line_scale_val(int(percent)))


def line_frame_ranges_batch(frames, width, height, line_length, layout, ranges, *, band=None, n_frames=None,
                            frame_stride=None, targets=True, stream=None):
    """The line sensors with a V range per frame, read on the device
    (trik_hsv_line_frame_ranges_batch).  LAYOUT_OV7670: the ov7670 line
    sensor, sums int64 [N, 3] = {points, sum_x, cross points} as line_batch
    gives them frame by frame; LAYOUT_YUYV: the webcam line sensor, {points,
    sum_x, sum_y} over every column and row (`band` unused).  `ranges` is a
    CUDA tensor [N, 6] (or [N, 1, 6], as ranges_of_detect returns it) of int16 /
    uint16 whose entries 4 and 5 are valFrom and valTo in percent: used as it
    is, never copied, read by the kernel in stream order.  Or one (val_from,
    val_to) pair for every frame, or a sequence of N pairs, expanded into such
    a tensor on the stream.  Returns (sums, targets int8 [N, 4]); targets is
    None with targets=False."""
    import torch

    b = _batch(frames, width, height, line_length, layout, n_frames, frame_stride)
    s = stream if stream is not None else torch.cuda.current_stream(frames.device)
    if not isinstance(ranges, torch.Tensor):
        pairs = torch.tensor(ranges, dtype=torch.int32).reshape(-1, 2)
        if pairs.shape[0] == 1:
            pairs = pairs.expand(b.n_frames, 2)
        if pairs.shape[0] != b.n_frames:
            raise ValueError("ranges: one (val_from, val_to) pair, or one per frame")
        host = torch.zeros((b.n_frames, 6), dtype=torch.int32)
        host[:, 4:] = pairs
        with torch.cuda.stream(s):
            ranges = host.to(torch.int16).pin_memory().to(frames.device, non_blocking=True)  # (uint16 bits)
    if (not ranges.is_cuda or ranges.dtype.itemsize != 2 or ranges.dtype.is_floating_point
            or ranges.shape not in ((b.n_frames, 6), (b.n_frames, 1, 6)) or not ranges.is_contiguous()):
        raise ValueError("ranges must be a contiguous CUDA (HIP) tensor [n_frames, 6] of int16 or uint16")
    band = (height // 2, height // 2 + 80) if band is None else band
    sums = torch.empty((b.n_frames, 3), dtype=torch.int64, device=frames.device)
    tg = torch.empty((b.n_frames, 4), dtype=torch.int8, device=frames.device) if targets else None
    rc = _lib.trik_hsv_line_frame_ranges_batch(C.byref(b), C.c_void_p(ranges.data_ptr()), int(band[0]), int(band[1]),
                                               C.c_void_p(sums.data_ptr()), _ptr(tg), C.c_void_p(s.cuda_stream))
    if rc:
        raise TrikHsvError(rc, "trik_hsv_line_frame_ranges_batch")
    return sums, tg


def frame_ranges_batch(frames, width, height, line_length, layout, ranges, *, n_frames=None, frame_stride=None,
                       stream=None, sums=None, targets=None):
    """The object sensor with HSV ranges per frame (trik_hsv_frame_ranges_batch):
    returns (sums int64 [N,T,3], targets int8 [N,T,4]) as process_batch does,
    frame f under ranges[f].  `ranges` is a CUDA tensor [N,T,6] of int16 /
    uint16 (hue_from, hue_to, sat_from, sat_to, val_from, val_to), read by the
    kernel in stream order, or a host sequence [N][T][6], uploaded on the
    stream."""
    import torch

    b = _batch(frames, width, height, line_length, layout, n_frames, frame_stride)
    s = stream if stream is not None else torch.cuda.current_stream(frames.device)
    if not isinstance(ranges, torch.Tensor):
        host = torch.tensor(ranges, dtype=torch.int32).to(torch.int16)  # (uint16 bits)
        host = host.reshape(0, 1, 6) if host.numel() == 0 else host
        with torch.cuda.stream(s):
            ranges = host.pin_memory().to(frames.device, non_blocking=True)
    if (not ranges.is_cuda or ranges.dtype.itemsize != 2 or ranges.dtype.is_floating_point or ranges.dim() != 3
            or ranges.shape[0] != b.n_frames or ranges.shape[2] != 6 or not ranges.is_contiguous()):
        raise ValueError("ranges must be a contiguous CUDA (HIP) tensor [n_frames, T, 6] of int16 or uint16")
    T = ranges.shape[1]
    if sums is None:
        sums = torch.empty((b.n_frames, T, 3), dtype=torch.int64, device=frames.device)
    if targets is None:
        targets = torch.empty((b.n_frames, T, 4), dtype=torch.int8, device=frames.device)
    rc = _lib.trik_hsv_frame_ranges_batch(C.byref(b), C.c_void_p(ranges.data_ptr()), T, C.c_void_p(sums.data_ptr()),
                                          C.c_void_p(targets.data_ptr()), C.c_void_p(s.cuda_stream))
    if rc:
        raise TrikHsvError(rc, "trik_hsv_frame_ranges_batch")
    return sums, targets


def convert_batch(frames, width, height, line_length, layout, form=CONVERT_HSV_PLANES, *, out=None, n_frames=None,
                  frame_stride=None, stream=None):
    """The reference's RGB888/HSV image of every frame (trik_hsv_convert_batch),
    bit for bit.  CONVERT_RGB888HSV: int64 [N, H, W], each value the
    s_rgb888hsv entry 0x00RRGGBB << 32 | 0x00VVSSHH.  CONVERT_HSV_PLANES /
    CONVERT_RGB_PLANES: uint8 [N, 3, H, W], planes H, S, V / R, G, B.  Returns
    a dense tensor it allocates, or fills `out` (a CUDA tensor of that shape and
    dtype whose last axis is contiguous; its other strides are taken as they
    are, and the elements between its rows, planes and frames are not
    written)."""
    import torch

    b = _batch(frames, width, height, line_length, layout, n_frames, frame_stride)
    planes = form != CONVERT_RGB888HSV
    shape = (b.n_frames, 3, height, width) if planes else (b.n_frames, height, width)
    dtype = torch.uint8 if planes else torch.int64
    if out is None:
        out = torch.empty(shape, dtype=dtype, device=frames.device)
    elif not out.is_cuda or out.dtype != dtype or tuple(out.shape) != shape or (width > 1 and out.stride(-1) != 1):
        raise ValueError(f"out must be a CUDA (HIP) {dtype} tensor of shape {shape} with a contiguous last axis")
    if out.numel() == 0:  # no frame or no pixel: the call writes nothing (and an empty tensor has no address)
        return out
    item = out.element_size()
    st = [s * item for s in out.stride()]
    # (the stride of an axis of length 0 or 1 addresses nothing: the dense one stands for it)
    row = st[-2] if height > 1 else width * item
    plane = (st[1] if planes else 0)
    frame = st[0] if b.n_frames > 1 else (2 * plane if planes else 0) + height * row
    o = _abi.ConvertOut(out.data_ptr(), frame, plane, row, int(form))
    rc = _lib.trik_hsv_convert_batch(C.byref(b), C.byref(o), _stream_ptr(stream, frames))
    if rc:
        raise TrikHsvError(rc, "trik_hsv_convert_batch")
    return out


def mask_batch(frames, width, height, line_length, layout, ranges, form=MASK_BITS, *, out=None, n_frames=None,
               frame_stride=None, stream=None):
    """The per-pixel detection mask of every frame (trik_hsv_mask_batch), bit for
    bit the reference's detectHsvPixel: uint8 [N, T, H, W // 8] for MASK_BITS
    (pixel c is bit c & 7 of byte c >> 3 of its row, least significant first)
    or [N, T, H, W] for MASK_BYTES (0xFF detected, 0x00 not), plane t under
    range t.  `ranges` is a CUDA tensor of int16 / uint16 read by the kernel in
    stream order and never copied: [T, 6] is one set shared by every frame,
    [N, T, 6] a set per frame (frame_ranges_batch's and ranges_of_detect's
    buffer; its first stride may be larger than 6 T, the other axes
    contiguous).  A host sequence [T][6] or [N][T][6] is uploaded on the
    stream.  Returns a dense tensor it allocates, or fills `out` (a CUDA uint8
    tensor of that shape whose last axis is contiguous; its other strides are
    taken as they are, and the elements between its rows, planes and frames
    are not written)."""
    import torch

    b = _batch(frames, width, height, line_length, layout, n_frames, frame_stride)
    s = stream if stream is not None else torch.cuda.current_stream(frames.device)
    if not isinstance(ranges, torch.Tensor):
        host = torch.tensor(ranges, dtype=torch.int32).to(torch.int16)  # (uint16 bits)
        with torch.cuda.stream(s):
            ranges = host.pin_memory().to(frames.device, non_blocking=True)
    if (not ranges.is_cuda or ranges.dtype.itemsize != 2 or ranges.dtype.is_floating_point or ranges.dim() not in (2, 3)
            or ranges.shape[-1] != 6 or ranges.shape[-2] < 1 or ranges.stride(-1) != 1 or ranges.stride(-2) != 6
            or (ranges.dim() == 3 and ranges.shape[0] != b.n_frames)):
        raise ValueError("ranges must be a CUDA (HIP) tensor [T, 6] or [n_frames, T, 6] of int16 or uint16 "
                         "with contiguous tuples")
    T = ranges.shape[-2]
    ranges_stride = 0 if ranges.dim() == 2 else (ranges.stride(0) if b.n_frames > 1 else 6 * T)
    row_bytes = width // 8 if form == MASK_BITS else width
    shape = (b.n_frames, T, height, row_bytes)
    if out is None:
        out = torch.empty(shape, dtype=torch.uint8, device=frames.device)
    elif not out.is_cuda or out.dtype != torch.uint8 or tuple(out.shape) != shape or (row_bytes > 1 and out.stride(-1) != 1):
        raise ValueError(f"out must be a CUDA (HIP) uint8 tensor of shape {shape} with a contiguous last axis")
    if out.numel() == 0:  # no frame or no pixel: the call writes nothing (and an empty tensor has no address)
        return out
    st = out.stride()
    # (the stride of an axis of length 1 addresses nothing: the dense one stands for it)
    row = st[2] if height > 1 else row_bytes
    plane = st[1] if T > 1 else height * row
    frame = st[0] if b.n_frames > 1 else (T - 1) * plane + height * row
    o = _abi.MaskOut(out.data_ptr(), frame, plane, row, int(form))
    rc = _lib.trik_hsv_mask_batch(C.byref(b), C.c_void_p(ranges.data_ptr()), T, ranges_stride, C.byref(o),
                                  C.c_void_p(s.cuda_stream))
    if rc:
        raise TrikHsvError(rc, "trik_hsv_mask_batch")
    return out


def ranges_of_detect(detect, *, ranges=None, n_ranges=1, t=0, stream=None):
    """detect [N,6] (hue, hueTol, sat, satTol, val, valTol: batch_auto_range's
    or batch_auto_range_exact's output, on the device) -> entry t of each
    frame's ranges, from/to form (trik_hsv_ranges_of_detect).  Returns the
    ranges tensor int16 [N, n_ranges, 6]: `ranges`, or a new one (zeros but for
    entry t)."""
    import torch

    if not detect.is_cuda or detect.dtype.itemsize != 2 or detect.dim() != 2 or detect.shape[1] != 6 \
            or not detect.is_contiguous():
        raise ValueError("detect must be a contiguous CUDA (HIP) tensor [N, 6] of int16 or uint16")
    n = detect.shape[0]
    s = stream if stream is not None else torch.cuda.current_stream(detect.device)
    if ranges is None:
        with torch.cuda.stream(s):
            ranges = torch.zeros((n, n_ranges, 6), dtype=torch.int16, device=detect.device)
    elif (not ranges.is_cuda or ranges.dtype.itemsize != 2 or ranges.dim() != 3 or ranges.shape[0] != n
          or ranges.shape[2] != 6 or not ranges.is_contiguous()):
        raise ValueError("ranges must be a contiguous CUDA (HIP) tensor [N, T, 6] of int16 or uint16")
    rc = _lib.trik_hsv_ranges_of_detect(C.c_void_p(detect.data_ptr()), n, C.c_void_p(ranges.data_ptr()),
                                        ranges.shape[1], int(t), C.c_void_p(s.cuda_stream))
    if rc:
        raise TrikHsvError(rc, "trik_hsv_ranges_of_detect")
    return ranges


def edge_batch(frames, width, height, line_length, threshold=50, *, edges=False, n_frames=None,
               frame_stride=None, stream=None):
    """The ov7670 edge-line sensor over N frames (ESEQ:154-205, 397-417): sums
    int64 [N, 3] = {points, sum_x, 0} and targets int8 [N, 4] (targetX,
    targetY, targetSize); with `edges`, also the thresholded Sobel map uint8
    [N, height, width].  line_length must equal width."""
    import torch

    b = _batch(frames, width, height, line_length, LAYOUT_OV7670, n_frames, frame_stride)
    sums = torch.empty((b.n_frames, 3), dtype=torch.int64, device=frames.device)
    targets = torch.empty((b.n_frames, 4), dtype=torch.int8, device=frames.device)
    emap = torch.empty((b.n_frames, height, width), dtype=torch.uint8, device=frames.device) if edges else None
    rc = _lib.trik_hsv_edge_batch(C.byref(b), int(threshold), C.c_void_p(sums.data_ptr()),
                                  C.c_void_p(targets.data_ptr()), C.c_void_p(emap.data_ptr()) if edges else None,
                                  _stream_ptr(stream, frames))
    if rc:
        raise TrikHsvError(rc, "trik_hsv_edge_batch")
    return (sums, targets, emap) if edges else (sums, targets)


def edge_targets(points: int, sum_x: int, width: int, height: int) -> Tuple[int, int, int]:
    """The edge-line sensor's (targetX, targetY, targetSize) of one frame's
    sums: trik_hsv_edge_targets, host code."""
    s = _abi.TargetSums(int(points), int(sum_x), 0)
    t = _abi.Target()
    rc = _lib.trik_hsv_edge_targets(C.byref(s), int(width), int(height), C.byref(t))
    if rc:
        raise TrikHsvError(rc, "trik_hsv_edge_targets")
    return int(t.x), int(t.y), int(t.size)


def mxn_color(h: int, s: int, v: int) -> int:
    """The MxN sensor's 0x00RRGGBB colour of histogram bin (h 0..31, s 0..3,
    v 0..3): trik_hsv_mxn_color, host code."""
    return int(_lib.trik_hsv_mxn_color(int(h), int(s), int(v)))


def jpeg_header(quality: int, black_and_white: bool, width: int, height: int) -> bytes:
    """The JPEG encoder's header (SOI .. SOS) for a width x height frame:
    trik_hsv_jpeg_header, host code."""
    buf = (C.c_uint8 * 608)()
    n = int(_lib.trik_hsv_jpeg_header(int(quality), int(bool(black_and_white)), int(width), int(height), buf, 608))
    if n <= 0:
        raise TrikHsvError(IVIDTRANSCODE_EFAIL, "trik_hsv_jpeg_header")
    return bytes(buf[:n])


def batch_auto_range(frames, width, height, line_length, layout, *, n_frames=None,
                     frame_stride=None, stream=None):
    """autoDetectHsv per frame: uint16 [N, 6] = hue, hueTol, sat, satTol, val, valTol."""
    import torch

    b = _batch(frames, width, height, line_length, layout, n_frames, frame_stride)
    out = torch.empty((b.n_frames, 6), dtype=torch.int16, device=frames.device)
    rc = _lib.trik_hsv_batch_auto_range(C.byref(b), C.c_void_p(out.data_ptr()), _stream_ptr(stream, frames))
    if rc:
        raise TrikHsvError(rc, "trik_hsv_batch_auto_range")
    return out


# the detectors behind trik_hsv_auto_scores / trik_hsv_batch_auto_range_exact
AUTO_OV7670_OBJECT, AUTO_OV7670_LINE, AUTO_WEBCAM_LINE = 0, 1, 2
AUTO_MAX_SIDE = 2048


def _auto_layout(kind: int) -> int:
    return LAYOUT_YUYV if kind == AUTO_WEBCAM_LINE else LAYOUT_OV7670


def auto_bins(kind: int) -> int:
    """Bins of a kind's score histogram: 32 x 32 (H >> 3, S >> 3) or 256 (V)."""
    return 1024 if kind == AUTO_OV7670_OBJECT else 256


def auto_scores(frames, width, height, line_length, kind, *, n_frames=None, frame_stride=None, stream=None):
    """The deterministic half of the ov7670 object sensor's and the line
    sensors' autoDetectHsv (trik_hsv_auto_scores): the detector's final score
    histogram int32 [N, bins] and start int32 [N, 4] = the start cell's h (or
    v), s (or 0), max_value, 0."""
    import torch

    b = _batch(frames, width, height, line_length, _auto_layout(kind), n_frames, frame_stride)
    scores = torch.empty((b.n_frames, auto_bins(kind)), dtype=torch.int32, device=frames.device)
    start = torch.empty((b.n_frames, 4), dtype=torch.int32, device=frames.device)
    rc = _lib.trik_hsv_auto_scores(C.byref(b), int(kind), C.c_void_p(scores.data_ptr()),
                                   C.c_void_p(start.data_ptr()), _stream_ptr(stream, frames))
    if rc:
        raise TrikHsvError(rc, "trik_hsv_auto_scores")
    return scores, start


def batch_auto_range_exact(frames, width, height, line_length, kind, *, n_frames=None, frame_stride=None,
                           stream=None):
    """autoDetectHsv per frame by the exact search (trik_hsv_batch_auto_range_exact):
    out int16 [N, 6] = hue, hueTol, sat, satTol, val, valTol (uint16 bits) and
    best int32 [N, 5] = the maximum L and its box h1, h2, s1, s2 (v0, v1, 0, 0
    for the line kinds)."""
    import torch

    b = _batch(frames, width, height, line_length, _auto_layout(kind), n_frames, frame_stride)
    out = torch.empty((b.n_frames, 6), dtype=torch.int16, device=frames.device)
    best = torch.empty((b.n_frames, 5), dtype=torch.int32, device=frames.device)
    rc = _lib.trik_hsv_batch_auto_range_exact(C.byref(b), int(kind), C.c_void_p(out.data_ptr()),
                                              C.c_void_p(best.data_ptr()), _stream_ptr(stream, frames))
    if rc:
        raise TrikHsvError(rc, "trik_hsv_batch_auto_range_exact")
    return out, best


def auto_range_of(kind: int, h1: int, h2: int, s1: int = 0, s2: int = 0) -> Tuple[int, ...]:
    """The detectors' output scaling of a box (line kinds: v0, v1 as h1, h2):
    (hue, hueTol, sat, satTol, val, valTol).  trik_hsv_auto_range_of, host code."""
    out = (C.c_uint16 * 6)()
    rc = _lib.trik_hsv_auto_range_of(int(kind), int(h1), int(h2), int(s1), int(s2), out)
    if rc:
        raise TrikHsvError(rc, "trik_hsv_auto_range_of")
    return tuple(int(v) for v in out)


BLOB_CHUNK_SLOTS = _abi.BLOB_CHUNK_SLOTS  # (frame, range) slots per chunk of blob_batch_ranges


def blob_range_of(hsv: Sequence[int]) -> Range:
    """The from/to range blob_batch uses for hsv = (hue, hueTol, sat, satTol,
    val, valTol) (BMB:110-130), as blob_batch_ranges and process_batch take
    it.  trik_hsv_blob_range_of, host code."""
    alg = _abi.OV7670InArgsAlg(1, *[int(v) for v in hsv], 0)
    out = _abi.InArgsAlg()
    rc = _lib.trik_hsv_blob_range_of(C.byref(alg), C.byref(out))
    if rc:
        raise TrikHsvError(rc, "trik_hsv_blob_range_of")
    return (out.detectHueFrom, out.detectHueTo, out.detectSatFrom, out.detectSatTo, out.detectValFrom,
            out.detectValTo)


def batch_targets(sums, width, height, *, stream=None):
    """Epilogue only: sums int64 [N,T,3] -> targets int8 [N,T,4]."""
    import torch

    N, T = sums.shape[0], sums.shape[1]
    targets = torch.empty((N, T, 4), dtype=torch.int8, device=sums.device)
    b = _abi.FrameBatch(None, 0, N, width, height, 2 * width, LAYOUT_YUYV)
    rc = _lib.trik_hsv_batch_targets(C.byref(b), T, C.c_void_p(sums.data_ptr()),
                                     C.c_void_p(targets.data_ptr()), _stream_ptr(stream, sums))
    if rc:
        raise TrikHsvError(rc, "trik_hsv_batch_targets")
    return targets


def batch_totals_device(sums, *, stream=None):
    """Per-target batch totals on the device (trik_hsv_batch_totals):
    sums int64 [N,T,3] -> [T,3]."""
    import torch

    N, T = sums.shape[0], sums.shape[1]
    totals = torch.empty((T, 3), dtype=torch.int64, device=sums.device)
    rc = _lib.trik_hsv_batch_totals(N, T, C.c_void_p(sums.data_ptr()), C.c_void_p(totals.data_ptr()),
                                    _stream_ptr(stream, sums))
    if rc:
        raise TrikHsvError(rc, "trik_hsv_batch_totals")
    return totals


class Group:
    """One process driving several GPUs through the C ABI's group
    (trik_hsv_group_*): a handle, a stream and a host worker thread per
    device, and one RCCL all-reduce of the per-target totals."""

    def __init__(self, devices):
        self.devices = [int(d) for d in devices]
        arr = (C.c_int32 * len(self.devices))(*self.devices)
        h = C.c_void_p()
        rc = _lib.trik_hsv_group_create(len(self.devices), arr, C.byref(h))
        if rc:
            raise TrikHsvError(rc, "trik_hsv_group_create")
        self._h = h

    def process(self, shards, width, height, line_length, layout, ranges):
        """shards[d]: (frames tensor on devices[d], n_frames).  Returns per
        device (sums [n,T,3], targets [n,T,4], totals [T,3]) -- enqueued on the
        group's streams; call sync() before reading them."""
        import torch

        n = len(self.devices)
        if len(shards) != n:
            raise ValueError("one shard per device")
        arr, T = _ranges(ranges)
        batches = (_abi.FrameBatch * n)()
        out, keep = [], []
        for d, (frames, nf) in enumerate(shards):
            dev = torch.device("cuda", self.devices[d])
            batches[d] = _batch(frames, width, height, line_length, layout, nf)
            sums = torch.zeros((max(nf, 0), T, 3), dtype=torch.int64, device=dev)
            targets = torch.zeros((max(nf, 0), T, 4), dtype=torch.int8, device=dev)
            totals = torch.zeros((T, 3), dtype=torch.int64, device=dev)
            out.append((sums, targets, totals))
        torch.cuda.synchronize()  # the allocations above ran on torch's streams
        ptrs = [(C.c_void_p * n)(*[C.c_void_p(o[k].data_ptr()) for o in out]) for k in range(3)]
        rc = _lib.trik_hsv_group_process(self._h, batches, arr, T, ptrs[0], ptrs[1], ptrs[2])
        if rc:
            raise TrikHsvError(rc, "trik_hsv_group_process")
        self._keep = (batches, ptrs, out)
        return out

    def sync(self):
        rc = _lib.trik_hsv_group_sync(self._h)
        if rc:
            raise TrikHsvError(rc, "trik_hsv_group_sync")

    def close(self):
        if getattr(self, "_h", None):
            _lib.trik_hsv_group_delete(self._h)
            self._h = None

    def __del__(self):
        self.close()


COMM_ID_BYTES = 128  # TRIK_HSV_COMM_ID_BYTES (= NCCL_UNIQUE_ID_BYTES)


def comm_id() -> bytes:
    """A fresh communicator id (rank 0 makes it; every rank passes the same
    bytes to Comm): trik_hsv_comm_id."""
    buf = (C.c_uint8 * COMM_ID_BYTES)()
    rc = _lib.trik_hsv_comm_id(buf)
    if rc:
        raise TrikHsvError(rc, "trik_hsv_comm_id")
    return bytes(buf)


class Comm:
    """One process per GPU: the library's own RCCL communicator over the ranks
    (trik_hsv_comm_create on the current device) and its one collective, the
    sum of the per-target totals (trik_hsv_comm_all_reduce_totals) -- the call
    a C++ host links, not torch.distributed's."""

    def __init__(self, n_ranks: int, rank: int, uid: bytes):
        if len(uid) != COMM_ID_BYTES:
            raise ValueError(f"comm id must be {COMM_ID_BYTES} bytes")
        buf = (C.c_uint8 * COMM_ID_BYTES).from_buffer_copy(uid)
        h = C.c_void_p()
        rc = _lib.trik_hsv_comm_create(int(n_ranks), int(rank), buf, C.byref(h))
        if rc:
            raise TrikHsvError(rc, "trik_hsv_comm_create")
        self._h = h
        self.n_ranks, self.rank = int(n_ranks), int(rank)

    def all_reduce_totals(self, totals, *, stream=None):
        """Sum totals [T, 3] int64 (device) over the ranks in place, enqueued
        on `stream` (default: torch's current stream)."""
        import torch

        if totals.dtype != torch.int64 or totals.dim() != 2 or totals.shape[1] != 3 or not totals.is_contiguous():
            raise ValueError("totals must be a contiguous [T, 3] int64 device tensor")
        rc = _lib.trik_hsv_comm_all_reduce_totals(self._h, C.c_void_p(totals.data_ptr()), int(totals.shape[0]),
                                                  _stream_ptr(stream, totals))
        if rc:
            raise TrikHsvError(rc, "trik_hsv_comm_all_reduce_totals")
        return totals

    def close(self):
        if getattr(self, "_h", None):
            _lib.trik_hsv_comm_delete(self._h)
            self._h = None

    def __del__(self):
        self.close()


def synth(frames, width, height, line_length, layout, kind, seed, *, first_frame=0, n_frames=None,
          frame_stride=None, stream=None):
    """Fill a uint8 device tensor with synthetic frames (kind 0 uniform, 1 scene)."""
    b = _batch(frames, width, height, line_length, layout, n_frames, frame_stride)
    rc = _lib.trik_hsv_synth(C.byref(b), first_frame, kind, seed, _stream_ptr(stream, frames))
    if rc:
        raise TrikHsvError(rc, "trik_hsv_synth")
    return frames


# ---------------------------------------------------------------------------
# ObjectSensor: the codec instance (XDAIS quartet)
# ---------------------------------------------------------------------------
def _default_params(num_output_streams=1, fmt_in=FORMAT_YUV422, max_w=640, max_h=480):
    """TRIK_VIDTRANSCODE_CV_Params defaults (WGLUE:153-184), caps adjustable."""
    p = _abi.Params()
    b = p.base
    b.size = C.sizeof(_abi.Params)
    b.numOutputStreams = num_output_streams
    b.formatInput = fmt_in
    b.formatOutput[0], b.formatOutput[1] = (FORMAT_RGB565X if num_output_streams else FORMAT_UNKNOWN,
                                            FORMAT_UNKNOWN)
    b.maxHeightInput, b.maxWidthInput, b.maxFrameRateInput, b.maxBitRateInput = max_h, max_w, 60000, -1
    b.maxHeightOutput[0], b.maxHeightOutput[1] = max_h, -1
    b.maxWidthOutput[0], b.maxWidthOutput[1] = max_w, -1
    b.maxFrameRateOutput[0] = b.maxFrameRateOutput[1] = -1
    b.maxBitRateOutput[0] = b.maxBitRateOutput[1] = -1
    b.dataEndianness = 1
    if num_output_streams == 0:  # caps checks still read index 0
        b.maxHeightOutput[0], b.maxWidthOutput[0] = max_h, max_w
    return p


def dynamic_params(width, height, line_length, out_width=320, out_height=240, out_line_length=640):
    d = _abi.DynamicParams()
    d.base.size = C.sizeof(_abi.DynamicParams)
    d.base.keepInputResolutionFlag[1] = 1
    d.base.outputHeight[0], d.base.outputWidth[0] = out_height, out_width
    d.base.keepInputFrameRateFlag[0] = d.base.keepInputFrameRateFlag[1] = 1
    d.base.inputFrameRate = -1
    d.base.forceFrame[0] = d.base.forceFrame[1] = -1
    d.inputHeight, d.inputWidth, d.inputLineLength = height, width, line_length
    d.outputLineLength[0], d.outputLineLength[1] = out_line_length, -1
    return d


class ObjectSensor(_HotKernel):
    """One TRIK_VIDTRANSCODE_CV codec instance (vidtranscode_cv_fxns.c)."""

    _create = "TRIK_VIDTRANSCODE_CV_create"

    def __init__(self, params: _abi.Params | None = None):
        h = C.c_void_p()
        rc = getattr(_lib, self._create)(C.byref(params) if params is not None else None, C.byref(h))
        if rc != IALG_EOK:
            raise TrikHsvError(rc, self._create)
        self._h = h
        self.params = params if params is not None else _default_params(1)

    def close(self):
        if getattr(self, "_h", None):
            _lib.TRIK_VIDTRANSCODE_CV_delete(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def control(self, cmd: int, dyn: _abi.DynamicParams | None = None,
                status: _abi.Status | None = None):
        st = status if status is not None else _abi.Status()
        rc = _lib.TRIK_VIDTRANSCODE_CV_control(self._h, cmd, C.byref(dyn) if dyn is not None else None,
                                               C.byref(st))
        return rc, st

    def set_params(self, width, height, line_length, **kw) -> int:
        rc, _ = self.control(XDM_SETPARAMS, dynamic_params(width, height, line_length, **kw))
        return rc

    def process(self, frame, hsv_range: Sequence[int], out_buffer=None, auto_detect=False,
                num_bytes=None, input_id=0):
        """One host frame (bytes / numpy uint8) -> (rc, OutArgs)."""
        import numpy as np

        fr = np.ascontiguousarray(np.frombuffer(frame, np.uint8) if isinstance(frame, (bytes, bytearray))
                                  else frame, dtype=np.uint8)
        ib = _abi.BufDesc1()
        ib.numBufs = 1
        ib.descs[0].buf = fr.ctypes.data
        ib.descs[0].bufSize = fr.size
        ob = _abi.BufDesc()
        keep = []
        if out_buffer is not None:
            ob_arr = (C.c_void_p * 1)(out_buffer.ctypes.data)
            sz_arr = (C.c_int32 * 1)(out_buffer.nbytes)
            keep += [ob_arr, sz_arr]
            ob.bufs, ob.numBufs, ob.bufSizes = ob_arr, 1, sz_arr
        ia = _abi.InArgs()
        ia.base.size = C.sizeof(_abi.InArgs)
        ia.base.numBytes = fr.size if num_bytes is None else num_bytes
        ia.base.inputID = input_id
        ia.alg = _abi.InArgsAlg(*[int(v) for v in hsv_range[:6]], int(bool(auto_detect)))
        oa = _abi.OutArgs()
        oa.base.size = C.sizeof(_abi.OutArgs)
        rc = _lib.TRIK_VIDTRANSCODE_CV_process(self._h, C.byref(ib), C.byref(ob), C.byref(ia),
                                               C.byref(oa))
        return rc, oa

    def _bufs(self, frame, out_buffer, num_bytes):
        import numpy as np

        fr = np.ascontiguousarray(np.frombuffer(frame, np.uint8) if isinstance(frame, (bytes, bytearray))
                                  else frame, dtype=np.uint8)
        ib = _abi.BufDesc1()
        ib.numBufs = 1
        ib.descs[0].buf = fr.ctypes.data
        ib.descs[0].bufSize = fr.size
        ob = _abi.BufDesc()
        keep = [fr]
        if out_buffer is not None:
            ob_arr = (C.c_void_p * 1)(out_buffer.ctypes.data)
            sz_arr = (C.c_int32 * 1)(out_buffer.nbytes)
            keep += [ob_arr, sz_arr]
            ob.bufs, ob.numBufs, ob.bufSizes = ob_arr, 1, sz_arr
        return fr, ib, ob, keep


class _AutoDetect:
    """autoDetectHsv of the three codecs whose detectors are annealings
    (trik_hsv_set_auto_detect)."""

    def set_auto_detect(self, mode: int) -> int:
        """0 (the default): process() ignores autoDetectHsv and leaves
        detect* untouched.  1: a set autoDetectHsv fills detect* from the
        exact search (batch_auto_range_exact of the frame).  Returns the
        previous mode."""
        prev = _lib.trik_hsv_set_auto_detect(self._h, int(mode))
        if prev < 0:
            raise ValueError(f"set_auto_detect({mode}): {_abi.last_error()}")
        return prev


class LineSensor(_AutoDetect, ObjectSensor):
    """The ov7670 line sensor's codec instance (trik/ov7670/line_sensor glue,
    LineDetector<YUV422P, RGB565X>): same quartet, YUV422P input; process()
    uses only detectValFrom/To of the range and ignores autoDetectHsv unless
    set_auto_detect(1); OutArgs targetY carries the cross size."""

    _create = "TRIK_VIDTRANSCODE_CV_create_line"

    def __init__(self, params: _abi.Params | None = None):
        super().__init__(params)
        if params is None:
            self.params = _default_params(1, fmt_in=FORMAT_YUV422P)


class WebcamLineSensor(_AutoDetect, ObjectSensor):
    """The webcam line sensor's codec instance (trik/webcam/line_sensor glue,
    LineDetector<YUV422, RGB565X>): same quartet and InArgs/OutArgs as the
    object sensor, packed YUYV input; process() uses only detectValFrom/To,
    targetY is always 0, autoDetectHsv is ignored unless set_auto_detect(1)."""

    _create = "TRIK_VIDTRANSCODE_CV_create_webcam_line"


class BlobSensor(_AutoDetect, ObjectSensor):
    """The ov7670 object sensor's codec instance (trik/ov7670/object_sensor:
    BallDetector<YUV422P, RGB565X> with BitmapBuilder + Clusterizer): its own
    InArgs (centre/tolerance, sticky via setHsvRange) and OutArgs (target[8])."""

    _create = "TRIK_VIDTRANSCODE_CV_create_ov7670"

    def __init__(self, params: _abi.Params | None = None):
        super().__init__(params)
        if params is None:
            self.params = _default_params(1, fmt_in=FORMAT_YUV422P)

    def process(self, frame, hsv=None, out_buffer=None, auto_detect=False, num_bytes=None, input_id=0):
        """One host frame -> (rc, OV7670OutArgs).  hsv = (hue, hueTol, sat,
        satTol, val, valTol) sets the range (setHsvRange); None keeps it."""
        fr, ib, ob, keep = self._bufs(frame, out_buffer, num_bytes)
        ia = _abi.OV7670InArgs()
        ia.base.size = C.sizeof(_abi.OV7670InArgs)
        ia.base.numBytes = fr.size if num_bytes is None else num_bytes
        ia.base.inputID = input_id
        vals = [int(v) for v in hsv] if hsv is not None else [0] * 6
        ia.alg = _abi.OV7670InArgsAlg(1 if hsv is not None else 0, *vals, int(bool(auto_detect)))
        oa = _abi.OV7670OutArgs()
        oa.base.size = C.sizeof(_abi.OV7670OutArgs)
        rc = _lib.TRIK_VIDTRANSCODE_CV_process(self._h, C.byref(ib), C.byref(ob), C.byref(ia), C.byref(oa))
        return rc, oa


class MxnSensor(ObjectSensor):
    """The ov7670 MxN colour-grid sensor's codec instance (trik/ov7670/mxn_sensor:
    BallDetector<YUV422P, RGB565X> behind the ov7670 object sensor's glue): its
    own InArgs (widthM = cell rows, heightN = cell columns) and OutArgs
    (outColor[100])."""

    _create = "TRIK_VIDTRANSCODE_CV_create_mxn"

    def __init__(self, params: _abi.Params | None = None):
        super().__init__(params)
        if params is None:
            self.params = _default_params(1, fmt_in=FORMAT_YUV422P)

    def process(self, frame, m, n, out_buffer=None, num_bytes=None, input_id=0, out_args=None):
        """One host frame -> (rc, MxnOutArgs, colors): colors is the list of
        the m * n cell colours (None unless rc is EOK).  `out_args`: a
        prepared MxnOutArgs to fill instead of a fresh one."""
        fr, ib, ob, keep = self._bufs(frame, out_buffer, num_bytes)
        ia = _abi.MxnInArgs()
        ia.base.size = C.sizeof(_abi.MxnInArgs)
        ia.base.numBytes = fr.size if num_bytes is None else num_bytes
        ia.base.inputID = input_id
        ia.alg = _abi.MxnInArgsAlg(int(m), int(n))
        oa = out_args if out_args is not None else _abi.MxnOutArgs()
        if out_args is None:
            oa.base.size = C.sizeof(_abi.MxnOutArgs)
        rc = _lib.TRIK_VIDTRANSCODE_CV_process(self._h, C.byref(ib), C.byref(ob), C.byref(ia), C.byref(oa))
        colors = list(oa.alg.outColor[: int(m) * int(n)]) if rc == IVIDTRANSCODE_EOK else None
        return rc, oa, colors


class JpegSensor(ObjectSensor):
    """The ov7670 JPEG encoder's codec instance (trik/ov7670/jpeg_encoder:
    JPGEncoderWrapper<YUV422P, RGB565X> behind the ov7670 object sensor's
    glue): its own InArgs (jpgImageQuality, ifBlackAndWhite) and OutArgs
    (size).  The output buffer receives the JPEG stream."""

    _create = "TRIK_VIDTRANSCODE_CV_create_jpeg"

    def __init__(self, params: _abi.Params | None = None):
        super().__init__(params)
        if params is None:
            self.params = _default_params(1, fmt_in=FORMAT_YUV422P)

    def process(self, frame, quality, black_and_white=False, out_buffer=None, num_bytes=None, input_id=0,
                out_args=None):
        """One host frame -> (rc, JpegOutArgs, stream): stream is the JPEG's
        bytes from out_buffer (None unless rc is EOK and there is a buffer).
        `out_args`: a prepared JpegOutArgs to fill instead of a fresh one."""
        fr, ib, ob, keep = self._bufs(frame, out_buffer, num_bytes)
        ia = _abi.JpegInArgs()
        ia.base.size = C.sizeof(_abi.JpegInArgs)
        ia.base.numBytes = fr.size if num_bytes is None else num_bytes
        ia.base.inputID = input_id
        ia.alg = _abi.JpegInArgsAlg(int(quality) & 0xFF, int(bool(black_and_white)))
        oa = out_args if out_args is not None else _abi.JpegOutArgs()
        if out_args is None:
            oa.base.size = C.sizeof(_abi.JpegOutArgs)
        rc = _lib.TRIK_VIDTRANSCODE_CV_process(self._h, C.byref(ib), C.byref(ob), C.byref(ia), C.byref(oa))
        stream = None
        if rc == IVIDTRANSCODE_EOK and out_buffer is not None:
            stream = bytes(out_buffer.reshape(-1).view("uint8")[: int(oa.alg.size)])
        return rc, oa, stream


class EdgeLineSensor(ObjectSensor):
    """The ov7670 edge-line sensor's codec instance (trik/ov7670/edge_line_sensor:
    BallDetector<YUV422P, RGB565X> -- Sobel, threshold 50, column centroid --
    behind the ov7670 object sensor's glue): the object sensor's InArgs and
    OutArgs; every InArgs field is ignored, the detect* OutArgs stay untouched.
    inputLineLength must equal inputWidth.  The preview is native uint16 RGB565."""

    _create = "TRIK_VIDTRANSCODE_CV_create_edge_line"

    def __init__(self, params: _abi.Params | None = None):
        super().__init__(params)
        if params is None:
            self.params = _default_params(1, fmt_in=FORMAT_YUV422P)

    def process(self, frame, out_buffer=None, hsv_range: Sequence[int] = (0, 0, 0, 0, 0, 0), auto_detect=False,
                num_bytes=None, input_id=0):
        """One host frame -> (rc, OutArgs); hsv_range and auto_detect only fill
        the InArgs the sensor ignores."""
        return super().process(frame, hsv_range, out_buffer, auto_detect, num_bytes, input_id)
