"""The reference's own algorithm classes, built on the host (oracle/ref) and
driven through ctypes -- test code, not product.

One shared library per reference sensor lies in oracle/_ref/ (every sensor
defines the same class names in trik::cv, so each is loaded RTLD_LOCAL).  The
libraries are built on first use when a reference checkout is present
($TRIK_REFERENCE, or the default of oracle/ref/Makefile); a build that fails
then is an error, not a skip.  With neither a checkout nor built libraries the
calling test skips.

The wrappers return what the matching oracle.* / mxn_ref / jpeg_ref call
returns, so a test compares the two results field by field.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_MAKE = os.path.join(ROOT, "oracle", "ref")
REF_OUT = os.path.join(ROOT, "oracle", "_ref")
SENSORS = ("webcam_object", "webcam_line", "ov7670_line", "ov7670_object", "ov7670_mxn", "ov7670_jpeg")

_vp, _i32, _i64 = C.c_void_p, C.c_int32, C.c_int64
_libs = {}
_state = {}


def lib_path(sensor):
    return os.path.join(REF_OUT, "libref_%s.so" % sensor)


def reference_dir():
    """The reference checkout the Makefile would use, or None when it is absent."""
    out = subprocess.run(["make", "-s", "-C", REF_MAKE, "where"], check=True, capture_output=True, text=True)
    d = out.stdout.strip().splitlines()[-1].strip() if out.stdout.strip() else ""
    marker = os.path.join(d, "trik", "webcam", "object_sensor", "include", "internal", "cv_ball_detector.hpp")
    return d if d and os.path.exists(marker) else None


def build():
    """make -C oracle/ref: a no-op that succeeds without a reference checkout."""
    subprocess.run(["make", "-s", "-C", REF_MAKE], check=True)


def available():
    """True when the six libraries can be loaded (building them first when a
    reference checkout is present); False when there is neither a checkout nor
    a built set.  Raises when a checkout is present and the build fails."""
    if "ok" not in _state:
        have_tree = reference_dir() is not None
        if have_tree:
            build()
            missing = [s for s in SENSORS if not os.path.exists(lib_path(s))]
            if missing:
                raise RuntimeError("the reference build left no library for: " + ", ".join(missing))
        _state["tree"] = have_tree
        _state["ok"] = all(os.path.exists(lib_path(s)) for s in SENSORS)
    return _state["ok"]


def require():
    """Skip the calling test when the reference build cannot exist here."""
    if not available():
        pytest.skip("no reference checkout ($TRIK_REFERENCE) and no built libraries in oracle/_ref")


def lib(sensor):
    require()
    if sensor not in _libs:
        L = C.CDLL(lib_path(sensor), mode=os.RTLD_LOCAL | os.RTLD_NOW)
        L.ref_destroy.argtypes, L.ref_destroy.restype = [_vp], None
        L.ref_create.restype = _vp
        if sensor == "ov7670_jpeg":
            L.ref_create.argtypes = [C.c_int] * 3
            L.ref_run.argtypes, L.ref_run.restype = [_vp, _vp, _i64, _vp, _i64, C.c_int, C.c_int], _i64
        else:
            L.ref_create.argtypes = [C.c_int] * 6
        if sensor == "webcam_object":
            L.ref_run.argtypes, L.ref_run.restype = [_vp, _vp, _i64, _vp, _i64, _vp, C.c_int, _vp], C.c_int
            L.ref_pixel_tables.argtypes, L.ref_pixel_tables.restype = [_vp, _vp], C.c_int
        elif sensor in ("webcam_line", "ov7670_line"):
            L.ref_run.argtypes = [_vp, _vp, _i64, _vp, _i64, C.c_int, C.c_int, _vp, _vp, _vp]
            L.ref_run.restype = C.c_int
        elif sensor == "ov7670_object":
            L.ref_run.argtypes = [_vp, _vp, _i64, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _vp]
            L.ref_run.restype = C.c_int
            L.ref_pixel_table.argtypes, L.ref_pixel_table.restype = [_vp, C.c_int], C.c_int
        elif sensor == "ov7670_mxn":
            L.ref_run.argtypes, L.ref_run.restype = [_vp, _vp, _i64, _vp, _i64, C.c_int, C.c_int, _vp], C.c_int
        _libs[sensor] = L
    return _libs[sensor]


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _out_geom(width, height, out_width, out_height, out_line_length):
    ow = width // 2 if out_width is None else out_width
    oh = height // 2 if out_height is None else out_height
    oll = 2 * ow if out_line_length is None else out_line_length
    return ow, oh, oll


class Instance:
    """One algorithm instance: setup() on entry, destroyed on exit.  None as
    `handle` when the reference's setup() returns false."""

    def __init__(self, sensor, *geom):
        self.lib = lib(sensor)
        self.handle = self.lib.ref_create(*[int(g) for g in geom])

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        if self.handle:
            self.lib.ref_destroy(self.handle)
            self.handle = None


OUTARG_KEYS = ("target_x", "target_y", "target_size")
DETECT_KEYS = ("detect_hue", "detect_hue_tol", "detect_sat", "detect_sat_tol", "detect_val", "detect_val_tol")


def webcam_pixel_tables():
    """(first, second): the webcam detector's per-pixel functions on every
    (Y, U, V), for the first and the second pixel of a YUYV word."""
    with Instance("webcam_object", 32, 4, 64, 16, 2, 32) as inst:
        assert inst.handle
        a, b = np.zeros(1 << 24, np.uint64), np.zeros(1 << 24, np.uint64)
        assert inst.lib.ref_pixel_tables(_ptr(a), _ptr(b)) == 0
    return a, b


def ov7670_pixel_table(rot):
    """The ov7670 object sensor's unpacking and per-pixel path on every
    (Y, U, V), every luma at position (Y - rot) % 4 of its 4-pixel group."""
    out = np.zeros(1 << 24, np.uint64)
    assert lib("ov7670_object").ref_pixel_table(_ptr(out), rot) == 0
    return out


def webcam_run(frame, width, height, line_length, rng, auto_detect=False, out_width=None,
               out_height=None, out_line_length=None):
    """As oracle.run for LAYOUT_YUYV: (rc, outargs dict, preview)."""
    fr = np.ascontiguousarray(frame, dtype=np.uint8)
    ow, oh, oll = _out_geom(width, height, out_width, out_height, out_line_length)
    out = np.zeros(max(1, oh * oll), np.uint8)
    with Instance("webcam_object", width, height, line_length, ow, oh, oll) as inst:
        if not inst.handle:
            return -1, None, None
        r = np.array([int(v) for v in rng], np.int32)
        res = np.zeros(9, np.int32)
        rc = inst.lib.ref_run(inst.handle, _ptr(fr), fr.size, _ptr(out), oh * oll, _ptr(r),
                              1 if auto_detect else 0, _ptr(res))
    if rc != 0:
        return rc, None, None
    d = dict(zip(OUTARG_KEYS + DETECT_KEYS, (int(v) for v in res)))
    d["detect_written"] = 1 if auto_detect else 0
    return 0, d, out[:oh * oll]


def _line_run(sensor, frame, width, height, line_length, val_from, val_to, band, ow, oh, oll):
    fr = np.ascontiguousarray(frame, dtype=np.uint8)
    out = np.zeros(max(1, oh * oll), np.uint8)
    b = np.array(band, np.int32)
    res, sums = np.zeros(3, np.int32), np.zeros(3, np.int64)
    with Instance(sensor, width, height, line_length, ow, oh, oll) as inst:
        if not inst.handle:
            return -1, None, None, None, None
        rc = inst.lib.ref_run(inst.handle, _ptr(fr), fr.size, _ptr(out), oh * oll, int(val_from), int(val_to),
                              _ptr(b), _ptr(res), _ptr(sums))
    if rc != 0:
        return rc, None, None, None, None
    return 0, dict(zip(OUTARG_KEYS, (int(v) for v in res))), out[:oh * oll], sums, tuple(int(v) for v in b)


def line_run(frame, width, height, line_length, val_from, val_to, band=None, out_width=None,
             out_height=None, out_line_length=None):
    """As oracle.line_run: (rc, outargs, preview, sums, band_out)."""
    ow, oh, oll = _out_geom(width, height, out_width, out_height, out_line_length)
    band = band if band is not None else (height // 2, height // 2 + 80)
    return _line_run("ov7670_line", frame, width, height, line_length, val_from, val_to, band, ow, oh, oll)


def wline_run(frame, width, height, line_length, val_from, val_to, out_width=240, out_height=320,
              out_line_length=None):
    """As oracle.wline_run: (rc, outargs, preview, sums)."""
    oll = 2 * out_width if out_line_length is None else out_line_length
    return _line_run("webcam_line", frame, width, height, line_length, val_from, val_to, (0, 0), out_width,
                     out_height, oll)[:4]


class BlobSensor:
    """The ov7670 object sensor kept alive over a sequence of frames (its HSV
    range is sticky from call to call).  run() returns a dict shaped like
    oracle.blob_run's, plus `sorted` (every cluster after the reference's
    sort, [n, 3] of size, sum x, sum y) and `detect` (the six detect* fields)."""

    def __init__(self, width, height, line_length, out_width=None, out_height=None, out_line_length=None):
        self.w, self.h, self.ll = width, height, line_length
        self.ow, self.oh, self.oll = _out_geom(width, height, out_width, out_height, out_line_length)
        self.inst = Instance("ov7670_object", width, height, line_length, self.ow, self.oh, self.oll)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.inst.__exit__()

    def run(self, frame, hsv=None, auto_detect=False):
        if not self.inst.handle:
            return {"rc": -1}
        fr = np.ascontiguousarray(frame, dtype=np.uint8)
        out = np.zeros(max(1, self.oh * self.oll), np.uint8)
        args = np.array([1 if hsv is not None else 0] + ([int(v) for v in hsv] if hsv is not None else [0] * 6)
                        + [1 if auto_detect else 0], np.int32)
        bw, bh = self.w // 4, self.h // 4
        room = bw * bh + 2
        targets, top, info = np.zeros(24, np.int8), np.zeros(24, np.int32), np.zeros(10, np.int64)
        srt = np.zeros(3 * room, np.int32)
        meta, labels = np.zeros(max(1, bw * bh), np.uint8), np.zeros(max(1, bw * bh), np.uint16)
        rc = self.inst.lib.ref_run(self.inst.handle, _ptr(fr), fr.size, _ptr(out), self.oh * self.oll, _ptr(args),
                                   _ptr(targets), _ptr(top), _ptr(info), _ptr(srt), room, _ptr(meta), _ptr(labels))
        if rc != 0:
            return {"rc": rc}
        n = int(info[0])
        return {"rc": 0, "targets": targets.reshape(8, 3), "preview": out[:self.oh * self.oll],
                "meta": meta[:bw * bh].reshape(bh, bw), "labels": labels[:bw * bh].reshape(bh, bw),
                "top": top.reshape(8, 3), "n_labels": n, "state": tuple(int(v) for v in info[1:4]),
                "sorted": srt[:3 * min(n, room)].reshape(-1, 3), "detect": [int(v) for v in info[4:10]]}


def blob_run(frame, width, height, line_length, hsv, out_width=None, out_height=None, out_line_length=None):
    with BlobSensor(width, height, line_length, out_width, out_height, out_line_length) as s:
        return s.run(frame, hsv)


def mxn_run(frame, width, height, line_length, m, n, out_width=None, out_height=None, out_line_length=None):
    """(rc, colors list [m * n], preview uint8 [out_height, out_line_length])."""
    fr = np.ascontiguousarray(frame, dtype=np.uint8)
    ow, oh, oll = _out_geom(width, height, out_width, out_height, out_line_length)
    out = np.zeros(max(1, oh * oll), np.uint8)
    colors = np.zeros(100, np.int32)
    with Instance("ov7670_mxn", width, height, line_length, ow, oh, oll) as inst:
        if not inst.handle:
            return -1, None, None
        rc = inst.lib.ref_run(inst.handle, _ptr(fr), fr.size, _ptr(out), oh * oll, int(m), int(n), _ptr(colors))
    if rc != 0:
        return rc, None, None
    return 0, [int(c) for c in colors[:m * n]], out[:oh * oll].reshape(oh, oll)


def compact(frame, width, height, line_length):
    """The two planes of an ov7670 frame without their line padding."""
    fr = np.asarray(frame, np.uint8).reshape(-1)[:2 * height * line_length].reshape(2 * height, line_length)
    return np.ascontiguousarray(fr[:, :width]).reshape(-1)


def jpeg_encode(frame, width, height, line_length, quality, bw):
    """The reference encoder's stream of one frame.  The reference strides by
    `width` and never reads lineLength, so a padded frame is compacted first."""
    fr = compact(frame, width, height, line_length) if line_length != width else \
        np.ascontiguousarray(frame, dtype=np.uint8)
    room = 4 * width * height + 4096
    with Instance("ov7670_jpeg", width, height, width) as inst:
        assert inst.handle, "the reference's setup() rejected %dx%d" % (width, height)
        while True:
            out = np.zeros(room, np.uint8)
            n = inst.lib.ref_run(inst.handle, _ptr(fr), fr.size, _ptr(out), room, int(quality), 1 if bw else 0)
            assert n >= 0
            if n <= room:
                return out[:n].tobytes()
            room = int(n)
