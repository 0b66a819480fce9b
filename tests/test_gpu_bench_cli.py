"""bench.py's command line: a plain run, --dump-outputs and --full.

A plain run (64 frames, 3 steps) prints the headline line without the
measurements that live behind --full, and --dump-outputs writes what its last
timed step returned: the sums, targets and totals of the seeded batch, held
here to the CPU oracle on every frame.  The same run with --full carries the
extra fields.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from gpu_util import BENCH_RANGES, LAYOUT_YUYV

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, LL, N = 640, 480, 1280, 64
SEED = 0x7A1C
FULL_ONLY = ("totals_check", "cold_batch", "scene", "cpu_baseline", "cpu_sample_parity")


def _bench(*extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
           "--frames", str(N)] + list(extra)
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=240, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_dumps_outputs(oracle_mod, tmp_path):
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    out = tmp_path / "dump"
    d = _bench("--dump-outputs", str(out))
    assert d["steps"] == 3 and d["warmup"] == 1
    assert d["unit"] == "Mpix/s" and d["higher_is_better"] is True and d["dtype"] == "u8"
    assert d["value"] > 0 and d["ms_per_step"] > 0
    # value and ms_per_step are the same measurement; ms_per_step is rounded
    # to 1e-4 ms in the line (half a unit each way, doubled for the value's own rounding)
    assert d["value"] == pytest.approx(N * W * H / (d["ms_per_step"] / 1e3) / 1e6, rel=1e-4 / d["ms_per_step"])
    assert not [k for k in FULL_ONLY if k in d]

    assert sorted(os.listdir(out)) == ["sums.npy", "targets.npy", "totals.npy"]
    sums, targets, totals = (np.load(out / f"{n}.npy") for n in ("sums", "targets", "totals"))
    T = len(BENCH_RANGES)
    assert sums.dtype == np.float64 and sums.shape == (N, T, 3)
    assert targets.dtype == np.float32 and targets.shape == (N, T, 4)
    assert totals.dtype == np.float64 and totals.shape == (T, 3)
    host = oracle_mod.synth(N, W, H, LL, LAYOUT_YUYV, 0, SEED)
    want_s, want_t = oracle_mod.batch(host, H * LL, N, W, H, LL, LAYOUT_YUYV, BENCH_RANGES, n_threads=16)
    assert np.array_equal(sums, want_s)
    assert np.array_equal(targets[:, :, :3], want_t)
    assert np.array_equal(totals, want_s.sum(axis=0))


def test_full_run_carries_the_rest():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    d = _bench("--full", "--cpu-frames-all", "64", "--cpu-frames", "64", "--scene-launches", "4")
    assert not [k for k in FULL_ONLY if k not in d]
    assert d["totals_check"]["ok"] is True and d["cpu_sample_parity"] is True
    assert d["scene"]["launches"] == 4 and d["cold_batch"]["first_call_ms"] > 0
