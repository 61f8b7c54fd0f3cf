"""bench.py --dump-outputs: what the timed path returned in its last step, as float64 .npy files, identical from run to run
with the same arguments; and a plain run does only its timed path (the CPU baseline is --full's)."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, require_gpu


def _bench_module():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_dump_keeps_a_fixed_sample_within_its_budget(tmp_path, monkeypatch):
    bench = _bench_module()
    monkeypatch.setattr(bench, "DUMP_BYTES", 2 * 8 * 100)            # 100 rows of one float64 per array
    big = torch.arange(1000, dtype=torch.int32)
    small = torch.arange(12, dtype=torch.int64).reshape(3, 4)
    for d in ("a", "b"):
        args = type("A", (), {"dump_outputs": str(tmp_path / d)})()
        bench.dump_outputs(args, 0, {"big": big, "small": small})
        bench.dump_outputs(args, 1, {"other_rank": small})            # only rank 0 writes
    a, b = np.load(tmp_path / "a" / "big.npy"), np.load(tmp_path / "b" / "big.npy")
    assert a.dtype == np.float64 and a.nbytes <= 8 * 100 and (a == b).all()
    assert (np.diff(a) > 0).all() and np.isin(a, np.arange(1000)).all()   # rows of the original, in order
    s = np.load(tmp_path / "a" / "small.npy")
    assert s.dtype == np.float64 and (s == small.numpy()).all()
    assert sorted(os.listdir(tmp_path / "a")) == ["big.npy", "small.npy"]


@pytest.mark.gpu
def test_plain_run_dumps_identical_outputs_and_honours_steps(tmp_path):
    require_gpu()
    outs = []
    for d in ("one", "two"):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                            "--batch", "1024", "--dump-outputs", str(tmp_path / d)], cwd=ROOT, capture_output=True, text=True,
                           timeout=420)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        assert len(lines) == 1, r.stdout[-2000:]
        outs.append(json.loads(lines[0]))
    line = outs[0]
    assert line["steps"] == 3 and line["ms_per_step"] > 0 and "cpu_baseline" not in line
    assert abs(line["value"] * line["ms_per_step"] * 1e-3 - 1024) < 1e-6 * 1024
    names = sorted(os.listdir(tmp_path / "one"))
    assert names == ["counters.npy", "run.npy"] and names == sorted(os.listdir(tmp_path / "two"))
    for n in names:
        a, b = np.load(tmp_path / "one" / n), np.load(tmp_path / "two" / n)
        assert a.dtype == np.float64 and a.shape == b.shape and (a == b).all(), n
    cnt, run = np.load(tmp_path / "one" / "counters.npy"), np.load(tmp_path / "one" / "run.npy")
    assert cnt.shape == (1024, 7)                                    # every counter but the fixpoint's barrier rounds
    frame_err, frames = run[1], run[7]                               # RUN_NAMES without "iterations"
    assert frames == 3 * 1024 and line["results"]["FER"] == frame_err / frames
