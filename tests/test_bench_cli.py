"""bench.py's output contract: the plain run's result line, --dump-outputs (what the timed path computed, bounded in size,
the same for the same arguments) and the sampling of large outputs (CPU)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")


def test_dump_outputs_dtypes_and_seeded_sample(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_MAX_ELEMENTS", 1000)
    big = torch.arange(5000, dtype=torch.float32).reshape(50, 100)
    arrays = {"small": torch.linspace(0, 1, 7), "f64": np.arange(3, dtype=np.float64), "half": torch.ones(4, dtype=torch.bfloat16),
              "big": big}
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), arrays)
    a = {n: np.load(tmp_path / "a" / f"{n}.npy") for n in arrays}
    assert a["small"].dtype == np.float32 and np.array_equal(a["small"], arrays["small"].numpy())
    assert a["f64"].dtype == np.float64 and np.array_equal(a["f64"], arrays["f64"])
    assert a["half"].dtype == np.float32 and np.array_equal(a["half"], np.ones(4, np.float32))
    # larger than the cap: a sorted sample of the flat elements (here each element's value is its position)
    s = a["big"]
    assert s.dtype == np.float32 and s.shape == (1000,)
    assert np.all(np.diff(s) >= 0) and s.min() >= 0 and s.max() < 5000 and len(np.unique(s)) > 800
    for n in arrays:
        assert np.array_equal(a[n], np.load(tmp_path / "b" / f"{n}.npy")), n


def _plain_run(out_dir):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--batch", "8",
           "--dump-outputs", str(out_dir)]
    p = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, timeout=600)
    assert p.returncode == 0
    lines = [l for l in p.stdout.decode().splitlines() if l.strip()]
    assert len(lines) == 1, lines
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_dumps_the_same_outputs_twice(tmp_path):
    """A plain run prints the headline without the --full figures and writes the last timed step's loss tails and weights;
    two runs with the same arguments write the same arrays (seeded inputs, deterministic kernels)."""
    out = _plain_run(tmp_path / "a")
    for k in HEADLINE:
        assert k in out, k
    assert out["steps"] == 2 and out["warmup"] == 1 and out["ms_per_step"] > 0 and out["value"] > 0
    assert out["unit"] == "samples/s" and out["higher_is_better"] is True and out["dtype"] == "f32"
    assert not {"roofline", "iteration_ms", "cpu_baseline"} & set(out)
    names = ("critic_loss_tail", "generator_loss_tail", "generator_weights", "critic_weights")
    assert sorted(os.listdir(tmp_path / "a")) == sorted(n + ".npy" for n in names)
    assert sum(os.path.getsize(tmp_path / "a" / f"{n}.npy") for n in names) <= 64 << 20
    a = {n: np.load(tmp_path / "a" / f"{n}.npy") for n in names}
    assert all(v.dtype == np.float32 and np.all(np.isfinite(v)) for v in a.values())
    dl, gl = a["critic_loss_tail"], a["generator_loss_tail"]
    assert dl.shape == gl.shape == (5,) and dl[4] == 0 and gl[4] == 0
    assert out["final_losses"]["d_loss"] == round(float(0.5 * (dl[1] + dl[2])), 5)
    assert out["final_losses"]["g_loss"] == round(float(gl[0]), 5)
    _plain_run(tmp_path / "b")
    for n in names:
        assert np.array_equal(a[n], np.load(tmp_path / "b" / f"{n}.npy")), n
