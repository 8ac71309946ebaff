"""bench.py's own contract: a plain run times the steps it is asked for and prints the headline line, `--full` adds the
measurements behind it, and `--dump-outputs DIR` writes what the timed path computed in its last step (float64, a seeded
sample of trajectories when the whole would exceed the size limit)."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench_module():
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    return b


def test_dump_outputs_samples_the_same_rows_within_the_limit(tmp_path, monkeypatch):
    import torch
    b = _bench_module()
    B, N = 500, 40
    g = torch.Generator().manual_seed(0)
    per = {"x": torch.randn(B, N, 6, generator=g, dtype=torch.float64), "u": torch.randn(B, N, 3, generator=g, dtype=torch.float64),
           "status": torch.arange(B, dtype=torch.int32), "absent": None}
    table = np.arange(5.0).reshape(1, 5)
    b.dump_outputs(str(tmp_path / "whole"), per, {"convergence_table": table})
    files = sorted(os.listdir(tmp_path / "whole"))
    assert files == ["convergence_table.npy", "status.npy", "trajectory_index.npy", "u.npy", "x.npy"]
    idx = np.load(tmp_path / "whole" / "trajectory_index.npy")
    assert idx.dtype == np.float64 and np.array_equal(idx, np.arange(B))
    assert np.array_equal(np.load(tmp_path / "whole" / "x.npy"), per["x"].numpy())

    limit = 200_000                                       # the whole set is 500 * (1920 + 960 + 8 + 8) bytes: sampled
    monkeypatch.setattr(b, "DUMP_LIMIT_BYTES", limit)
    for d in ("s1", "s2"):
        b.dump_outputs(str(tmp_path / d), per, {"convergence_table": table})
    total = sum(os.path.getsize(tmp_path / "s1" / f) for f in os.listdir(tmp_path / "s1"))
    assert total <= limit
    idx = np.load(tmp_path / "s1" / "trajectory_index.npy").astype(np.int64)
    assert 0 < len(idx) < B and np.all(np.diff(idx) > 0)
    for name in ("x", "u", "status", "trajectory_index", "convergence_table"):
        a1, a2 = np.load(tmp_path / "s1" / f"{name}.npy"), np.load(tmp_path / "s2" / f"{name}.npy")
        assert a1.dtype == np.float64 and np.array_equal(a1, a2)   # fixed seed: the same sample every run
    assert np.array_equal(np.load(tmp_path / "s1" / "x.npy"), per["x"].numpy()[idx])
    assert np.array_equal(np.load(tmp_path / "s1" / "status.npy"), idx.astype(np.float64))


def _run(args, tmp_path):
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env, capture_output=True, text=True,
                       timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_and_full_runs_dump_the_same_last_step(tmp_path):
    """A plain run and a --full run with the same arguments: `steps` timed steps in both, the headline keys in both, the extra
    measurements in the --full line only, and the same results of the last timed step (the --full legs run after it).  From
    512 trajectories on the timed region runs the headline's form (the passes on the model's structure), so --full adds the
    general-layout leg."""
    size = ["--gpus", "1", "--steps", "5", "--warmup", "2", "--batch", "512", "--horizon", "40"]
    plain = _run(size + ["--dump-outputs", str(tmp_path / "plain")], tmp_path)
    full = _run(size + ["--full", "--no-cpu-baseline", "--dump-outputs", str(tmp_path / "full")], tmp_path)
    for out in (plain, full):
        assert out["steps"] == 5 and out["n_gpus"] == 1 and out["unit"] == "iterations/s" and out["dtype"] == "f64"
        assert out["higher_is_better"] is True and out["value"] > 0
        assert abs(out["ms_per_step"] - 1e3 / out["value"]) <= 1e-9 * out["ms_per_step"]
        assert out["cpu_baseline"] is None
        assert out["convergence"]["active"] == 512.0
    assert "roofline" not in plain and plain["config"]["general_ab_iterations_per_s"] is None
    assert plain["config"]["lti_stride0_layout_iterations_per_s"] is None
    assert full["roofline"]["families"] and full["event_sampled_steps"] == 2
    assert full["config"]["general_ab_iterations_per_s"] > 0 and full["config"]["lti_stride0_layout_iterations_per_s"] > 0

    shapes = {"x": (512, 40, 6), "u": (512, 40, 3), "cost": (512,), "z_u": (512, 40, 3), "admm_residuals": (512, 2),
              "status": (512,), "convergence_table": (1, 5), "trajectory_index": (512,)}
    assert sorted(os.listdir(tmp_path / "plain")) == sorted(f"{k}.npy" for k in shapes)
    for k, shape in shapes.items():
        a, f = np.load(tmp_path / "plain" / f"{k}.npy"), np.load(tmp_path / "full" / f"{k}.npy")
        assert a.dtype == np.float64 and a.shape == shape and np.isfinite(a).all(), k
        np.testing.assert_allclose(f, a, rtol=1e-12, atol=0, err_msg=k)
    assert np.abs(np.load(tmp_path / "plain" / "u.npy")).max() > 0
