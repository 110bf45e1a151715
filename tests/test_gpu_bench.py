"""bench.py on one GPU: a plain run reports the headline fields only, `--steps` sets the timed steps, and `--dump-outputs` writes
what the last timed step computed -- the same arrays from run to run, and (headline) true inverses of the inputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def _bench(*args):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])


def test_plain_run_dumps_the_last_step(tmp_path):
    import torch
    sys.path.insert(0, ROOT)
    import bench
    n, batch = 64, 5000
    dumps = []
    for d in ("a", "b"):
        out = _bench("--steps", "3", "--warmup", "1", "--batch", str(batch), "--dump-outputs", str(tmp_path / d))
        assert out["steps"] == 3 and out["ms_per_step"] > 0 and out["unit"] == "inversions/s" and out["dtype"] == "f64"
        assert "cpu_baseline" not in out and "other_workloads" not in out and "mixed" not in out
        dumps.append({k: np.load(tmp_path / d / f"{k}.npy") for k in ("inverse", "info")})
    inv, info = dumps[0]["inverse"], dumps[0]["info"]
    idx = bench.sample_rows(batch, n * n * 8)
    assert inv.dtype == np.float64 and inv.shape == (len(idx), n * n) and info.dtype == np.float32 and info.shape == (len(idx),)
    assert inv.nbytes + info.nbytes <= 64 << 20
    assert not info.any()
    for k in ("inverse", "info"):
        assert np.array_equal(dumps[0][k], dumps[1][k]), k
    a = bench.make_spd(n, batch, 0x5EED, torch.device("cuda", 0)).view(batch, n * n)[torch.from_numpy(idx).cuda()].cpu().numpy()
    resid = np.abs(np.matmul(a.reshape(-1, n, n), inv.reshape(-1, n, n)) - np.eye(n)).max()
    assert resid < 1e-11 * n, resid


def test_mixed_workload_dumps_its_means(tmp_path):
    out = _bench("--workload", "mixed", "--steps", "2", "--warmup", "1", "--dump-outputs", str(tmp_path))
    assert out["steps"] == 2 and out["ms_per_step"] > 0 and out["unit"] == "items/s" and "per_bin" not in out
    means = np.load(tmp_path / "means.npy")
    assert means.dtype == np.float32 and means.shape == (sum(out["config"]["mix_items_per_step_per_gpu"].values()),)
    assert np.isfinite(means).all()
