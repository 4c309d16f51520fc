"""bench.py's plain run, the one every change is timed with: one line of the contract's keys only, exactly `--steps` timed
steps, no side file, and `--dump-outputs` writing what the last timed step computed -- held against the library's own
product on the same seeded inputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, relerr

pytestmark = pytest.mark.gpu

KEYS = {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
        "dtype", "data", "config"}


@pytest.mark.timeout(600)
def test_plain_run_prints_the_headline_and_dumps_the_last_step(tmp_path):
    n = 200_000
    dump = tmp_path / "outputs"
    detail = tmp_path / "bench_detail.json"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--points", str(n), "--steps", "3",
                        "--warmup", "1", "--dump-outputs", str(dump), "--detail-file", str(detail)],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=500)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    lines = [ln for ln in p.stdout.decode().splitlines() if ln.strip()]
    assert len(lines) == 1, lines
    j = json.loads(lines[0])
    assert set(j) == KEYS, sorted(set(j) ^ KEYS)
    assert j["steps"] == 3 and j["warmup"] == 1 and j["n_gpus"] == 1 and j["dtype"] == "f64" and j["higher_is_better"] is True
    assert j["value"] > 0 and abs(j["ms_per_step"] * j["value"] - 1e3) < 1e-3
    assert j["config"]["points"] == n and j["config"]["parallelism"] == "single GPU"
    assert not detail.exists()                                   # the full record is --full's
    assert sorted(os.listdir(dump)) == ["potentials.npy"]        # 1.6 MB: whole, no column sample
    y = np.load(dump / "potentials.npy")
    assert y.shape == (1, n) and y.dtype == np.float64 and np.isfinite(y).all()

    import ferreus_rbf_rs_amd as F
    pts = np.random.default_rng(42).random((n, 3))               # bench.py's seeded inputs
    w = np.random.default_rng(43).random((1, n))
    tree = F.FmmTree(pts, 7, F.KernelParams(F.FmmKernelType.LinearRbf), True, True)
    assert relerr(y[0], tree.fast_matrix_vector_product(w[0].copy())) < 1e-11
