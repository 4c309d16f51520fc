"""SURVEY.md 8(e) with two real processes: the partitioned device matvec + the owned-rows exchange, and
bench.py's own N > 1 launcher, on a one-GPU box (both ranks on cuda:0, exchange over gloo through pinned host
buffers; on an 8-GPU node the same code runs one rank per GPU over RCCL)."""
import json
import os
import socket
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _run_two_ranks(backend):
    n, k, world = 130000, 2, 2
    port = _free_port()
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "two_rank_worker.py"), str(n), str(k), backend],
                                      env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE))
    res = []
    for p in procs:
        out, err = p.communicate(timeout=800)
        assert p.returncode == 0, err.decode()[-2000:]
        res.append(json.loads(out.decode().strip().splitlines()[-1]))
    assert sorted(r["rank"] for r in res) == [0, 1]
    assert all(r["cover"] and not r["nan_left"] for r in res), res
    assert sum(r["owned"] for r in res) == n and all(0 < r["owned"] < n for r in res), res
    assert all(r["n_w"] > 0 for r in res)                      # mixed-level tree: M2P / P2L run partitioned too
    assert all(r["coarse_count"] > 0 for r in res)             # the upward pass really was split and exchanged
    assert all(r["err"] < 1e-12 for r in res), res


@pytest.mark.timeout(900)
def test_two_processes_partitioned_matvec_and_exchange_equal_the_single_rank_product():
    _run_two_ranks("gloo")


@pytest.mark.timeout(900)
def test_two_ranks_over_rccl_one_gpu_each():
    """The same two-rank product with the collectives on RCCL (all-reduce of the coarse multipoles, all-gather of the
    owned rows), one GPU per rank: runs on the first box that has two GPUs."""
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs (RCCL refuses two ranks on one device)")
    _run_two_ranks("nccl")


def _bench_ranks(world, points, config5_points, tmp_path):
    """`python bench.py --gpus N` with no launcher around it on the one GPU of the box (gloo exchange): returns the
    parsed stdout line, the raw line and the full record of the side file."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}
    detail = str(tmp_path / "bench_detail.json")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(world), "--exchange", "gloo",
                        "--points", str(points), "--steps", "3", "--warmup", "1", "--full", "--cpu-baseline", "off",
                        "--configs", "config5", "--config5-points", str(config5_points), "--detail-file", detail],
                       env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=1100)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    lines = [ln for ln in p.stdout.decode().splitlines() if ln.strip()]
    assert len(lines) == 1 and len(lines[0]) < 4096, [len(ln) for ln in lines]       # ONE line the driver can parse
    with open(detail) as f:
        full = json.load(f)
    return json.loads(lines[0]), lines[0], full


@pytest.mark.timeout(900)
def test_bench_launches_its_own_ranks(tmp_path):
    """`python bench.py --gpus 2` with no launcher around it: the parent starts two rank processes before
    touching the GPU and relays rank 0's line (here with the gloo exchange so that both fit one GPU)."""
    j, _, full = _bench_ranks(2, 400000, 300000, tmp_path)
    assert j["n_gpus"] == 2 and j["steps"] == 3 and j["value"] > 0 and j["scaling"] == "strong"
    assert "target-subtree partition x2" in j["config"]["parallelism"]
    # the N > 1 line is a checked claim: dense rows of the exchanged result, and config 5's workload on the same ranks
    assert j["dense_rows_rel_err"] is not None and j["dense_rows_rel_err"] < 1e-6
    assert j["partition_covers_every_row_once"] is True
    c5 = j["configs"]["config5_spheroidal3_40M"]
    assert "error" not in c5, c5
    assert c5["ms_per_step"] > 0 and c5["dense_rows_rel_err"] < 1e-5 and c5["roofline"]["frac"] > 0
    f5 = full["configs"]["config5_spheroidal3_40M"]
    assert f5["n_gpus"] == 2 and "Spheroidal3Rbf" in f5["workload"] and f5["workload"].startswith("300000 ")


@pytest.mark.timeout(900)
def test_bench_under_the_drivers_launcher(tmp_path):
    """The driver starts N > 1 as `python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1
    --master-port P bench.py --gpus N ...` (ranks from the environment, no file store): the same two-rank run through
    that launcher, gloo exchange on the one GPU.  stdout of the whole launch = rank 0's one line."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT", "MASTER_ADDR")}
    detail = str(tmp_path / "bench_detail.json")
    p = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                        "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.join(ROOT, "bench.py"),
                        "--gpus", "2", "--exchange", "gloo", "--points", "300000", "--steps", "3", "--warmup", "1",
                        "--full", "--cpu-baseline", "off", "--configs", "off", "--detail-file", detail],
                       env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=800)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    lines = [ln for ln in p.stdout.decode().splitlines() if ln.strip()]
    assert len(lines) == 1 and len(lines[0]) < 4096, p.stdout.decode()[-1000:]
    j = json.loads(lines[0])
    assert j["n_gpus"] == 2 and j["steps"] == 3 and j["warmup"] == 1 and j["value"] > 0
    assert j["dense_rows_rel_err"] < 1e-6 and j["partition_covers_every_row_once"] is True


@pytest.mark.timeout(1200)
def test_bench_eight_ranks_rehearsal_on_one_gpu(tmp_path):
    """The driver's 8-GPU run has no retry, so the 8-rank path is rehearsed here first: eight
    fresh rank processes on the one GPU, exchange over gloo -- NEVER a scaling number.  rc 0, one line under 4 KB,
    n_gpus == 8, both workloads checked against dense rows (2M LinearRbf; config 5's Spheroidal3 at 1M points, whose
    BBFMM accuracy at order 7 is itself 1e-6: bound 2e-6), every row owned exactly once (bench.py asserts
    `check_partition` on every rank before timing and records it).  The split rehearsed: bbfmm.rs:383-401, 444-507."""
    j, raw, full = _bench_ranks(8, 2_000_000, 1_000_000, tmp_path)
    assert j["n_gpus"] == 8 and j["steps"] == 3 and j["value"] > 0
    assert "target-subtree partition x8" in j["config"]["parallelism"]
    assert j["partition_covers_every_row_once"] is True
    assert j["dense_rows_rel_err"] < 1e-6
    c5 = j["configs"]["config5_spheroidal3_40M"]
    assert "error" not in c5 and c5["dense_rows_rel_err"] < 2e-6 and c5["ms_per_step"] > 0
    assert full["configs"]["config5_spheroidal3_40M"]["n_gpus"] == 8
    out = os.path.join(ROOT, "gpurun_out")
    if os.path.isdir(out):                          # kept for profiles/ (labelled: never a scaling number)
        with open(os.path.join(out, "bench_8ranks_gloo_one_gpu.json"), "w") as f:
            f.write(raw + "\n")
