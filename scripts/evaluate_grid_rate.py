"""Rate of FmmTree.evaluate_grid on full-size grids, beside the existing path (evaluate_leaves on the same host coordinates,
what RBFInterpolator.evaluate_targets runs), for the two cases of DESIGN.md section 12 "Measured": the albatite
Spheroidal3 fit and the 1M-point LinearRbf cloud, each on the box of its isosurface lattice (207 x 250 x 287 and
219 x 221 x 312 nodes at the lattice's own axis spacings -- a cube of spacing 5, or 0.02, with these counts does not fit
the evaluator's tree).  Everything of one case runs in one process on the same tree: the existing path, then
evaluate_grid with max_job_targets in --caps, each the best of --repeats after a warm-up, all timings kept so that the
run-to-run spread can be read.  Then one `rocprofv3 --kernel-trace --stats` run each (no counters) for cap 0 and the best
cap says how the time splits over the kernels.  Every step is a child process under its own time limit.

    python scripts/evaluate_grid_rate.py [--cases albatite,cloud] [--caps 0,256,512,1024,2048] [--repeats 3]
                                         [--out profiles/evaluate_grid_rate.json] [--no-trace]
"""
import argparse
import csv
import glob
import json
import os
import shutil
import signal
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, repeats):
    fn()                                            # warm-up (arena, target-set scratch)
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return ts, out


def build_case(name):
    """(tree, weights, origin, steps, shape): the evaluator of the case and the box of its isosurface lattice as a grid"""
    import ferreus_rbf_rs_amd as F
    from ferreus_rbf_rs_amd import isosurface as I
    if name == "albatite":
        from ferreus_rbf_rs_amd import solvers as S
        from ferreus_rbf_rs_amd.ddm import DDMParams, InterpolantSettings, SchwarzPreconditioner
        from oracle import bbfmm_oracle as O
        z = np.load(os.path.join(ROOT, "tests", "golden", "albatite_SD_points.npz"))
        pts, vals = np.ascontiguousarray(z["rows"][:, :3]), z["rows"][:, 3].copy()
        kid = O.KERNEL_IDS["Spheroidal3Rbf"]
        kp = F.KernelParams(F.KernelType(kid), base_range=50.0, total_sill=10.0)
        tree = F.FmmTree(pts, 7, kp, True, True)
        pre = SchwarzPreconditioner(tree, pts, InterpolantSettings(kid, 3, None, 0.0, 50.0, 10.0), DDMParams())
        op = S.RbfSystemOperator(tree, 0, pre.monomial_matrix, 0.0)
        x, _ = S.fgmres(op, vals.copy(), pre, None, 20, 5, S.FittingAccuracy(0.01, S.FittingAccuracyType.Absolute))
        w, res = x[:, None].copy(), 5.0
        del tree, pre
    else:
        rng = np.random.default_rng(1)
        n = 1_000_000
        pts = rng.normal(size=(n, 3))
        pts = pts / np.linalg.norm(pts, axis=1)[:, None] * rng.uniform(0.5, 1.5, (n, 1))
        w, res = rng.standard_normal((n, 1)) / n, 0.02
        kp = F.KernelParams(F.FmmKernelType.LinearRbf)
    ext = np.concatenate([pts.min(0), pts.max(0)])
    te = F.FmmTree(pts, 7, kp, True, False, extents=list(ext[:3] - 10 * res) + list(ext[3:] + 10 * res))
    te.set_weights(w)
    te.set_local_coefficients(w)
    info = I.lattice_info(ext, res)
    sp = np.array([res / 2.0, res * np.sqrt(2.0) / 2.0, res / np.sqrt(2.0)])          # the lattice's x, y, z spacings
    origin = ext[:3] + info["lo"].astype(np.float64) * sp
    steps = np.array([[0.0, 0.0, sp[2]], [0.0, sp[1], 0.0], [sp[0], 0.0, 0.0]])         # index order (k, j, i)
    return te, w, origin, steps, list(info["shape"])


def child(a):
    te, w, origin, steps, shape = build_case(a.child)
    caps = [int(c) for c in a.caps.split(",")]
    nodes = int(np.prod(shape))
    rec = {"case": a.child, "shape": shape, "nodes": nodes, "sources": te.n_points, "steps_diagonal": [steps[2, 0], steps[1, 1], steps[0, 2]]}
    if not a.grid_only:
        k, j, i = np.meshgrid(*(np.arange(n, dtype=np.float64) for n in shape), indexing="ij")
        x = np.empty((nodes, 3), order="F")
        x[:, 0] = (origin[0] + i * steps[2, 0]).ravel()
        x[:, 1] = (origin[1] + j * steps[1, 1]).ravel()
        x[:, 2] = (origin[2] + k * steps[0, 2]).ravel()
        del k, j, i
        ts, ref = timed(lambda: te.evaluate_leaves(w, x), a.repeats)
        rec["existing_path_ms"] = ts
        del x
    else:
        ref = None
    rec["grid"] = {}
    for cap in caps:
        ts, (v, st) = timed(lambda: te.evaluate_grid(origin, steps, shape, max_job_targets=cap, return_stats=True), a.repeats)
        entry = {"ms": ts, "stats": st}
        if ref is not None:
            entry["max_abs_diff_to_existing"] = float(np.abs(v.reshape(-1, 1) - ref).max())
            entry["max_abs_value"] = float(np.abs(ref).max())
        rec["grid"][str(cap)] = entry
        print(f"[{a.child}] cap {cap}: {min(ts):.1f} ms  {st}", file=sys.stderr, flush=True)
    print("RESULT " + json.dumps(rec), flush=True)


def run_step(cmd, limit, quiet=False):
    """(exit status, stdout) of one step in a process group of its own; at the time limit the whole group is killed (the
    profiler's grandchild holds the device, not the profiler) and the status is None"""
    p = subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL if quiet else None, cwd=ROOT, start_new_session=True)
    try:
        out, _ = p.communicate(timeout=limit)
        return p.returncode, out.decode()
    except subprocess.TimeoutExpired:
        try:
            os.killpg(p.pid, signal.SIGKILL)
        except ProcessLookupError:
            pass
        p.communicate()
        return None, ""


def run_child(args, limit):
    status, out = run_step([sys.executable, os.path.abspath(__file__)] + args, limit)
    if status is None:
        return None, f"time limit of {limit} s"
    if status != 0:
        return None, f"exit status {status}"
    for line in out.splitlines():
        if line.startswith("RESULT "):
            return json.loads(line[7:]), None
    return None, "no result line"


def trace(case, cap, limit):
    """kernel name -> (calls, total ms, percentage) of one traced child that runs the grid alone at one cap"""
    prof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    out = tempfile.mkdtemp(prefix="evaluate_grid_trace_")
    cmd = [prof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "--", sys.executable, os.path.abspath(__file__), "--child", case, "--caps", str(cap),
           "--repeats", "1", "--grid-only"]
    try:
        status, _ = run_step(cmd, limit, quiet=True)
        if status is None:
            return {"error": f"time limit of {limit} s"}
        if status != 0:
            return {"error": f"exit status {status}"}
        rows = []
        for path in glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True):
            with open(path) as f:
                rows += list(csv.DictReader(f))
        if not rows or not {"Name", "Calls", "TotalDurationNs", "Percentage"} <= set(rows[0]):
            return {"error": "no kernel statistics in the profiler's output"}
        kernels = {r["Name"].split("(")[0][:90]: {"calls": int(r["Calls"]), "total_ms": float(r["TotalDurationNs"]) / 1e6,
                                                  "percent": float(r["Percentage"])} for r in rows}
        top = dict(sorted(kernels.items(), key=lambda kv: -kv[1]["total_ms"])[:8])
        return {"note": "fit or tree build, warm-up and one timed grid call in one process: the leaf-pass kernels run twice", "kernels": top}
    finally:
        shutil.rmtree(out, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="albatite,cloud")
    ap.add_argument("--caps", default="0,256,512,1024,2048")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "evaluate_grid_rate.json"))
    ap.add_argument("--limit", type=int, default=400, help="seconds per step")
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--grid-only", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    recs = []
    for case in a.cases.split(","):
        rec, err = run_child(["--child", case, "--caps", a.caps, "--repeats", str(a.repeats)], a.limit)
        if rec is None:
            recs.append({"case": case, "error": err})
            print(json.dumps(recs[-1]), flush=True)
            break                                   # a step that failed or ran out of time: start nothing more on the device
        best = {cap: min(e["ms"]) for cap, e in rec["grid"].items()}
        spread = max(max(e["ms"]) - min(e["ms"]) for e in rec["grid"].values())
        rec["best_ms"] = best
        rec["existing_path_best_ms"] = min(rec["existing_path_ms"])
        rec["largest_spread_ms"] = spread
        rec["best_cap"] = int(min(best, key=best.get))
        if not a.no_trace:
            rec["trace"] = {}
            for cap in sorted({0, rec["best_cap"]}):
                rec["trace"][str(cap)] = trace(case, cap, a.limit)
                if "error" in rec["trace"][str(cap)]:
                    break
        recs.append(rec)
        print(json.dumps(rec), flush=True)
        if any("error" in t for t in rec.get("trace", {}).values()):
            break                                   # likewise after a traced step that failed
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(recs, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
