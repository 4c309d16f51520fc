#!/usr/bin/env python3
"""FGMRES with host vectors against FGMRES with device vectors (solvers.fgmres vectors=) on the same operators, in one
process on one device: a warm-up solve of each route, then the two routes alternating, wall time around the whole solve
(which ends in a stream synchronise), iteration counts and residual histories side by side.  Cases: "config3" (uniform
random points, thin-plate spline, DDMParams.for_points: the workload of profiles/r03_z_config3_tps_10M_stage_times.txt)
and "albatite" (tests/golden/albatite_SD_points.npz, Linear kernel, the examples' absolute tolerance 0.01).  One JSON
line per case; the stage split (operator, preconditioner, vectors) comes from a separate run with BBFMM_VERBOSE set,
which synchronises around the stages."""
import argparse, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ferreus_rbf_rs_amd as F
from ferreus_rbf_rs_amd import solvers as S
from ferreus_rbf_rs_amd.ddm import DDMParams, InterpolantSettings, SchwarzPreconditioner

ap = argparse.ArgumentParser()
ap.add_argument("--case", choices=["config3", "albatite"], default="config3")
ap.add_argument("--points", type=int, default=10_000_000, help="config3 only")
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--deterministic", action="store_true", help="BBFMM_FLAG_DETERMINISTIC on the tree")
a = ap.parse_args()

if a.case == "config3":
    kid, order, n = 1, 9, a.points
    pts = np.random.default_rng(42).random((n, 3))
    vals = np.sin(3 * pts[:, 0]) * np.cos(2 * pts[:, 1]) + 0.5 * pts[:, 2] ** 2
    ddm, tol = DDMParams.for_points(n), S.FittingAccuracy(1e-6)
else:
    rows = np.load(os.path.join(ROOT, "tests", "golden", "albatite_SD_points.npz"))["rows"]
    pts, vals = rows[:, :3].copy(), rows[:, 3].copy()
    kid, order, n = 0, 7, len(pts)
    ddm, tol = DDMParams(), S.FittingAccuracy(0.01, S.FittingAccuracyType.Absolute)
st = InterpolantSettings(kid, 3)
t0 = time.time()
tree = F.FmmTree(pts, order, F.KernelParams(F.KernelType(kid)), True, True, deterministic=a.deterministic)
pre = SchwarzPreconditioner(tree, pts, st, ddm)
op = S.RbfSystemOperator(tree, st.basis_size, pre.monomial_matrix, 0.0)
t_setup = time.time() - t0
rhs = np.concatenate([vals, np.zeros(st.basis_size)])


def solve(vectors):
    t = time.time()
    x, hist = S.fgmres(op, rhs, pre, None, 20, 5, tol, vectors=vectors)
    return time.time() - t, x, [r for _, r in hist]


out = {"case": a.case, "points": n, "levels": pre.num_levels, "setup_s": round(t_setup, 2), "host_s": [], "device_s": []}
for vectors in ("host", "device"):                    # warm-up: code objects, plans, the device operator's upload
    solve(vectors)
for _ in range(a.repeats):                            # alternating, so that drift of the machine hits both alike
    for vectors in ("host", "device"):
        dt, x, hist = solve(vectors)
        out[vectors + "_s"].append(round(dt, 4))
        out[vectors + "_history"], out[vectors + "_x"] = hist, x
hh, hd = out["host_history"], out["device_history"]
xh, xd = out.pop("host_x"), out.pop("device_x")
out["iterations"] = [len(hh), len(hd)]
out["final_residuals"] = [hh[-1], hd[-1]]
out["largest_relative_history_difference"] = max(abs(p - q) / p for p, q in zip(hh, hd)) if len(hh) == len(hd) else None
out["largest_coefficient_difference_over_max"] = float(np.abs(xh - xd).max() / np.abs(xh).max())
out["best_host_s"], out["best_device_s"] = min(out["host_s"]), min(out["device_s"])
print(json.dumps(out), flush=True)
