"""Host wall times of ferreus_rbf_rs_amd.rbf.RBFInterpolator: the three example flows of the reference on the albatite
fixture (isosurface_linear, isosurface_spheroidal_drift, isosurface_trend_linear: fit, then build_isosurface at
resolution 5) and a uniform cloud (default 1M points, Linear kernel, absolute 0.01).  Per case: duplicate removal on the
host path against the device path in the same run (the only comparison made here: nobody has measured the rest before,
so there is no yardstick for it), the trend and setup, the solver's setup and the solve (from the fit's own stage
clock), a one-shot evaluate of 1M targets and build_isosurface.  Every figure is the best of --repeats after one
warm-up, except a fit marked "single_run".  One JSON document to --out.

    python scripts/rbf_interpolator_rate.py [--repeats 3] [--cloud-points 1000000] [--cases albatite,cloud] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def best(fn, repeats, warm=True):
    if warm:
        fn()
    ts, out = [], None
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
    return min(ts), out


def dedup_times(RBF, pts, st, repeats):
    ext = np.concatenate([pts.min(0), pts.max(0)])
    tol = RBF.duplicate_cutoff_distance(st, float((ext[3:] - ext[:3]).max()))
    t_host, kh = best(lambda: RBF.remove_duplicates(pts, tol, 0), repeats)
    t_dev, (kd, rounds) = best(lambda: RBF.remove_duplicates(pts, tol, 1, return_rounds=True), repeats)
    assert np.array_equal(kh, kd)
    return {"tolerance": tol, "kept": int(len(kd)), "host_s": t_host, "device_s": t_dev, "device_rounds": int(rounds),
            "device_over_host": t_dev / t_host}


def flow(RBF, name, pts, vals, st, trend, extents, resolution, repeats, fit_repeats, targets):
    fits = []
    for _ in range(fit_repeats + (1 if fit_repeats > 1 else 0)):          # the first of several is the warm-up
        fits.append(RBF.RBFInterpolator(pts, vals, st, global_trend=trend))
    timed = fits[1:] if fit_repeats > 1 else fits
    fit = min(timed, key=lambda f: f.stage_seconds["total"])
    rec = {"case": name, "points": int(len(pts)), "kernel": st.kernel_type.name, "drift": st.drift.name, "trend": trend is not None,
           "fit": "best_of_%d" % fit_repeats if fit_repeats > 1 else "single_run",
           "iterations": [len(h) for h in fit.residual_histories], "final_residual": [h[-1][1] for h in fit.residual_histories if h],
           "stage_seconds": {k: float(v) for k, v in fit.stage_seconds.items()},
           "duplicate_removal": dedup_times(RBF, pts, st, repeats)}
    t_eval, v = best(lambda: fit.evaluate(targets), repeats)
    rec["evaluate"] = {"targets": int(len(targets)), "seconds": t_eval, "targets_per_s": len(targets) / t_eval}
    t_iso, mesh = best(lambda: fit.build_isosurface(extents, resolution, 0.0), repeats)
    rec["build_isosurface"] = {"resolution": resolution, "seconds": t_iso, "vertices": int(len(mesh.vertices)),
                               "facets": int(len(mesh.facets))}
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--cloud-points", type=int, default=1_000_000)
    ap.add_argument("--cases", default="albatite,cloud")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from ferreus_rbf_rs_amd import rbf as RBF
    K = RBF.RBFKernelType
    acc = RBF.FittingAccuracy(0.01, RBF.FittingAccuracyType.Absolute)
    rng = np.random.default_rng(0)
    recs = []
    if "albatite" in a.cases:
        rows = np.load(os.path.join(ROOT, "tests", "golden", "albatite_SD_points.npz"))["rows"]
        pts, vals = np.ascontiguousarray(rows[:, :3]), np.ascontiguousarray(rows[:, 3])
        ext = np.concatenate([np.floor(pts.min(0)), np.ceil(pts.max(0))])
        targets = ext[:3] + (ext[3:] - ext[:3]) * rng.random((1_000_000, 3))
        flows = [("isosurface_linear", RBF.InterpolantSettings(K.Linear, fitting_accuracy=acc), None),
                 ("isosurface_spheroidal_drift", RBF.InterpolantSettings(K.Spheroidal, RBF.SpheroidalOrder.Three, RBF.Drift.Constant,
                                                                         base_range=50.0, total_sill=10.0, fitting_accuracy=acc), None),
                 ("isosurface_trend_linear", RBF.InterpolantSettings(K.Linear, fitting_accuracy=acc),
                  RBF.GlobalTrend.three(87, 255, 25, 4, 2, 1))]
        for name, st, trend in flows:
            recs.append(flow(RBF, name, pts, vals, st, trend, ext, 5.0, a.repeats, a.repeats, targets))
    if "cloud" in a.cases:
        n = a.cloud_points
        pts = rng.random((n, 3))
        vals = np.linalg.norm(pts - 0.5, axis=1) - 0.3 + 0.05 * np.sin(7.0 * pts[:, 0])
        targets = rng.random((1_000_000, 3))
        res = 1.0 / 200.0
        recs.append(flow(RBF, "cloud", pts, vals, RBF.InterpolantSettings(K.Linear, fitting_accuracy=acc), None,
                         np.array([0.0, 0.0, 0.0, 1.0, 1.0, 1.0]), res, a.repeats, a.repeats, targets))
    doc = {"what": "host wall seconds of RBFInterpolator stages; best of %d after a warm-up unless a fit says single_run" % a.repeats,
           "compared": "duplicate removal: host path against device path in the same run; nothing else has a yardstick",
           "cases": recs}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
