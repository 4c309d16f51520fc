"""Whole-call times of the isosurfacer's three kinds of field on the albatite fit (Linear kernel, absolute 0.01) at one
resolution, all in one job on one device, one warm-up and the best of --repeats each:

  (a) RBFInterpolator.build_isosurface: one tree's field with its terms;
  (b) the same model as a one-operand rmt.FieldExpr: what the operand column, the extra synchronisation and the program
      kernel cost;
  (c) the same model as a Python callable (evaluate_targets, with evaluate_targets_with_gradients for the seeds): every batch
      crosses the host and Python, as the reference's isosurface_linear_rmt does;
  (d) the model under a synthetic 2-D topography fit, maximum(field(model), height_field(topo)): FieldExpr against callable.

Every case runs with the facade's defaults (curvature clusters, followed from the data points, clipped, rollback).  Per
case: seconds (best and all), nodes evaluated, vertices and facets.  One JSON document to --out.

    python scripts/composite_field_rate.py [--repeats 3] [--resolution 5] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, repeats):
    fn()                                                             # warm-up
    ts, out = [], None
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
    return ts, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--resolution", type=float, default=5.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from ferreus_rbf_rs_amd import rbf as RBF
    from ferreus_rbf_rs_amd import rmt
    K = RBF.RBFKernelType
    acc = RBF.FittingAccuracy(0.01, RBF.FittingAccuracyType.Absolute)
    rows = np.load(os.path.join(ROOT, "tests", "golden", "albatite_SD_points.npz"))["rows"]
    pts, vals = np.ascontiguousarray(rows[:, :3]), np.ascontiguousarray(rows[:, 3])
    ext = np.concatenate([np.floor(pts.min(0)), np.ceil(pts.max(0))])
    res = a.resolution
    model = RBF.RBFInterpolator(pts, vals, RBF.InterpolantSettings(K.Linear, fitting_accuracy=acc))
    src = model.source_points
    ev = np.concatenate([np.minimum(src.min(0), ext[:3]) - 10.0 * res, np.maximum(src.max(0), ext[3:]) + 10.0 * res])
    # a topography through the middle of the data: 2,000 of its (x, y) with a smooth height
    rng = np.random.default_rng(0)
    xy = src[rng.choice(len(src), min(2000, len(src)), replace=False)][:, :2]
    mid, span = 0.5 * (ext[2] + ext[5]), ext[3:] - ext[:3]
    height = mid + 0.15 * span[2] * np.sin(2.0 * np.pi * (xy[:, 0] - ext[0]) / span[0]) * np.cos(2.0 * np.pi * (xy[:, 1] - ext[1]) / span[1])
    topo = RBF.RBFInterpolator(xy, height, RBF.InterpolantSettings(K.Linear, fitting_accuracy=acc))
    ev2 = np.concatenate([np.minimum(xy.min(0), ext[:2]) - 10.0 * res, np.maximum(xy.max(0), ext[3:5]) + 10.0 * res])
    counted = [0]

    def counting(fn):
        def f(x):
            counted[0] += len(x)
            return fn(x)
        return f

    def model_callable():
        model.build_evaluator(ev)
        counted[0] = 0
        return rmt.build_isosurface(src, ext, res, 0.0, counting(model.evaluate_targets),
                                    gradient_fn=counting(model.evaluate_targets_with_gradients), return_stats=True)

    def clipped_values(x):
        return np.maximum(model.evaluate_targets(x)[:, 0], x[:, 2] - topo.evaluate_targets(np.ascontiguousarray(x[:, :2]))[:, 0])

    def clipped_callable():
        model.build_evaluator(ev)
        topo.build_evaluator(ev2)
        counted[0] = 0
        return rmt.build_isosurface(src, ext, res, 0.0, counting(clipped_values), return_stats=True)

    clipped = rmt.maximum(rmt.field(model), rmt.height_field(topo, axis=2))
    cases = [("a_interpolator", lambda: model.build_isosurface(ext, res, 0.0, return_stats=True), False),
             ("b_field_expr_one_operand", lambda: rmt.build_isosurface(src, ext, res, 0.0, rmt.field(model), return_stats=True), False),
             ("c_callable_evaluate_targets", model_callable, True),
             ("d_clipped_field_expr", lambda: rmt.build_isosurface(src, ext, res, 0.0, clipped, return_stats=True), False),
             ("d_clipped_callable", clipped_callable, True)]
    doc = {"points": int(len(src)), "topography_points": int(len(xy)), "resolution": res, "extents": ext.tolist(), "repeats": a.repeats,
           "cases": {}}
    for name, fn, is_callable in cases:
        ts, mesh = timed(fn, a.repeats)
        fol = mesh.stats["follow"]
        rec = {"seconds": min(ts), "all_seconds": ts, "nodes_evaluated": int(fol["nodes_evaluated"]), "nodes": int(fol["nodes"]),
               "newton_steps": int(fol["newton_steps"]), "vertices": int(len(mesh.vertices)), "facets": int(len(mesh.facets))}
        if is_callable:
            rec["points_handed_to_python"] = int(counted[0])
        doc["cases"][name] = rec
        print(name, json.dumps(rec), flush=True)
    ta = doc["cases"]["a_interpolator"]["all_seconds"]
    doc["a_spread_seconds"] = max(ta) - min(ta)
    doc["b_minus_a_seconds"] = doc["cases"]["b_field_expr_one_operand"]["seconds"] - doc["cases"]["a_interpolator"]["seconds"]
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
    print(json.dumps({k: v for k, v in doc.items() if k != "cases"}))


if __name__ == "__main__":
    main()
