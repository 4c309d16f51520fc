"""Host wall time of the boundary closure (finish="close_positive") against finish="clipped" in the same job: the
albatite isosurface_linear flow (Linear kernel, absolute 0.01, RBFInterpolator.build_isosurface with its defaults) at
resolution 5 and 2.5.  Per resolution: the two calls, best of --repeats after a warm-up, what the closure adds, the run-to-run
spread of the clipped call, the band's share of the cap (cut cells over all cap cells, band points, band triangles) and the
host time of the band (triangulation and selection, from the call's own clock).  On a checkout without the closure only the
clipped call is timed (the yardstick for "unchanged").  One JSON document to --out.

    python scripts/isosurface_closure_rate.py [--repeats 3] [--resolutions 5,2.5] [--out profiles/isosurface_closure.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def times(fn, repeats):
    fn()                                                        # warm-up
    ts, out = [], None
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
    return ts, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--resolutions", default="5,2.5")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from ferreus_rbf_rs_amd import isosurface as I
    from ferreus_rbf_rs_amd import rbf as RBF
    rows = np.load(os.path.join(ROOT, "tests", "golden", "albatite_SD_points.npz"))["rows"]
    pts, vals = np.ascontiguousarray(rows[:, :3]), np.ascontiguousarray(rows[:, 3])
    ext = np.concatenate([np.floor(pts.min(0)), np.ceil(pts.max(0))])
    acc = RBF.FittingAccuracy(0.01, RBF.FittingAccuracyType.Absolute)
    fit = RBF.RBFInterpolator(pts, vals, RBF.InterpolantSettings(RBF.RBFKernelType.Linear, fitting_accuracy=acc))
    has_closure = hasattr(I, "FINISH_CLOSE")
    recs = []
    for res in [float(x) for x in a.resolutions.split(",")]:
        t_clip, mesh = times(lambda: fit.build_isosurface(ext, res, 0.0, finish="clipped"), a.repeats)
        rec = {"case": "albatite_isosurface_linear", "resolution": res, "clipped_s": min(t_clip), "clipped_runs_s": t_clip,
               "clipped_spread_s": max(t_clip) - min(t_clip), "clipped_facets": int(len(mesh.facets))}
        if has_closure:
            t_close, closed = times(lambda: fit.build_isosurface(ext, res, 0.0, finish="close_positive", return_stats=True), a.repeats)
            c = closed.stats["closure"]
            cells = 2 * sum(int(np.ceil((ext[3 + u] - ext[u]) / res)) * int(np.ceil((ext[3 + v] - ext[v]) / res)) for u, v in ((1, 2), (0, 2), (0, 1)))
            rec.update({"close_positive_s": min(t_close), "close_positive_runs_s": t_close, "closure_adds_s": min(t_close) - min(t_clip),
                        "facets": int(len(closed.facets)), "cap_facets": int(len(closed.facets) - len(mesh.facets)),
                        "cap_cells": cells, "cut_cells": int(sum(c["cut_cells"])), "cut_share": sum(c["cut_cells"]) / cells,
                        "band_points": c["band_points"], "band_triangles": c["band_triangles"], "whole_cells_kept": int(sum(c["whole_cells_kept"])),
                        "band_host_s": c["band_host_us"] * 1e-6, "closure_stats": c})
        print(json.dumps(rec), flush=True)
        recs.append(rec)
    doc = {"what": "host wall seconds of RBFInterpolator.build_isosurface on the albatite isosurface_linear fit, finish=clipped against "
                   "finish=close_positive in the same job; best of %d after a warm-up; band_host_s from the call's own clock (last run)" % a.repeats,
           "cases": recs}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
