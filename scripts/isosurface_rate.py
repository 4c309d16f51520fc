"""Rate of the device isosurface extraction (FmmTree.build_isosurface): the albatite Spheroidal example at resolution
5 (examples/isosurface_spheroidal.rs) and a 1M-point cloud.  Reports the field pass alone (return_field off, one
isovalue; measured as the extraction of an isovalue that no node crosses), the whole call, the extraction share
(whole minus field) and triangles per second: one JSON line per case, and the list to --out when given.  With
--clusters none,average every case is timed with each method in the same run on the same tree (the field pass is the
same work for both), and the clustering counts are recorded.

    python scripts/isosurface_rate.py [--repeats 3] [--clusters none,average] [--out FILE]
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
    fn()                                            # warm-up (arena, target-set scratch)
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
    return min(ts) * 1e3, out


def measure(te, ext, res, iso, repeats, label, cluster="none"):
    from ferreus_rbf_rs_amd import isosurface as I
    info = I.lattice_info(ext, res)
    kw = {"cluster": cluster, "return_stats": True}
    t_all, (v, f, stats) = timed(lambda: te.build_isosurface(ext, res, iso, **kw), repeats)
    t_field, _ = timed(lambda: te.build_isosurface(ext, res, 1e300, **kw), repeats)   # nothing crosses: field + classify
    rec = {"case": label, "cluster": cluster, "resolution": res, "lattice_shape": list(info["shape"]),
           "nodes_evaluated": info["n_nodes"],
           "keys": info["n_keys"], "vertices": int(len(v)), "facets": int(len(f)), "call_ms": t_all,
           "field_ms": t_field, "extraction_ms": t_all - t_field, "triangles_per_s": len(f) / (t_all * 1e-3),
           "nodes_per_s": info["n_nodes"] / (t_all * 1e-3)}
    if cluster != "none":
        rec["stats"] = stats
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--clusters", default="none", help="comma-separated cluster methods, each timed on every case")
    ap.add_argument("--out", default=None, help="JSON file for the list of results")
    a = ap.parse_args()
    import ferreus_rbf_rs_amd as F
    from ferreus_rbf_rs_amd import solvers as S
    from ferreus_rbf_rs_amd.ddm import DDMParams, InterpolantSettings, SchwarzPreconditioner
    from oracle import bbfmm_oracle as O
    recs = []
    # albatite, Spheroidal order 3, range 50, sill 10, fitted on the device
    z = np.load(os.path.join(ROOT, "tests", "golden", "albatite_SD_points.npz"))
    pts, vals = np.ascontiguousarray(z["rows"][:, :3]), z["rows"][:, 3].copy()
    kid = O.KERNEL_IDS["Spheroidal3Rbf"]
    kp = F.KernelParams(F.KernelType(kid), base_range=50.0, total_sill=10.0)
    tree = F.FmmTree(pts, 7, kp, True, True)
    pre = SchwarzPreconditioner(tree, pts, InterpolantSettings(kid, 3, None, 0.0, 50.0, 10.0), DDMParams())
    op = S.RbfSystemOperator(tree, 0, pre.monomial_matrix, 0.0)
    x, _ = S.fgmres(op, vals.copy(), pre, None, 20, 5, S.FittingAccuracy(0.01, S.FittingAccuracyType.Absolute))
    res = 5.0
    ext = np.concatenate([pts.min(0), pts.max(0)])
    te = F.FmmTree(pts, 7, kp, True, False, extents=list(ext[:3] - 10 * res) + list(ext[3:] + 10 * res))
    te.set_weights(x[:, None].copy())
    te.set_local_coefficients(x[:, None].copy())
    for method in a.clusters.split(","):
        recs.append(measure(te, ext, res, 0.0, a.repeats, "albatite_spheroidal_r5", method))
    del te, tree, pre
    # 1M points on and around a sphere of radius 1, Linear kernel, random weights (a smooth field, not a fit)
    rng = np.random.default_rng(1)
    n = 1_000_000
    p = rng.normal(size=(n, 3))
    p = p / np.linalg.norm(p, axis=1)[:, None] * rng.uniform(0.5, 1.5, (n, 1))
    w = rng.standard_normal((n, 1)) / n
    res = 0.02
    ext = np.concatenate([p.min(0), p.max(0)])
    t1 = F.FmmTree(p, 7, F.KernelParams(F.FmmKernelType.LinearRbf), True, False,
                   extents=list(ext[:3] - 10 * res) + list(ext[3:] + 10 * res))
    t1.set_weights(w)
    t1.set_local_coefficients(w)
    fmid = float(np.median(t1.evaluate_leaves(None, p[:2000])))
    for method in a.clusters.split(","):
        recs.append(measure(t1, ext, res, fmid, a.repeats, "cloud_1M_linear", method))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(recs, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
