"""Rate of the device isosurface extraction (FmmTree.build_isosurface): the albatite Spheroidal example at resolution
5 (examples/isosurface_spheroidal.rs) and a 1M-point cloud.  Reports the field pass alone (return_field off, one
isovalue; measured as the extraction of an isovalue that no node crosses), the whole call, the extraction share
(whole minus field) and triangles per second: one JSON line per case, and the list to --out when given.  With
--clusters none,average every case is timed with each method in the same run on the same tree (the field pass is the
same work for both), and the clustering counts are recorded.  With --finish raw,clipped every method is also timed
with the mesh clipped to the extents and cleaned on the device: finish_ms is what "clipped" adds to the whole call of
"raw" in the same run, clip_mesh_ms the same stage alone on the raw mesh (clip_mesh: with the upload of the mesh), and
the finish counts are recorded.  With --self-intersections ignore,rollback the clustered raw call of every case is
also timed with the self-intersection rollback on: rollback_ms is what it adds to the clustered call without it in the
same run (the yardstick), and its counts are recorded; a third case, the noisy sphere (0.15 * standard_normal(seed 1) at
resolution 0.1, a caller's field), is one where the rollback has sample points to roll back.  With --follow
dense,surface the unclustered raw call of every case is also timed with follow="surface" from the default seeds (the
source points), beside the dense call of the same run on the same tree, with brick sides 8 and 16: the whole call, the
nodes evaluated of the nodes of E, the rounds, and the host time of the seed stage, the wavefront and the extraction.
With "curvature" among the --clusters the field of every case is also fetched once and each clustered method is timed on
it as a caller's field (source "values": the upload and the extraction, no field pass, so the methods differ by what
their kernels cost): curvature_ms is what "curvature" adds to "average" in the same run (the yardstick: the parent's
path), and its counts are recorded.  --cases picks the cases, --values-only leaves the calls on the tree out (the run to
put under a kernel trace for the share of curvature_weights_kernel).

    python scripts/isosurface_rate.py [--repeats 3] [--clusters none,average] [--finish raw,clipped]
                                      [--self-intersections ignore,rollback] [--follow dense,surface] [--out FILE]
                                      [--cases albatite,cloud] [--values-only]
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


def measure(te, ext, res, iso, repeats, label, cluster="none", finish="raw", raw=None):
    from ferreus_rbf_rs_amd import isosurface as I
    info = I.lattice_info(ext, res)
    kw = {"cluster": cluster, "return_stats": True}
    if finish != "raw":
        kw["finish"] = finish
    t_all, (v, f, stats) = timed(lambda: te.build_isosurface(ext, res, iso, **kw), repeats)
    t_field, _ = timed(lambda: te.build_isosurface(ext, res, 1e300, **kw), repeats)   # nothing crosses: field + classify
    rec = {"case": label, "cluster": cluster, "finish": finish, "resolution": res, "lattice_shape": list(info["shape"]),
           "nodes_evaluated": info["n_nodes"],
           "keys": info["n_keys"], "vertices": int(len(v)), "facets": int(len(f)), "call_ms": t_all,
           "field_ms": t_field, "extraction_ms": t_all - t_field, "triangles_per_s": len(f) / (t_all * 1e-3),
           "nodes_per_s": info["n_nodes"] / (t_all * 1e-3)}
    if cluster != "none":
        rec["stats"] = {k: x for k, x in stats.items() if k != "finish"}
    if finish != "raw":
        rec["finish_stats"] = stats["finish"]
        if raw is not None:                         # the raw record of the same run and its mesh
            rec["finish_ms"] = t_all - raw[0]["call_ms"]
            rec["clip_mesh_ms"], _ = timed(lambda: I.clip_mesh(raw[1], raw[2], ext, tree=te), repeats)
    print(json.dumps(rec), flush=True)
    return (rec, v, f) if finish == "raw" else rec


def measure_rollback(call, repeats, label, res, yardstick_ms=None):
    """The clustered raw call with the rollback on, beside the same call without it (timed here unless given)."""
    kw = {"cluster": "average", "return_stats": True}
    if yardstick_ms is None:
        yardstick_ms, _ = timed(lambda: call(**kw), repeats)
    t_roll, (v, f, stats) = timed(lambda: call(self_intersections="rollback", **kw), repeats)
    rec = {"case": label, "cluster": "average", "finish": "raw", "self_intersections": "rollback", "resolution": res,
           "vertices": int(len(v)), "facets": int(len(f)), "call_ms": t_roll, "call_ms_without": yardstick_ms,
           "rollback_ms": t_roll - yardstick_ms, "intersection_stats": stats["self_intersections"],
           "stats": {k: x for k, x in stats.items() if k != "self_intersections"}}
    print(json.dumps(rec), flush=True)
    return rec


def measure_follow(te, ext, res, iso, repeats, label, dense):
    """follow="surface" with the default seeds beside the dense record of the same run, per brick side."""
    recs = []
    for brick in ("8", "16"):
        os.environ["BBFMM_ISO_BRICK"] = brick
        try:
            t_all, (v, f, stats) = timed(lambda: te.build_isosurface(ext, res, iso, return_stats=True, follow="surface"), repeats)
        finally:
            del os.environ["BBFMM_ISO_BRICK"]
        fol = {k: x for k, x in stats["follow"].items() if k != "visited"}
        rec = {"case": label, "cluster": "none", "finish": "raw", "follow": "surface", "brick": int(brick), "resolution": res,
               "vertices": int(len(v)), "facets": int(len(f)), "call_ms": t_all, "call_ms_dense": dense["call_ms"],
               "facets_dense": dense["facets"], "nodes_evaluated": fol["nodes_evaluated"], "nodes": fol["nodes"],
               "share_evaluated": fol["nodes_evaluated"] / max(fol["nodes"], 1), "rounds": fol["rounds"],
               "seed_ms": fol["seed_ms"], "wavefront_ms": fol["wavefront_ms"], "extract_ms": fol["extract_ms"],
               "follow_stats": fol}
        print(json.dumps(rec), flush=True)
        recs.append(rec)
    return recs


def measure_values(te, ext, res, iso, repeats, label, methods):
    """The clustered methods on the tree's field taken as a caller's field: the extraction without the field pass."""
    from ferreus_rbf_rs_amd import isosurface as I
    _, field = te.build_isosurfaces(ext, res, [iso], return_field=True)
    recs, yardstick = [], None
    for method in methods:
        t, (v, f, stats) = timed(lambda: I.isosurface_from_values(field, ext, res, iso, tree=te, cluster=method, return_stats=True),
                                 repeats)
        rec = {"case": label, "source": "values", "cluster": method, "resolution": res, "lattice_shape": list(field.shape),
               "vertices": int(len(v)), "facets": int(len(f)), "call_ms": t, "stats": stats}
        if method == "average":
            yardstick = t
        if method == "curvature" and yardstick is not None:
            rec["call_ms_average"], rec["curvature_ms"] = yardstick, t - yardstick
        print(json.dumps(rec), flush=True)
        recs.append(rec)
    return recs


def measure_all(te, ext, res, iso, a, label):
    recs = []
    methods = a.clusters.split(",")
    if "curvature" in methods:
        recs += measure_values(te, ext, res, iso, a.repeats, label, [m for m in methods if m != "none"])
    if a.values_only:
        return recs
    for method in methods:
        raw = None
        for finish in a.finish.split(","):
            if finish == "raw":
                raw = measure(te, ext, res, iso, a.repeats, label, method)
                recs.append(raw[0])
                if method == "none" and "surface" in a.follow.split(","):
                    recs += measure_follow(te, ext, res, iso, a.repeats, label, raw[0])
                if method == "average" and "rollback" in a.self_intersections.split(","):
                    recs.append(measure_rollback(lambda **kw: te.build_isosurface(ext, res, iso, **kw), a.repeats, label, res,
                                                 raw[0]["call_ms"]))
            else:
                recs.append(measure(te, ext, res, iso, a.repeats, label, method, finish, raw))
    return recs


def noisy_sphere(a):
    """A caller's field on [0, 6]^3 at resolution 0.1: |x - (3, 3, 3)| - 2 + 0.15 * standard_normal(seed 1)."""
    import ferreus_rbf_rs_amd as F
    from ferreus_rbf_rs_amd import isosurface as I
    ext, res = [0.0, 0.0, 0.0, 6.0, 6.0, 6.0], 0.1
    info = I.lattice_info(ext, res)
    nk, nj, ni = info["shape"]
    k, j, i = np.meshgrid(np.arange(nk), np.arange(nj), np.arange(ni), indexing="ij")
    sp = np.array([res / 2.0, res * np.sqrt(2.0) / 2.0, res / np.sqrt(2.0)])
    w = np.stack([(i + info["lo"][0]) * sp[0], (j + info["lo"][1]) * sp[1], (k + info["lo"][2]) * sp[2]], -1)
    field = np.linalg.norm(w - 3.0, axis=-1) - 2.0 + 0.15 * np.random.default_rng(1).standard_normal((nk, nj, ni))
    return [measure_rollback(lambda **kw: F.isosurface_from_values(field, ext, res, 0.0, **kw), a.repeats,
                             "noisy_sphere_r0.1", res)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--clusters", default="none", help="comma-separated cluster methods, each timed on every case")
    ap.add_argument("--finish", default="raw", help="comma-separated finishes (raw first), each timed with every method")
    ap.add_argument("--self-intersections", default="ignore",
                    help="ignore,rollback: also time the clustered call with the self-intersection rollback")
    ap.add_argument("--follow", default="dense", help="dense,surface: also time the raw call with follow='surface'")
    ap.add_argument("--out", default=None, help="JSON file for the list of results")
    ap.add_argument("--cases", default="albatite,cloud", help="comma-separated cases to run")
    ap.add_argument("--values-only", action="store_true", help="with curvature among the clusters: only the caller's-field timings")
    a = ap.parse_args()
    import ferreus_rbf_rs_amd as F
    from ferreus_rbf_rs_amd import solvers as S
    from ferreus_rbf_rs_amd.ddm import DDMParams, InterpolantSettings, SchwarzPreconditioner
    from oracle import bbfmm_oracle as O
    recs = []
    if "albatite" in a.cases.split(","):
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
        recs += measure_all(te, ext, res, 0.0, a, "albatite_spheroidal_r5")
        del te, tree, pre
    if "cloud" in a.cases.split(","):
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
        recs += measure_all(t1, ext, res, fmid, a, "cloud_1M_linear")
        del t1
    if "rollback" in a.self_intersections.split(",") and "average" in a.clusters.split(","):
        recs += noisy_sphere(a)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(recs, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
