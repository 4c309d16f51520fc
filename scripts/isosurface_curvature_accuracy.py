"""Accuracy of cluster="curvature" on the device against the numpy restatement (tests/isosurface_curvature_restatement.py),
in units of the bar of the tests: with G_v the largest |v64 - v80| / r over the vertex coordinates between the
restatement in float64 and in long double, the bar is 200 * max(G_v, 1e-15) * r.  Cases: the four analytic fields of the
tests on [0, 2]^3 at r = 0.25 and the noisy spheres of the clustered tests.  Per case: G_v, G_w, the bar, the largest
device gap and that gap in bars, whether the facets are the restatement's, and the counts.  One JSON line per case, and
the list to --out when given.

    python scripts/isosurface_curvature_accuracy.py [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="JSON file for the list of results")
    a = ap.parse_args()
    import ferreus_rbf_rs_amd as F
    import isosurface_restatement as R
    import isosurface_curvature_restatement as K
    cases = []
    lat = R.Lattice(K.EXT2, K.R2)
    for name in K.FIELDS:
        cases.append((name, K.EXT2, K.R2, lat, K.analytic(name, lat.world(lat.node_ijk()))))
    ext = [0.0, 0.0, 0.0, 6.0, 6.0, 6.0]
    for amp, seed, r in ((0.2, 3, 0.2), (0.05, 1, 0.1), (0.15, 1, 0.1)):
        big = R.Lattice(ext, r)
        field = (np.linalg.norm(big.world(big.node_ijk()) - [3.0, 3.0, 3.0], axis=-1) - 2.0
                 + amp * np.random.default_rng(seed).standard_normal(big.shape))
        cases.append((f"noisy_sphere_{amp}_r{r}", ext, r, big, field))
    recs = []
    for name, e, r, lt, field in cases:
        gv, gw, want, far = K.gaps(lt, field, 0.0)
        bar = K.bars(gv, gw, r)[0]
        v, f, stats = F.isosurface_from_values(field, e, r, 0.0, cluster="curvature", return_stats=True)
        same = bool(np.array_equal(f, want["facets"]) and v.shape == want["vertices"].shape)
        gap = float(np.abs(v - want["vertices"]).max(initial=0.0)) if same else float("nan")
        rec = {"case": name, "resolution": r, "lattice_shape": [int(x) for x in lt.shape], "G_v": gv, "G_w": gw,
               "same_fallback_edges": bool(np.array_equal(want["fallback"], far["fallback"])), "bar": bar,
               "device_gap": gap, "device_gap_in_bars": gap / bar, "facets_equal": same,
               "curvature_stats": stats["curvature"], "stats_equal": stats["curvature"] == want["curvature"]}
        print(json.dumps(rec), flush=True)
        recs.append(rec)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(recs, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
