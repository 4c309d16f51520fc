"""Measured accuracy of the Schwarz preconditioner's local solvers (csrc/ddm_kernels.hip) against the long-double restatement
and the derived bounds of tests/ddm_local_reference.py, through the test hook bbfmm_ddm_debug_level_*: for every case of
tests/test_gpu_ddm_local.py and every domain, the measured error divided by its bound for the assembled Q^T A Q, the factor
(A - L L^T) and the solve (backward error; rows of the special points), with kappa_blk (the 64 x 64 diagonal blocks of the
factor) and, on the large path, kappa_1024.  The inputs and the checks are those of the tests (tests/ddm_local_cases.py); a
bound that does not hold raises, as in the tests.  Needs a GPU.

    python scripts/ddm_local_accuracy.py [--out profiles/ddm_local_accuracy.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ddm_local_accuracy.json"))
    ap.add_argument("--no-build", action="store_true", help="use the library as it lies in the tree")
    args = ap.parse_args()
    if not args.no_build:
        import __graft_entry__ as entry
        entry.build()
    import numpy as np
    import torch

    import bench
    import ddm_local_cases as C
    import ddm_local_reference as R

    rec = {"source_hash": bench.source_hash(), "device": torch.cuda.get_device_name(0),
           "unit": "measured error / derived bound (1 = the bound); u = 2^-53", "bounds": "tests/ddm_local_reference.py",
           "inputs": "tests/ddm_local_cases.py", "cases": []}

    def measure(name, pts, doms, st, pick=None, rows_of=None):
        lv = C.make_level(pts, doms, st)
        assembled, factor = lv.assembled(), lv.factor()
        values = np.random.default_rng(1).standard_normal(pts.shape[0])
        out = lv.solve(values, np.full(pts.shape[0], C.SENTINEL), True)
        for i in (range(len(doms)) if pick is None else pick):
            rows = rows_of(lv.m[i]) if rows_of else None
            e = {"case": name, "kernel_id": st.kernel_type, "domain": i, "m": lv.m[i], "k": lv.k[i], "mode": lv.mode[i],
                 "path": "large" if lv.is_big else "per-domain",
                 "assembly": round(C.check_assembly(lv, pts, st, assembled, i, rows=rows), 4)}
            if lv.mode[i] == 0 and not lv.lu_taken:
                f = C.check_factor(lv, assembled, factor, i, rows=rows)
                s = C.check_solve(lv, factor, values, out, i)
                e.update({"factor": round(f["ratio"], 4), "kappa_blk": round(f["kappa_blk"], 2),
                          "factor_bound_over_u_LLt": round(f["c_eff"], 1), "solve": float(f"{s['ratio']:.4g}"),
                          "solve_special_rows": round(s["ratio_special"], 4)})
                if lv.is_big:
                    e["kappa_1024"] = round(s["kappa_1024"], 1)
            rec["cases"].append(e)
            print(e, flush=True)
        lv.close()

    pts, doms, st, _ = C.flagship()
    measure("every block edge, linear drift in 3-D, a coplanar domain, duplicated points", pts, doms, st)
    for dim, drift, k in ((3, -1, 0), (3, 0, 1), (3, 2, 10), (1, 1, 2), (1, 2, 3), (2, 1, 3), (2, 2, 6)):
        pts, doms, st, _ = C.sized(100 + 10 * dim + k, dim, drift, C.M_FEW, k)
        measure(f"polynomial part: {dim}-D, degree {drift}", pts, doms, st)
    for kid, drift, nugget, br in ((0, 0, 0.0, 1.0), (1, 1, 0.0, 1.0), (2, 1, 0.0, 1.0), (3, -1, 0.02, 0.3), (4, 0, 0.02, 0.3),
                                   (5, 1, 0.02, 0.5), (6, 2, 0.02, 0.4)):
        k = {-1: 0, 0: 1, 1: 4, 2: 10}[drift]
        pts, doms, st, _ = C.sized(200 + kid, 3, drift, C.M_KERNELS, k, kid=kid, nugget=nugget, base_range=br, total_sill=br)
        measure(f"kernel id {kid}, degree {drift}", pts, doms, st)
    pts, doms, st, _ = C.many_small()
    measure("512 domains", pts, doms, st, pick=list(range(0, 512, 16)) + [511])
    pts, doms, st, _ = C.fallback()
    measure("negative nugget: clustered (mode 1) and spread (mode 0) domains", pts, doms, st)
    for m, k in C.BIG_CASES:
        pts, doms, st = C.big(m, k)
        measure("one large domain", pts, doms, st, rows_of=R.big_rows)

    def worst(key, path):
        v = [c[key] for c in rec["cases"] if key in c and c["path"] == path]
        return max(v) if v else None

    rec["largest"] = {p: {key: worst(key, p) for key in ("assembly", "factor", "solve", "solve_special_rows", "kappa_blk",
                                                         "factor_bound_over_u_LLt", "kappa_1024")}
                      for p in ("per-domain", "large")}
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
    print("largest:", rec["largest"])
    print("wrote", args.out)


if __name__ == "__main__":
    main()
