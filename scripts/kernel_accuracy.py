"""Measured accuracy of the kernel functions of csrc/kernels.hpp against extended precision, through the test hooks
bbfmm_debug_math / bbfmm_debug_kernel_values: per arithmetic primitive the largest error in ulps of the correctly rounded
result, per kernel id, output path (value, value of the gradient path, gradient factor) and base_range the largest measure
relative to the derived bound of tests/kernel_pointwise.py and the largest error in u |g| (u = 2^-53) -- for the host branch
(where = 0) and, when a device is present, the device branch (where = 1).  The tables and the measure are those of the tests
(tests/kernel_reference.py); a bound that does not hold raises, as in the tests.

    python scripts/kernel_accuracy.py [--host-only] [--out profiles/kernel_function_accuracy.json]
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
    ap.add_argument("--host-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kernel_function_accuracy.json"))
    args = ap.parse_args()
    import __graft_entry__ as entry
    entry.build()
    import bench
    import ferreus_rbf_rs_amd as F
    import kernel_pointwise as KP
    import kernel_reference as KR
    from test_kernel_reference_host import CASES, SILL

    wheres = [0]
    if not args.host_only:
        import torch
        if torch.cuda.is_available():
            wheres.append(1)
    rec = {"source_hash": bench.source_hash(), "unit": "u = 2^-53; 1 ulp = 2u at the bottom of a binade",
           "tables": "tests/kernel_reference.py r2_table / table_for", "bounds": "tests/kernel_pointwise.py",
           "total_sill": SILL, "primitives": [], "kernels": []}
    if 1 in wheres:
        rec["device"] = torch.cuda.get_device_name(0)
    for where in wheres:
        side = "device" if where == 1 else "host"
        for which in F.fmm_tree.DEBUG_MATH:
            x = KP.primitive_inputs(which)
            res = KP.check_primitive(where, which, F.debug_math(where, which, x))
            bounds = KP.PRIMITIVE_ULPS if where == 1 else KP.HOST_PRIMITIVE_ULPS
            for name in [k for k in res if not k.endswith("_rel_u")]:
                prim = "rsqrt" if name == "out2" else which
                rec["primitives"].append({"where": side, "primitive": which, "output": "1/sqrt" if name == "out2" else which.split("_")[0],
                                          "inputs": int(x.size), "max_ulp": round(res[name], 4), "bound_ulp": bounds[prim],
                                          "max_relative_u": round(res[name + "_rel_u"], 4),
                                          "bound_relative_u": KP.REL_U.get(prim) if where == 1 else None})
        for kid, br in CASES:
            r2 = KR.table_for(kid, br)
            res = KP.check_kernel(where, kid, br, SILL, F.debug_kernel_values(where, kid, br, SILL, r2))
            bud = {k: list(v) for k, v in KP.budget(where, kid).items()}
            for path, (ratio, rel) in res.items():
                rec["kernels"].append({"where": side, "kernel_id": kid, "kernel": F.KernelType(kid).name, "base_range": br,
                                       "path": path, "inputs": int(r2.size), "max_measure_over_bound": round(ratio, 4),
                                       "max_error_u_rel": round(rel, 3) if rel < 1e6 else float(f"{rel:.3e}"),
                                       "budget_a_b": {k: v for k, v in bud.items() if k.startswith(path) and
                                                      (path != "value" or not k.startswith("value_g"))}})
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
