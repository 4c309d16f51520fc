"""Child process of tests/test_gpu_pair_kernels.py::test_wx_separate_kernels_in_a_child_process: the matvec of a few
kernels on the clustered cloud of that module with whatever BBFMM_* switches the parent put in the environment (they are
read once per process).  Saves the products and the local coefficients to the .npz named on the command line.

`wx_worker.py OUT two-level D NAME ORDER` (tests/test_gpu_wx_passes.py): LinearRbf on a two-level layout of
tests/far_field_cases.py, the first column of that module's dense weights through matvec_device; saves the product, M, L
and the answer of debug_wx_jobs()."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def two_level(out_path, d, name, order):
    import torch
    import far_field_cases as C
    import test_gpu_wx_passes as T
    cloud = (d, name)
    pts, w = T.cloud_points(cloud), T.dense_weights(cloud)
    n = len(pts)
    t = C.make_tree(pts, order, T.cloud_limit(cloud), kernel=(0, T.BR, T.SILL))
    dw = torch.from_numpy(np.ascontiguousarray(w[:, :1].T)).cuda()
    out = torch.zeros((1, n), dtype=torch.float64, device="cuda")
    t.matvec_device(dw.data_ptr(), n, 1, out.data_ptr(), n, True)
    jobs = t.debug_wx_jobs()
    np.savez(out_path, y=out.cpu().numpy().T, M=t.debug_get_coefficients("M", 1), L=t.debug_get_coefficients("L", 1),
             jobs=np.array([jobs[k] for k in t.WX_JOB_FIELDS]))


def main():
    if sys.argv[2] == "two-level":
        return two_level(sys.argv[1], int(sys.argv[3]), sys.argv[4], int(sys.argv[5]))
    out_path, kids = sys.argv[1], [int(a) for a in sys.argv[2:]]
    import torch
    import ferreus_rbf_rs_amd as F
    import test_gpu_pair_kernels as T
    pts, w, _ = T.wx_cloud()
    n = pts.shape[0]
    res = {}
    for kid in kids:
        t = F.FmmTree(pts, T.WX_ORDER, F.KernelParams(F.KernelType(kid), base_range=T.BR, total_sill=T.SILL), True, True,
                      params=F.FmmParams(*T.WX_PARAMS))
        res[f"n_w_{kid}"] = t.stats().n_w
        res[f"y1_{kid}"] = t.fast_matrix_vector_product(w[:, 0].copy())
        dw = torch.from_numpy(np.ascontiguousarray(w[:, :3].T)).cuda()
        out = torch.zeros((3, n), dtype=torch.float64, device="cuda")
        t.matvec_device(dw.data_ptr(), n, 3, out.data_ptr(), n, True)
        res[f"y3_{kid}"] = out.cpu().numpy().T
        res[f"L3_{kid}"] = t.debug_get_coefficients("L", 3)
    np.savez(out_path, **res)


if __name__ == "__main__":
    main()
