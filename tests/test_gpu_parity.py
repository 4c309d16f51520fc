"""Parity of the HIP path (through the C ABI) with the CPU oracle, on a real MI355X.

Tolerances (floating point, f64 throughout):
  * 1e-11 relative (max norm) against the oracle running the SAME host-computed M2L operators:
    only the summation order differs;
  * the BBFMM accuracy (~10^-order * O(10)) against the oracle with its own operators and against
    the dense direct sum.
Tree indexing is compared for exact equality in tests/test_host_structure.py (no GPU needed)."""
import numpy as np
import pytest

import ferreus_rbf_rs_amd as F
from conftest import clustered_points, inject_product_operators, relerr
from oracle import bbfmm_oracle as O

pytestmark = pytest.mark.gpu
TOL = 1e-11


def make(pts, kid=0, order=7, adaptive=True, sparse=True, extents=None, params=None, br=1.0, sill=1.0, inject=True):
    fp = None if params is None else F.FmmParams(*params)
    op = None if params is None else O.FmmParams(*params)
    t = F.FmmTree(pts, order, F.KernelParams(F.KernelType(kid), base_range=br, total_sill=sill), adaptive, sparse,
                  extents=extents, params=fp)
    r = O.FmmTree(pts, order, kid, adaptive, sparse, extents, op, base_range=br, total_sill=sill)
    if inject:
        inject_product_operators(t, r)
    return t, r


def check(pts, nrhs=1, targets=None, grads=False, dense_tol=1e-6, seed=0, **kw):
    rng = np.random.default_rng(seed)
    t, r = make(pts, **kw)
    w = rng.random((pts.shape[0], nrhs))
    t.set_weights(w)
    r.set_weights(w)
    assert relerr(t.debug_get_coefficients("M", nrhs), r.M) < TOL           # P2M + M2M
    tp = pts if targets is None else targets
    if grads:
        y, g = t.evaluate_with_gradients(w, tp)
        yr, gr = r.evaluate_with_gradients(w, tp)
        assert relerr(g, gr) < 1e-9
    else:
        y, yr = t.evaluate(w, tp), r.evaluate(w, tp)
    if targets is None:                                                      # all cells carry targets
        assert relerr(t.debug_get_coefficients("L", nrhs), r.L) < TOL       # M2L + P2L + L2L
    assert relerr(y, yr) < TOL                                               # + P2P + M2P + L2P
    kid = kw.get("kid", 0)
    idx = rng.choice(len(tp), min(len(tp), 300), replace=False)
    yd = O.dense_sum(kid, kw.get("br", 1.0), kw.get("sill", 1.0), tp[idx], pts, w)
    assert relerr(y[idx], yd) < dense_tol
    return t, r, w


def test_mfma_lane_layout_and_peak():
    tf, errs = F.mfma_f64_selftest()
    assert errs == 0                       # the v_mfma_f64_4x4x4 lane maps the M2L kernels assume
    assert tf > 20.0                       # sanity: a bare MFMA loop reaches tens of TFLOP/s


def test_fp64_valu_microbenchmark():
    tf, mhz = F.fp64_valu_selftest()       # the issue roofline the bench quotes the pair kernels against
    assert 20.0 < tf < 90.0 and 1000.0 < mhz < 3000.0


def test_get_distance_doctest_through_the_device_near_field():
    """ferreus_rbf_utils/src/utils.rs:263-280: the distance from (1, 2) to (4, 6) is 5.  Two points, linear kernel
    phi(r) = -r (rbf_kernels.rs:25-36), unit weights: both potentials are -5 -- exactly: the device square root
    (v_rsq_f64 + one cubic step, kernels.hpp) is within 2 ulp of the correctly rounded root in general
    (tests/test_gpu_kernel_pointwise.py) and exact at this argument; through evaluate (ordered pairs) and through the
    matvec entry point (unordered pairs)."""
    pts = np.array([[1.0, 2.0], [4.0, 6.0]])
    w = np.ones((2, 1))
    t = F.FmmTree(pts, 4, F.KernelParams(F.FmmKernelType.LinearRbf), True, True)
    t.set_weights(w)
    assert t.evaluate(w, pts)[:, 0].tolist() == [-5.0, -5.0]
    assert t.fast_matrix_vector_product(w[:, 0].copy()).tolist() == [-5.0, -5.0]


def test_config1_50k_linear():
    # BASELINE.json configs[0]: 50k random points, single rhs (reference-native kernel)
    check(np.random.default_rng(1).random((50000, 3)))


def test_mixed_levels_two_rhs():
    t, r, _ = check(np.random.default_rng(2).random((130000, 3)), nrhs=2)
    assert t.stats().n_w > 0 and t.stats().n_x == t.stats().n_w


def test_gradients_cubic_mixed_levels():
    check(np.random.default_rng(3).random((130000, 3)), kid=2, grads=True)


def test_clustered_tps_order9():
    check(clustered_points(np.random.default_rng(4), 60000, 3), kid=1, order=9, dense_tol=1e-8)


@pytest.mark.parametrize("kid,br,sill,tol", [(3, 0.5, 0.4, 5e-6), (4, 0.5, 0.4, 5e-6), (5, 0.5, 0.4, 5e-6),
                                             (6, 0.5, 0.4, 5e-6), (7, 1, 1, 1e-6), (8, 1, 1, 5e-6), (9, 1, 1, 5e-5),
                                             (100, 1.0, 1.0, 1e-5), (101, 0.3, 0.3, 1e-6)])
def test_every_kernel(kid, br, sill, tol):
    check(np.random.default_rng(5).random((20000, 3)), kid=kid, br=br, sill=sill, dense_tol=tol)


def test_narrow_gaussian_extension_device_equals_restatement_where_the_method_is_inaccurate():
    """Config 4's second instance: the Gaussian EXTENSION kernel exp(-(r / 0.1)^2).  Its width is below the
    cell size of the upper levels, where an order-7 Chebyshev interpolant does not resolve it: the BBFMM itself is only
    ~1e-2 accurate against the dense sum here (oracle alone: 2.4e-3 at 50k points, 1.3e-2 at 400k; bench.py's 10M x 8 rhs
    line shows 1.2e-2) -- a property of the method on this kernel, not of the device code: device and restatement still
    agree to 1e-11 on M, L and the potentials."""
    check(np.random.default_rng(8).random((60000, 3)), kid=100, br=0.1, sill=0.1, nrhs=2, dense_tol=3e-2)


def test_two_and_one_dimensions():
    check(np.random.default_rng(6).random((30000, 2)))
    check(np.random.default_rng(7).random((5000, 1)), dense_tol=1e-10)


def test_evaluator_flow_non_sparse_extents_arbitrary_targets():
    # ferreus_bbfmm/src/lib.rs:236-293
    rng = np.random.default_rng(8)
    pts = rng.random((20000, 3)) * 2 - 1
    tg = rng.random((3000, 3)) * 4 - 2
    t, r, w = check(pts, nrhs=2, targets=tg, sparse=False, extents=[-2, -2, -2, 2, 2, 2])
    t.set_local_coefficients(w)
    r.set_local_coefficients(w)
    assert relerr(t.debug_get_coefficients("L", 2), r.L) < TOL
    for m in (100, 1000):
        x = rng.random((m, 3)) * 4 - 2
        assert relerr(t.evaluate_leaves(w, x), r.evaluate_leaves(w, x)) < TOL
    y, g = t.evaluate_leaves_with_gradients(w, x)
    yr, gr = r.evaluate_leaves_with_gradients(w, x)
    assert relerr(y, yr) < TOL and relerr(g, gr) < 1e-9 and g.shape == (1000, 6)
    # weights left on the device (w = NULL, header: bbfmm_evaluate_leaves): same result without the upload
    y0, g0 = t.evaluate_leaves_with_gradients(None, x)
    assert relerr(t.evaluate_leaves(None, x), t.evaluate_leaves(w, x)) < 1e-14   # M2P adds atomically: not bitwise
    assert relerr(y0, y) < 1e-14 and relerr(g0, g) < 1e-14
    xl = rng.random((6000, 3)) * 4 - 2                                          # device grouping path
    assert relerr(t.evaluate_leaves(None, xl), r.evaluate_leaves(w, xl)) < TOL
    with pytest.raises((TypeError, ValueError)):
        t.evaluate(None, x)                                                     # only the leaves-only calls accept NULL
    assert t.evaluate(w, np.zeros((0, 3))).shape == (0, 2)                   # empty target set


def test_regular_tree_and_compression_modes():
    pts = np.random.default_rng(9).random((20000, 3))
    check(pts, adaptive=False)
    check(pts, adaptive=False, sparse=False)
    check(pts, kid=2, params=(256, 1, 1e-7, 1024))      # SVD
    check(pts[:8000], kid=2, params=(64, 0, 1e-7, 1024))  # uncompressed


def test_other_orders():
    pts = np.random.default_rng(10).random((20000, 3))
    check(pts, order=5, dense_tol=1e-4)
    check(pts, order=6, dense_tol=1e-4)
    check(pts, order=8, dense_tol=1e-6)
    check(pts, kid=2, order=11, params=(400, 2, 1e-9, 1024), dense_tol=1e-8)


def test_independent_operators_agree_to_bbfmm_accuracy():
    """Oracle with its OWN ACA/SVD operators (no injection): agreement to the compression tolerance."""
    pts = np.random.default_rng(11).random((30000, 3))
    t, r = make(pts, inject=False)
    w = np.random.default_rng(12).random((30000, 1))
    t.set_weights(w)
    r.set_weights(w)
    assert relerr(t.evaluate(w, pts), r.evaluate(w, pts)) < 1e-6


@pytest.mark.parametrize("kid,order", [(0, 5), (2, 6), (3, 4)])
def test_independent_uncompressed_operators_agree_to_rounding(kid, order):
    """M2lCompressionType::None leaves nothing to the factorisation: the M2L operators are the kernel at the node
    pairs of a transfer vector.  Oracle and product then build them independently (no injection), and everything --
    operator tables, transfer-vector numbering, permutations, the stacked GEMMs -- must agree to rounding, not to the
    compression tolerance of the ACA / SVD comparisons."""
    pts = np.random.default_rng(40 + kid).random((6000, 3))
    prm = (48, 0, 1e-7, 1024)
    t, r = make(pts, kid=kid, order=order, params=prm, inject=False, br=0.5, sill=0.25)
    w = np.random.default_rng(41).random((pts.shape[0], 2))
    t.set_weights(w)
    r.set_weights(w)
    y, yr = t.evaluate(w, pts), r.evaluate(w, pts)
    assert relerr(t.debug_get_coefficients("L", 2), r.L) < TOL
    assert relerr(y, yr) < TOL


def test_errors_match_the_reference():
    # ferreus_bbfmm/src/bbfmm.rs:1464-1500 through the whole ABI (set_weights included)
    t = F.FmmTree(np.array([[0.5]]), 3, F.KernelParams(F.FmmKernelType.LinearRbf), True, False, extents=[0.0, 1.0])
    t.set_weights(np.array([[1.0]]))
    with pytest.raises(F.PointOutsideTree) as e:
        t.evaluate(np.array([[1.0]]), np.array([[0.5], [10.0]]))
    assert e.value.point_index == 1 and isinstance(e.value, ValueError)
    assert "target point at row 1 lies outside the tree extents" in str(e.value)
    y = t.evaluate(np.array([[1.0]]), np.array([[0.5], [0.25]]))
    assert y[0, 0] == 0.0 and y[1, 0] == pytest.approx(-0.25, abs=1e-15)
    with pytest.raises(F.PointOutsideTree):
        t.evaluate_leaves(np.array([[1.0]]), np.array([[7.0]])) if t.set_local_coefficients(np.array([[1.0]])) is None else None
    t2 = F.FmmTree(np.random.rand(100, 3), 4, F.KernelParams(F.FmmKernelType.LinearRbf), True, True)
    with pytest.raises(ValueError):
        t2.evaluate(np.ones((100, 1)), np.random.rand(5, 3))                 # set_weights not called yet


def test_fast_matrix_vector_product_semantics():
    # ferreus_rbf/src/rbf.rs:1338-1379: subset rows, nugget, polynomial tail, zero elsewhere
    rng = np.random.default_rng(13)
    n = 20000
    pts = rng.random((n, 3))
    t, r = make(pts)
    wf = rng.random(n + 4)
    P = np.hstack([np.ones((n, 1)), pts])
    full = t.fast_matrix_vector_product(wf, 4, None, P, 0.01)
    assert relerr(full, O.fast_matrix_vector_product(r, wf, 4, None, P, 0.01)) < TOL
    assert np.all(full[n:] == 0.0)
    sub = rng.choice(n, 3000, replace=False)
    part = t.fast_matrix_vector_product(wf, 4, sub, P, 0.01)
    assert relerr(part, O.fast_matrix_vector_product(r, wf, 4, sub, P, 0.01)) < TOL
    mask = np.ones(n + 4, bool)
    mask[sub] = False
    assert np.all(part[mask] == 0.0) and relerr(part[sub], full[sub]) < TOL
    # every row, in order, given as an index set (the finest Schwarz level): served by the all-rows product
    allrows = t.fast_matrix_vector_product(wf, 4, np.arange(n), P, 0.01)
    assert relerr(allrows, full) < 1e-14 and np.all(allrows[n:] == 0.0)
    perm = rng.permutation(n)                     # every row, shuffled: an ordinary subset plan, same values
    assert relerr(t.fast_matrix_vector_product(wf, 4, perm, P, 0.01), full) < TOL


def test_device_resident_matvec_and_partition_union():
    """bbfmm_matvec_device on torch tensors; the owned rows of a 4-way partition reassemble it."""
    import torch
    rng = np.random.default_rng(14)
    n, k = 60000, 2
    pts = rng.random((n, 3))
    t, r = make(pts)
    w = rng.random((n, k))
    dw = torch.from_numpy(np.ascontiguousarray(w.T)).cuda()
    out = torch.zeros((k, n), dtype=torch.float64, device="cuda")
    t.matvec_device(dw.data_ptr(), n, k, out.data_ptr(), n, True)
    r.set_weights(w)
    yr = r.evaluate(w, pts)
    assert relerr(out.cpu().numpy().T, yr) < TOL
    acc = torch.full((k, n), float("nan"), dtype=torch.float64, device="cuda")
    total = 0
    for rank in range(4):
        t.set_partition(rank, 4)
        rows = torch.from_numpy(t.partition_rows()).cuda()
        tmp = torch.full((k, n), float("nan"), dtype=torch.float64, device="cuda")
        t.matvec_device(dw.data_ptr(), n, k, tmp.data_ptr(), n, True)
        acc[:, rows] = tmp[:, rows]
        total += rows.numel()
    t.set_partition(0, 1)
    assert total == n and relerr(acc.cpu().numpy().T, yr) < TOL


def test_full_size_10m_properties():
    """BASELINE.json's 10M-point size: linearity, symmetry of the kernel matrix, sampled dense rows."""
    import torch
    n = 10_000_000
    pts = np.random.default_rng(42).random((n, 3))
    t = F.FmmTree(pts, 7, F.KernelParams(F.FmmKernelType.LinearRbf), True, True)
    s = t.stats()
    assert s.depth == 6 and s.n_points == n
    g = torch.Generator(device="cuda").manual_seed(1)
    w = torch.rand((2, n), dtype=torch.float64, device="cuda", generator=g)
    y = torch.zeros_like(w)
    t.matvec_device(w.data_ptr(), n, 2, y.data_ptr(), n, True)
    a, b = 0.75, -1.5
    wc = (a * w[0] + b * w[1]).reshape(1, n).contiguous()
    yc = torch.zeros_like(wc)
    t.matvec_device(wc.data_ptr(), n, 1, yc.data_ptr(), n, True)
    lin = (yc[0] - (a * y[0] + b * y[1])).abs().max() / yc.abs().max()
    assert float(lin) < 1e-12                                   # linearity of the whole pipeline
    sym = abs(float(torch.dot(w[1], y[0]) - torch.dot(w[0], y[1]))) / abs(float(torch.dot(w[1], y[0])))
    assert sym < 1e-7                                           # K = K^T up to the far-field approximation
    idx = np.random.default_rng(2).choice(n, 64, replace=False)
    yd = O.dense_sum(0, 1.0, 1.0, pts[idx], pts, w[0].cpu().numpy()[:, None])
    assert relerr(y[0].cpu().numpy()[idx][:, None], yd) < 1e-6


@pytest.mark.parametrize("order", [2, 3, 4, 5, 6, 8, 9, 10, 11, 12])
def test_every_order_3d(order):
    """Every template instance of the order-specialised kernels (P2M, L2P, the 3-D M2M / L2L register
    kernels up to 10 / 12 and the general ones beyond) and every M2L chunk plan (n_pad = 32 ... 1728)."""
    n = 6000 if order <= 9 else 2500
    pts = np.random.default_rng(100 + order).random((n, 3))
    check(pts, nrhs=2 if order % 2 else 1, order=order, params=(60, O.COMPRESSION_ACA, 10.0 ** -min(order, 9), 1024),
          dense_tol=5.0 * 10.0 ** -min(order - 1, 6), seed=order)


@pytest.mark.parametrize("order,grads", [(13, True), (14, False), (16, False)])
def test_orders_above_12_3d(order, grads):
    """The reference takes any interpolation order (bbfmm.rs:77-104; CubicRbf defaults to 11, config.rs:200-207):
    3-D orders 13-16 run through the same templates with fewer waves per workgroup and the general M2M / L2L
    kernels (slower per node, same results)."""
    pts = np.random.default_rng(300 + order).random((2200, 3))
    check(pts, nrhs=2 if grads else 1, order=order, grads=grads, kid=2 if grads else 0,
          params=(120, O.COMPRESSION_ACA, 1e-9, 1024), dense_tol=1e-6, seed=order)


@pytest.mark.parametrize("d,order", [(1, 4), (1, 16), (2, 3), (2, 7), (2, 12), (2, 16)])
def test_orders_1d_2d(d, order):
    n = 3000
    pts = np.random.default_rng(200 + 10 * d + order).random((n, d))
    check(pts, nrhs=1, order=order, params=(40, O.COMPRESSION_ACA, 1e-8, 1024),
          dense_tol=5.0 * 10.0 ** -min(order - 1, 6), seed=order + d)


def test_partial_matvec_plans_and_restricted_evaluate():
    """matvec_partial (rbf.rs:119-133) with cached target-subset plans, and evaluate() on few targets:
    both run the downward pass over cells_with_targets only and must match the whole-tree results."""
    n = 40000
    pts = clustered_points(np.random.default_rng(31), n, 3)
    t, r = make(pts, kid=0, order=6, params=(80, O.COMPRESSION_ACA, 1e-6, 1024))
    rng = np.random.default_rng(32)
    w = rng.random(n)
    full = t.fast_matrix_vector_product(w, nugget=0.25)
    subsets = [np.sort(rng.choice(n, m, replace=False)).astype(np.int64) for m in (7, 300, 5000, 20000)]
    subsets += [rng.choice(n, 50, replace=True).astype(np.int64) for _ in range(7)]   # > 8 plans: eviction
    t.prepare_target_subset(subsets[2])                                               # plan built ahead of the first product
    with pytest.raises(ValueError):
        t.prepare_target_subset(np.array([0, n], dtype=np.int64))                     # index out of range
    for rep in range(2):                                                              # second round: cached or rebuilt
        for idx in subsets:
            y = t.fast_matrix_vector_product(w, target_indices=idx, nugget=0.25)
            assert relerr(y[idx], full[idx]) < TOL
            mask = np.ones(n, bool)
            mask[idx] = False
            assert not y[mask].any()                                                  # other rows stay 0 (rbf.rs:1346)
    # evaluate() on few targets in Full mode (no set_local_coefficients): restricted pass vs oracle
    w2 = rng.random((n, 2))
    t.set_weights(w2)
    r.set_weights(w2)
    x = pts[rng.choice(n, 200, replace=False)] + 1e-3 * rng.standard_normal((200, 3))
    x = np.clip(x, pts.min(0), pts.max(0))
    assert relerr(t.evaluate(w2, x), r.evaluate(w2, x)) < TOL
    # Leaves mode: set_local_coefficients, then evaluate() must leave the stored expansions intact
    t.set_local_coefficients(w2)
    r.set_local_coefficients(w2)
    a = t.evaluate_leaves(w2, x)
    t.evaluate(w2, x[:10])
    assert relerr(t.evaluate_leaves(w2, x), a) < 1e-14       # (M2P adds with atomics: order may differ)
    assert relerr(a, r.evaluate_leaves(w2, x)) < TOL


@pytest.mark.gpu
@pytest.mark.parametrize("d", [1, 2, 3])
def test_device_target_grouping_equals_host_grouping(d):
    # targets.hip (points_to_leaves + stable grouping on the device, batches >= 4096 rows) against the
    # host path (smaller batches): same leaves (linear_tree.rs:487-534), same values and gradients,
    # and the smallest row outside the tree is the one reported (linear_tree.rs:514-517)
    rng = np.random.default_rng(100 + d)
    n = 30000
    pts = clustered_points(rng, n, d)
    t = F.FmmTree(pts, 5, F.KernelParams(F.FmmKernelType.CubicRbf), True, False,
                  extents=[-1.0] * d + [2.0] * d)
    w = rng.standard_normal((n, 1))
    t.set_weights(w)
    m = 9000
    x = rng.random((m, d)) * 2.5 - 0.75
    big, gbig = t.evaluate_with_gradients(w, x)
    parts = [t.evaluate_with_gradients(w, x[i:i + 3000]) for i in range(0, m, 3000)]
    small = np.vstack([p[0] for p in parts]); gsmall = np.vstack([p[1] for p in parts])
    assert np.abs(big - small).max() <= 1e-13 * np.abs(small).max()
    assert np.abs(gbig - gsmall).max() <= 1e-13 * np.abs(gsmall).max()
    assert np.array_equal(t.evaluate(w, x), big) or np.abs(t.evaluate(w, x) - big).max() <= 1e-13 * np.abs(big).max()
    # rows far outside: whatever the host path decides (the 16-bit anchor masks of morton.rs:58-119 can
    # alias such a row into the tree) the device path must decide too, and report the same first row
    xb = x.copy(); xb[7000] = 50.0; xb[8123] = -50.0

    def first_bad(arr):
        try:
            t.evaluate(w, arr)
            return None
        except F.PointOutsideTree as e:
            return e.point_index
    host = [first_bad(xb[i:i + 3000]) for i in range(0, m, 3000)]
    expect = next((i * 3000 + b for i, b in enumerate(host) if b is not None), None)
    assert first_bad(xb) == expect
    if d > 1:
        assert expect == 7000
    # sparse tree, targets = a permutation of the sources: every row has a leaf, grouping must undo the shuffle
    ts = F.FmmTree(pts, 5, F.KernelParams(F.FmmKernelType.CubicRbf), True, True)
    ts.set_weights(w)
    perm = rng.permutation(n)
    assert relerr(ts.evaluate(w, pts[perm]), ts.evaluate(w, pts)[perm]) < 1e-13


def test_twelve_clusters_sparse_levels_order7():
    """The soak run's cloud (twelve Gaussian clusters of very different widths, clipped to the unit cube): sparse
    coarse levels, classes with a handful of cells, W / X lists at every level -- values, M and L against the
    oracle and the dense sum.  (Caught a wrong contraction in M2L stage 1 that uniform clouds did not.)"""
    rng = np.random.default_rng(123)
    k, n = 12, 100000
    c, s, which = rng.random((k, 3)), 0.01 + 0.08 * rng.random(k), rng.integers(0, k, n)
    pts = np.clip(c[which] + rng.normal(size=(n, 3)) * s[which, None], 0.0, 0.999)
    t, r, _ = check(pts, nrhs=1, dense_tol=1e-6)
    assert t.stats().depth >= 7 and t.stats().n_w > 0
    check(pts, nrhs=3, adaptive=False, dense_tol=1e-6)


@pytest.mark.parametrize("jobs", ["wave_per_small_leaf", "size_rule"])
@pytest.mark.parametrize("name", ["coincident", "planar_in_3d", "two_points", "far_from_origin", "negative_box", "collinear"])
def test_degenerate_clouds(name, jobs, monkeypatch):
    """Clouds the tree build has to survive: many coincident points (subdivision down to level 16, one leaf over
    the limit), a plane or a line embedded in 3-D (most cells empty), two points, coordinates far from the origin
    (root box from floor / ceil of the extents), a box in the negative octant."""
    # (small leaves as one wave each -- what the suite runs, conftest.py -- and as the library's size rule gives them out in
    # trees this small: workgroup jobs, leaves of one or two rows included)
    if jobs == "size_rule":
        monkeypatch.delenv("BBFMM_P2P_SYM_WAVE_MIN", raising=False)
    seeds = {"coincident": 11, "planar_in_3d": 12, "two_points": 13, "far_from_origin": 14, "negative_box": 15, "collinear": 16}
    rng = np.random.default_rng(seeds[name])             # fixed per name (hash() is randomised per process)
    if name == "coincident":
        pts = np.vstack([rng.random((3000, 3)), np.tile(rng.random((1, 3)), (600, 1))])
    elif name == "planar_in_3d":
        pts = np.column_stack([rng.random((8000, 2)), np.full(8000, 0.37)])
    elif name == "two_points":
        pts = np.array([[0.1, 0.2, 0.3], [0.8, 0.7, 0.9]])
    elif name == "far_from_origin":
        pts = rng.random((6000, 3)) * 0.8 + np.array([1.0e5, -3.0e4, 7.0e3])
    elif name == "negative_box":
        pts = -rng.random((6000, 3)) * 5.0
    else:
        pts = np.outer(rng.random(5000), np.array([0.6, 0.3, 0.2])) + 0.1
    t, r, w = check(pts, nrhs=1, order=5, params=(50, O.COMPRESSION_ACA, 1e-5, 1024), dense_tol=1e-3)
    assert t.tree_built_on_device()
    # the matvec entry point (unordered near field, fused adaptive lists) on the same cloud
    y = t.fast_matrix_vector_product(w[:, 0].copy())
    assert relerr(y, r.evaluate(w, pts)[:, 0]) < TOL


@pytest.mark.timeout(900)
def test_random_call_sequences_equal_the_oracle_call_by_call():
    """tests/checks/handle_sequence_fuzz.py in small: random sequences of the evaluator's calls on a handle and on the oracle's
    restatement of the reference's FmmTree -- the state one call leaves to the next (the multipoles of set_weights under another
    call's weights, stored local expansions, right-hand-side counts, row subsets) gives the same values at 1e-11, or the same
    refusal with the same offending row, after every call."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if not k.startswith("BBFMM_")}
    p = subprocess.run([sys.executable, os.path.join(root, "tests", "checks", "handle_sequence_fuzz.py"), "8", "17", "12"], env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=800)
    lines = p.stdout.decode().strip().splitlines()
    assert p.returncode == 0, "\n".join(l for l in lines if '"ok": false' in l)[:3000] + p.stderr.decode()[-1500:]
    assert '"failures": 0' in lines[-1]
