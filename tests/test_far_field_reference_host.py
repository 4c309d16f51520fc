"""The long-double restatement of the far-field passes (tests/far_field_reference.py) proven without a GPU: against the
oracle's double passes cell by cell, against the host walk of the product's own M2L tables under every switch setting,
its 1-D transfers against the product's dense M2M matrices, and the per-cell checker against altered data that the global
norm lets through."""
import numpy as np
import pytest

import far_field_cases as C
import far_field_reference as R
from conftest import inject_product_operators, relerr
from far_field_reference import LD, U
from oracle import bbfmm_oracle as O

CLOUDS = {"lattice8": (C.lattice8_cloud, C.LATTICE_LIMIT), "clustered": (C.clustered_cloud, C.CLUSTERED_LIMIT)}
cached = C.cached


def setup(cloud, order):
    """(points, host-only handle, its geometry, the oracle's tree on the product's operators), built once."""
    def make():
        fn, limit = CLOUDS[cloud]
        pts = cached(("pts", cloud), fn)
        t = C.make_tree(pts, order, limit, host_only=True)
        geo = R.Geometry(t)
        r = O.FmmTree(pts, order, 0, True, True, None, O.FmmParams(limit, C.ACA, 1e-7, 1024))
        inject_product_operators(t, r)
        assert geo.keys == [int(k) for k in r.cell_keys]
        return pts, t, geo, r
    return cached(("setup", cloud, order), make)


def oracle_passes(cloud, order, w):
    pts, t, geo, r = setup(cloud, order)
    r.set_weights(w)
    r.set_local_coefficients(w)
    return r.M.copy(), r.L.copy()


def upward_reference(geo, pts, w, M, terms):
    """ref / bound dicts of every cell below the root: leaves from the points, parents from the children's M."""
    ref, bound = {}, {}
    for c, (m, s_abs, s_fac, n_pts) in R.p2m(geo, pts, w).items():
        ref[c], bound[c] = m, R.p2m_bound(geo, s_abs, s_fac, n_pts)
    xf = R.Transfers(geo)
    for c in range(geo.C):
        if geo.level[c] >= 1 and not geo.is_leaf[c]:
            ref[c], bound[c] = R.m2m(geo, xf, M, c, terms)
    return ref, bound


# ------------------------------------------------------------------ against the oracle
@pytest.mark.parametrize("order", [4, 5])
@pytest.mark.parametrize("cloud", ["lattice8", "clustered"])
def test_restatement_against_the_oracle_cell_by_cell(cloud, order):
    """The oracle multiplies by the dense n x n transfer matrices: n + 3 terms where the device has 3p + 3; its M2L
    (n terms, then the rank columns, pair after pair) and its P2L (the host's kernel functions) are inside the bounds of
    the module docstring as they stand."""
    pts, t, geo, r = setup(cloud, order)
    if cloud == "lattice8":
        C.assert_lattice8(t, geo)
    else:
        assert t.stats().n_w > 0
    w = C.dense_weights(len(pts), 1, 5)
    M, L = oracle_passes(cloud, order, w)
    ref, bound = upward_reference(geo, pts, w, M, geo.n + 3)
    R.check_cells("M", M, ref, bound, sorted(ref), f"{cloud} order {order}")
    cells = np.nonzero(geo.level >= 1)[0]
    ref, bound = R.downward(geo, R.M2L(geo, t), R.Transfers(geo), M, L, cells, ((0, 1.0, 1.0), pts, w, 0), geo.n + 3)
    R.check_cells("L", L, ref, bound, cells, f"{cloud} order {order}")


# ------------------------------------------------------------------ the product's M2L tables, walked on the host
CONFIGS = [{}] + [dict(s1, BBFMM_M2L_S2_PAIRS=s2) for s1 in ({"BBFMM_M2L_S1_PAIRS": "0"}, {"BBFMM_M2L_S1_AXES": "1"},
                                                              {"BBFMM_M2L_S1_AXES": "2"}) for s2 in ("0", "1")]


def lattice8_weights(kind):
    pts = cached(("pts", "lattice8"), C.lattice8_cloud)
    return C.dense_weights(len(pts), 1, 7) if kind == "dense" else C.sparse_lattice_weights(pts, 8, 9, C.FEW_COLUMNS)


def m2l_reference(order, kind):
    def make():
        pts, t, geo, r = setup("lattice8", order)
        M, _ = oracle_passes("lattice8", order, lattice8_weights(kind))
        m2l = R.M2L(geo, t)
        Lr, S, Rc = m2l.apply(M)
        return M, Lr, m2l.bound(S, Rc), t.m2l_factors(3, 0)
    return cached(("host m2l", order, kind), make)


@pytest.mark.parametrize("env", CONFIGS, ids=lambda e: ",".join(f"{k[10:]}={v}" for k, v in e.items()) or "default")
@pytest.mark.parametrize("order,kind", [(3, "dense"), (3, "sparse"), (4, "dense"), (4, "sparse"), (5, "dense"), (5, "sparse"),
                                        (7, "sparse")])
def test_host_walk_of_the_m2l_tables_stays_inside_the_m2l_bound(order, kind, env):
    pts, _, geo, _ = setup("lattice8", order)
    M, Lr, bound, f0 = m2l_reference(order, kind)
    t = C.make_tree(pts, order, C.LATTICE_LIMIT, env=env, host_only=True)
    if "BBFMM_M2L_S1_PAIRS" in env:
        assert not t.debug_m2l_pairs()[0]
    if "BBFMM_M2L_S1_AXES" in env:
        assert t.debug_m2l_pairs_axes()[0]["axes"] == int(env["BBFMM_M2L_S1_AXES"])
    if "BBFMM_M2L_S2_PAIRS" in env:
        assert t.debug_m2l_pairs(stage=2)[0] == (env["BBFMM_M2L_S2_PAIRS"] == "1")
    for a, b in zip(f0, t.m2l_factors(3, 0)):                       # the switches change the tables, not the operators
        assert np.array_equal(a, b)
    Lh = np.stack([t.debug_apply_m2l_tables_host(M[k]) for k in range(M.shape[0])])
    if kind == "sparse":                                            # cells no source reaches hold exact zeros
        untouched = bound == 0
        assert untouched.any() and (Lh[untouched] == 0).all()
    R.check_cells("M2L tables", Lh, Lr.transpose(1, 0, 2), bound.T, range(geo.C), f"order {order} {kind} {env}")


# ------------------------------------------------------------------ the 1-D transfers, multiplied out
@pytest.mark.parametrize("d,orders", [(3, range(2, 9)), (2, range(2, 13)), (1, range(2, 13))])
def test_transfers_against_the_dense_m2m_matrices(d, orders):
    """Entry X0 X1 X2 of the product's double table against long double: u (e_S sum_a prod_{b != a} |X_b| + 2 |X0 X1 X2|)."""
    pts = C.random_cloud(d, 60, 11)
    worst = 0.0
    for p in orders:
        t = C.make_tree(pts, p, 256, host_only=True)
        A = [np.abs(x) for x in R.transfer_1d(p)]
        for ci in range(1 << d):
            ref = R.dense_transfer(p, d, ci)
            fac = 0
            for a in range(d):
                acc = None
                for b in range(d):
                    m = np.ones_like(A[0]) if b == a else A[(ci >> b) & 1]
                    acc = m if acc is None else np.kron(acc, m)
                fac = fac + acc.T
            bound = LD(U) * (R.e_S(p) * fac + 2 * np.abs(ref))
            err = np.abs(t.debug_dense_m2m(ci).astype(LD) - ref)
            worst = max(worst, float((err / bound).max()))
            assert (err <= bound).all(), (d, p, ci, float((err / bound).max()))
    print(f"transfers d = {d}: largest error / bound {worst:.3g}")


# ------------------------------------------------------------------ the checker catches what the global norm misses
def altered_setup():
    def make():
        pts, t, geo, r = setup("lattice8", 4)
        w = C.dense_weights(len(pts), 1, 13)
        leaf = int(np.nonzero(geo.is_leaf & (np.diff(geo.src_ptr) == 3))[0][0])
        w[geo.src_idx[geo.src_ptr[leaf]:geo.src_ptr[leaf + 1]]] *= 1e-3         # a small cell: its coefficients are small
        M, L = oracle_passes("lattice8", 4, w)
        refM, boundM = upward_reference(geo, pts, w, M, geo.n + 3)
        cells = np.nonzero(geo.level == 3)[0]
        m2l, xf = R.M2L(geo, t), R.Transfers(geo)
        refL, boundL = R.downward(geo, m2l, xf, M, L, cells, ((0, 1.0, 1.0), pts, w, 0), geo.n + 3)
        R.check_cells("M", M, refM, boundM, sorted(refM), "unaltered")
        R.check_cells("L", L, refL, boundL, cells, "unaltered")
        return pts, t, geo, w, leaf, M, L, refM, boundM, cells, refL, boundL, m2l, xf
    return cached(("altered",), make)


def test_checker_catches_one_entry_of_a_small_cell_that_the_global_norm_passes():
    pts, t, geo, w, leaf, M, L, refM, boundM, cells, refL, boundL, m2l, xf = altered_setup()
    s_c = float(R.p2m(geo, pts, w, cells=[leaf])[leaf][1].max())
    bad = M.copy()
    bad[0, leaf, 1] += 1e-9 * s_c
    assert bad[0, leaf, 1] != M[0, leaf, 1]
    assert relerr(bad, M) < 1e-11                                    # the gap being closed
    with pytest.raises(AssertionError):
        R.check_cells("M", bad, refM, boundM, sorted(refM), "one entry off by 1e-9 s_c")


def test_checker_catches_two_cells_with_their_rows_swapped():
    pts, t, geo, w, leaf, M, L, refM, boundM, cells, refL, boundL, m2l, xf = altered_setup()
    bad = L.copy()
    a, b = int(cells[10]), int(cells[11])
    bad[0, [a, b]] = bad[0, [b, a]]
    with pytest.raises(AssertionError):
        R.check_cells("L", bad, refL, boundL, cells, "rows swapped")


def test_checker_catches_a_transfer_vector_dropped_from_a_boundary_cell():
    pts, t, geo, w, leaf, M, L, refM, boundM, cells, refL, boundL, m2l, xf = altered_setup()
    n_v = np.diff(geo.lists["V"][0])
    c = int(next(c for c in cells if 0 < n_v[c] < 60))                 # a corner cell: few of the 189 vectors
    src = int(geo.v_src[geo.v_tgt == c][0])
    part, _ = R.downward(geo, m2l, xf, M, L, [c], ((0, 1.0, 1.0), pts, w, 0), geo.n + 3, skip=[(c, src)])
    bad = L.copy()
    bad[0, c] -= (refL[c] - part[c])[0].astype(np.float64)
    with pytest.raises(AssertionError):
        R.check_cells("L", bad, refL, boundL, cells, "one vector dropped")


# ------------------------------------------------------------------ L2P and its gradients
@pytest.mark.parametrize("d,order", [(3, 5), (2, 7), (1, 4)])
def test_l2p_restatement_against_the_oracle_target_by_target(d, order):
    """The oracle's leaf pass with only its L2P term (flags = 4) from its own L: values and gradients per target.  The
    oracle sums the n tensor entries one by one: n + 4 terms where the device's sum-factorised loop has 3p + 4 (the bounds
    of the module docstring then hold with n - 3p added to the count, which the check below does)."""
    pts = C.populations_cloud()[0] if d == 3 else C.random_cloud(d, 600, 23)
    limit = C.POPULATIONS_LIMIT if d == 3 else 40
    t = C.make_tree(pts, order, limit, host_only=True)
    geo = R.Geometry(t)
    r = O.FmmTree(pts, order, 0, True, True, None, O.FmmParams(limit, C.ACA, 1e-7, 1024))
    inject_product_operators(t, r)
    w = C.dense_weights(len(pts), 2, 25)
    r.set_weights(w)
    y, g = r._eval(w, pts, True, flags=4)
    g = g.reshape(len(pts), 2, d)
    leaf_of = t.points_to_leaves(pts)
    extra = geo.n - 3 * geo.p
    worst = worst_g = 0.0
    for c in np.unique(leaf_of):
        rows = np.nonzero(leaf_of == c)[0]
        yr, yb, gr, gb = R.l2p(geo, r.L, c, pts[rows], with_grads=True)
        s_abs = R._interpolate([np.abs(s) for s in geo.factors(c, pts[rows])], np.abs(r.L[:, c]).astype(LD), geo.P)
        yb = yb + LD(U) * extra * s_abs
        S, D = geo.factors(c, pts[rows], deriv=True)
        for a in range(d):
            F = [np.abs(s) for s in S]
            F[a] = np.abs(D[a])
            gb[:, :, a] += LD(U) * extra * R._interpolate(F, np.abs(r.L[:, c]).astype(LD), geo.P)
        e, eg = np.abs(y[rows].astype(LD) - yr), np.abs(g[rows].astype(LD) - gr)
        assert (e <= yb).all() and (eg <= gb).all(), (c, float((e / yb).max()), float((eg / gb).max()))
        worst, worst_g = max(worst, float((e / yb).max())), max(worst_g, float((eg / gb).max()))
    print(f"L2P d = {d} order {order}: largest error / bound {worst:.3g}, gradients {worst_g:.3g}")
    assert worst > 0 and worst_g > 0
