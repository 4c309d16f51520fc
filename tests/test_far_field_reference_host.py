"""The long-double restatement of the far-field passes (tests/far_field_reference.py) proven without a GPU: against the
oracle's double passes cell by cell, against the host walk of the product's own M2L tables under every switch setting,
its 1-D transfers against the product's dense M2M matrices, and the per-cell checker against altered data that the global
norm lets through.  In three, two and one dimension, and with uncompressed operators.  M2P: against the oracle's
multipole-to-particle on the same multipoles, the altered-data proof of its bound, the two-level layouts and the job hook.

THE STAGE-2 KERNEL INSTANCE OF EVERY ORDER (debug_m2l_s2_plan() of host-only handles; far_field_cases.S2_PLANS is this
table as data and test_stage2_plan_of_every_order_is_the_table_of_the_docstring holds the two to the handles).  One axis:
(GA, GB) of m2l_s2_pairs_kernel x (chunks of the x-even half, of the x-odd half); two axes: (GA, YA, GB, YB) of
m2l_s2_pairs2_kernel x the same.  The plan depends on the dimension, the order and the axes alone; unset, BBFMM_M2L_S2_AXES
is picked per tree by executed work.  With BBFMM_M2L_S2_PAIRS=0, without compression and in one dimension there is no
plan (all zeros: stage 2 runs in the node basis).

   d  order   one axis             two axes
   3    2     (1, 1)   x (1, 1)    (2, 1, 2, 1)   x (1, 1)
   3   3, 4   (2, 2)   x (1, 1)    (2, 1, 2, 1)   x (1, 1)
   3    5     (5, 4)   x (1, 1)    (5, 3, 4, 2)   x (1, 1)
   3    6     (7, 7)   x (1, 1)    (8, 4, 8, 4)   x (1, 1)
   3    7     (13, 10) x (1, 1)    (13, 7, 10, 6) x (1, 1)
   3    8     (8, 8)   x (2, 2)    (8, 4, 8, 4)   x (2, 2)
   3    9     (13, 11) x (2, 2)    (14, 8, 11, 6) x (2, 2)
   3   10     (8, 8)   x (4, 4)    (8, 4, 8, 4)   x (4, 4)
   2   2 - 5  (1, 1)   x (1, 1)    (2, 1, 2, 1)   x (1, 1)
   2   6 - 8  (2, 2)   x (1, 1)    (2, 1, 2, 1)   x (1, 1)
   2   9, 10  (4, 4)   x (1, 1)    (4, 2, 4, 2)   x (1, 1)
   2   11     (5, 4)   x (1, 1)    (5, 3, 4, 2)   x (1, 1)
   2  12 - 14 (7, 7)   x (1, 1)    (8, 4, 8, 4)   x (1, 1)
   2  15, 16  (8, 8)   x (1, 1)    (8, 4, 8, 4)   x (1, 1)

Every entry of M2L_S2_PAIR_WIDTHS and of M2L_S2_PAIR2_WIDTHS (device_m2l.hip) is selected by some order of this range:
none is unreachable here.  3-D orders 6, 8, 9 and 10 select (7, 7), (8, 8), (13, 11), (8, 4, 8, 4) and (14, 8, 11, 6), which
orders 3, 4, 5 and 7 never reach, and the only plans with more than one chunk per half: far_field_cases.GPU_INSTANCES, what
tests/test_gpu_far_field_orders.py covers on the device."""
import os
import re

import numpy as np
import pytest

import far_field_cases as C
import far_field_reference as R
from conftest import ROOT, inject_product_operators, relerr
from far_field_reference import LD, U
from oracle import bbfmm_oracle as O

CLOUDS = {"lattice8": (C.lattice8_cloud, C.LATTICE_LIMIT), "clustered": (C.clustered_cloud, C.CLUSTERED_LIMIT),
          "lattice2d": (C.lattice2d_cloud, C.LATTICE_LIMIT), "line": (C.line_cloud, C.LINE_LIMIT)}
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
@pytest.mark.parametrize("cloud,order", [("lattice8", 4), ("clustered", 4), ("lattice8", 5), ("clustered", 5), ("lattice2d", 4),
                                         ("lattice2d", 7), ("line", 4), ("line", 16)])
def test_restatement_against_the_oracle_cell_by_cell(cloud, order):
    """The oracle multiplies by the dense n x n transfer matrices: n + 3 terms where the device has 3p + 3; its M2L
    (n terms, then the rank columns, pair after pair) and its P2L (the host's kernel functions) are inside the bounds of
    the module docstring as they stand."""
    pts, t, geo, r = setup(cloud, order)
    if cloud == "clustered":
        assert t.stats().n_w > 0
    else:
        {"lattice8": C.assert_lattice8, "lattice2d": C.assert_lattice2d, "line": C.assert_line}[cloud](t, geo)
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


WALK_CLOUD = {"dense": "lattice8", "sparse": "lattice8", "every-vector": "lattice8", "two-cells": "lattice8",
              "dense-2d": "lattice2d"}


def walk_weights(kind):
    """dense, sparse: lattice8 as before; every-vector: lattice8 with the columns that between them reach all 316 vectors;
    dense-2d: lattice2d."""
    pts = cached(("pts", WALK_CLOUD[kind]), CLOUDS[WALK_CLOUD[kind]][0])
    if kind in ("dense", "dense-2d"):
        return C.dense_weights(len(pts), 1, 7)
    return C.sparse_lattice_weights(pts, 8, 9, {"sparse": C.FEW_COLUMNS, "every-vector": C.EVERY_VECTOR_COLUMNS,
                                                "two-cells": [13, 18]}[kind])


def m2l_reference(order, kind):
    def make():
        pts, t, geo, r = setup(WALK_CLOUD[kind], order)
        w = walk_weights(kind)
        if kind in ("every-vector", "dense-2d"):
            C.assert_every_vector_is_live(geo, w)
        M, _ = oracle_passes(WALK_CLOUD[kind], order, w)
        m2l = R.M2L(geo, t)
        Lr, S, Rc = m2l.apply(M)
        return M, Lr, m2l.bound(S, Rc), t.m2l_factors(3, 0)
    return cached(("host m2l", order, kind), make)


@pytest.mark.parametrize("env", CONFIGS, ids=lambda e: ",".join(f"{k[10:]}={v}" for k, v in e.items()) or "default")
@pytest.mark.parametrize("order,kind", [(3, "dense"), (3, "sparse"), (4, "dense"), (4, "sparse"), (5, "dense"), (5, "sparse"),
                                        (7, "sparse"), (6, "every-vector"), (8, "every-vector"), (9, "every-vector")] +
                         [(p, "dense-2d") for p in (3, 6, 7, 10, 16)])
def test_host_walk_of_the_m2l_tables_stays_inside_the_m2l_bound(order, kind, env):
    """every-vector (orders 6, 8, 9, where a walk takes up to ten seconds per right-hand side): all seven columns under the
    default configuration, the two interior cells of classes 1 and 6 under the six others.  Measured on eight cores with
    other work beside it, the seven cases of an order together: order 6 about 45 s (default 22 s), order 8 141 s (default
    38 s, the others 12 s with stage-2 pairs and 20 to 24 s without), order 9 249 s (default 79 s, the others 15 to 23 s and
    34 to 43 s) -- the walk, not the restatement, is the cost: it visits every stacked table of every cell whatever the
    weights.  With all of FEW_COLUMNS under every configuration orders 8 and 9 would take about 2.5 times as long."""
    pts, _, geo, _ = setup(WALK_CLOUD[kind], order)
    M, Lr, bound, f0 = m2l_reference(order, "two-cells" if kind == "every-vector" and env else kind)
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
    if kind in ("sparse", "every-vector"):                          # cells no source reaches hold exact zeros
        untouched = bound == 0
        assert untouched.any() and (Lh[untouched] == 0).all()
    R.check_cells("M2L tables", Lh, Lr.transpose(1, 0, 2), bound.T, range(geo.C), f"order {order} {kind} {env}")


def test_host_walk_of_the_uncompressed_m2l_tables_stays_inside_the_m2l_bound():
    """M2LCompressionType none: no Vt, the rank is n, nothing pairs (the multipoles do not depend on the compression: they
    are those of the compressed setup)."""
    pts, _, geo, _ = setup("lattice8", 4)
    w = walk_weights("every-vector")
    C.assert_every_vector_is_live(geo, w)
    M, _ = oracle_passes("lattice8", 4, w)
    t = C.make_tree(pts, 4, C.LATTICE_LIMIT, host_only=True, compression=C.NO_COMPRESSION)
    assert not t.debug_m2l_pairs()[0] and not t.debug_m2l_pairs(stage=2)[0] and t.debug_m2l_s2_plan() == (0,) * 6
    u, vt = t.m2l_factors(3, 0)
    assert vt is None and u.shape == (geo.n, geo.n) and (t.m2l_ranks()[2:] == geo.n).all()
    m2l = R.M2L(geo, t)
    Lr, S, Rc = m2l.apply(M)
    bound = m2l.bound(S, Rc)
    Lh = np.stack([t.debug_apply_m2l_tables_host(M[k]) for k in range(M.shape[0])])
    untouched = bound == 0
    assert untouched.any() and (Lh[untouched] == 0).all()
    R.check_cells("M2L tables", Lh, Lr.transpose(1, 0, 2), bound.T, range(geo.C), "order 4 uncompressed")


# ------------------------------------------------------------------ the stage-2 kernel instance of every order
def s2_plan_table():
    """{(d, order, axes): (ga, gb, ce, co, ya, yb)} from host-only handles; the plan depends on d, the order and the axes."""
    def make():
        table = {}
        for d, orders in ((2, range(2, 17)), (3, range(2, 11))):
            pts = C.random_cloud(d, 400, 27)
            for order in orders:
                for axes in (1, 2):
                    t = C.make_tree(pts, order, 30, env={"BBFMM_M2L_S2_AXES": str(axes)}, host_only=True)
                    assert t.debug_m2l_pairs_axes(stage=2)[0]["axes"] == axes
                    table[d, order, axes] = t.debug_m2l_s2_plan()
        return table
    return cached(("s2 plans",), make)


def kernel_widths(macro):
    """The entries X(...) of a width list of csrc/device_m2l.hip, from which the planner's table and the launcher's dispatch
    are generated: a set of tuples."""
    path = os.path.join(ROOT, "ferreus_rbf_rs_amd", "csrc", "device_m2l.hip")
    line = re.search(r"^#define %s\(X\)(.*)$" % macro, open(path).read(), re.M).group(1)
    assert "\\" not in line                                         # the list is one line
    return {tuple(int(v) for v in e.split(",")) for e in re.findall(r"X\(([\d, ]+)\)", line)}


def test_stage2_plan_of_every_order_is_the_table_of_the_docstring():
    table = s2_plan_table()
    assert table == C.S2_PLANS
    for (d, order, axes), (ga, gb, ce, co, ya, yb) in table.items():
        n_e, n_o = (order + 1) // 2 * order ** (d - 1), order // 2 * order ** (d - 1)
        assert (ya > 0 and yb > 0) == (axes == 2)
        if axes == 1:                                               # each half fits its chunks
            assert n_e <= 16 * ga * ce and n_o <= 16 * gb * co
    # every instance the kernels are built for is selected somewhere in the range: none is unreachable
    one, two = kernel_widths("M2L_S2_PAIR_WIDTHS"), kernel_widths("M2L_S2_PAIR2_WIDTHS")
    assert len(one) == 8 and len(two) == 6 and (13, 11) in one and (14, 8, 11, 6) in two
    assert {(p[0], p[1]) for k, p in table.items() if k[2] == 1} == one
    assert {(p[0], p[4], p[1], p[5]) for k, p in table.items() if k[2] == 2} == two
    # the switches that turn stage 2's pairs off, and a tree without pairs at all
    pts = C.random_cloud(3, 400, 27)
    assert C.make_tree(pts, 6, 30, env={"BBFMM_M2L_S2_PAIRS": "0"}, host_only=True).debug_m2l_s2_plan() == (0,) * 6
    assert C.make_tree(C.random_cloud(1, 64, 22), 6, 9, host_only=True).debug_m2l_s2_plan() == (0,) * 6
    # unset, the axes are picked by executed work, and the plan is that of the picked axes
    for d, order in ((2, 4), (2, 10), (3, 5), (3, 9)):
        t = C.make_tree(C.random_cloud(d, 400, 27), order, 30, host_only=True)
        assert t.debug_m2l_s2_plan() == table[d, order, t.debug_m2l_pairs_axes(stage=2)[0]["axes"]]
    assert C.GPU_INSTANCES == {(p[0], p[1], p[4], p[5]) for k, p in table.items() if k[0] == 3 and k[1] in (6, 8, 9, 10)}


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


# ------------------------------------------------------------------ M2P and the two-level clouds
def test_the_two_level_layouts_show_every_required_population_and_w_list_length():
    pops, lengths = set(), set()
    for name, (refined, leaves) in C.TWO_LEVEL[3].items():
        pops |= set(leaves.values())
        lengths |= {C.two_level_w_length(3, name, o) for o in leaves}
        assert sum(leaves.values()) + len(refined) * (max(leaves.values()) + 8) <= 3000
    assert C.TWO_LEVEL_POPULATIONS <= pops, sorted(C.TWO_LEVEL_POPULATIONS - pops)
    # the chunks of add_w_jobs (8) and of the fused jobs (16): below, at, between, at and above
    assert 4 in lengths and 8 in lengths and lengths & set(range(9, 16)) and 16 in lengths and max(lengths) >= 17
    assert all(max(C.TWO_LEVEL[3][name][1].values()) <= 66 for name in C.SMALL_TWO_LEVEL)
    small = {C.two_level_w_length(3, name, o) for name in C.SMALL_TWO_LEVEL for o in C.TWO_LEVEL[3][name][1]}
    assert {4, 8, 16, 17} <= small                                    # the layouts of the high orders show every chunk edge too


@pytest.mark.parametrize("d,name", [(d, name) for d in (3, 2, 1) for name in C.TWO_LEVEL[d]])
def test_two_level_geometry_and_jobs_from_host_only_handles(d, name):
    pts = C.two_level_cloud(d, name)
    t = C.make_tree(pts, 3, C.two_level_limit(d, name), host_only=True)
    C.assert_two_level(t, R.Geometry(t), d, name)
    assert t.debug_wx_jobs() == C.expected_wx_jobs(d, name)


M2P_KERNELS = [(0, 1.0, 1.0), (3, 0.5, 0.4)]                        # LinearRbf; Spheroidal3 with both branches inside the cube


def m2p_setup(d, name, order, kernel, K=2):
    """(points, geometry, level-1 leaves, oracle tree with its multipoles of dense weights), built once."""
    def make():
        pts = C.two_level_cloud(d, name)
        limit = C.two_level_limit(d, name)
        t = C.make_tree(pts, order, limit, host_only=True, kernel=kernel)
        geo = R.Geometry(t)
        leaves = C.assert_two_level(t, geo, d, name)
        r = O.FmmTree(pts, order, kernel[0], True, True, None, O.FmmParams(limit, C.ACA, 1e-7, 1024), base_range=kernel[1],
                      total_sill=kernel[2])
        inject_product_operators(t, r)
        assert geo.keys == [int(k) for k in r.cell_keys]
        w = C.dense_weights(len(pts), K, 61)
        r.set_weights(w)
        return pts, geo, leaves, r, w
    return cached(("m2p setup", d, name, order, kernel, K), make)


@pytest.mark.parametrize("kernel", M2P_KERNELS, ids=lambda k: f"kernel{k[0]}")
@pytest.mark.parametrize("d,name,order", [(3, "w8-12", 4), (2, "w2-3", 5), (1, "low", 6)])
def test_m2p_restatement_against_the_oracle_target_by_target(d, name, order, kernel):
    """The oracle's leaf pass with only its M2P term (flags = 2) on its own multipoles: values and gradients to 1e-13 of the
    largest value per leaf, and inside the bound of the module docstring (the host's kernel functions); targets in the
    level-2 leaves, which have no W list, receive exact zeros."""
    pts, geo, leaves, r, w = m2p_setup(d, name, order, kernel)
    K = w.shape[1]
    extra = [C.inside_copies(geo, c, pts[geo.src_idx[geo.src_ptr[c]:geo.src_ptr[c + 1]]], 12, 63 + o) for o, c in leaves.items()]
    targets = np.ascontiguousarray(np.concatenate([pts] + extra))
    y, g = r._eval(w, targets, True, flags=2)
    z = r._eval(w, targets, False, flags=2)[0]
    g = g.reshape(len(targets), K, d)
    leaf_of = np.asarray(r._assign_targets(targets)[3])
    level1 = np.isin(leaf_of, list(leaves.values()))
    assert (y[~level1] == 0).all() and (g[~level1] == 0).all() and (~level1).any()
    worst = [0.0, 0.0, 0.0]
    for o, c in leaves.items():
        rows = np.nonzero(leaf_of == c)[0]
        assert len(rows) == C.TWO_LEVEL[d][name][1][o] + 12
        yr, yb, gr, gb = R.m2p(geo, kernel, r.M, c, targets[rows], with_grads=True, where=0)
        zr, zb = R.m2p(geo, kernel, r.M, c, targets[rows], where=0)
        assert relerr(y[rows], yr) < 1e-13 and relerr(z[rows], zr) < 1e-13 and relerr(g[rows], gr) < 1e-13
        for i, (got, ref, bound) in enumerate(((z[rows], zr, zb), (y[rows], yr, yb), (g[rows], gr, gb))):
            ratio = float((np.abs(got.astype(LD) - ref) / bound).max())
            worst[i] = max(worst[i], ratio)
            assert ratio <= 1, (o, i, ratio)
    print(f"M2P d = {d} {name} order {order} kernel {kernel[0]}: largest error / bound, values {worst[0]:.3g}, values of the "
          f"gradient call {worst[1]:.3g}, gradients {worst[2]:.3g}")
    assert min(worst) > 0


@pytest.mark.parametrize("what", ["entry", "nodes", "cell", "rhs"])
@pytest.mark.parametrize("kernel", M2P_KERNELS, ids=lambda k: f"kernel{k[0]}")
def test_m2p_bound_catches_altered_multipoles(kernel, what):
    """From the restatement alone: one entry of M scaled by 1 + 1e-9, two nodes of one W cell swapped, one W cell dropped,
    right-hand sides 0 and 1 exchanged -- each moves every target it touches by more than its bound, in the values and in
    the largest gradient component.  The leaf with the longest W list of the layout (19 cells): the largest N, the widest
    bound."""
    d, name, order = 3, "w14-19-small", 4
    pts, geo, leaves, r, w = m2p_setup(d, name, order, kernel)
    c = leaves[6]
    wp, wi = geo.lists["W"]
    cells = wi[wp[c]:wp[c + 1]]
    assert len(cells) == 19
    own = pts[geo.src_idx[geo.src_ptr[c]:geo.src_ptr[c + 1]]]
    targets = np.concatenate([own, C.inside_copies(geo, c, own, 12, 65)])
    M = np.array(r.M)
    bad = M.copy()
    touched = [0]
    if what == "entry":                                               # the largest entry of one cell, first right-hand side
        j = int(np.argmax(np.abs(M[0, cells[3]])))
        bad[0, cells[3], j] *= 1 + 1e-9
    elif what == "nodes":                                             # opposite corners of the cell
        bad[0, cells[5], [0, geo.n - 1]] = M[0, cells[5], [geo.n - 1, 0]]
    elif what == "cell":
        bad[0, cells[-1]] = 0
    else:
        bad[[0, 1]] = M[[1, 0]]
        touched = [0, 1]
    assert not np.array_equal(bad, M)
    yr, yb, gr, gb = R.m2p(geo, kernel, M, c, targets, with_grads=True)
    ya, _, ga, _ = R.m2p(geo, kernel, bad, c, targets, with_grads=True)
    zr, zb = R.m2p(geo, kernel, M, c, targets)
    za = R.m2p(geo, kernel, bad, c, targets)[0]
    ratios = [(np.abs(zr - za) / zb)[:, touched], (np.abs(yr - ya) / yb)[:, touched], (np.abs(gr - ga) / gb)[:, touched].max(axis=2)]
    print(f"M2P altered ({what}, kernel {kernel[0]}): smallest |reference - altered| / bound over the targets: values "
          f"{float(ratios[0].min()):.3g}, values of the gradient call {float(ratios[1].min()):.3g}, gradients {float(ratios[2].min()):.3g}")
    assert all(float(q.min()) > 1 for q in ratios)
    rest = [k for k in range(M.shape[0]) if k not in touched]
    assert np.array_equal(zr[:, rest], za[:, rest])                  # the other right-hand sides are untouched
