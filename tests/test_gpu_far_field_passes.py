"""P2M, M2M, M2L + L2L (+ P2L) and L2P on the device, each pinned to the long-double restatement of
tests/far_field_reference.py cell by cell (L2P: target by target) with the bounds derived there.  Every pass is restated one
step from the device's own input, read back with debug_get_coefficients, so a failure names its pass, cell and right-hand
side; every assertion prints its largest error / bound ratio.  The clouds are those of tests/far_field_cases.py."""
import hashlib

import numpy as np
import pytest

import far_field_cases as C
import far_field_reference as R
from far_field_reference import LD

pytestmark = pytest.mark.gpu

cached = C.cached


@pytest.fixture(autouse=True)
def _one_group_of_cases_at_a_time(request):
    """Handles and references are shared by the cases of one test function at one order, which run next to each other;
    when the next group starts they are dropped (the clouds stay), and everything goes when the module is done."""
    params = getattr(getattr(request.node, "callspec", None), "params", {})
    group = (request.function.__name__, params.get("name"), params.get("order"))
    if C.cached(("group",), lambda: [None])[0] != group:
        C.drop_cached(keep=("cloud",))
        C.cached(("group",), lambda: [None])[0] = group
    yield


@pytest.fixture(scope="module", autouse=True)
def _release_everything_at_the_end():
    yield
    C.drop_cached()


def cloud(name):
    return cached(("cloud", name), {"populations": lambda: C.populations_cloud()[0], "lattice8": C.lattice8_cloud,
                                    "lattice16": C.lattice16_cloud, "clustered": C.clustered_cloud,
                                    "2d": lambda: C.random_cloud(2, 16 ** 3, 21), "1d": lambda: C.random_cloud(1, 64, 22),
                                    "lattice2d": C.lattice2d_cloud, "clustered2d": C.clustered2d_cloud, "line": C.line_cloud}[name])


LIMITS = {"populations": C.POPULATIONS_LIMIT, "lattice8": C.LATTICE_LIMIT, "lattice16": C.LATTICE_LIMIT,
          "clustered": C.CLUSTERED_LIMIT, "2d": 70, "1d": 9, "lattice2d": C.LATTICE_LIMIT, "clustered2d": C.CLUSTERED_LIMIT,
          "line": C.LINE_LIMIT}


def tree(name, order, env=None, kernel=(0, 1.0, 1.0), epsilon=1e-7, compression=C.ACA):
    """(handle, geometry) of a cloud, built once per configuration; the populations tree stores its empty cells."""
    def make():
        t = C.make_tree(cloud(name), order, LIMITS[name], env=env, kernel=kernel, sparse=name != "populations", epsilon=epsilon,
                        compression=compression)
        geo = R.Geometry(t)
        if name == "populations":
            C.assert_populations(t, C.populations_cloud()[1])
        if name == "lattice8":
            C.assert_lattice8(t, geo)
        if name == "lattice2d":
            C.assert_lattice2d(t, geo)
        if name == "line":
            C.assert_line(t, geo)
        return t, geo
    return cached(("tree", name, order, tuple(sorted((env or {}).items())), kernel, epsilon, compression), make)


# ------------------------------------------------------------------ P2M
P2M_CASES = ([("populations", p, K) for p in list(range(4, 11)) + [2, 3, 11, 12] for K in (1, 2, 3)] +   # mfma; KB 1, 2, k0 = 2
             [("populations", p, K) for p in (13, 16) for K in (1, 2)] +                                 # one rhs per pass
             [("2d", p, K) for p in (3, 7, 16) for K in (1, 3)] + [("1d", p, K) for p in (4, 16) for K in (1, 3)])


@pytest.mark.parametrize("name,order,K", P2M_CASES)
def test_p2m_leaf_by_leaf(name, order, K):
    t, geo = tree(name, order)
    pts = cloud(name)
    w = C.dense_weights(len(pts), K, 31 + K)                         # other weights for every K: no case leans on the last
    res = R.p2m(geo, pts, w)
    t.set_weights(w)
    M = t.debug_get_coefficients("M", K)
    ref = {c: v[0] for c, v in res.items()}
    bound = {c: R.p2m_bound(geo, v[1], v[2], v[3]) for c, v in res.items()}
    R.check_cells("P2M", M, ref, bound, sorted(ref), f"{name} order {order} K {K}")
    empty = geo.is_leaf & (np.diff(geo.src_ptr) == 0)
    if name == "populations":
        assert empty.sum() == 2
    assert (M[:, empty] == 0).all()                                  # cells without points: exactly zero


# ------------------------------------------------------------------ M2M
@pytest.mark.parametrize("K", [1, 2])                               # (the upper decorator varies fastest: one handle per order)
@pytest.mark.parametrize("name,order", [("lattice8", p) for p in (2, 5, 7, 10, 11, 13, 16)] + [("2d", 7), ("1d", 16)])
def test_m2m_each_parent_from_its_childrens_device_coefficients(name, order, K):
    t, geo = tree(name, order)
    w = C.dense_weights(len(cloud(name)), K, 33 + K)
    t.set_weights(w)
    M = t.debug_get_coefficients("M", K)
    xf = R.Transfers(geo)
    parents = [c for c in range(geo.C) if geo.level[c] >= 1 and not geo.is_leaf[c]]
    if name == "lattice8":                                           # every child count of the cloud
        assert sorted({len(geo.children[c]) for c in parents}) == [1, 2, 3, 5, 7, 8]
    ref, bound = {}, {}
    for c in parents:
        ref[c], bound[c] = R.m2m(geo, xf, M, c)
    R.check_cells("M2M", M, ref, bound, parents, f"{name} order {order} K {K}")


# ------------------------------------------------------------------ M2L + L2L (+ P2L)
def device_passes(t, w):
    K = w.shape[1]
    t.set_weights(w)
    t.set_local_coefficients(w)
    return t.debug_get_coefficients("M", K), t.debug_get_coefficients("L", K)


def check_downward(t, geo, key, pts, w, what, kernel=(0, 1.0, 1.0), cells=None, M=None, L=None, p2l_cache=None):
    """Every cell from level 2 down (or the listed ones) against M2L of the device's M plus L2L of the device's parent L
    plus the X-list term; returns the largest ratio and the number of (right-hand side, cell) pairs nothing reaches.  The
    M2L restatement depends on M alone, which the M2L switches do not touch: it is shared by the handles whose M agrees
    bit for bit.  p2l_cache: see far_field_reference.downward; with listed cells it also keeps the M2L restatement of those
    cells column by column (M2L treats the right-hand sides independently), so that calls which differ in the number of
    right-hand sides, or handles whose M agrees bit for bit, restate a column once."""
    if M is None:
        M, L = device_passes(t, w)
    m2l = cached(("m2l operators", key), lambda: R.M2L(geo, t))
    full = cells is None
    cells = np.nonzero(geo.level >= 2)[0] if full else np.asarray(cells)
    res = cached(("m2l result", key, hashlib.sha256(M.tobytes()).hexdigest()), lambda: m2l.apply(M)) if full else None
    if p2l_cache is not None and not full:
        live = (M != 0).any(axis=2)
        assert (live == live[:1]).all()                               # the same sources are live in every column: one R for all
        cols = []
        for k in range(M.shape[0]):
            col = ("m2l column", hashlib.sha256(M[k].tobytes()).hexdigest(), len(cells))
            if col not in p2l_cache:
                p2l_cache[col] = m2l.apply(M[k:k + 1], cells=cells)
            cols.append(p2l_cache[col])
        res = (np.concatenate([c[0] for c in cols]), np.concatenate([c[1] for c in cols]), cols[0][2])
    ref, bound = R.downward(geo, m2l, R.Transfers(geo), M, L, cells, (kernel, pts, w, 1), m2l_result=res, p2l_cache=p2l_cache)
    untouched = [(k, c) for c in cells for k in range(L.shape[0]) if bound[c][k] == 0]   # nothing reaches them: exact zeros
    assert all((L[k, c] == 0).all() for k, c in untouched)
    ratio = R.check_cells("M2L + L2L", L, ref, bound, cells, what,
                          lambda c: f"level {geo.level[c]}, class {geo.octant[c]}, anchor {geo.anchor[c].tolist()}")
    return ratio, len(untouched)


SWITCHES = [{}, {"BBFMM_M2L_S1_PAIRS": "0"}, {"BBFMM_M2L_S1_AXES": "1"}, {"BBFMM_M2L_S1_AXES": "2"}, {"BBFMM_M2L_S2_PAIRS": "0"}]


@pytest.mark.parametrize("env", SWITCHES, ids=lambda e: ",".join(f"{k[10:]}={v}" for k, v in e.items()) or "default")
@pytest.mark.parametrize("order,kind", [(3, "dense"), (3, "sparse"), (4, "dense"), (4, "sparse"), (5, "dense"), (5, "sparse"),
                                        (7, "sparse")])
def test_m2l_and_l2l_on_the_lattice_under_every_switch(order, kind, env):
    t, geo = tree("lattice8", order, env)
    pts = cloud("lattice8")
    if "BBFMM_M2L_S1_PAIRS" in env:
        assert not t.debug_m2l_pairs()[0]
    if "BBFMM_M2L_S1_AXES" in env:
        assert t.debug_m2l_pairs_axes()[0]["axes"] == int(env["BBFMM_M2L_S1_AXES"])
    if "BBFMM_M2L_S2_PAIRS" in env:
        assert not t.debug_m2l_pairs(stage=2)[0]
    w = C.dense_weights(len(pts), 1, 35) if kind == "dense" else C.sparse_lattice_weights(pts, 8, 37)
    _, n_zero = check_downward(t, geo, ("lattice8", order), pts, w, f"lattice8 order {order} {kind} {env}")
    if kind == "sparse":
        assert n_zero > 0


def test_m2l_and_l2l_three_right_hand_sides():
    t, geo = tree("lattice8", 5)
    pts = cloud("lattice8")
    check_downward(t, geo, ("lattice8", 5), pts, C.dense_weights(len(pts), 3, 39), "lattice8 order 5 K 3")


def test_m2l_full_tiles_on_the_16_lattice_sparse_weights():
    t, geo = tree("lattice16", 5)
    pts = cloud("lattice16")
    assert t.stats().depth == 4 and (geo.level == 4).sum() == 4096           # 512 cells per class
    w = C.sparse_lattice_weights(pts, 16, 41, C.FEW_COLUMNS)
    _, n_zero = check_downward(t, geo, ("lattice16", 5), pts, w, "lattice16 order 5 sparse")
    assert n_zero > 0


def test_m2l_level_cut_into_groups():
    t, geo = tree("lattice16", 4, {"BBFMM_M2L_CBUF_MB": "8"})
    pts = cloud("lattice16")
    assert any(op["kind"] == 1 and op["pairs"] for op in t.debug_m2l_pairs()[1])  # one stage-1 operator per group
    w = C.sparse_lattice_weights(pts, 16, 43, C.FEW_COLUMNS)
    check_downward(t, geo, ("lattice16", 4), pts, w, "lattice16 order 4 sparse, groups")


def test_m2l_low_rank_gaussian_on_the_clustered_cloud():
    kernel = (100, 0.5, 0.4)
    t, geo = tree("clustered", 5, kernel=kernel, epsilon=1e-5)
    pts = cloud("clustered")
    assert t.stats().n_w > 0
    print("ranks at the deepest level:", t.m2l_ranks()[t.stats().depth].tolist())
    check_downward(t, geo, ("clustered", 5, kernel), pts, C.dense_weights(len(pts), 1, 45), "clustered Gaussian order 5", kernel)


@pytest.mark.parametrize("order", [9, 12, 13, 16])
def test_l2l_alone_where_m2l_vanishes(order):
    """Weights on one corner leaf: a cell more than three cells from it receives nothing through its own V list (restated
    as exact zeros), so its L is L2L of the device's parent L alone -- l2l3_kernel at 9 and 12, the general kernel above."""
    t, geo = tree("lattice8", order)
    pts = cloud("lattice8")
    leaf = int(np.nonzero((geo.level == 3) & (geo.anchor == np.array([0, 0, 7])).all(axis=1))[0][0])
    w = C.leaf_weights(geo, len(pts), leaf, 2, 47)
    M, L = device_passes(t, w)
    live = (M != 0).any(axis=(0, 2))
    has_live_source = np.zeros(geo.C, dtype=bool)
    has_live_source[geo.v_tgt[live[geo.v_src]]] = True
    parent_live = (L[:, np.maximum(geo.parent, 0)] != 0).any(axis=(0, 2)) & (geo.parent >= 0)
    no_x = np.diff(geo.lists["X"][0]) == 0
    cells = np.nonzero((geo.level >= 3) & ~has_live_source & parent_live & no_x)[0]
    assert len(cells) > 100 and set(geo.octant[cells]) == set(range(8))
    val, bnd = R.l2l_many(geo, R.Transfers(geo), L, cells)           # (M2L is not restated: no operator is read)
    ref = {int(c): val[:, i] for i, c in enumerate(cells)}
    bound = {int(c): bnd[:, i] for i, c in enumerate(cells)}
    R.check_cells("L2L alone", L, ref, bound, [int(c) for c in cells], f"lattice8 order {order}")


def test_restricted_downward_pass_active_flags():
    """evaluate at 40 targets: only the cells on the paths to those targets' leaves are computed, and asserted."""
    t, geo = tree("clustered", 4)
    pts = cloud("clustered")
    w = C.dense_weights(len(pts), 1, 49)
    targets = np.ascontiguousarray(pts[np.random.default_rng(51).choice(len(pts), 40, replace=False)])
    t.set_weights(w)
    t.evaluate(w, targets)
    M, L = t.debug_get_coefficients("M", 1), t.debug_get_coefficients("L", 1)
    cells = set()
    for c in t.points_to_leaves(targets):
        while c >= 0 and geo.level[c] >= 2:
            cells.add(int(c))
            c = geo.parent[c]
    check_downward(t, geo, ("clustered", 4), pts, w, "clustered order 4, 40 targets", cells=sorted(cells), M=M, L=L)


# ------------------------------------------------------------------ P2L
@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("kid", [0, 2])
def test_p2l_cells_with_an_x_list(kid, K):
    kernel = (kid, 1.0, 1.0)
    t, geo = tree("clustered", 4, kernel=kernel)
    pts = cloud("clustered")
    assert t.stats().n_w > 0
    w = C.dense_weights(len(pts), K, 53)
    M, L = device_passes(t, w)
    cells = np.nonzero((np.diff(geo.lists["X"][0]) > 0) & (geo.level >= 2))[0]
    assert len(cells) > 0
    check_downward(t, geo, ("clustered", 4, kernel), pts, w, f"P2L kernel {kid} K {K}", kernel, cells=cells, M=M, L=L)


# ------------------------------------------------------------------ L2P
def l2p_only_leaves(geo, w, M):
    """Leaves whose U and W lists hold only zero weights: evaluate returns L2P of their L and nothing else."""
    up, ui = geo.lists["U"]
    wp, wi = geo.lists["W"]
    weight = np.zeros(geo.C, dtype=bool)
    for c in np.nonzero(np.diff(geo.src_ptr) > 0)[0]:
        weight[c] = np.any(w[geo.src_idx[geo.src_ptr[c]:geo.src_ptr[c + 1]]] != 0)
    live_M = (M != 0).any(axis=(0, 2))
    return [c for c in np.nonzero(geo.is_leaf)[0]
            if not weight[ui[up[c]:up[c + 1]]].any() and not live_M[wi[wp[c]:wp[c + 1]]].any()]


def corner_leaves(geo):
    """The leaves of the first and the last point-holding cell in key order: opposite corners of the domain."""
    holds = np.nonzero(geo.is_leaf & (np.diff(geo.src_ptr) > 0))[0]
    lo = holds[np.argmin(geo.centres[holds].sum(axis=1))]
    hi = holds[np.argmax(geo.centres[holds].sum(axis=1))]
    return int(lo), int(hi)


L2P_CASES = ([("populations", p, K, False) for p in (2, 5, 7, 12, 13, 14, 16) for K in (1, 3)] +   # four waves, two, one
             [("populations", 5, 1, True), ("2d", 7, 1, False), ("2d", 7, 3, False), ("1d", 4, 1, False), ("1d", 4, 3, False)])


@pytest.mark.parametrize("name,order,K,superset", L2P_CASES)
def test_l2p_target_by_target(name, order, K, superset):
    """Values and gradients, every right-hand side."""
    t, geo = tree(name, order)
    pts = cloud(name)
    targets = pts
    if superset:                                                      # other per-leaf target counts, another order
        rng = np.random.default_rng(57)
        targets = np.concatenate([pts, C.on_grid(0.02 + 0.96 * rng.random((500, geo.d)))])
        targets = np.ascontiguousarray(targets[rng.permutation(len(targets))])
    leaf_of = t.points_to_leaves(targets)
    done, worst, worst_g = set(), 0.0, 0.0
    for corner in corner_leaves(geo):
        w = C.leaf_weights(geo, len(pts), corner, K, 59)
        t.set_weights(w)
        y, g = t.evaluate_with_gradients(w, targets)
        g = g.reshape(len(targets), K, geo.d)
        M, L = t.debug_get_coefficients("M", K), t.debug_get_coefficients("L", K)
        for c in l2p_only_leaves(geo, w, M):
            rows = np.nonzero(leaf_of == c)[0]
            if c in done or len(rows) == 0:
                continue
            done.add(c)
            out = R.l2p(geo, L, c, targets[rows], with_grads=True)
            err = np.abs(y[rows].astype(LD) - out[0])
            assert (err <= out[1]).all(), ("L2P", name, order, K, "leaf", c, float((err / out[1]).max()))
            with np.errstate(all="ignore"):
                worst = max(worst, float(np.where(err > 0, err / out[1], 0).max()))
            err = np.abs(g[rows].astype(LD) - out[2])
            assert (err <= out[3]).all(), ("L2P gradient", name, order, K, "leaf", c, float((err / out[3]).max()))
            with np.errstate(all="ignore"):
                worst_g = max(worst_g, float(np.where(err > 0, err / out[3], 0).max()))
    print(f"L2P {name} order {order} K {K}: largest error / bound {worst:.3g}, gradients {worst_g:.3g}, {len(done)} leaves")
    assert set(np.unique(leaf_of).tolist()) <= done                   # every leaf is an L2P-only leaf in one of the two runs
