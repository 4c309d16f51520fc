"""The changes of basis of the M2L stages inside M2M and L2L (BBFMM_FUSED_PASSES): the fused kernels against the standalone
passes bit for bit where the order of the sums is the same, and against the long-double restatement of
tests/far_field_reference.py (its bounds, cell by cell) where cells with an X list add in another order or the buffers
start dirty.  Handles are created under each setting of the switch; the clouds are those of tests/far_field_cases.py.
"""
import hashlib

import numpy as np
import pytest

import ferreus_rbf_rs_amd as F
import far_field_cases as C
import far_field_reference as R

pytestmark = pytest.mark.gpu

cached = C.cached
OFF = {"BBFMM_FUSED_PASSES": "0"}


@pytest.fixture(scope="module", autouse=True)
def _release_everything_at_the_end():
    yield
    C.drop_cached()


@pytest.fixture(autouse=True)
def _one_tree_at_a_time(request):
    params = getattr(getattr(request.node, "callspec", None), "params", {})
    group = (request.function.__name__, params.get("order"), str(params.get("env")))
    if C.cached(("group",), lambda: [None])[0] != group:
        C.drop_cached(keep=("cloud",))
        C.cached(("group",), lambda: [None])[0] = group
    yield


def cloud(name):
    return cached(("cloud", name), {"populations": lambda: C.populations_cloud()[0], "lattice8": C.lattice8_cloud,
                                    "clustered": C.clustered_cloud, "depth1": lambda: C.random_cloud(3, 200, 23),
                                    "small": lambda: C.random_cloud(3, 20000, 24)}[name])


LIMITS = {"populations": C.POPULATIONS_LIMIT, "lattice8": C.LATTICE_LIMIT, "clustered": C.CLUSTERED_LIMIT, "depth1": 100, "small": 100}


def tree(name, order, env=None, deterministic=False):
    """(handle, geometry); deterministic: BBFMM_FLAG_DETERMINISTIC, under which no stage-2 launch splits its contraction --
    on trees this small the only handles whose Lp is not cleared."""
    def make():
        if not deterministic:
            t = C.make_tree(cloud(name), order, LIMITS[name], env=env, sparse=name != "populations")
        else:
            with C.environment(env or {}):
                t = F.FmmTree(cloud(name), order, F.KernelParams(F.KernelType(0), base_range=1.0, total_sill=1.0), True, True,
                              params=F.FmmParams(LIMITS[name], F.M2LCompressionType(C.ACA), 1e-7, 1024), deterministic=True)
        return t, R.Geometry(t)
    return cached(("tree", name, order, tuple(sorted((env or {}).items())), deterministic), make)


def passes(t, w):
    """set_weights + the whole-tree downward pass: (M, Mp, L) as the device holds them."""
    K = w.shape[1]
    t.set_weights(w)
    t.set_local_coefficients(w)
    P = t.debug_get_coefficients("P", K) if t.stats().m2l_batches > 0 else None    # (a tree without M2L keeps no Mp)
    return t.debug_get_coefficients("M", K), P, t.debug_get_coefficients("L", K)


def no_x(geo):
    return np.diff(geo.lists["X"][0]) == 0


def plain_cells(geo):
    """Cells whose L the two sequences form by the same additions: no X list in the cell or in any ancestor.  In a cell with an
    X list the standalone sequence adds the P2L terms onto the M2L part one atomic at a time, the fused one sums them first and
    adds the M2L part to the sum: equal values, another rounding, which L2L hands down to the descendants."""
    tainted = ~no_x(geo)
    for c in np.argsort(geo.level, kind="stable"):
        if geo.parent[c] >= 0 and tainted[geo.parent[c]]:
            tainted[c] = True
    return ~tainted


def assert_same_as_standalone(name, order, K, env=None, seed=61, deterministic=False):
    """M, Mp and -- in the cells without an X list above or in them (plain_cells) -- L of the fused handle equal those of the
    standalone passes bit for bit; the pads of Mp are exactly zero."""
    pts = cloud(name)
    w = C.dense_weights(len(pts), K, seed + K)
    (tf, geo), (ts, _) = tree(name, order, env, deterministic), tree(name, order, dict(env or {}, **OFF), deterministic)
    Mf, Pf, Lf = passes(tf, w)
    Ms, Ps, Ls = passes(ts, w)
    assert np.array_equal(Mf, Ms)
    assert Pf.shape == Ps.shape and Pf.shape[2] >= geo.n
    assert np.array_equal(Pf, Ps), int((Pf != Ps).any(axis=(0, 2)).sum())
    pads = (Ps[:, geo.level >= 2] == 0).all(axis=(0, 1))            # dense weights: a column that is zero in every row is a pad
    assert pads.sum() == Pf.shape[2] - geo.n, (int(pads.sum()), Pf.shape[2], geo.n)
    assert (Pf[:, :, pads] == 0).all()
    plain = plain_cells(geo)
    assert plain.sum() > 0 and np.isfinite(Lf).all()
    if tf.debug_m2l_s2_last_ksplit() == 1 and ts.debug_m2l_s2_last_ksplit() == 1:
        assert np.array_equal(Lf[:, plain], Ls[:, plain]), np.nonzero((Lf != Ls).any(axis=(0, 2)) & plain)[0][:10]
    else:
        # Stage 2 split its contraction and the parts met in Lp by atomic additions, in an order that changes from run to run
        # (two runs of either sequence differ in the last bits): the fused L against the restatement instead.
        # Every cell with an X list and every fifth of the others (all octant classes and levels): the restatement of a cell
        # does not depend on the other cells, and the bit-for-bit cases cover every cell.
        assert not deterministic
        some = np.nonzero((geo.level >= 2) & (~no_x(geo) | (np.arange(geo.C) % 5 == 0)))[0]
        assert set(geo.octant[some]) == set(range(8)) and set(geo.level[some]) == set(geo.level[geo.level >= 2])
        check_L(tf, geo, (name, order, tuple(sorted((env or {}).items()))), pts, w, Mf, Lf, f"{name} order {order} K {K} {env or ''}",
                cells=some)
    return tf, geo, w, Mf, Lf


def check_L(t, geo, key, pts, w, M, L, what, cells=None):
    """check_downward of test_gpu_far_field_passes.py: every cell from level 2 down (or the listed ones) against M2L of the
    device's M plus L2L of the device's parent L plus the X-list term, with the bounds of far_field_reference."""
    m2l = cached(("m2l operators", key), lambda: R.M2L(geo, t))
    full = cells is None
    cells = np.nonzero(geo.level >= 2)[0] if full else np.asarray(cells)
    res = cached(("m2l result", key, hashlib.sha256(M.tobytes()).hexdigest()), lambda: m2l.apply(M)) if full else None
    ref, bound = R.downward(geo, m2l, R.Transfers(geo), M, L, cells, ((0, 1.0, 1.0), pts, w, 1), m2l_result=res)
    untouched = [(k, c) for c in cells for k in range(L.shape[0]) if bound[c][k] == 0]   # nothing reaches them: exact zeros
    assert all((L[k, c] == 0).all() for k, c in untouched)
    R.check_cells("fused M2L + L2L", L, ref, bound, cells, what,
                  lambda c: f"level {geo.level[c]}, class {geo.octant[c]}, anchor {geo.anchor[c].tolist()}")
    return len(untouched)


# ------------------------------------------------------------------ against the standalone passes, bit for bit
@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("deterministic", [False, True])
@pytest.mark.parametrize("order", [4, 5, 7, 9])
def test_lattice_equals_the_standalone_passes(order, deterministic, K):
    """An even order, odd orders with centre planes, the second stage-2 instance (order 9).  Deterministic handles never
    split the contraction: L is compared bit for bit at every order and K, and the fused handle does not clear Lp."""
    tf = assert_same_as_standalone("lattice8", order, K, deterministic=deterministic)[0]
    if deterministic:
        assert tf.debug_m2l_s2_last_ksplit() == 1


@pytest.mark.parametrize("order,env", [(3, {}), (7, {"BBFMM_M2L_S1_AXES": "1", "BBFMM_M2L_S2_AXES": "1"})])
def test_one_axis_layouts_equal_the_standalone_passes(order, env):
    """Order 3 keeps the one-axis layout under the unset rule; order 7 is forced to it."""
    tf = assert_same_as_standalone("lattice8", order, 2, env)[0]
    assert tf.debug_m2l_pairs_axes()[0]["axes"] == 1
    if env:
        assert tf.debug_m2l_pairs_axes(stage=2)[0]["axes"] == 1
    print("order", order, "axes of stage 2:", tf.debug_m2l_pairs_axes(stage=2)[0]["axes"])
    td = assert_same_as_standalone("lattice8", order, 2, env, deterministic=True)[0]
    assert td.debug_m2l_pairs_axes()[0]["axes"] == 1 and td.debug_m2l_s2_last_ksplit() == 1


# ------------------------------------------------------------------ cells with an X list, leaves at several levels
def test_clustered_cloud_against_the_reference_and_no_carry_over():
    """Every cell against the restatement; two matvecs with different weights on one handle, the second checked alone:
    the rows P2L adds to must not carry the first."""
    t, geo = tree("clustered", 4)
    pts = cloud("clustered")
    assert t.stats().n_w > 0 and (~no_x(geo) & (geo.level >= 2)).sum() > 0
    assert len({int(l) for l in geo.level[geo.is_leaf]}) > 1
    w1 = 1e6 * C.dense_weights(len(pts), 2, 63)
    passes(t, w1)
    w2 = C.dense_weights(len(pts), 2, 64)
    M, _, L = passes(t, w2)
    check_L(t, geo, ("clustered", 4), pts, w2, M, L, "clustered order 4, second matvec")
    ts, _ = tree("clustered", 4, OFF)
    Ms, _, Ls = passes(ts, w2)
    assert np.array_equal(M, Ms)


# ------------------------------------------------------------------ dirty buffers: Lp is not cleared
def test_dirty_lp_large_weights_then_one_leaf():
    """A matvec with large weights everywhere, then one with weights in one corner leaf: the cells nothing reaches must hold
    exact zeros and every other cell its own value -- a stale row of Lp or an unread flag is a wrong cell."""
    t, geo = tree("lattice8", 5, deterministic=True)
    pts = cloud("lattice8")
    passes(t, 1e8 * C.dense_weights(len(pts), 1, 65))
    leaf = int(np.nonzero((geo.level == 3) & (geo.anchor == np.array([0, 0, 7])).all(axis=1))[0][0])
    w = C.leaf_weights(geo, len(pts), leaf, 1, 66)
    M, _, L = passes(t, w)
    assert t.debug_m2l_s2_last_ksplit() == 1                        # no launch split its contraction: Lp was not cleared
    n_zero = check_L(t, geo, ("lattice8", 5), pts, w, M, L, "lattice8 order 5, one leaf after large weights")
    assert n_zero > 0
    ts, _ = tree("lattice8", 5, OFF, deterministic=True)
    _, _, Ls = passes(ts, w)
    plain = plain_cells(geo)
    assert np.array_equal(L[:, plain], Ls[:, plain])


# ------------------------------------------------------------------ shallow trees
def test_depth_two_level_two_cells_only():
    """The parents hold zeros: L of a level-2 cell is its M2L part alone."""
    tf, geo, w, M, L = assert_same_as_standalone("populations", 5, 2)
    assert tf.stats().depth == 2
    check_L(tf, geo, ("populations", 5), cloud("populations"), w, M, L, "populations order 5")
    assert (L[:, geo.level < 2] == 0).all()


def test_depth_one_nothing_to_do():
    """No M2L batches: the fused path does nothing at all."""
    pts = cloud("depth1")
    (tf, geo), (ts, _) = tree("depth1", 5), tree("depth1", 5, OFF)
    assert tf.stats().depth == 1 and tf.stats().m2l_batches == 0
    w = C.dense_weights(len(pts), 2, 67)
    Mf, Pf, Lf = passes(tf, w)
    Ms, Ps, Ls = passes(ts, w)
    assert Pf is None and Ps is None
    assert np.array_equal(Mf, Ms) and np.array_equal(Lf, Ls)
    assert (Lf == 0).all()
    assert np.array_equal(tf.evaluate(w, pts), ts.evaluate(w, pts))


# ------------------------------------------------------------------ a small tree: stage 2 splits its contraction, Lp is cleared
def test_small_tree_split_contraction_keeps_the_clear():
    t, geo = tree("small", 4)
    pts = cloud("small")
    passes(t, 1e8 * C.dense_weights(len(pts), 1, 68))               # what a missing clear would add to
    w = C.dense_weights(len(pts), 1, 69)
    M, _, L = passes(t, w)
    assert t.debug_m2l_s2_last_ksplit() > 1, t.debug_m2l_s2_last_ksplit()
    check_L(t, geo, ("small", 4), pts, w, M, L, "20k points order 4, split contraction")


# ------------------------------------------------------------------ fallbacks after a fused matvec on the same handle
def test_restricted_plan_after_a_fused_matvec():
    """test_restricted_downward_pass_active_flags of test_gpu_far_field_passes.py behind a whole-tree pass."""
    t, geo = tree("clustered", 4)
    pts = cloud("clustered")
    passes(t, 1e6 * C.dense_weights(len(pts), 1, 70))
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
    check_L(t, geo, ("clustered", 4), pts, w, M, L, "clustered order 4, 40 targets after a fused pass", cells=sorted(cells))
    M, _, L = passes(t, w)                                          # and the fused pass again behind the restricted one
    check_L(t, geo, ("clustered", 4), pts, w, M, L, "clustered order 4, fused after restricted")


def test_chunked_right_hand_sides_after_a_fused_matvec():
    t, geo = tree("lattice8", 4, {"BBFMM_M2L_CBUF_MB": "4"})
    pts = cloud("lattice8")
    passes(t, 1e6 * C.dense_weights(len(pts), 1, 71))               # one right-hand side fits a pass: fused
    K = 3
    w = C.dense_weights(len(pts), K, 72)
    M, _, L = passes(t, w)
    assert t.stats().m2l_rhs_per_pass < K, t.stats().m2l_rhs_per_pass
    check_L(t, geo, ("lattice8", 4, "cbuf"), pts, w, M, L, "lattice8 order 4, K 3 in chunks")
    ts, _ = tree("lattice8", 4, dict(OFF, BBFMM_M2L_CBUF_MB="4"))
    Ms, _, _ = passes(ts, w)
    assert np.array_equal(M, Ms)


def test_deterministic_handle():
    t, geo = tree("lattice8", 4, deterministic=True)
    pts = cloud("lattice8")
    passes(t, 1e6 * C.dense_weights(len(pts), 2, 73))
    w = C.dense_weights(len(pts), 2, 74)
    M, _, L = passes(t, w)
    assert t.debug_m2l_s2_last_ksplit() == 1
    check_L(t, geo, ("lattice8", 4, "det"), pts, w, M, L, "lattice8 order 4, deterministic")


# ------------------------------------------------------------------ L2P writes the caller's order
@pytest.mark.parametrize("K", [1, 2])
def test_l2p_writes_the_callers_order_bit_for_bit(K):
    """matvec_device with ldo > N under the mask with and without bit 8, and evaluate at the sources: one add in the same
    order, so the potentials are equal bit for bit; the rows of the output between N and ldo are left alone.  Deterministic
    handles: without atomics two runs of the same sequence agree bit for bit, so a difference is the fused store's."""
    import torch
    pts = cloud("clustered")
    N, ldo = len(pts), len(pts) + 5
    w = C.dense_weights(N, K, 75)
    got = {}
    for mask in ("7", "15"):
        t, _ = tree("clustered", 4, {"BBFMM_FUSED_PASSES": mask}, deterministic=True)
        d_w = torch.tensor(np.asfortranarray(w).T.copy(), device="cuda")                 # K columns of N rows
        d_out = torch.full((K, ldo), -7.0, dtype=torch.float64, device="cuda")
        t.matvec_device(d_w.data_ptr(), N, K, d_out.data_ptr(), ldo)
        y = d_out.cpu().numpy()
        assert (y[:, N:] == -7.0).all()
        t.set_weights(w)
        got[mask] = (y[:, :N].copy(), t.evaluate(w, pts))
        assert t.last_evaluate_path() == 1
    assert np.isfinite(got["15"][0]).all() and np.abs(got["15"][0]).max() > 0
    assert np.array_equal(got["7"][0], got["15"][0])
    assert np.array_equal(got["7"][1], got["15"][1])
