"""M2L + L2L (+ P2L) on the device where tests/test_gpu_far_field_passes.py does not go: the stage-2 kernel instances of 3-D
orders 6, 8, 9 and 10, trees of two dimensions and of one, uncompressed operators, and more right-hand sides than one pass
takes.  Every case goes through check_downward of that module (each cell's L against the long-double restatement under the
derived bounds of tests/far_field_reference.py) and prints its largest error / bound ratio.  Every M2L case asserts from
the geometry that its live (source, target) pairs reach every transfer vector of its dimension, and every case with stage-2
pairs that the handle runs the instance the table of tests/test_far_field_reference_host.py names."""
import numpy as np
import pytest

import far_field_cases as C
import test_gpu_far_field_passes as P

pytestmark = pytest.mark.gpu

ids = lambda e: ",".join(f"{k[10:]}={v}" for k, v in e.items()) or "default"   # noqa: E731
SEEN = {}                                                             # 3-D case -> the stage-2 instance it ran


@pytest.fixture(autouse=True)
def _one_group_of_cases_at_a_time(request):
    """As in tests/test_gpu_far_field_passes.py: the handles and references of one test function at one order are shared."""
    params = getattr(getattr(request.node, "callspec", None), "params", {})
    group = (request.function.__name__, params.get("order"))
    if C.cached(("group",), lambda: [None])[0] != group:
        C.drop_cached(keep=("cloud",))
        C.cached(("group",), lambda: [None])[0] = group
    yield


@pytest.fixture(scope="module", autouse=True)
def _release_everything_at_the_end():
    yield
    C.drop_cached()


# ------------------------------------------------------------------ three dimensions, the other instances
S2_SWITCHES = [{"BBFMM_M2L_S2_AXES": "1"}, {"BBFMM_M2L_S2_AXES": "2"}, {"BBFMM_M2L_S2_PAIRS": "0"}, {"BBFMM_M2L_S1_PAIRS": "0"}]
# (8, {AXES: 1}): the instance (8, 8) of one axis, which only a forced axis selects at these orders.  One order after the other:
# the handles of an order share its restatement.
ORDER_CASES = sorted([(p, {}) for p in (6, 8, 9, 10)] + [(p, e) for p in (6, 9) for e in S2_SWITCHES] +
                     [(8, {"BBFMM_M2L_S2_AXES": "1"})], key=lambda c: c[0])


@pytest.mark.parametrize("order,env", ORDER_CASES, ids=lambda v: ids(v) if isinstance(v, dict) else str(v))
def test_m2l_and_l2l_at_the_orders_of_the_other_stage2_instances(order, env):
    t, geo = P.tree("lattice8", order, env)
    pts = P.cloud("lattice8")
    if "BBFMM_M2L_S1_PAIRS" in env:
        assert not t.debug_m2l_pairs()[0]
    SEEN[order, ids(env)] = C.assert_s2_plan(t, 3, order, env)
    w = C.sparse_lattice_weights(pts, 8, 61, C.EVERY_VECTOR_COLUMNS)
    assert C.assert_every_vector_is_live(geo, w) == 3
    _, n_zero = P.check_downward(t, geo, ("lattice8", order), pts, w, f"lattice8 order {order} sparse {env}")
    assert n_zero > 0


def test_the_3d_cases_run_every_instance_of_their_orders():
    """The union over the cases above.  A case that did not run in this process (deselected, another worker) is asked for
    its instance here, from a handle of its own, so the answer does not depend on which tests ran before."""
    for order, env in ORDER_CASES:
        if (order, ids(env)) not in SEEN:
            SEEN[order, ids(env)] = C.assert_s2_plan(P.tree("lattice8", order, env)[0], 3, order, env)
    assert C.GPU_INSTANCES <= set(SEEN.values()), C.GPU_INSTANCES - set(SEEN.values())


# ------------------------------------------------------------------ two dimensions
def lattice2d_weights(geo, n, kind):
    return C.dense_weights(n, 1, 63) if kind == "dense" else C.one_leaf_weights(geo, n, C.lattice2d_leaves(geo), 65)


@pytest.mark.parametrize("kind", ["dense", "one-leaf"])
@pytest.mark.parametrize("order,env", sorted([(p, {}) for p in (3, 6, 7, 10, 16)] +
                                              [(p, e) for p in (6, 10) for e in P.SWITCHES[1:]], key=lambda c: c[0]),
                         ids=lambda v: ids(v) if isinstance(v, dict) else str(v))
def test_m2l_and_l2l_on_the_2d_lattice(order, env, kind):
    t, geo = P.tree("lattice2d", order, env)
    pts = P.cloud("lattice2d")
    if "BBFMM_M2L_S1_PAIRS" in env:
        assert not t.debug_m2l_pairs()[0]
    if "BBFMM_M2L_S1_AXES" in env:
        assert t.debug_m2l_pairs_axes()[0]["axes"] == int(env["BBFMM_M2L_S1_AXES"])
    C.assert_s2_plan(t, 2, order, env)
    w = lattice2d_weights(geo, len(pts), kind)
    assert C.assert_every_vector_is_live(geo, w) == 4
    _, n_zero = P.check_downward(t, geo, ("lattice2d", order), pts, w, f"lattice2d order {order} {kind} {env}")
    if kind == "one-leaf":
        assert n_zero > 0


def test_m2l_and_l2l_on_the_2d_lattice_five_right_hand_sides_in_three_passes():
    """The intermediate of the two stages holds two and a half right-hand sides: one batch, m2l_rhs_chunk_ = 2, so the five go
    in passes of 2, 2 and 1 -- Lp cleared per pass, the later passes written at their offset k0 C n_pad into L."""
    pts = P.cloud("lattice2d")
    slots = C.make_tree(pts, 6, C.LATTICE_LIMIT, host_only=True).stats().m2l_slots_bytes_per_rhs
    env = {"BBFMM_M2L_CBUF_MB": "%.6f" % (2.5 * slots / 1048576.0)}
    t, geo = P.tree("lattice2d", 6, env)
    C.assert_s2_plan(t, 2, 6, env)
    w = C.dense_weights(len(pts), 5, 67)
    C.assert_every_vector_is_live(geo, w)
    P.check_downward(t, geo, ("lattice2d", 6), pts, w, "lattice2d order 6 K 5, passes of 2")
    st = t.stats()
    assert st.m2l_batches == 1 and st.m2l_slots_bytes_per_rhs == slots
    assert 2 * slots <= st.m2l_intermediate_bytes < 3 * slots        # room for two of the five (and the batch's padding)


@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("kid", [0, 2])
def test_p2l_in_two_dimensions_cells_with_an_x_list(kid, K):
    kernel = (kid, 1.0, 1.0)
    t, geo = P.tree("clustered2d", 5, kernel=kernel)
    pts = P.cloud("clustered2d")
    assert t.stats().n_w > 0 and geo.d == 2
    C.assert_s2_plan(t, 2, 5)
    w = C.dense_weights(len(pts), K, 69)
    M, L = P.device_passes(t, w)
    cells = np.nonzero((np.diff(geo.lists["X"][0]) > 0) & (geo.level >= 2))[0]
    assert len(cells) > 0
    P.check_downward(t, geo, ("clustered2d", 5, kernel), pts, w, f"P2L 2-D kernel {kid} K {K}", kernel, cells=cells, M=M, L=L)


# ------------------------------------------------------------------ one dimension
@pytest.mark.parametrize("kind,K", [("dense", 1), ("dense", 3), ("one-leaf", 3)])
@pytest.mark.parametrize("order", [4, 16])
def test_m2l_l2l_and_p2l_on_the_line(order, kind, K):
    """Every cell from level 2 down, those with an X list among them; no pairs: m2l_gemm_k4 in the node basis."""
    t, geo = P.tree("line", order)
    pts = P.cloud("line")
    C.assert_s2_plan(t, 1, order)
    w = C.dense_weights(len(pts), K, 71) if kind == "dense" else C.one_leaf_weights(geo, len(pts), C.line_leaves(geo), 73)
    assert w.shape[1] == K and C.assert_every_vector_is_live(geo, w) == 4
    assert ((np.diff(geo.lists["X"][0]) > 0) & (geo.level >= 2)).any()
    _, n_zero = P.check_downward(t, geo, ("line", order), pts, w, f"line order {order} {kind} K {K}")
    if kind == "one-leaf":
        assert n_zero > 0


# ------------------------------------------------------------------ uncompressed operators
@pytest.mark.parametrize("name,order,kind", [("lattice8", 4, "dense"), ("lattice8", 4, "sparse"), ("lattice8", 5, "dense"),
                                             ("lattice8", 5, "sparse"), ("populations", 3, "dense")])
def test_m2l_and_l2l_with_uncompressed_operators(name, order, kind):
    t, geo = P.tree(name, order, compression=C.NO_COMPRESSION)
    pts = P.cloud(name)
    assert t.m2l_factors(2, 0)[1] is None and (t.m2l_ranks()[2:] == geo.n).all()
    C.assert_s2_plan(t, 3, order, {"BBFMM_M2L_S2_PAIRS": "0"})       # nothing pairs without compression
    w = C.dense_weights(len(pts), 1, 75) if kind == "dense" else C.sparse_lattice_weights(pts, 8, 77, C.EVERY_VECTOR_COLUMNS)
    C.assert_every_vector_is_live(geo, w)
    _, n_zero = P.check_downward(t, geo, (name, order, "uncompressed"), pts, w, f"{name} order {order} {kind} uncompressed")
    if kind == "sparse":
        assert n_zero > 0
