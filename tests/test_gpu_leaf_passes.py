"""P2M and L2P with the factor table q (S_j = sum_k T_k(x) q[j][k], no division) and L2P over runs of leaves
(BBFMM_LEAF_PASSES), pinned to the long-double restatements and bounds of tests/far_field_reference.py: P2M leaf by leaf,
L2P target by target, every switchable path with the switch unset and with BBFMM_LEAF_PASSES=0.

The cloud (leaf limit 130, depth 4) puts next to each other in sorted order what the run kernel has to tell apart: the eight
children of one level-1 cell hold 0, 1, 63, 64, 65, 130, 7 and 20 points (65 and 130 are more than one 64-lane batch and
stay on the one-leaf kernel, so the runs around them end in the middle of a workgroup), one level-2 cell is split into
level-3 leaves and one of those into level-4 leaves (different lengths and centres within one batch), and a level-3 family
holds three leaves of one point and an empty one.  A few points lie on a face of their leaf (x = -1, +1) and on its nodes."""
import numpy as np
import pytest

import far_field_cases as C
import far_field_reference as R
from far_field_reference import LD

pytestmark = pytest.mark.gpu

cached = C.cached

LIMIT = 130
ORDERS = (2, 4, 7, 10, 11, 13)
ROOT_LO, ROOT_SIDE = 0.5 - 0.501, 2 * 0.501        # the tree of [0, 1]^3: centre 0.5, radius 0.501 (far_field_cases.py)
SPECIAL_CELL = (1, 1, 2)                            # the level-2 leaf of the points on faces and nodes
# (a handle takes the runs only when there are enough of them to fill the device, BBFMM_L2P_RUNS_MIN: these clouds have a few)
ENVS = [{"BBFMM_L2P_RUNS_MIN": "0"}, {"BBFMM_LEAF_PASSES": "0"}]
env_id = lambda e: ",".join(f"{k[6:]}={v}" for k, v in e.items()) or "default"   # noqa: E731


@pytest.fixture(autouse=True)
def _one_group_of_cases_at_a_time(request):
    """As in test_gpu_far_field_passes.py: the cases of one function at one order share handles and references."""
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


# ------------------------------------------------------------------ the cloud
def _spec():
    """Populations of the level-2 cells by level-1 octant and child (bit a of an index <-> axis a); a list is a split cell."""
    rng = np.random.default_rng(20261020)
    spec = [[int(rng.integers(1, 65)) for _ in range(8)] for _ in range(8)]
    spec[0][0], spec[7][7] = 40, 38                                   # the corners (0, 0, 0) and (3, 3, 3): plain leaves
    spec[1] = [0, 1, 63, 64, 65, 130, 7, 20]
    spec[2][3] = [30, 2, 40, 17, [20, 15, 25, 10, 30, 5, 18, 17], 9, 33, 12]
    spec[5][0] = [1, 1, 1, 0, 50, 60, 10, 14]
    return spec


def _total(s):
    return s if isinstance(s, int) else sum(_total(c) for c in s)


def _fill(lo, side, spec, rng, out, pops, level):
    if isinstance(spec, int):
        out.append(C.on_grid(lo + side * (0.06 + 0.88 * rng.random((spec, 3)))))
        pops.append((level, spec))
        return
    assert _total(spec) > LIMIT                                       # the cell splits
    for c, s in enumerate(spec):
        _fill(lo + np.array([c & 1, (c >> 1) & 1, (c >> 2) & 1]) * (side / 2), side / 2, s, rng, out, pops, level + 1)


def special_points():
    """Points of the leaf SPECIAL_CELL: eight spacings inside its low and its high x face (x = -1 and +1 to 4e-15), on the
    faces as the doubles give them (whichever cell owns them, |x| = 1), and on a node of every order along every axis."""
    side = ROOT_SIDE / 4
    lo = ROOT_LO + np.array(SPECIAL_CELL) * side
    centre, half = lo + side / 2, side / 2
    inside = centre + half * np.array([0.0, 0.31, -0.47])
    pts = []
    for x in (lo[0] + 8 * np.spacing(lo[0]), lo[0] + side - 8 * np.spacing(lo[0] + side), lo[0], lo[0] + side):
        pts.append([x, inside[1] + 0.01 * len(pts), inside[2]])
    for p in ORDERS:
        nd = R.nodes(p).astype(np.float64)
        pts.append(list(centre + half * nd[[0, p // 2, p - 1]]))
    return np.array(pts)


def leaf_cloud():
    """(points, populations [(level, count)] of the prescribed leaves, rows of the special points)."""
    rng = np.random.default_rng(20261021)
    out, pops = [], []
    _fill(np.full(3, ROOT_LO), ROOT_SIDE, _spec(), rng, out, pops, 0)
    pts = np.concatenate(out)
    sp = special_points()
    pts = np.concatenate([pts, sp])
    assert pts.min() > 0 and pts.max() < 1 and len(np.unique(pts, axis=0)) == len(pts)
    return np.ascontiguousarray(pts), pops, np.arange(len(pts) - len(sp), len(pts))


def cloud(name):
    return cached(("cloud", name), {"leaves": lambda: leaf_cloud()[0], "2d": lambda: C.random_cloud(2, 16 ** 3, 21),
                                    "1d": lambda: C.random_cloud(1, 64, 22)}[name])


LIMITS = {"leaves": LIMIT, "2d": 70, "1d": 9}


def assert_leaf_cloud(t, geo):
    """The leaves are the prescribed ones: depth 4, leaves at levels 2, 3 and 4, and the populations the runs are about."""
    assert t.stats().depth == 4
    pops = np.diff(geo.src_ptr)
    leaves = geo.is_leaf & (pops > 0)
    assert {2, 3, 4} == set(geo.level[leaves].tolist())
    want = sorted(n for _, n in leaf_cloud()[1] if n > 0)
    got = sorted(pops[leaves].tolist())
    assert len(got) == len(want) and sum(got) == sum(want) + len(leaf_cloud()[2])
    assert {1, 63, 64, 65, 130} <= set(got), got                      # (the special points raise two or three other leaves)
    assert (np.sort(pops[leaves & (geo.level == 4)]) == np.sort([20, 15, 25, 10, 30, 5, 18, 17])).all()


def assert_runs(t, geo, name, order, env):
    """The switch bites: with BBFMM_LEAF_PASSES unset and no minimum, a handle whose order has the run kernel (at most 512 nodes)
    holds runs, on the leaf cloud also jobs outside them (65 and 130 points); at 0, and with the minimum of a whole device, none."""
    r = t.debug_leaf_runs()
    assert r["jobs"] == int((geo.is_leaf & (np.diff(geo.src_ptr) > 0)).sum())
    if env.get("BBFMM_LEAF_PASSES") == "0":
        assert r["mask"] == 0 and r["runs"] == 0 and r["rest"] == 0
        return
    assert r["mask"] == 1
    if env.get("BBFMM_L2P_RUNS_MIN") == "0" and order ** geo.d <= 512:
        assert r["runs"] > 0 and 2 * r["runs"] <= r["jobs"] - r["rest"] <= 8 * r["runs"]
        if name == "leaves":
            assert r["rest"] >= 2                                   # the leaves of 65 and of 130 points at the least
    else:
        assert r["runs"] == 0 and r["rest"] == 0


def tree(name, order, env=None):
    def make():
        t = C.make_tree(cloud(name), order, LIMITS[name], env=env)
        geo = R.Geometry(t)
        if name == "leaves":
            assert_leaf_cloud(t, geo)
        assert_runs(t, geo, name, order, env or {})
        return t, geo
    return cached(("tree", name, order, tuple(sorted((env or {}).items()))), make)


# ------------------------------------------------------------------ P2M (no switch: the table q serves every kernel)
# 4, 7, 10: the matrix pipe; 2, 11, 13: the vector kernel
P2M_CASES = ([("leaves", p, K) for p in ORDERS for K in (1, 2, 3)] +
             [("2d", p, K) for p in (4, 11) for K in (1, 3)] + [("1d", p, K) for p in (2, 13) for K in (1, 2)])


@pytest.mark.parametrize("name,order,K", P2M_CASES)
def test_p2m_leaf_by_leaf(name, order, K):
    t, geo = tree(name, order)
    pts = cloud(name)
    w = C.dense_weights(len(pts), K, 71 + K)
    res = R.p2m(geo, pts, w)
    t.set_weights(w)
    M = t.debug_get_coefficients("M", K)
    ref = {c: v[0] for c, v in res.items()}
    bound = {c: R.p2m_bound(geo, v[1], v[2], v[3]) for c, v in res.items()}
    R.check_cells("P2M", M, ref, bound, sorted(ref), f"{name} order {order} K {K}")
    assert (M[:, geo.is_leaf & (np.diff(geo.src_ptr) == 0)] == 0).all()


@pytest.mark.parametrize("order", ORDERS)
def test_p2m_of_one_point_is_the_product_of_its_factor_rows(order):
    """One right-hand side per special point, weight 1 there and 0 elsewhere: M of its leaf is the tensor product of the three
    factor rows of that point, which checks the table q against long double within e_S(p) roundings per factor."""
    t, geo = tree("leaves", order)
    pts, rows = cloud("leaves"), leaf_cloud()[2]
    leaf_of = np.empty(len(pts), dtype=np.int64)
    for c in np.nonzero(np.diff(geo.src_ptr) > 0)[0]:
        leaf_of[geo.src_idx[geo.src_ptr[c]:geo.src_ptr[c + 1]]] = c
    w = np.zeros((len(pts), len(rows)))
    w[rows, np.arange(len(rows))] = 1.0
    t.set_weights(w)
    M = t.debug_get_coefficients("M", len(rows))
    x = np.array([geo.points_x(leaf_of[r], pts[r:r + 1])[0].astype(np.float64) for r in rows])
    assert abs(x[0, 0] + 1) < 1e-14 and abs(x[1, 0] - 1) < 1e-14 and (np.abs(np.abs(x[2:4, 0]) - 1) < 1e-14).all()
    nd = R.nodes(order).astype(np.float64)
    at = 4 + ORDERS.index(order)
    assert np.abs(x[at] - nd[[0, order // 2, order - 1]]).max() < 1e-13      # on a node of this order along every axis
    worst = 0.0
    for k, r in enumerate(rows):
        c = int(leaf_of[r])
        F = geo.factors(c, pts[r:r + 1])
        ref = (F[0][0][:, None, None] * F[1][0][None, :, None] * F[2][0][None, None, :]).reshape(-1)
        A = [np.abs(f[0]) for f in F]
        s_fac = (A[1][None, :, None] * A[2][None, None, :] + A[0][:, None, None] * A[2][None, None, :]
                 + A[0][:, None, None] * A[1][None, :, None]).reshape(-1)
        bound = LD(R.U) * (4 * np.abs(ref) + R.e_S(order) * s_fac).max()   # R.p2m_bound for a leaf of one point
        err = np.abs(M[k, c].astype(LD) - ref).max()
        worst = max(worst, float(err / bound))
        assert err <= bound, (order, k, c, float(err), float(bound))
        others = np.ones(geo.C, dtype=bool)
        others[c] = False
        assert (M[k, others & geo.is_leaf] == 0).all()
    print(f"P2M of one point, order {order}: largest error / bound {worst:.3g} over {len(rows)} points")


# ------------------------------------------------------------------ L2P
def l2p_only_leaves(geo, w, M):
    """Leaves whose U and W lists hold only zero weights: the far field of their targets is L2P of their L and nothing else."""
    up, ui = geo.lists["U"]
    wp, wi = geo.lists["W"]
    weight = np.zeros(geo.C, dtype=bool)
    for c in np.nonzero(np.diff(geo.src_ptr) > 0)[0]:
        weight[c] = np.any(w[geo.src_idx[geo.src_ptr[c]:geo.src_ptr[c + 1]]] != 0)
    live_M = (M != 0).any(axis=(0, 2))
    return [c for c in np.nonzero(geo.is_leaf)[0]
            if not weight[ui[up[c]:up[c + 1]]].any() and not live_M[wi[wp[c]:wp[c + 1]]].any()]


def corner_leaves(geo):
    holds = np.nonzero(geo.is_leaf & (np.diff(geo.src_ptr) > 0))[0]
    lo = holds[np.argmin(geo.centres[holds].sum(axis=1))]
    hi = holds[np.argmax(geo.centres[holds].sum(axis=1))]
    return int(lo), int(hi)


def check_l2p(t, geo, name, order, K, targets, run, grads, what):
    """run(w) -> (y (m, K), g (m, K, d) or None) at `targets` for weights on one corner leaf at a time; every leaf with
    targets must be an L2P-only leaf in one of the two runs and is checked there against R.l2p, target by target."""
    pts = cloud(name)
    leaf_of = t.points_to_leaves(targets)
    done, worst, worst_g = set(), 0.0, 0.0
    for corner in corner_leaves(geo):
        w = C.leaf_weights(geo, len(pts), corner, K, 83)
        y, g = run(w)
        M, L = t.debug_get_coefficients("M", K), t.debug_get_coefficients("L", K)
        for c in l2p_only_leaves(geo, w, M):
            rows = np.nonzero(leaf_of == c)[0]
            if c in done or len(rows) == 0:
                continue
            done.add(c)
            out = R.l2p(geo, L, c, targets[rows], with_grads=grads)
            err = np.abs(y[rows].astype(LD) - out[0])
            assert (err <= out[1]).all(), ("L2P", what, "leaf", c, len(rows), float((err / out[1]).max()))
            with np.errstate(all="ignore"):
                worst = max(worst, float(np.where(err > 0, err / out[1], 0).max()))
            if grads:
                err = np.abs(g[rows].astype(LD) - out[2])
                assert (err <= out[3]).all(), ("L2P gradient", what, "leaf", c, float((err / out[3]).max()))
                with np.errstate(all="ignore"):
                    worst_g = max(worst_g, float(np.where(err > 0, err / out[3], 0).max()))
    print(f"L2P {what}: largest error / bound {worst:.3g}, gradients {worst_g:.3g}, {len(done)} leaves")
    assert set(np.unique(leaf_of).tolist()) <= done
    assert np.abs(L).max() > 0


L2P_CASES = [("leaves", p, K) for p in ORDERS for K in (1, 3)] + [("leaves", 7, 2), ("2d", 7, 2), ("2d", 16, 1), ("1d", 4, 3)]


@pytest.mark.parametrize("env", ENVS, ids=env_id)
@pytest.mark.parametrize("name,order,K", L2P_CASES)
def test_l2p_through_the_device_matvec(name, order, K, env):
    """matvec_device at the resident target set: the runs (3-D orders up to 8, every 2-D and 1-D order) and the one-leaf
    kernel for the rest, both writing the caller's order through perm."""
    import torch
    t, geo = tree(name, order, env)
    pts = cloud(name)

    def run(w):
        dw = torch.from_numpy(np.ascontiguousarray(w.T)).cuda()
        out = torch.zeros_like(dw)
        t.matvec_device(dw.data_ptr(), len(pts), K, out.data_ptr(), len(pts), True)
        return out.cpu().numpy().T, None
    check_l2p(t, geo, name, order, K, pts, run, False, f"matvec {name} order {order} K {K} {env_id(env)}")


@pytest.mark.parametrize("env", ENVS, ids=env_id)
@pytest.mark.parametrize("name,order,K", [("leaves", 4, 2), ("leaves", 7, 1), ("2d", 7, 2)])
def test_l2p_with_gradients(name, order, K, env):
    t, geo = tree(name, order, env)
    pts = cloud(name)

    def run(w):
        t.set_weights(w)
        y, g = t.evaluate_with_gradients(w, pts)
        return y, g.reshape(len(pts), K, geo.d)
    check_l2p(t, geo, name, order, K, pts, run, True, f"gradients {name} order {order} K {K} {env_id(env)}")


@pytest.mark.parametrize("env", ENVS, ids=env_id)
@pytest.mark.parametrize("name,order,K", [("leaves", 7, 2), ("leaves", 4, 1)])
def test_l2p_through_evaluate(name, order, K, env):
    """evaluate at the sources (the resident target set) and at a general target set: a shuffled part of the sources and
    other points, whose jobs are cut on the device and take the one-leaf kernel under every setting."""
    t, geo = tree(name, order, env)
    pts = cloud(name)
    rng = np.random.default_rng(91)
    mid = []                                  # other points: midpoints of two sources of one leaf (the tree stores no empty cell)
    for c in np.nonzero(np.diff(geo.src_ptr) > 1)[0]:
        idx = geo.src_idx[geo.src_ptr[c]:geo.src_ptr[c + 1]]
        mid.append(C.on_grid((pts[idx[:-1:3]] + pts[idx[1::3][:len(idx[:-1:3])]]) / 2))
    other = np.concatenate([pts[rng.permutation(len(pts))[:len(pts) // 3]]] + mid)
    other = np.ascontiguousarray(other[rng.permutation(len(other))])
    for targets, tag, path in ((pts, "sources", 1), (other, "general", None)):
        def run(w):
            t.set_weights(w)
            y = t.evaluate(w, targets)
            assert path is None or t.last_evaluate_path() == path
            return y, None
        check_l2p(t, geo, name, order, K, targets, run, False, f"evaluate {tag} {name} order {order} K {K} {env_id(env)}")
