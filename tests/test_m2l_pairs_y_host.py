"""Stage 1 of M2L in the parity basis of two axes: the vectors the x pairing leaves alone pair by
their y reflection.  The pair tables and the column-block kinds against the definition, the host walk of the three
layouts (two axes, one axis, pairs off) against each other and the oracle, the rule behind the unset switch, and
BBFMM_M2L_S1_AXES=1 against the one-axis tables.  No GPU."""
import numpy as np
import pytest

import ferreus_rbf_rs_amd as F
from conftest import clustered_points, inject_product_operators, relerr
from oracle import bbfmm_oracle as O
from test_m2l_pairs_host import admissible, lattice_cloud, oracle_m2l, reflect


def host_tree(pts, order, params, monkeypatch, axes="2", pairs=True, kernel=(0, 1.0, 1.0), **env):
    """axes: "2", "1" or None (the switch unset).  The switches and the table options are read when a handle is created."""
    monkeypatch.setenv("BBFMM_M2L_S1_PAIRS", "1" if pairs else "0")
    if axes is None:
        monkeypatch.delenv("BBFMM_M2L_S1_AXES", raising=False)
    else:
        monkeypatch.setenv("BBFMM_M2L_S1_AXES", axes)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    t = F.FmmTree(pts, order, F.KernelParams(F.KernelType(kernel[0]), base_range=kernel[1], total_sill=kernel[2]), True, True,
                  params=F.FmmParams(*params), host_only=True)
    for k in env:
        monkeypatch.delenv(k)
    monkeypatch.delenv("BBFMM_M2L_S1_AXES", raising=False)
    return t


def reflect_y(t):
    return (t[0], -t[1]) + tuple(t[2:])


def check_operator(op):
    """x pairs = {t, R_x t both in the list, t0 != 0}; y pairs = {t, R_y t both in the list, neither in an x pair, t1 != 0};
    singles = the rest; nothing missing, nothing twice; no column block holds columns of both kinds of pairs, and yb0 is
    where the blocks in y order begin.  Returns the operator's list as a set."""
    xp, yp, sg = op["x_pairs"], op["y_pairs"], op["singles"]
    flat = list(xp) + [reflect(t) for t in xp] + list(yp) + [reflect_y(t) for t in yp] + list(sg)
    vecs = set(flat)
    assert len(flat) == len(vecs), "a transfer vector appears twice"
    want_x = {t for t in vecs if t[0] > 0 and reflect(t) in vecs}
    in_x = want_x | {reflect(t) for t in want_x}
    want_y = {t for t in vecs - in_x if t[1] > 0 and reflect_y(t) in vecs - in_x}
    assert set(xp) == want_x
    assert set(yp) == want_y
    assert set(sg) == vecs - in_x - want_y - {reflect_y(t) for t in want_y}
    kinds, yb0 = op["block_kinds"], op["yb0"]
    assert kinds == [1 if b >= yb0 else 0 for b in range(len(kinds))]
    for first, last in xp.values():
        assert first < 0 or all(kinds[b] == 0 for b in range(first, last + 1)), "an x pair in a block of y order"
    for first, last in yp.values():
        assert first < 0 or all(kinds[b] == 1 for b in range(first, last + 1)), "a y pair in a block of x order"
    y_blocks = [first for first, _ in yp.values() if first >= 0]
    assert yb0 == (min(y_blocks) if y_blocks else len(kinds))
    assert 0 <= op["pad_cols"] < 160 and (op["pad_cols"] == 0 or (xp and yp))
    return vecs


@pytest.mark.parametrize("d,order", [(2, 4), (2, 5), (3, 4), (3, 5)])
def test_pair_structure_of_the_class_lists(d, order, monkeypatch):
    rng = np.random.default_rng(40 + d)
    pts = rng.random((3000 if d == 3 else 2000, d))
    t = host_tree(pts, order, (30, 2, 1e-5, 1024), monkeypatch)
    info, ops = t.debug_m2l_pairs_axes()
    assert info["axes"] == 2 and ops
    for op in ops:
        vecs = check_operator(op)
        if op["kind"] == 0:  # a class operator stacks the whole admissible list
            assert vecs == admissible(op["octant"], d)
            assert (len(op["x_pairs"]), len(op["y_pairs"]), len(op["singles"])) == ((63, 21, 21) if d == 3 else (9, 3, 3))
            assert all(p[0] == 0 or p[0] == 3 - 6 * (op["octant"] & 1) for p in op["y_pairs"])  # x singles only
    assert {op["octant"] for op in ops if op["kind"] == 0} == set(range(1 << d))
    # the stage-1 entry of the one-axis tables keeps its meaning: the x pairs, every other vector a single
    on, ops1 = t.debug_m2l_pairs()
    assert on and len(ops1) == len(ops)
    for op, op1 in zip(ops, ops1):
        assert set(op1["pairs"]) == set(op["x_pairs"])
        assert set(op1["singles"]) == set(op["singles"]) | set(op["y_pairs"]) | {reflect_y(p) for p in op["y_pairs"]}


def test_pair_structure_of_boundary_variants_and_group_operators(monkeypatch):
    rng = np.random.default_rng(43)
    pts = lattice_cloud(rng, 32, 3, 2)  # the faces of the 32^3 level hold runs of 256 cells of a class
    t = host_tree(pts, 3, (6, 2, 1e-3, 1024), monkeypatch, BBFMM_M2L_VARIANTS="1")
    info, ops = t.debug_m2l_pairs_axes()
    variants = [op for op in ops if op["kind"] == 1]
    assert info["axes"] == 2 and len(variants) >= 6 * 8 and len(variants) == t.debug_m2l_variants()[0]
    lost_partner = 0
    for op in variants:
        vecs = check_operator(op)
        adm = admissible(op["octant"], 3)
        assert vecs < adm  # a boundary variant leaves transfer vectors out
        # y faces: R_y s is admissible for the class but its target is gone, and s has no x partner here either
        lost_partner += sum(1 for s in op["singles"] if s[1] != 0 and reflect_y(s) in adm and reflect_y(s) not in vecs)
    assert lost_partner > 0
    # a level cut into groups of target classes: per (group, source class) one operator over part of the list
    pts = np.random.default_rng(44).random((6000, 3))
    t = host_tree(pts, 4, (30, 2, 1e-5, 1024), monkeypatch, BBFMM_M2L_CBUF_MB="0.25")
    info, ops = t.debug_m2l_pairs_axes()
    groups = [op for op in ops if op["kind"] == 1]
    assert info["axes"] == 2 and groups and any(op["y_pairs"] for op in groups)
    union, n_pairs = {}, {}
    for op in groups:
        vecs = check_operator(op)
        seen = union.setdefault((op["level"], op["octant"]), set())
        n_pairs[(op["level"], op["octant"])] = n_pairs.get((op["level"], op["octant"]), np.zeros(2, int)) + [len(op["x_pairs"]), len(op["y_pairs"])]
        assert not (seen & vecs)  # the groups of a class share no transfer vector
        seen |= vecs
        assert all(reflect_y(p) in vecs for p in op["y_pairs"])  # t and R_y t end in the same target class, hence group
    for (level, octant), vecs in union.items():
        assert vecs == admissible(octant, 3)
        assert list(n_pairs[(level, octant)]) == [63, 21]  # the cut into groups separates no pair


WALK_CASES = {
    "uniform3d": lambda rng: (rng.random((5000, 3)), 5, (40, 2, 1e-6, 1024)),
    "clustered3d": lambda rng: (clustered_points(rng, 3000, 3), 4, (30, 2, 1e-5, 1024)),
    "planar2d": lambda rng: (rng.random((3000, 2)), 6, (30, 2, 1e-6, 1024)),
    "low_ranks": lambda rng: (np.unique(clustered_points(rng, 6000, 3), axis=0), 5, (40, 2, 1e-5, 1024)),
    # 8^3 lattice cells of two points, leaf limit 6: levels 2 and 3 with interior, face, edge and corner cells
    "lattice_order7": lambda rng: (lattice_cloud(rng, 8, 3, 2), 7, (6, 2, 1e-6, 1024)),  # odd: centre planes on both axes
    "lattice_order4": lambda rng: (lattice_cloud(rng, 8, 3, 2), 4, (6, 2, 1e-6, 1024)),  # even: none
}


@pytest.mark.parametrize("name", list(WALK_CASES))
def test_host_walk_of_the_three_layouts(name, monkeypatch):
    """Two axes against one axis and against pairs off: the same n <= 343 products in another summation order, with two
    more roundings per term than the one-axis basis has (the second level of the combined operator entry and of the
    combined multipole) -- a few n eps ~ 1e-13 of max|L|; the bound is the one-axis test's 1e-12, also against the oracle."""
    rng = np.random.default_rng(45)
    kernel = (100, 0.5, 0.4) if name == "low_ranks" else (0, 1.0, 1.0)
    pts, order, params = WALK_CASES[name](rng)
    t_off = host_tree(pts, order, params, monkeypatch, axes=None, pairs=False, kernel=kernel)
    t_x = host_tree(pts, order, params, monkeypatch, axes="1", kernel=kernel)
    t_xy = host_tree(pts, order, params, monkeypatch, axes="2", kernel=kernel)
    assert [t.debug_m2l_pairs_axes()[0]["axes"] for t in (t_off, t_x, t_xy)] == [0, 1, 2]
    assert any(op["y_pairs"] for op in t_xy.debug_m2l_pairs_axes()[1])
    r = O.FmmTree(pts, order, kernel[0], True, True, None, O.FmmParams(*params), base_range=kernel[1], total_sill=kernel[2])
    inject_product_operators(t_off, r)
    r.set_weights(rng.random((pts.shape[0], 1)))
    M = r.M[0].copy()
    L_ref = oracle_m2l(r)
    L_off, L_x, L_xy = (t.debug_apply_m2l_tables_host(M) for t in (t_off, t_x, t_xy))
    e = {"off vs oracle": relerr(L_off, L_ref), "x vs oracle": relerr(L_x, L_ref), "xy vs oracle": relerr(L_xy, L_ref),
         "xy vs x": relerr(L_xy, L_x), "xy vs off": relerr(L_xy, L_off)}
    print(name, ", ".join(f"{k} {v:.2e}" for k, v in e.items()))
    for k, v in e.items():
        assert v < 1e-12, k


@pytest.mark.parametrize("d,order", [(3, 3), (3, 4), (3, 5), (2, 6)])
def test_the_unset_switch_takes_the_cheaper_layout(d, order, monkeypatch):
    rng = np.random.default_rng(46)
    pts = rng.random((2000, d))
    t = host_tree(pts, order, (30, 2, 1e-5, 1024), monkeypatch, axes=None)
    info = t.debug_m2l_pairs_axes()[0]
    assert info["work_x"] > 0 and info["work_xy"] > 0
    assert info["axes"] == (2 if info["work_xy"] < info["work_x"] else 1)
    if order == 3:  # four parts of 16 against 32 + 16: 64 contraction indices against 48, more than the pairs save
        assert info["work_xy"] > info["work_x"] and info["axes"] == 1
    # both forced settings report the same two figures
    for axes in ("1", "2"):
        forced = host_tree(pts, order, (30, 2, 1e-5, 1024), monkeypatch, axes=axes).debug_m2l_pairs_axes()[0]
        assert forced == {"axes": int(axes), "work_x": info["work_x"], "work_xy": info["work_xy"]}


def test_one_axis_setting_reproduces_the_one_axis_tables(monkeypatch):
    """At order 3 the unset switch keeps one axis (the test above), which is the layout from before the switch existed:
    BBFMM_M2L_S1_AXES=1 gives the same tables and, bit for bit, the same walk; so does a cloud with boundary variants."""
    rng = np.random.default_rng(47)
    for pts, params, env in [(rng.random((3000, 3)), (30, 2, 1e-5, 1024), {}),
                             (lattice_cloud(rng, 16, 3, 2), (6, 2, 1e-3, 1024), {"BBFMM_M2L_VARIANTS": "1"})]:
        t_unset = host_tree(pts, 3, params, monkeypatch, axes=None, **env)
        t_one = host_tree(pts, 3, params, monkeypatch, axes="1", **env)
        assert t_unset.debug_m2l_pairs_axes()[0]["axes"] == 1
        assert t_unset.debug_m2l_pairs() == t_one.debug_m2l_pairs()
        assert t_unset.debug_m2l_pairs_axes() == t_one.debug_m2l_pairs_axes()
        M = rng.standard_normal((t_one.stats().n_cells, t_one.stats().n_nodes))
        assert np.array_equal(t_unset.debug_apply_m2l_tables_host(M), t_one.debug_apply_m2l_tables_host(M))
