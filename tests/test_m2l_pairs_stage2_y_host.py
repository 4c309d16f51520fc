"""Stage 2 of M2L in the parity basis of two axes: the target-side vectors the x pairing leaves alone
pair by their y reflection.  The pair structure and the slot layout [A | B | S] of the target lists against the definition,
the identity the pairing rests on, BBFMM_M2L_S2_AXES=1 against the one-axis layout, and the host walk of the new tables
against the one-axis walk, the walk with the pairs off and the oracle.  No GPU.

Clouds and bounds are those of test_m2l_pairs_stage2_host.py: the uniform, the clustered, the planar and the low-rank cloud
of its walk test and 6000 uniform points cut into several batches by BBFMM_M2L_CBUF_MB=0.25, plus the 8^3 lattice of
test_m2l_pairs_y_host.py (interior, face, edge and corner cells; order 7 has centre planes on both axes, order 4 none) and
the 32^3 lattice of test_m2l_pairs_host.py for the boundary variants.
Every walk is held to 1e-12 of max|L| against every other and against the oracle: the layouts differ by exact factors (1,
1/2, 1/4) and by the order of at most n <= 343 sums per entry, a few n eps."""
import numpy as np
import pytest

import ferreus_rbf_rs_amd as F
from conftest import clustered_points, inject_product_operators, relerr
from oracle import bbfmm_oracle as O
from test_m2l_pairs_host import lattice_cloud, oracle_m2l, reflect
from test_m2l_pairs_stage2_host import admissible_targets
from test_m2l_pairs_y_host import reflect_y


def host_tree(pts, order, params, monkeypatch, axes="2", s2=True, kernel=(0, 1.0, 1.0), **env):
    """axes: "2", "1" or None (the switch unset).  The switches and the table options are read when a handle is created."""
    env = dict(env, BBFMM_M2L_S2_PAIRS="1" if s2 else "0")
    if axes is not None:
        env["BBFMM_M2L_S2_AXES"] = axes
    monkeypatch.delenv("BBFMM_M2L_S2_AXES", raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    t = F.FmmTree(pts, order, F.KernelParams(F.KernelType(kernel[0]), base_range=kernel[1], total_sill=kernel[2]), True, True,
                  params=F.FmmParams(*params), host_only=True)
    for k in env:
        monkeypatch.delenv(k)
    return t


def check_class(op, d):
    """x pairs = {t, R_x t both in the list, t0 > 0}; y pairs = {t, R_y t both in the list, neither in an x pair, t1 > 0};
    singles = the rest.  Slot: the x leaders from 0 without gaps, the y leaders from kpy without gaps, all inside A = [0, kp);
    every partner kp behind its leader; the singles from 2 kp without gaps; k_pad the end rounded up to 16."""
    xp, yp, sg = op["x_pairs"], op["y_pairs"], op["singles"]
    flat = list(xp) + [reflect(t) for t in xp] + list(yp) + [reflect_y(t) for t in yp] + list(sg)
    vecs = set(flat)
    assert len(flat) == len(vecs), "a transfer vector appears twice"
    assert vecs == admissible_targets(op["octant"], d)
    want_x = {t for t in vecs if t[0] > 0 and reflect(t) in vecs}
    in_x = want_x | {reflect(t) for t in want_x}
    want_y = {t for t in vecs - in_x if t[1] > 0 and reflect_y(t) in vecs - in_x}
    assert set(xp) == want_x and set(yp) == want_y
    assert set(sg) == vecs - in_x - want_y - {reflect_y(t) for t in want_y}
    kp, kpy, k_pad = op["kp"], op["kpy"], op["k_pad"]
    assert kp % 16 == 0 and kpy % 16 == 0 and k_pad % 16 == 0 and 0 <= kpy <= kp

    def packed(entries, start):
        """the segments (rank rounded up to 2) follow each other from `start`; returns the end"""
        pos = start
        for off, _, rank in sorted(entries.values()):
            assert off == pos
            pos += rank + (rank & 1)
        return pos

    end_x = packed(xp, 0)
    for off, off2, _ in list(xp.values()) + list(yp.values()):
        assert off2 == kp + off  # partners at equal offsets in A and B
    if yp:
        assert kpy == -(-end_x // 16) * 16 and op["pad"] == kpy - end_x
        assert kp == -(-packed(yp, kpy) // 16) * 16
    else:
        assert kpy == kp == -(-end_x // 16) * 16 and op["pad"] == 0
    assert all(off2 == -1 for _, off2, _ in sg.values())
    assert k_pad == max(16, -(-packed(sg, 2 * kp) // 16) * 16)
    return vecs


@pytest.mark.parametrize("d,order", [(2, 3), (2, 4), (2, 5), (2, 7), (3, 3), (3, 4), (3, 5), (3, 7)])
def test_pair_structure_and_slot_layout_of_the_target_lists(d, order, monkeypatch):
    rng = np.random.default_rng(70 + d)
    pts = rng.random((2000, d))
    params = (30, 2, 1e-4, 1024)
    t = host_tree(pts, order, params, monkeypatch)
    info, ops = t.debug_m2l_pairs_axes(stage=2)
    assert info["axes"] == 2 and ops
    for op in ops:
        check_class(op, d)
        assert (len(op["x_pairs"]), len(op["y_pairs"]), len(op["singles"])) == ((63, 21, 21) if d == 3 else (9, 3, 3))
        assert all(p[0] == 0 or p[0] == 6 * (op["octant"] & 1) - 3 for p in op["y_pairs"])  # x singles only
    assert {op["octant"] for op in ops} == set(range(1 << d))
    # the one-axis accessor keeps its meaning: the x pairs, every other vector a single
    on, ops1 = t.debug_m2l_pairs(stage=2)
    assert on and len(ops1) == len(ops)
    for op, op1 in zip(ops, ops1):
        assert set(op1["pairs"]) == set(op["x_pairs"])
        assert set(op1["singles"]) == set(op["singles"]) | set(op["y_pairs"]) | {reflect_y(p) for p in op["y_pairs"]}
    # BBFMM_M2L_S2_AXES=1: the one-axis layout -- no y pairs, no y boundary inside A, no padding, the same x pairs
    t1 = host_tree(pts, order, params, monkeypatch, axes="1")
    info1, ops_x = t1.debug_m2l_pairs_axes(stage=2)
    assert info1 == dict(info, axes=1)  # both handles report the same two work figures
    on_x, ops1_x = t1.debug_m2l_pairs(stage=2)  # (the same pairs and singles; the lists order their singles differently)
    assert on_x and [(o["level"], o["octant"], o["pairs"], set(o["singles"])) for o in ops1_x] == \
        [(o["level"], o["octant"], o["pairs"], set(o["singles"])) for o in ops1]
    for op, opx in zip(ops, ops_x):
        assert not opx["y_pairs"] and opx["kpy"] == opx["kp"] and opx["pad"] == 0
        assert opx["x_pairs"].keys() == op["x_pairs"].keys()
        end = 0
        for off, off2, rank in sorted(opx["x_pairs"].values()):
            assert off == end and off2 == opx["kp"] + off
            end += rank + (rank & 1)
        assert opx["kp"] == -(-end // 16) * 16
        for off, _, rank in sorted(opx["singles"].values()):
            assert off == max(end, 2 * opx["kp"])
            end = off + rank + (rank & 1)
        assert opx["k_pad"] == max(16, -(-end // 16) * 16)
    # pairs off: neither kind
    info0, ops0 = host_tree(pts, order, params, monkeypatch, axes="2", s2=False).debug_m2l_pairs_axes(stage=2)
    assert info0["axes"] == 0 and all(not op["x_pairs"] and not op["y_pairs"] and op["kp"] == 0 for op in ops0)


@pytest.mark.parametrize("d,order", [(3, 3), (3, 4), (3, 5), (3, 7), (2, 5), (2, 7)])
def test_the_unset_switch_takes_two_axes_only_where_strictly_cheaper(d, order, monkeypatch):
    pts = np.random.default_rng(46).random((2000, d))
    info = host_tree(pts, order, (30, 2, 1e-4, 1024), monkeypatch, axes=None).debug_m2l_pairs_axes(stage=2)[0]
    assert info["work_x"] > 0 and info["work_xy"] > 0
    assert info["axes"] == (2 if info["work_xy"] < info["work_x"] else 1)
    if (d, order) == (2, 5):  # four parts of one column group each against 1 + 1: twice the columns, more than the pairs save
        assert info["work_xy"] > info["work_x"] and info["axes"] == 1
    if (d, order) == (3, 7):  # 13 + 10 column groups either way, and the y pairs save steps
        assert info["axes"] == 2


@pytest.mark.parametrize("d,order", [(2, 4), (2, 5), (3, 4), (3, 5), (3, 7)])
def test_u_identity_of_every_y_pair(d, order, monkeypatch):
    """UAll_{R_y t}[kk][i] = UAll_t[kk][rho_y i] with UAll_t[kk][i] = U_ref(t)[kk][invperm_t[i]]: t and R_y t share the
    reference operator and invperm_{R_y t}[i] = invperm_t[rho_y i], rho_y the reflection of the second node digit -- so the
    two gathers read the same entries of U_ref, shown here bit for bit on a random U_ref.  As in
    test_m2l_pairs_stage2_host.py this pins the RULE on the oracle's symmetry tables for every pair the product formed; the
    product's own check at setup leaves a failing candidate as two singles, which the structure test would report."""
    rng = np.random.default_rng(80 + d)
    pts = rng.random((1500, d))
    t = host_tree(pts, order, (30, 2, 1e-4, 1024), monkeypatch)
    r = O.FmmTree(pts, order, 0, True, True, None, O.FmmParams(30, 2, 1e-4, 1024))
    n = order ** d
    p2 = n // (order * order)
    i = np.arange(n)
    rho_y = i + (order - 1 - 2 * ((i // p2) % order)) * p2
    invperm = np.asarray(r.ops.invperm).reshape(-1, n)
    perm_lookup, ref_lookup = np.asarray(r.ops.perm_lookup), np.asarray(r.ops.ref_lookup)
    vec_index = {tuple(int(c) for c in v): k for k, v in enumerate(np.asarray(r.ops.all_vecs).reshape(-1, d))}
    candidates = {tv for op in t.debug_m2l_pairs_axes(stage=2)[1] for tv in op["y_pairs"]}
    assert candidates
    u_ref = rng.standard_normal((5, n))
    for tv in candidates:
        a, b = vec_index[tv], vec_index[reflect_y(tv)]
        assert ref_lookup[a] == ref_lookup[b]
        assert (invperm[perm_lookup[b]] == invperm[perm_lookup[a]][rho_y]).all()
        assert np.array_equal(u_ref[:, invperm[perm_lookup[b]]], u_ref[:, invperm[perm_lookup[a]]][:, rho_y])


WALK_CASES = {
    "uniform3d": lambda rng: (rng.random((5000, 3)), 5, (40, 2, 1e-6, 1024)),
    "clustered3d": lambda rng: (clustered_points(rng, 3000, 3), 4, (30, 2, 1e-5, 1024)),
    "planar2d": lambda rng: (rng.random((3000, 2)), 6, (30, 2, 1e-6, 1024)),
    "low_ranks": lambda rng: (np.unique(clustered_points(rng, 6000, 3), axis=0), 5, (40, 2, 1e-5, 1024)),
    "lattice_order7": lambda rng: (lattice_cloud(rng, 8, 3, 2), 7, (6, 2, 1e-6, 1024)),
    "lattice_order4": lambda rng: (lattice_cloud(rng, 8, 3, 2), 4, (6, 2, 1e-6, 1024)),
}


@pytest.mark.parametrize("name", list(WALK_CASES))
def test_host_walk_of_the_three_layouts(name, monkeypatch):
    rng = np.random.default_rng(45)
    kernel = (100, 0.5, 0.4) if name == "low_ranks" else (0, 1.0, 1.0)
    pts, order, params = WALK_CASES[name](rng)
    t_off = host_tree(pts, order, params, monkeypatch, axes=None, s2=False, kernel=kernel)
    t_x = host_tree(pts, order, params, monkeypatch, axes="1", kernel=kernel)
    t_xy = host_tree(pts, order, params, monkeypatch, axes="2", kernel=kernel)
    assert [t.debug_m2l_pairs_axes(stage=2)[0]["axes"] for t in (t_off, t_x, t_xy)] == [0, 1, 2]
    assert all(op["y_pairs"] for op in t_xy.debug_m2l_pairs_axes(stage=2)[1])
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


@pytest.mark.parametrize("s1_axes", ["1", "2"])
def test_host_walk_with_several_batches_and_group_operators(s1_axes, monkeypatch):
    """A budget that cuts the levels into groups and several batches: the zero segments of absent members (of either kind of
    pair) lie on the new offsets and the buffer is not cleared between batches; the rows of stage 1's group operators
    follow the new slot offsets, with stage 1 on one axis and on two."""
    rng = np.random.default_rng(46)
    pts, order, params = rng.random((6000, 3)), 4, (30, 2, 1e-5, 1024)
    env = {"BBFMM_M2L_CBUF_MB": "0.25", "BBFMM_M2L_S1_AXES": s1_axes}
    t = host_tree(pts, order, params, monkeypatch, axes="2", **env)
    t_x = host_tree(pts, order, params, monkeypatch, axes="1", **env)
    assert t.debug_m2l_pairs_axes(stage=2)[0]["axes"] == 2 and t.debug_m2l_pairs_axes()[0]["axes"] == int(s1_axes)
    assert any(op["kind"] == 1 for op in t.debug_m2l_pairs()[1])  # group operators
    r = O.FmmTree(pts, order, 0, True, True, None, O.FmmParams(*params))
    inject_product_operators(t, r)
    r.set_weights(rng.random((pts.shape[0], 1)))
    M = r.M[0].copy()
    L_ref, L_xy, L_x = oracle_m2l(r), t.debug_apply_m2l_tables_host(M), t_x.debug_apply_m2l_tables_host(M)
    e, e_x = relerr(L_xy, L_ref), relerr(L_xy, L_x)
    print(f"S1 axes {s1_axes}: walk vs oracle {e:.2e}, vs the one-axis walk {e_x:.2e}")
    assert e < 1e-12 and e_x < 1e-12


@pytest.mark.parametrize("s1_axes", ["1", "2"])
def test_host_walk_with_boundary_variants(s1_axes, monkeypatch):
    """The 32^3 lattice of test_m2l_pairs_host.py, whose faces hold runs of 256 cells of a class: stage 1's boundary variants
    store to the new slot offsets.  The oracle's tree of 65,536 points takes a minute of Python, so the two-axis walk is
    held to the one-axis walk and to the walk with stage 2's pairs off on random multipoles (the walk with the pairs off is
    pinned to the oracle on boundary variants by test_m2l_pairs_host.py)."""
    rng = np.random.default_rng(47)
    pts, params = lattice_cloud(rng, 32, 3, 2), (6, 2, 1e-3, 1024)
    env = {"BBFMM_M2L_VARIANTS": "1", "BBFMM_M2L_S1_AXES": s1_axes}
    t = host_tree(pts, 3, params, monkeypatch, axes="2", **env)
    t_x = host_tree(pts, 3, params, monkeypatch, axes="1", **env)
    t_off = host_tree(pts, 3, params, monkeypatch, axes=None, s2=False, **env)
    assert t.debug_m2l_pairs_axes(stage=2)[0]["axes"] == 2 and t.debug_m2l_variants()[0] >= 6 * 8
    M = rng.standard_normal((t.stats().n_cells, t.stats().n_nodes))
    L_xy, L_x, L_off = (h.debug_apply_m2l_tables_host(M) for h in (t, t_x, t_off))
    e_x, e_off = relerr(L_xy, L_x), relerr(L_xy, L_off)
    print(f"S1 axes {s1_axes}: two axes vs one axis {e_x:.2e}, vs pairs off {e_off:.2e}")
    assert e_x < 1e-12 and e_off < 1e-12
