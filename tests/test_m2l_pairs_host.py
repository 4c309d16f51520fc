"""Stage 1 of M2L in the parity basis of the x reflection: the pair tables against the
definition, and the host walk of the new tables against the walk of the unpaired ones and the oracle.  No GPU."""
import itertools

import numpy as np
import pytest

import ferreus_rbf_rs_amd as F
from conftest import clustered_points, inject_product_operators, relerr
from oracle import bbfmm_oracle as O


def host_tree(pts, order, params, pairs, monkeypatch, kernel=(0, 1.0, 1.0), **env):
    """The switch and the table options are read when a handle is created."""
    monkeypatch.setenv("BBFMM_M2L_S1_PAIRS", "1" if pairs else "0")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    t = F.FmmTree(pts, order, F.KernelParams(F.KernelType(kernel[0]), base_range=kernel[1], total_sill=kernel[2]), True, True,
                  params=F.FmmParams(*params), host_only=True)
    for k in env:
        monkeypatch.delenv(k)
    return t


def admissible(octant, d):
    """Far transfer vectors of a source of octant class `octant`: B = V + t with both children of neighbouring parents."""
    out = set()
    for t in itertools.product(range(-3, 4), repeat=d):
        if max(abs(c) for c in t) < 2:
            continue
        if all(-2 - ((octant >> a) & 1) <= t[a] <= 3 - ((octant >> a) & 1) for a in range(d)):
            out.add(t)
    return out


def reflect(t):
    return (-t[0],) + tuple(t[1:])


def check_operator(op, d):
    """Pairs = {t, Rt both in the operator's list, t0 != 0}, listed by the member with t0 > 0; singles = the rest;
    no vector missing from the operator's list and none twice.  Returns the list as a set."""
    pairs, singles = op["pairs"], op["singles"]
    flat = list(pairs) + [reflect(t) for t in pairs] + list(singles)
    vecs = set(flat)
    assert len(flat) == len(vecs), "a transfer vector appears twice"
    want_pairs = {t for t in vecs if t[0] > 0 and reflect(t) in vecs}
    assert set(pairs) == want_pairs
    assert set(singles) == vecs - want_pairs - {reflect(t) for t in want_pairs}
    return vecs


@pytest.mark.parametrize("d,order", [(2, 4), (2, 5), (3, 4), (3, 5)])
def test_pair_structure_of_the_class_lists(d, order, monkeypatch):
    rng = np.random.default_rng(40 + d)
    pts = rng.random((3000 if d == 3 else 2000, d))
    t = host_tree(pts, order, (30, 2, 1e-5, 1024), True, monkeypatch)
    on, ops = t.debug_m2l_pairs()
    assert on and ops
    for op in ops:
        vecs = check_operator(op, d)
        if op["kind"] == 0:  # a class operator stacks the whole admissible list
            assert vecs == admissible(op["octant"], d)
            # a source of x bit o0 has t0 in [-2 - o0, 3 - o0]: the pairs +-1, +-2 and two values without a partner
            assert {p[0] for p in op["pairs"]} == {1, 2}
            assert {s[0] for s in op["singles"]} == {0, 3 - 6 * (op["octant"] & 1)}
    assert {op["octant"] for op in ops if op["kind"] == 0} == set(range(1 << d))
    # the switch: every vector a single, in today's layout
    t0 = host_tree(pts, order, (30, 2, 1e-5, 1024), False, monkeypatch)
    off, ops0 = t0.debug_m2l_pairs()
    assert not off and all(not op["pairs"] for op in ops0)
    for op in ops0:
        if op["kind"] == 0:
            assert set(op["singles"]) == admissible(op["octant"], d)


def lattice_cloud(rng, m, d, per_cell):
    g = np.stack(np.meshgrid(*[np.arange(m)] * d, indexing="ij"), -1).reshape(-1, d)[:, None, :]
    return ((g + 0.15 + 0.7 * rng.random((m ** d, per_cell, d))).reshape(-1, d)) / m


def test_pair_structure_of_boundary_variants_and_group_operators(monkeypatch):
    rng = np.random.default_rng(43)
    pts = lattice_cloud(rng, 32, 3, 2)  # the faces of the 32^3 level hold runs of 256 cells of a class
    t = host_tree(pts, 3, (6, 2, 1e-3, 1024), True, monkeypatch, BBFMM_M2L_VARIANTS="1")
    on, ops = t.debug_m2l_pairs()
    variants = [op for op in ops if op["kind"] == 1]
    assert on and len(variants) >= 6 * 8 and len(variants) == t.debug_m2l_variants()[0]
    lost_partner = 0
    for op in variants:
        vecs = check_operator(op, 3)
        assert vecs < admissible(op["octant"], 3)  # a boundary variant leaves transfer vectors out
        lost_partner += sum(1 for s in op["singles"] if s[0] != 0 and reflect(s) in admissible(op["octant"], 3))
    assert lost_partner > 0  # x faces: one of a pair is gone, the other stays as a single
    # a level cut into groups of target classes: per (group, source class) one operator over part of the list
    pts = np.random.default_rng(44).random((6000, 3))
    t = host_tree(pts, 4, (30, 2, 1e-5, 1024), True, monkeypatch, BBFMM_M2L_CBUF_MB="0.25")
    on, ops = t.debug_m2l_pairs()
    groups = [op for op in ops if op["kind"] == 1]
    assert on and groups
    union = {}
    for op in groups:
        vecs = check_operator(op, 3)
        seen = union.setdefault((op["level"], op["octant"]), set())
        assert not (seen & vecs)  # the groups of a class share no transfer vector
        seen |= vecs
        assert all(reflect(p) in vecs for p in op["pairs"])  # t and Rt end in the same target class, hence group
    for (level, octant), vecs in union.items():
        assert vecs == admissible(octant, 3)


def oracle_m2l(r, compressed=1):
    r.L = np.zeros_like(r.M)
    lib = O.lib()
    for level in range(2, r.depth + 1):
        cells = np.ascontiguousarray(r.level_cells[level])
        buf, u_off, vt_off, rank = r.opbuf[level]
        lib.oracle_m2l(O.I32(r.ops.n), O.I64(r.C), O.I32(1), O._p(cells), O.I64(len(cells)), O._p(r.v_ptr),
                       O._p(r.v_idx), O._p(r.v_tidx), O.I32(len(rank)), O._p(u_off), O._p(vt_off), O._p(rank),
                       O._p(buf), O.I32(compressed), O._p(r.ops.perm), O._p(r.ops.invperm),
                       O._p(r.ops.perm_lookup), O._p(r.ops.ref_lookup), O._p(r.M), O._p(r.L))
    return r.L[0]


@pytest.mark.parametrize("name", ["uniform3d", "clustered3d", "planar2d", "low_ranks"])
def test_host_walk_with_and_without_pairs(name, monkeypatch):
    """Switch off: the walk reproduces oracle_m2l at 1e-12 as before.  On against off: two summation orders of the same
    n <= 343 products plus two roundings per term (the combined operator entry, the combined multipole) -- a few
    n eps ~ 1e-13 of max|L|; the bound is 1e-12.  low_ranks: a short-range Gaussian whose fine levels have rank 2, so
    that a column block of pairs would span more list positions than the kernel's slot table holds and the tables
    start blocks early."""
    rng = np.random.default_rng(45)
    kernel = (100, 0.5, 0.4) if name == "low_ranks" else (0, 1.0, 1.0)
    pts, order, params = {"uniform3d": (rng.random((5000, 3)), 5, (40, 2, 1e-6, 1024)),
                          "clustered3d": (clustered_points(rng, 3000, 3), 4, (30, 2, 1e-5, 1024)),
                          "planar2d": (rng.random((3000, 2)), 6, (30, 2, 1e-6, 1024)),
                          "low_ranks": (np.unique(clustered_points(rng, 6000, 3), axis=0), 5, (40, 2, 1e-5, 1024))}[name]
    t_off = host_tree(pts, order, params, False, monkeypatch, kernel)
    t_on = host_tree(pts, order, params, True, monkeypatch, kernel)
    assert t_on.debug_m2l_pairs()[0] and not t_off.debug_m2l_pairs()[0]
    if name == "low_ranks":
        assert t_on.m2l_ranks()[t_on.stats().depth].max() <= 2
    r = O.FmmTree(pts, order, kernel[0], True, True, None, O.FmmParams(*params), base_range=kernel[1], total_sill=kernel[2])
    inject_product_operators(t_off, r)
    r.set_weights(rng.random((pts.shape[0], 1)))
    M = r.M[0].copy()
    L_ref = oracle_m2l(r)
    L_off = t_off.debug_apply_m2l_tables_host(M)
    L_on = t_on.debug_apply_m2l_tables_host(M)
    e_off, e_on, e_pair = relerr(L_off, L_ref), relerr(L_on, L_ref), relerr(L_on, L_off)
    print(f"{name}: off vs oracle {e_off:.2e}, on vs oracle {e_on:.2e}, on vs off {e_pair:.2e}")
    assert e_off < 1e-12
    assert e_pair < 1e-12
    assert e_on < 1e-12
