"""Stage 2 of M2L in the parity basis of the x reflection: the pair structure of the target lists
against the definition, the identity the pairing rests on, and the host walk of the new tables against the walk with the
switch off and against the oracle.  No GPU."""
import itertools

import numpy as np
import pytest

import ferreus_rbf_rs_amd as F
from conftest import clustered_points, inject_product_operators, relerr
from oracle import bbfmm_oracle as O
from test_m2l_pairs_host import check_operator, oracle_m2l, reflect


def host_tree(pts, order, params, s2, monkeypatch, kernel=(0, 1.0, 1.0), s1=None, **env):
    """Both switches and the table options are read when a handle is created."""
    monkeypatch.setenv("BBFMM_M2L_S2_PAIRS", "1" if s2 else "0")
    if s1 is not None:
        monkeypatch.setenv("BBFMM_M2L_S1_PAIRS", "1" if s1 else "0")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    t = F.FmmTree(pts, order, F.KernelParams(F.KernelType(kernel[0]), base_range=kernel[1], total_sill=kernel[2]), True, True,
                  params=F.FmmParams(*params), host_only=True)
    for k in list(env) + ["BBFMM_M2L_S2_PAIRS"] + (["BBFMM_M2L_S1_PAIRS"] if s1 is not None else []):
        monkeypatch.delenv(k)
    return t


def admissible_targets(octant, d):
    """Far transfer vectors that end in a target of octant class `octant`: B = V + t, both children of neighbouring parents."""
    out = set()
    for t in itertools.product(range(-3, 4), repeat=d):
        if max(abs(c) for c in t) < 2:
            continue
        if all(((octant >> a) & 1) - 3 <= t[a] <= ((octant >> a) & 1) + 2 for a in range(d)):
            out.add(t)
    return out


@pytest.mark.parametrize("d,order", [(2, 4), (2, 5), (3, 4), (3, 5)])
def test_pair_structure_of_the_target_lists(d, order, monkeypatch):
    rng = np.random.default_rng(70 + d)
    pts = rng.random((3000 if d == 3 else 2000, d))
    t = host_tree(pts, order, (30, 2, 1e-5, 1024), True, monkeypatch)
    on, ops = t.debug_m2l_pairs(stage=2)
    assert on and ops
    for op in ops:
        vecs = check_operator(op, d)  # pairs + singles, nothing missing from the list and nothing twice
        assert op["kind"] == 0 and vecs == admissible_targets(op["octant"], d)
        # a target of x bit o0 has t0 in [o0 - 3, o0 + 2]: the pairs +-1, +-2 and two values without a partner
        assert {p[0] for p in op["pairs"]} == {1, 2}
        assert {s[0] for s in op["singles"]} == {0, 6 * (op["octant"] & 1) - 3}
    assert {op["octant"] for op in ops} == set(range(1 << d))
    # the stage-1 accessor keeps reporting the source lists
    assert t.debug_m2l_pairs()[0]
    # the switch: every vector a single, in the plain layout
    t0 = host_tree(pts, order, (30, 2, 1e-5, 1024), False, monkeypatch)
    off, ops0 = t0.debug_m2l_pairs(stage=2)
    assert not off and all(not op["pairs"] for op in ops0)
    for op in ops0:
        assert set(op["singles"]) == admissible_targets(op["octant"], d)


@pytest.mark.parametrize("d,order", [(2, 4), (2, 5), (3, 4), (3, 5)])
def test_u_identity_of_every_candidate_pair(d, order, monkeypatch):
    """UAll_Rt[kk][i] = UAll_t[kk][rho i] with UAll_t[kk][i] = U_ref(t)[kk][invperm_t[i]]: t and Rt share the reference
    operator and invperm_Rt[i] = invperm_t[rho i], rho the reflection of the slowest node digit.  This pins the RULE, on the
    oracle's symmetry tables, for every pair the product formed; it does not read the product's own tables.  Those are
    guarded by the same check at setup in build_m2l_tables (a pair that fails stays two singles, which the pair-structure
    test above would report as a missing pair) and, end to end, by the walk tests below."""
    rng = np.random.default_rng(80 + d)
    pts = rng.random((1500, d))
    t = host_tree(pts, order, (30, 2, 1e-5, 1024), True, monkeypatch)
    r = O.FmmTree(pts, order, 0, True, True, None, O.FmmParams(30, 2, 1e-5, 1024))
    inject_product_operators(t, r)
    n = order ** d
    p1 = n // order
    i = np.arange(n)
    rho = i + (order - 1 - 2 * (i // p1)) * p1
    invperm = np.asarray(r.ops.invperm).reshape(-1, n)
    perm_lookup, ref_lookup = np.asarray(r.ops.perm_lookup), np.asarray(r.ops.ref_lookup)
    vec_index = {tuple(int(c) for c in v): k for k, v in enumerate(np.asarray(r.ops.all_vecs).reshape(-1, d))}
    on, ops = t.debug_m2l_pairs(stage=2)
    candidates = {tv for op in ops for tv in op["pairs"]}
    assert on and candidates
    for tv in candidates:
        a, b = vec_index[tv], vec_index[reflect(tv)]
        assert ref_lookup[a] == ref_lookup[b]
        assert (invperm[perm_lookup[b]] == invperm[perm_lookup[a]][rho]).all()


@pytest.mark.parametrize("name", ["uniform3d", "clustered3d", "planar2d", "low_ranks"])
def test_host_walk_with_and_without_stage2_pairs(name, monkeypatch):
    """The clouds of test_m2l_pairs_host.py.  Switch off: the walk reproduces oracle_m2l at 1e-12 as before.  On against
    off: two summation orders of the same products plus one rounding per combined operator entry and combined slot entry,
    a few n eps of max|L|; the bound is 1e-12, as for stage 1."""
    rng = np.random.default_rng(45)
    kernel = (100, 0.5, 0.4) if name == "low_ranks" else (0, 1.0, 1.0)
    pts, order, params = {"uniform3d": (rng.random((5000, 3)), 5, (40, 2, 1e-6, 1024)),
                          "clustered3d": (clustered_points(rng, 3000, 3), 4, (30, 2, 1e-5, 1024)),
                          "planar2d": (rng.random((3000, 2)), 6, (30, 2, 1e-6, 1024)),
                          "low_ranks": (np.unique(clustered_points(rng, 6000, 3), axis=0), 5, (40, 2, 1e-5, 1024))}[name]
    t_off = host_tree(pts, order, params, False, monkeypatch, kernel)
    t_on = host_tree(pts, order, params, True, monkeypatch, kernel)
    assert t_on.debug_m2l_pairs(stage=2)[0] and not t_off.debug_m2l_pairs(stage=2)[0]
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


@pytest.mark.parametrize("s1,s2", [(False, False), (False, True), (True, False), (True, True)])
def test_host_walk_of_the_four_switch_combinations_with_several_batches(s1, s2, monkeypatch):
    """A budget that cuts the levels into groups and several batches: the zero segments of absent members lie on the new
    offsets, and the buffer is not cleared between batches."""
    rng = np.random.default_rng(46)
    pts, order, params = rng.random((6000, 3)), 4, (30, 2, 1e-5, 1024)
    t = host_tree(pts, order, params, s2, monkeypatch, s1=s1, BBFMM_M2L_CBUF_MB="0.25")
    assert t.debug_m2l_pairs()[0] == s1 and t.debug_m2l_pairs(stage=2)[0] == s2
    r = O.FmmTree(pts, order, 0, True, True, None, O.FmmParams(*params))
    inject_product_operators(t, r)
    r.set_weights(rng.random((pts.shape[0], 1)))
    M = r.M[0].copy()
    e = relerr(t.debug_apply_m2l_tables_host(M), oracle_m2l(r))
    print(f"S1 {s1} S2 {s2}: walk vs oracle {e:.2e}")
    assert e < 1e-12
