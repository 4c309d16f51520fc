"""Every instance of the pair kernels against EXACT sums.

Trees with no far field: one level, the root split once, every leaf in every other leaf's U list (stats: n_v = n_w = 0).
`evaluate`, `evaluate_with_gradients`, `fast_matrix_vector_product` and `matvec_device` are then pure direct sums, and the
long-double dense sum of tests/kernel_reference.py is the answer itself, not an approximation at FMM accuracy.

Per row i and right-hand side, with u = 2^-53 (tests/kernel_pointwise.py holds the derivation of (a_k, b_k)):

    tau_i = u [ (a_k + 4 + n_src) sum_j |w_j| |phi_ij|  +  (b_k + 4) sum_j |w_j| |r2_ij phi'_ij| ]

4: the differences, their squares and the sum that form r2; n_src: the product with the weight and the worst case of a
recursive sum of n_src terms in any order.  The gradient components take the same form with |f_ij| |dx_a|.  Derived, not
measured; with n_src <= 2000 it sits more than twenty times under the 1e-11 of the oracle comparisons, and it is per row: a
mis-indexed pair, weight slot or right-hand side is wrong at O(1 / n_src).

Leaf populations are prescribed per octant (the points of an octant are drawn inside it; max_points_per_cell is the largest
population, so the root splits and no child does).  Between them the layouts show every row count 1..66 -- every NR of
sym3_pass, every register group of the wave kernel -- and 127-129, 255-257, 383-385, 511-513, 767-769, 1023-1025, 1537: the
source-tile edges of DIRECT_TILE (512), SYM_TILE (768) and SYM_TILE / 2 (384) and the pass boundaries of plan_targets.
Coordinates lie on a 2^-30 grid (differences are exact); weights are signed; pairs are planted along x at separations 0,
2^-53, 2^-52 (the value rule |r| < eps from both sides) and 2^-27, 2^-26, 2^-25 (the gradient rule r2 <= eps from both
sides): their r2 is an exact power of two on the device and in the reference whatever the compiler contracts.

What the parametrisation ids show (launch_p2p, launch_p2p_sym, launch_wx_sym, launch_m2p, launch_p2l):

    test_values_at_arbitrary_targets      p2p_kernel<ID, false, KB>   every id x K 1 (KB1), 2 / 4 (KB4), 5 / 8 (KB8), 9 (KB8 + KB1)
    test_gradients_at_arbitrary_targets   p2p_kernel<ID, true, KB>    every id x K 1 (KB1), 3 (KB4), 5 (KB4 + KB1)
    test_matvec_targets_are_the_sources   wave jobs: p2p_sym2_kernel<ID, 1 | 2 | 4>; size rule and leaves over 64 rows:
                                          p2p_sym3_kernel<ID, 8> (K = 1), p2p_sym_kernel<ID, 2 | 4> (K = 2, 3, 4, 7)
    (ids 0, 1, 3, 8 also in one and two dimensions)
    test_wx_gradients_off_the_sources     m2p_kernel<ID, true, 1 | 4>, p2p_kernel<ID, true, 1 | 4>, p2l_kernel<ID, 1 | 4>
    test_wx_values_off_the_sources        m2p_kernel<ID, false, 4 | 1>, p2l_kernel<ID, 4 | 1>
    test_wx_fused_matvec                  wx_sym3_kernel<ID, 8> (K = 1), wx_sym_kernel<ID, 4> (K = 3), both job kinds
    test_wx_separate_kernels_in_a_child_process   m2p_kernel / p2l_kernel inside the matvec (BBFMM_WX_FUSED=0), ids 1, 4, 7, 100
"""
import functools

import numpy as np
import pytest

import ferreus_rbf_rs_amd as F
import kernel_pointwise as KP
import kernel_reference as KR
from kernel_reference import LD, U

pytestmark = pytest.mark.gpu

BR, SILL = 0.5, 0.4                 # both Spheroidal branches occur inside the unit cube
NAMES = {int(k): k.name for k in F.KernelType}
ALL_IDS = KR.KERNEL_IDS
LOW_D_IDS = (0, 1, 3, 8)
GRID = 2.0 ** 30
SEPARATIONS = (0.0, 2.0 ** -53, 2.0 ** -52, 2.0 ** -27, 2.0 ** -26, 2.0 ** -25)
K_MAX, K_GRAD_MAX = 9, 5
VALUE_K = {1: "KB1", 2: "KB4", 4: "KB4", 5: "KB8", 8: "KB8", 9: "KB8+KB1"}        # launch_p2p: passes of 8 / 4 / 1
GRAD_K = {1: "KB1", 3: "KB4", 5: "KB4+KB1"}                                       # launch_p2p with gradients: 4 / 1
MATVEC_K = {1: "KB1", 2: "KB2", 3: "KB4", 4: "KB4", 7: "KB4+KB4"}                 # launch_p2p_sym: passes of at most 4

# ------------------------------------------------------------------ leaf populations
SMALL = [[c if c <= 66 else c - 33 for c in range(i + 1, i + 65, 9)] for i in range(9)]     # 1..66, eight per layout
BIG = [[1537, 127, 128, 129], [1023, 255, 256, 257], [1024, 383, 384], [1025, 385, 511], [767, 768, 2, 65], [769, 512, 513]]
LAYOUTS = {3: {**{f"small{i}": c for i, c in enumerate(SMALL)}, **{f"big{i}": c for i, c in enumerate(BIG)}},
           2: {"mixed": [66, 257, 7, 385]},
           1: {"mixed": [130, 513]}}
REQUIRED_ROWS = set(range(1, 67)) | {127, 128, 129, 255, 256, 257, 383, 384, 385, 511, 512, 513, 767, 768, 769, 1023, 1024,
                                      1025, 1537}


def layouts_of(kid, d):
    """Two 3-D layouts per kernel (one of small leaves, one of big ones), rotating so that every layout is used."""
    if d < 3:
        return ["mixed"]
    i = ALL_IDS.index(kid)
    return [f"small{i % 9}", f"big{i % 6}"]


def _used_layouts():
    used = {(3, l) for kid in ALL_IDS for l in layouts_of(kid, 3)}
    used |= {(d, "mixed") for d in (1, 2)}
    return used


def test_the_layouts_show_every_required_row_count():
    rows = set()
    for d, name in _used_layouts():
        rows |= set(LAYOUTS[d][name])
        assert sum(LAYOUTS[d][name]) <= 2000
    assert REQUIRED_ROWS <= rows, sorted(REQUIRED_ROWS - rows)
    assert {(3, n) for n in LAYOUTS[3]} <= _used_layouts()


@functools.lru_cache(maxsize=None)
def cloud(d, name):
    """(sources, targets, rows of the sources among the targets): deterministic per layout."""
    counts = LAYOUTS[d][name]
    rng = np.random.default_rng([d, sum(counts), len(name), counts[0]])
    octants = rng.permutation(2 ** d)[:len(counts)]
    order = np.argsort(counts)[::-1]                         # the planted pairs go round the leaves, largest first
    planted = {int(o): [] for o in range(len(counts))}
    k = 0
    while k < len(SEPARATIONS):
        for o in order:
            if k < len(SEPARATIONS) and counts[o] - 2 * len(planted[int(o)]) >= 2:
                planted[int(o)].append(SEPARATIONS[k])
                k += 1
    pts = []
    for o, (c, oc) in enumerate(zip(counts, octants)):
        lo = np.array([(int(oc) >> a) & 1 for a in range(d)]) * 0.5
        p = lo + np.floor(rng.random((c, d)) * (GRID / 2 - 2) + 1) / GRID         # strictly inside the octant, on the grid
        for j, sep in enumerate(planted[o]):
            x0 = lo[0] + 0.25 + np.floor(rng.random() * 0.2 * GRID) / GRID        # in [1/4, 1/2) or [3/4, 1): spacing <= 2^-53
            p[2 * j], p[2 * j + 1] = p[2 * j], p[2 * j].copy()
            p[2 * j, 0], p[2 * j + 1, 0] = x0, x0 + sep
            assert p[2 * j + 1, 0] - p[2 * j, 0] == sep
        pts.append(p)
    src = np.vstack(pts)
    src = src[rng.permutation(src.shape[0])]
    n = src.shape[0]
    # targets: the sources and, shuffled among them, copies displaced by 2^-12 .. 2^-10 per axis (grid multiples)
    extra = max(16, min(n // 4, 64))
    rows = rng.choice(n, extra, replace=n < extra)
    off = np.floor(rng.uniform(2.0 ** -12, 2.0 ** -10, (extra, d)) * GRID) / GRID * rng.choice([-1.0, 1.0], (extra, d))
    ext = np.clip(src[rows] + off, 1.0 / GRID, 1.0 - 1.0 / GRID)
    tgt = np.vstack([src, ext])
    perm = rng.permutation(tgt.shape[0])
    tgt = tgt[perm]
    src_rows = np.argsort(perm)[:n]                          # tgt[src_rows] == src
    assert np.array_equal(tgt[src_rows], src)
    for a in (src, tgt):
        a.setflags(write=False)
    return src, tgt, src_rows


@functools.lru_cache(maxsize=None)
def weights(d, name):
    n = cloud(d, name)[0].shape[0]
    w = np.random.default_rng(n).standard_normal((n, K_MAX))
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def exact(kid, d, name):
    """The long-double sums at the target superset, all right-hand sides: computed once per (kernel, layout)."""
    src, tgt, _ = cloud(d, name)
    return KR.PairSums(kid, BR, SILL, tgt, src, weights(d, name), K_GRAD_MAX)


_TREES = {}


def tree(kid, d, name, jobs, monkeypatch):
    """One handle per (kernel, layout, job kind): BBFMM_P2P_SYM_WAVE_MIN is read when the handle's job lists are built."""
    key = (kid, d, name, jobs)
    if key not in _TREES:
        if jobs == "size_rule":
            monkeypatch.delenv("BBFMM_P2P_SYM_WAVE_MIN", raising=False)
        else:
            monkeypatch.setenv("BBFMM_P2P_SYM_WAVE_MIN", "0")
        src = cloud(d, name)[0]
        counts = LAYOUTS[d][name]
        t = F.FmmTree(np.array(src), 5, F.KernelParams(F.KernelType(kid), base_range=BR, total_sill=SILL), True, True,
                      params=F.FmmParams(max(counts), F.M2LCompressionType.ACA, 1e-5, 1024))
        s = t.stats()
        assert s.n_v == 0 and s.n_w == 0 and s.depth <= 1, (s.n_v, s.n_w, s.depth)
        ptr, _ = t.leaf_sources()
        pops = np.diff(ptr)
        assert sorted(pops[pops > 0]) == sorted(counts)      # the prescribed populations are the leaves
        _TREES[key] = t
    return _TREES[key]


def teardown_module(module):
    _TREES.clear()
    _WX.clear()
    for f in (cloud, weights, exact, wx_cloud):
        f.cache_clear()


def bound(where_path, kid, n_src, s_main, s_arg):
    a, b = KP.sum_budget(1, kid, where_path)
    return LD(U) * ((a + 4 + n_src) * s_main + (b + 4) * s_arg)


def assert_within(got, ref, tol, what):
    err = np.abs(np.asarray(got, dtype=np.float64).astype(LD) - ref)
    assert np.isfinite(np.asarray(got)).all(), what
    worst = float((err / np.where(tol > 0, tol, LD(1))).max())
    print(f"{what}: largest error / bound {worst:.3f}")
    bad = np.argwhere(err > tol)
    assert bad.size == 0, (what, "rows/rhs", bad[:5].tolist(), "error / bound", worst)


def cases(ks, jobs_axis=False):
    out = []
    for d, ids in ((3, ALL_IDS), (2, LOW_D_IDS), (1, LOW_D_IDS)):
        for kid in ids:
            for name in layouts_of(kid, d):
                for K, kb in ks.items():
                    if not jobs_axis:
                        out.append(pytest.param(kid, d, name, K, id=f"{NAMES[kid]}-{d}d-{name}-K{K}-{kb}"))
                        continue
                    small = min(LAYOUTS[d][name]) <= 64
                    # wave jobs: leaves of at most 64 rows go to p2p_sym2_kernel, the others to the workgroup kernels;
                    # size rule: a tree this small gives every leaf to p2p_sym3_kernel (one rhs) / p2p_sym_kernel
                    kinds = [("wave", ("sym2+" if max(LAYOUTS[d][name]) > 64 else "sym2") if small else None)]
                    kinds.append(("size_rule", None))
                    for jobs, tag in kinds:
                        if jobs == "wave" and not small:
                            continue
                        wg = "sym3" if K == 1 else "sym"
                        tag = {"sym2": "sym2", "sym2+": "sym2+" + wg, None: wg}[tag]
                        out.append(pytest.param(kid, d, name, K, jobs, id=f"{NAMES[kid]}-{d}d-{name}-{jobs}-K{K}-{kb}-{tag}"))
    return out


@pytest.mark.parametrize("kid,d,name,K", cases(VALUE_K))
def test_values_at_arbitrary_targets(kid, d, name, K, monkeypatch):
    """p2p_kernel<ID, false, 1 | 4 | 8>, the passes with k0 > 0 included, at targets that are a shuffled superset of the
    sources."""
    t = tree(kid, d, name, "wave", monkeypatch)
    src, tgt, _ = cloud(d, name)
    ex = exact(kid, d, name)
    w = np.array(weights(d, name)[:, :K])
    t.set_weights(w)                               # (no far field here: it fixes the column count of the handle)
    y = t.evaluate(w, np.array(tgt))
    assert t.last_evaluate_path() == 0
    assert_within(y, ex.y[:, :K], bound("value", kid, ex.n_src, ex.s_phi[:, :K], ex.s_xd[:, :K]), "values")


@pytest.mark.parametrize("kid,d,name,K", cases(GRAD_K))
def test_gradients_at_arbitrary_targets(kid, d, name, K, monkeypatch):
    """p2p_kernel<ID, true, 1 | 4>: kernel_value_grad_r2 of every kernel id, both Spheroidal branches, the zero-filled
    gradients at r2 <= eps, every weight slot of the gradient accumulators."""
    t = tree(kid, d, name, "wave", monkeypatch)
    src, tgt, _ = cloud(d, name)
    ex = exact(kid, d, name)
    w = np.array(weights(d, name)[:, :K])
    t.set_weights(w)
    y, g = t.evaluate_with_gradients(w, np.array(tgt))
    assert g.shape == (tgt.shape[0], K * d)
    assert_within(y, ex.yg[:, :K], bound("value_g", kid, ex.n_src, ex.sg_phi[:, :K], ex.sg_xd[:, :K]), "values")
    assert_within(g.reshape(-1, K, d), ex.g[:, :K], bound("factor", kid, ex.n_src, ex.s_f[:, :K], ex.s_xf[:, :K]), "gradients")


@pytest.mark.parametrize("kid,d,name,K,jobs", cases(MATVEC_K, jobs_axis=True))
def test_matvec_targets_are_the_sources(kid, d, name, K, jobs, monkeypatch):
    """The unordered-pair kernels (p2p_sym2_kernel: wave jobs; p2p_sym3_kernel<ID, 8>: whole leaves, one rhs;
    p2p_sym_kernel<ID, 1 | 2 | 4>: workgroup chunks) through matvec_device, and for one right-hand side through
    fast_matrix_vector_product; `evaluate` at the sources (the ordered-pair kernel) meets the same bound."""
    import torch
    t = tree(kid, d, name, jobs, monkeypatch)
    src, _, src_rows = cloud(d, name)
    n = src.shape[0]
    ex = exact(kid, d, name)
    ref = ex.y[src_rows][:, :K]
    tol = bound("value", kid, ex.n_src, ex.s_phi[src_rows][:, :K], ex.s_xd[src_rows][:, :K])
    w = np.array(weights(d, name)[:, :K])
    dw = torch.from_numpy(np.ascontiguousarray(w.T)).cuda()
    out = torch.zeros((K, n), dtype=torch.float64, device="cuda")
    t.matvec_device(dw.data_ptr(), n, K, out.data_ptr(), n, True)
    assert_within(out.cpu().numpy().T, ref, tol, "matvec_device")
    if K == 1:
        assert_within(t.fast_matrix_vector_product(w[:, 0].copy())[:, None], ref, tol, "fast_matrix_vector_product")
    if jobs == "size_rule":
        t.set_weights(w)
        y = t.evaluate(w, np.array(src))
        assert t.last_evaluate_path() == 1
        assert_within(y, ref, tol, "evaluate at the sources")


# ------------------------------------------------------------------ W / X lists: M2P, P2L and the fused pass, every kernel id
# A clustered cloud whose tree has live W / X lists, against the oracle running the product's M2L operators (only the
# summation order differs), at the project's tolerances per right-hand side: 1e-11 for values and local coefficients,
# 1e-9 for gradients.
WX_TOL, WX_GRAD_TOL = 1e-11, 1e-9
WX_PARAMS = (40, 2, 1e-5, 1024)            # max_points_per_cell, ACA, epsilon, chunk
WX_ORDER = 5
WX_SEPARATE_IDS = (1, 4, 7, 100)           # the child process with BBFMM_WX_FUSED=0


@functools.lru_cache(maxsize=None)
def wx_cloud():
    from conftest import clustered_points
    rng = np.random.default_rng(77)
    pts = np.unique(clustered_points(rng, 20000, 3), axis=0)
    n = pts.shape[0]
    w = rng.standard_normal((n, 5))
    tg = pts[rng.choice(n, 3000, replace=False)] + 1e-4 * rng.standard_normal((3000, 3))     # off the sources
    tg = np.clip(tg, pts.min(0), pts.max(0))
    return pts, w, tg


_WX = {}


def wx_oracle(kid, product_tree):
    """The oracle's answers for one kernel, computed once: values and L for five rhs at the sources and at the targets,
    values and gradients for three rhs at the targets."""
    from conftest import inject_product_operators
    from oracle import bbfmm_oracle as O
    if ("oracle", kid) not in _WX:
        pts, w, tg = wx_cloud()
        r = O.FmmTree(pts, WX_ORDER, kid, True, True, None, O.FmmParams(*WX_PARAMS), base_range=BR, total_sill=SILL)
        inject_product_operators(product_tree, r)
        r.set_weights(w)
        res = {"y": r.evaluate(w, pts)}
        res["L"] = np.array(r.L)      # of the whole tree: a later evaluate restricts the downward pass to its targets' cells
        res["z"] = r.evaluate(w, tg)
        r.set_weights(w[:, :3])
        res["zg"], res["g"] = r.evaluate_with_gradients(w[:, :3], tg)
        _WX[("oracle", kid)] = res
    return _WX[("oracle", kid)]


def wx_tree(kid, jobs, monkeypatch):
    key = ("tree", kid, jobs)
    if key not in _WX:
        if jobs == "size_rule":
            monkeypatch.delenv("BBFMM_P2P_SYM_WAVE_MIN", raising=False)
        else:
            monkeypatch.setenv("BBFMM_P2P_SYM_WAVE_MIN", "0")
        t = F.FmmTree(wx_cloud()[0], WX_ORDER, F.KernelParams(F.KernelType(kid), base_range=BR, total_sill=SILL), True, True,
                      params=F.FmmParams(*WX_PARAMS))
        s = t.stats()
        assert s.n_w > 0 and s.n_x == s.n_w
        _WX[key] = t
    return _WX[key]


def per_rhs(got, ref, tol, what, width=1):
    from conftest import relerr
    got, ref = np.asarray(got), np.asarray(ref)
    for k in range(ref.shape[1] // width):
        e = relerr(got[:, k * width:(k + 1) * width], ref[:, k * width:(k + 1) * width])
        assert e < tol, (what, "rhs", k, e)


def coefficients_per_rhs(t, K, L_ref, what):
    from conftest import relerr
    L = t.debug_get_coefficients("L", K)
    for k in range(K):
        e = relerr(L[k], L_ref[k])
        assert e < WX_TOL, (what, "rhs", k, e)


@pytest.mark.parametrize("K", [1, 3], ids=["K1-KB1", "K3-KB4"])
@pytest.mark.parametrize("kid", ALL_IDS, ids=[NAMES[k] for k in ALL_IDS])
def test_wx_gradients_off_the_sources(kid, K, monkeypatch):
    """m2p_kernel<ID, true, 1 | 4> and p2p_kernel<ID, true, 1 | 4> on a tree with W lists; the downward pass behind them runs
    the separate p2l_kernel<ID, 1 | 4> into L."""
    t = wx_tree(kid, "wave", monkeypatch)
    ref = wx_oracle(kid, t)
    pts, w, tg = wx_cloud()
    t.set_weights(w[:, :K].copy())
    z, g = t.evaluate_with_gradients(w[:, :K].copy(), tg)    # (the downward pass is restricted to the targets' cells: L is seen through z)
    per_rhs(z, ref["zg"][:, :K], WX_TOL, "values")
    per_rhs(g, ref["g"][:, :3 * K], WX_GRAD_TOL, "gradients", width=3)


@pytest.mark.parametrize("kid", ALL_IDS, ids=[f"{NAMES[k]}-K5-KB4+KB1" for k in ALL_IDS])
def test_wx_values_off_the_sources(kid, monkeypatch):
    """m2p_kernel<ID, false, 4 | 1> (five rhs: a full pass and the k0 = 4 pass), p2l_kernel likewise."""
    t = wx_tree(kid, "wave", monkeypatch)
    ref = wx_oracle(kid, t)
    pts, w, tg = wx_cloud()
    t.set_weights(w)
    per_rhs(t.evaluate(w, tg), ref["z"], WX_TOL, "values")


@pytest.mark.parametrize("K", [1, 3], ids=["K1-wx_sym3", "K3-wx_sym"])
@pytest.mark.parametrize("jobs", ["wave", "size_rule"])
@pytest.mark.parametrize("kid", ALL_IDS, ids=[NAMES[k] for k in ALL_IDS])
def test_wx_fused_matvec(kid, jobs, K, monkeypatch):
    """wx_sym3_kernel (one rhs: whole leaves) and wx_sym_kernel<ID, 4> (three): M2P row sums and P2L column sums of one
    kernel evaluation per (point, node) pair, the latter atomically into L."""
    import torch
    t = wx_tree(kid, jobs, monkeypatch)
    ref = wx_oracle(kid, t)
    pts, w, _ = wx_cloud()
    n = pts.shape[0]
    dw = torch.from_numpy(np.ascontiguousarray(w[:, :K].T)).cuda()
    out = torch.zeros((K, n), dtype=torch.float64, device="cuda")
    t.matvec_device(dw.data_ptr(), n, K, out.data_ptr(), n, True)
    per_rhs(out.cpu().numpy().T, ref["y"][:, :K], WX_TOL, "matvec_device")
    coefficients_per_rhs(t, K, ref["L"], "L after the fused pass")


def test_wx_separate_kernels_in_a_child_process(tmp_path):
    """BBFMM_WX_FUSED=0 (read once per process): the matvec runs m2p_kernel and p2l_kernel instead of the fused pass, for a
    few kernels that are not LinearRbf (tests/test_gpu_switches.py flips the switch for that one)."""
    import os
    import subprocess
    import sys
    from conftest import ROOT
    env = {k: v for k, v in os.environ.items() if not k.startswith("BBFMM_")}
    env["BBFMM_WX_FUSED"] = "0"
    out = str(tmp_path / "wx_separate.npz")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "wx_worker.py"), out] + [str(k) for k in WX_SEPARATE_IDS],
                       env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    got = dict(np.load(out))
    pts, w, _ = wx_cloud()
    for kid in WX_SEPARATE_IDS:
        host = F.FmmTree(pts, WX_ORDER, F.KernelParams(F.KernelType(kid), base_range=BR, total_sill=SILL), True, True,
                         params=F.FmmParams(*WX_PARAMS), host_only=True)
        ref = wx_oracle(kid, host)
        assert int(got[f"n_w_{kid}"]) > 0
        per_rhs(got[f"y1_{kid}"][:, None], ref["y"][:, :1], WX_TOL, f"kernel {kid}: one rhs")
        per_rhs(got[f"y3_{kid}"], ref["y"][:, :3], WX_TOL, f"kernel {kid}: three rhs")
        from conftest import relerr
        for k in range(3):
            assert relerr(got[f"L3_{kid}"][k], ref["L"][k]) < WX_TOL, (kid, k)
