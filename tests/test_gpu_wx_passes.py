"""The pass that serves the W lists (csrc/device_wx.hip) pinned to long double, target by target: M2P alone, the leaf pass as
a whole where P2P, L2P and M2P meet in one output, and the fused unordered M2P + P2L pass of the matvec.  M2P is restated
one step from the device's own multipoles (far_field_reference.m2p, bound derived there), the U-list sum is exact
(kernel_reference.Dense, the bound of tests/test_gpu_pair_kernels.py), L2P is far_field_reference.l2p of the device's L, and
the column sums of the fused pass go through check_downward of tests/test_gpu_far_field_passes.py.  Every assertion prints
its largest error / bound.

The clouds are the two-level layouts of tests/far_field_cases.py (TWO_LEVEL: prescribed level-1 populations around the job
cuts, W lists of 1 to 19 cells around the chunks of 8 and 16) and clustered_cloud (W cells at several levels, M2L live).  A
case is (cloud, order, kernel, what); the cases of one (cloud, order, kernel) run next to each other and share handles,
kernel matrices and X-list terms.

    what                 runs
    m2p                  every level-1 leaf in turn, weights under its W cells only (no U source carries weight, nothing
                         reaches its L: both asserted as exact zeros), so the leaf pass is M2P alone:
                         evaluate_leaves, K = 1, 3, 5     m2p_kernel<ID, false, 1> (K = 1; K = 5: the pass at k0 = 4),
                                                          m2p_kernel<ID, false, 4> (K = 3: kb = 3; K = 5), p2l_kernel<ID, 1 | 4>
                         evaluate_with_gradients, K = 1, 3   m2p_kernel<ID, true, 1>, m2p_kernel<ID, true, 4>
    leaf                 dense weights, K = 3, evaluate_leaves at all leaves with a W list at once: U sum + L2P + M2P
    fused-<jobs>-K<K>    matvec_device under BBFMM_P2P_SYM_WAVE_MIN=0 (wave) or unset (size_rule); L of every cell with an X
                         list and below (the column sums), every row of every leaf with a W list (the row sums + P2P + L2P)
                         K = 1   wx_sym3_kernel<ID, 8>          K = 2   wx_sym_kernel<ID, 2>
                         K = 3   wx_sym_kernel<ID, 4>, kb = 3    K = 4   wx_sym_kernel<ID, 4>
                         K = 5   wx_sym_kernel<ID, 4>, then wx_sym3_kernel<ID, 8> at k0 = 4

Orders (LinearRbf and Spheroidal3, base range 0.5 and sill 0.4: both Spheroidal branches occur): 3-D 5 on every layout, 2,
7, 8, 9 and 10 on the two small layouts with W lists of 8 to 19 cells, 16 on the small layout with lists of 4 to 7 (the
long-double sums of a case stay under a few million pairs); 2-D 7 on every layout, 3 and 16 on two; 1-D 4 and 16.  Every
kernel id at order 5 on one 3-D layout (m2p, fused K = 1 and 3).  clustered_cloud at orders 4 and 7 (fused K = 1, 5; leaf
at order 4).  The jobs a case is meant to run are asserted from debug_wx_jobs() against the cuts restated from the layout
(far_field_cases.expected_wx_jobs).  wx_sym_kernel<ID, 1> and wx_sym3_kernel<ID, 6> run only under switches that are read
once per process: one child process each (tests/wx_worker.py), LinearRbf at order 5, the same checks on what it writes."""
import os
import subprocess
import sys

import numpy as np
import pytest

import far_field_cases as C
import far_field_reference as R
import ferreus_rbf_rs_amd as F
import kernel_pointwise as KP
import kernel_reference as KR
import test_gpu_far_field_passes as P
from far_field_reference import LD, U

pytestmark = pytest.mark.gpu

BR, SILL = 0.5, 0.4
NAMES = {int(k): k.name for k in F.KernelType}
COPIES = 8                                                            # displaced copies per leaf among the targets
K_ALL = 5
JOB_RULES = ("wave", "size_rule")
SWEEP_LAYOUT = "w8-12"
LONG_W = ("w8-12", "w14-19-small")
LEAF_ORDER = {3: 5, 2: 7, 1: 4}                                       # the order at which a dimension's layouts run `leaf`
INSTANCES = {"m2p_kernel<false,1>", "m2p_kernel<false,4>", "m2p_kernel<true,1>", "m2p_kernel<true,4>", "wx_sym_kernel<2>",
             "wx_sym_kernel<4>", "wx_sym3_kernel<8>", "p2l_kernel<1>", "p2l_kernel<4>"}
SEEN = set()
WORST = {}                                                            # (what, dimension) -> largest error / bound, for the report


def fused(ks):
    return [f"fused-{jobs}-K{K}" for jobs in JOB_RULES for K in ks]


def _cases():
    groups = []
    for kid in (0, 3):
        groups += [((3, name), 5, kid) for name in C.TWO_LEVEL[3]]
        groups += [((3, name), order, kid) for order in (2, 7, 8, 9, 10) for name in LONG_W]
        groups += [((3, "w4-7"), 16, kid)]
        groups += [((2, name), 7, kid) for name in C.TWO_LEVEL[2]]
        groups += [((2, name), order, kid) for order in (3, 16) for name in ("w2-3", "w7")]
        groups += [((1, name), order, kid) for order in (4, 16) for name in C.TWO_LEVEL[1]]
    out = []
    for cloud, order, kid in groups:
        whats = ["m2p"] + (["leaf"] if order == LEAF_ORDER[cloud[0]] else []) + fused((1, 2, 3, 4, 5))
        out += [(cloud, order, kid, w) for w in whats]
    for kid in KR.KERNEL_IDS:
        if kid not in (0, 3):
            out += [((3, SWEEP_LAYOUT), 5, kid, w) for w in ["m2p"] + fused((1, 3))]
    out += [(("clustered",), 4, 0, w) for w in ["leaf"] + fused((1, 5))] + [(("clustered",), 7, 0, w) for w in fused((1, 5))]
    return out


CASES = _cases()


def case_id(c):
    cloud, order, kid, what = c
    return f"{'-'.join(str(v) for v in cloud)}-p{order}-{NAMES[kid]}-{what}"


@pytest.fixture(autouse=True)
def _one_group_of_cases_at_a_time(request):
    """Handles, kernel matrices and X-list terms are shared by the cases of one (cloud, order, kernel), which run next to
    each other; the clouds, their targets and the exact U-list sums (they depend on neither the order nor the device) stay."""
    params = getattr(getattr(request.node, "callspec", None), "params", {})
    group = params.get("case", (None,))[:3]
    if C.cached(("group",), lambda: [None])[0] != group:
        C.drop_cached(keep=("cloud", "targets", "u sums"))
        C.cached(("group",), lambda: [None])[0] = group
    yield


@pytest.fixture(scope="module", autouse=True)
def _release_everything_at_the_end():
    yield
    C.drop_cached()


# ------------------------------------------------------------------ clouds, handles, references
def cloud_points(cloud):
    return C.cached(("cloud", "wx", cloud), C.clustered_cloud if cloud[0] == "clustered" else lambda: C.two_level_cloud(*cloud))


def cloud_limit(cloud):
    return C.CLUSTERED_LIMIT if cloud[0] == "clustered" else C.two_level_limit(*cloud)


def dense_weights(cloud):
    return C.cached(("cloud", "wx weights", cloud), lambda: C.dense_weights(len(cloud_points(cloud)), K_ALL, 83))


def tree(cloud, order, kid, jobs, monkeypatch):
    """(handle, geometry, leaves with a W list): BBFMM_P2P_SYM_WAVE_MIN is read when the handle's job lists are built."""
    def make():
        if jobs == "size_rule":
            monkeypatch.delenv("BBFMM_P2P_SYM_WAVE_MIN", raising=False)
        else:
            monkeypatch.setenv("BBFMM_P2P_SYM_WAVE_MIN", "0")
        t = C.make_tree(cloud_points(cloud), order, cloud_limit(cloud), kernel=(kid, BR, SILL))
        geo = C.cached(("geometry", cloud, order), lambda: R.Geometry(t))
        s = t.stats()
        assert s.n_x == s.n_w > 0
        w_leaves = [int(c) for c in np.nonzero(np.diff(geo.lists["W"][0]) > 0)[0]]
        assert geo.is_leaf[w_leaves].all()
        if cloud[0] != "clustered":
            level1 = C.assert_two_level(t, geo, *cloud)
            assert sorted(level1.values()) == w_leaves
        else:
            assert s.n_v > 0 and len(set(geo.level[w_leaves].tolist())) > 1
        return t, geo, w_leaves
    return C.cached(("tree", cloud, order, kid, jobs), make)


def assert_jobs(t, cloud, geo, w_leaves):
    """The jobs of the resident target set, from the hook: on a layout exactly the cuts restated from its table."""
    jobs = t.debug_wx_jobs()
    n_w = np.diff(geo.lists["W"][0])
    if cloud[0] != "clustered":
        assert jobs == C.expected_wx_jobs(*cloud), (jobs, C.expected_wx_jobs(*cloud))
    assert jobs["n_w_jobs"] == sum(-(-int(n_w[c]) // 8) for c in w_leaves) and jobs["max_cells_w"] == min(8, int(n_w.max()))
    if n_w.max() > 8:                                                 # several M2P jobs add into the same targets
        assert jobs["n_w_jobs"] > len(w_leaves)
    assert 0 < jobs["max_rows_wx"] <= 48 and 0 < jobs["max_cells_wx"] <= 16 and 0 < jobs["max_rows_wxl"] <= 256
    assert jobs["n_wx_jobs"] > 0 and jobs["n_wxl_jobs"] > 0
    return jobs


def leaf_targets(cloud, geo, leaf):
    """(targets, rows): the leaf's own points (rows of the cloud, in leaf order) and then COPIES displaced copies inside it."""
    def make():
        pts = cloud_points(cloud)
        rows = geo.src_idx[geo.src_ptr[leaf]:geo.src_ptr[leaf + 1]]
        tg = np.ascontiguousarray(np.concatenate([pts[rows], C.inside_copies(geo, leaf, pts[rows], COPIES, 85 + leaf)]))
        assert (box_leaf_of(geo, tg) == leaf).all()
        return tg, rows
    return C.cached(("targets", cloud, leaf), make)


def box_leaf_of(geo, x):
    """The leaf of every point by its box, from the geometry alone (the leaves tile the root box)."""
    leaves = np.nonzero(geo.is_leaf)[0]
    lo = geo.centres[leaves] - geo.lengths[leaves, None] / 2
    hi = geo.centres[leaves] + geo.lengths[leaves, None] / 2
    inside = ((x[:, None, :] > lo[None]) & (x[:, None, :] < hi[None])).all(axis=2)
    assert (inside.sum(axis=1) == 1).all()
    return leaves[np.argmax(inside, axis=1)]


def u_sums(cloud, kid, geo, leaf):
    """The exact U-list sums of the dense weights at the leaf's targets, all K_ALL columns: (y, s_phi, s_arg, n_src)."""
    def make():
        pts, w = cloud_points(cloud), dense_weights(cloud)
        up, ui = geo.lists["U"]
        srcs = np.concatenate([geo.src_idx[geo.src_ptr[c]:geo.src_ptr[c + 1]] for c in ui[up[leaf]:up[leaf + 1]]])
        D = KR.Dense(kid, BR, SILL, leaf_targets(cloud, geo, leaf)[0], pts[srcs])
        return D.sums(w[srcs]) + (len(srcs),)
    return C.cached(("u sums", cloud, kid, leaf), make)


def matrices(cloud, order, kid, geo, leaf, gradients=False):
    def make():
        return R.M2PMatrices(geo, (kid, BR, SILL), leaf, leaf_targets(cloud, geo, leaf)[0], 1, gradients)
    m = C.cached(("m2p matrices", cloud, order, kid, leaf), make)
    if gradients and m.D is None:
        m = make()
    return m


def within(got, ref, bound, what):
    """Largest |got - ref| / bound; a zero bound wants an exact zero."""
    got = np.asarray(got, dtype=np.float64)
    assert np.isfinite(got).all() and got.shape == ref.shape, what
    err = np.abs(got.astype(LD) - ref)
    with np.errstate(all="ignore"):
        r = np.where(err == 0, LD(0), err / np.where(bound > 0, bound, LD(1)) + np.where(bound > 0, LD(0), LD(np.inf)))
    return float(r.max()), np.unravel_index(int(np.argmax(r)), r.shape)


def report(tag, d, ratio, what, at):
    WORST[tag, d] = max(WORST.get((tag, d), 0.0), ratio)
    print(f"{what}: largest error / bound {ratio:.3g} at (leaf, row, rhs[, axis]) {at}")
    assert ratio <= 1.0, (what, ratio, at)


def leaf_pass_reference(cloud, order, kid, geo, leaf, M, L, rows=slice(None)):
    """What the leaf pass returns at the targets `rows` of a leaf under the dense weights: exact U-list sum + L2P of the
    device's L + M2P of the device's M, and the sum of the three bounds."""
    K = M.shape[0]
    y, s_phi, s_arg, n_src = u_sums(cloud, kid, geo, leaf)
    a, b = KP.sum_budget(1, kid, "value")
    bu = LD(U) * ((a + 4 + n_src) * s_phi[rows, :K] + (b + 4) * s_arg[rows, :K])
    yl, bl = R.l2p(geo, L, leaf, leaf_targets(cloud, geo, leaf)[0][rows])
    ym, bm = matrices(cloud, order, kid, geo, leaf).values(M, rows)
    return y[rows, :K] + yl + ym, bu + bl + bm


# ------------------------------------------------------------------ a. M2P alone
def run_m2p_alone(cloud, order, kid, monkeypatch):
    t, geo, w_leaves = tree(cloud, order, kid, "wave", monkeypatch)
    assert_jobs(t, cloud, geo, w_leaves)
    pts = cloud_points(cloud)
    d = geo.d
    up, ui = geo.lists["U"]
    worst = {"values": (0.0, None), "values of the gradient call": (0.0, None), "gradients": (0.0, None)}

    def keep(tag, got, ref, bound, leaf, K):
        ratio, at = within(got, ref, bound, (tag, leaf, K))
        if ratio > worst[tag][0]:
            worst[tag] = (ratio, (leaf,) + tuple(int(i) for i in at) + (f"K={K}",))

    for leaf in w_leaves:
        tg, rows = leaf_targets(cloud, geo, leaf)
        own = slice(0, len(rows))
        w = C.w_cell_weights(geo, len(pts), leaf, K_ALL, 87 + leaf)
        near = np.concatenate([geo.src_idx[geo.src_ptr[c]:geo.src_ptr[c + 1]] for c in ui[up[leaf]:up[leaf + 1]]])
        assert leaf in ui[up[leaf]:up[leaf + 1]] and (w[near] == 0).all() and (w != 0).any()     # no U source carries weight
        mats = None
        for K in (3, 1, 5):
            wk = np.ascontiguousarray(w[:, :K])
            t.set_weights(wk)
            t.set_local_coefficients(wk)
            M, L = t.debug_get_coefficients("M", K), t.debug_get_coefficients("L", K)
            c = leaf
            while c >= 0:                                             # nothing reaches L of the leaf or of an ancestor
                assert (L[:, c] == 0).all()
                c = geo.parent[c]
            if mats is None:
                mats = matrices(cloud, order, kid, geo, leaf, gradients=True)
            assert all((M[:, x] != 0).any() for x in mats.cells)     # every W cell is live
            sel = slice(None) if K == 3 else own                      # K = 1, 5: exactly the leaf's population
            yr, yb = mats.values(M, sel)
            keep("values", t.evaluate_leaves(wk, tg[sel]), yr, yb, leaf, K)
            SEEN.update({"m2p_kernel<false,1>", "p2l_kernel<1>"} if K == 1 else {"m2p_kernel<false,4>", "p2l_kernel<4>"})
            if K == 5:
                SEEN.update({"m2p_kernel<false,1>", "p2l_kernel<1>"})
            if K in (1, 3):
                sel = slice(None) if K == 1 else own
                y, g = t.evaluate_with_gradients(wk, tg[sel])
                yr, yb, gr, gb = mats.gradients(M)
                keep("values of the gradient call", y, yr[sel], yb[sel], leaf, K)
                keep("gradients", g.reshape(-1, K, d), gr[sel], gb[sel], leaf, K)
                SEEN.add("m2p_kernel<true,1>" if K == 1 else "m2p_kernel<true,4>")
        mats.D = None                                                 # the cases after this one need the value matrices only
    for tag, (ratio, at) in worst.items():
        report("M2P alone" if tag != "gradients" else "M2P alone, gradients", d, ratio,
               f"M2P alone {case_id((cloud, order, kid, tag))}", at)
    assert all(v[0] > 0 for v in worst.values())


# ------------------------------------------------------------------ b. the leaf pass as a whole
def run_leaf_pass(cloud, order, kid, monkeypatch, K=3):
    t, geo, w_leaves = tree(cloud, order, kid, "wave", monkeypatch)
    assert_jobs(t, cloud, geo, w_leaves)
    assert len(w_leaves) == int((np.diff(geo.lists["W"][0]) > 0).sum())
    w = np.ascontiguousarray(dense_weights(cloud)[:, :K])
    t.set_weights(w)
    t.set_local_coefficients(w)
    M, L = t.debug_get_coefficients("M", K), t.debug_get_coefficients("L", K)
    tg = [leaf_targets(cloud, geo, leaf)[0] for leaf in w_leaves]
    first = np.concatenate([[0], np.cumsum([len(x) for x in tg])])
    y = t.evaluate_leaves(w, np.ascontiguousarray(np.concatenate(tg)))
    SEEN.update({"m2p_kernel<false,4>", "p2l_kernel<4>"})
    worst, where, done = 0.0, None, 0
    for i, leaf in enumerate(w_leaves):
        ref, bound = leaf_pass_reference(cloud, order, kid, geo, leaf, M, L)
        ratio, at = within(y[first[i]:first[i + 1]], ref, bound, ("leaf pass", leaf))
        done += 1
        if ratio > worst:
            worst, where = ratio, (leaf,) + tuple(int(v) for v in at)
    assert done == len(w_leaves)
    report("leaf pass", geo.d, worst, f"leaf pass {case_id((cloud, order, kid, 'leaf'))}, {done} leaves", where)
    assert worst > 0


# ------------------------------------------------------------------ c. the fused pass
def x_cells_and_below(geo):
    cells = set(int(c) for c in np.nonzero(np.diff(geo.lists["X"][0]) > 0)[0])
    stack = list(cells)
    while stack:
        for ch in geo.children[stack.pop()]:
            if ch not in cells:
                cells.add(int(ch))
                stack.append(int(ch))
    assert cells and all(geo.level[c] >= 2 for c in cells)
    return sorted(cells)


def check_fused(cloud, order, kid, t, geo, w_leaves, K, y, M, L, what):
    """(i) the column sums: L of every cell with an X list and below; (ii) every row of every leaf with a W list."""
    pts, w = cloud_points(cloud), dense_weights(cloud)
    cache = C.cached(("p2l terms", cloud, order, kid), dict)
    ratio, _ = P.check_downward(t, geo, ("wx", cloud, order, kid), pts, w, what, (kid, BR, SILL), cells=x_cells_and_below(geo),
                                M=M, L=L, p2l_cache=cache)
    WORST["fused pass, L", geo.d] = max(WORST.get(("fused pass, L", geo.d), 0.0), ratio)
    worst, where = 0.0, None
    for leaf in w_leaves:
        rows = leaf_targets(cloud, geo, leaf)[1]
        ref, bound = leaf_pass_reference(cloud, order, kid, geo, leaf, M, L, slice(0, len(rows)))
        r, at = within(y[rows], ref, bound, (what, leaf))
        if r > worst:
            worst, where = r, (leaf,) + tuple(int(v) for v in at)
    report("fused pass, rows", geo.d, worst, f"fused pass {what}, rows of {len(w_leaves)} leaves", where)
    assert worst > 0


def run_fused(cloud, order, kid, jobs, K, monkeypatch):
    import torch
    t, geo, w_leaves = tree(cloud, order, kid, jobs, monkeypatch)
    hook = assert_jobs(t, cloud, geo, w_leaves)
    w = dense_weights(cloud)
    n = len(w)
    dw = torch.from_numpy(np.ascontiguousarray(w[:, :K].T)).cuda()
    out = torch.zeros((K, n), dtype=torch.float64, device="cuda")
    t.matvec_device(dw.data_ptr(), n, K, out.data_ptr(), n, True)
    M, L = t.debug_get_coefficients("M", K), t.debug_get_coefficients("L", K)
    if K % 4 == 1:
        assert hook["n_wxl_jobs"] > 0
        SEEN.add("wx_sym3_kernel<8>")
    if K > 1:
        assert hook["n_wx_jobs"] > 0
        SEEN.add("wx_sym_kernel<2>" if K == 2 else "wx_sym_kernel<4>")
    check_fused(cloud, order, kid, t, geo, w_leaves, K, out.cpu().numpy().T, M, L, case_id((cloud, order, kid, f"fused-{jobs}-K{K}")))


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_wx(case, monkeypatch):
    cloud, order, kid, what = case
    if what == "m2p":
        run_m2p_alone(cloud, order, kid, monkeypatch)
    elif what == "leaf":
        run_leaf_pass(cloud, order, kid, monkeypatch)
    else:
        _, jobs, K = what.split("-")
        run_fused(cloud, order, kid, jobs, int(K[1:]), monkeypatch)


# ------------------------------------------------------------------ the instances behind the process-wide switches
CHILD_CLOUD, CHILD_ORDER = (3, "w14-19"), 5


@pytest.mark.parametrize("env,instance", [({"BBFMM_WX_SYM_LEAF": "0"}, "wx_sym_kernel<1>"),
                                          ({"BBFMM_P2P_SYM_LEAF_PASS": "6"}, "wx_sym3_kernel<6>")], ids=lambda v: v if isinstance(v, str) else "")
def test_wx_fused_one_rhs_instances_in_a_child_process(env, instance, tmp_path, monkeypatch):
    """BBFMM_WX_SYM_LEAF=0: no whole-leaf jobs, the chunk jobs serve one right-hand side (wx_sym_kernel<ID, 1>);
    BBFMM_P2P_SYM_LEAF_PASS=6: the whole-leaf kernels with six rows per pass (wx_sym3_kernel<ID, 6>).  LinearRbf at order 5; the
    child runs the matvec and writes the product, M, L and the hook's answer, the parent checks them as in test_wx."""
    from conftest import ROOT
    cenv = {k: v for k, v in os.environ.items() if not k.startswith("BBFMM_")}
    cenv.update(env, BBFMM_P2P_SYM_WAVE_MIN="0")
    out = str(tmp_path / "wx_child.npz")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "wx_worker.py"), out, "two-level", str(CHILD_CLOUD[0]),
                        CHILD_CLOUD[1], str(CHILD_ORDER)], env=cenv, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    got = dict(np.load(out))
    t, geo, w_leaves = tree(CHILD_CLOUD, CHILD_ORDER, 0, "wave", monkeypatch)
    jobs = dict(zip(t.WX_JOB_FIELDS, got["jobs"].tolist()))
    expected = C.expected_wx_jobs(*CHILD_CLOUD)
    if instance == "wx_sym_kernel<1>":
        assert jobs["n_wxl_jobs"] == 0 and jobs["max_rows_wxl"] == 0
        assert {k: v for k, v in jobs.items() if "wxl" not in k} == {k: v for k, v in expected.items() if "wxl" not in k}
    else:
        assert jobs == expected
    check_fused(CHILD_CLOUD, CHILD_ORDER, 0, t, geo, w_leaves, 1, got["y"], got["M"], got["L"], f"child process {instance}")


# ------------------------------------------------------------------ every instance was run
def test_the_cases_ran_every_instance_of_the_table(monkeypatch):
    """The union over the cases above (the table of the module docstring).  Where cases did not run in this process
    (deselected, another worker), one group's cases are run here, so the answer does not depend on which tests ran before."""
    if not INSTANCES <= SEEN:
        cloud, order, kid = (3, SWEEP_LAYOUT), 5, 0
        run_m2p_alone(cloud, order, kid, monkeypatch)
        for K in (1, 2, 3):
            run_fused(cloud, order, kid, "wave", K, monkeypatch)
    assert INSTANCES <= SEEN, INSTANCES - SEEN
    for (tag, d), ratio in sorted(WORST.items()):
        print(f"largest error / bound, {tag}, {d}-D: {ratio:.3g}")
