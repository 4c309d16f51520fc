"""The sweep of the Schwarz preconditioner between its levels -- level_step() and the loop of the apply (csrc/schwarz.cpp), the
vector kernels of csrc/schwarz_kernels.hip -- through the trace hook (SchwarzPreconditioner.debug_apply_trace), every part of
every step restated in long double one step from the device's own input with the bounds of tests/schwarz_sweep_reference.py.
The local solves are tied bit for bit to the solvers test_gpu_ddm_local.py pins.  Every assertion prints its largest error /
bound ratio."""
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import ferreus_rbf_rs_amd as F
import schwarz_sweep_reference as W
from ferreus_rbf_rs_amd.ddm import DDMParams, DDMTree, DebugLevel, InterpolantSettings, SchwarzPreconditioner

# name: n, dim, kernel, drift, nugget, base_range, DDMParams, level sizes
CASES = {
    "3d_linear": (1500, 3, 3, 1, 0.05, 0.3, (48, 0.5, 0.25, 64), [1500, 384, 96, 24]),
    "3d_no_drift": (1500, 3, 3, -1, 0.05, 0.3, (48, 0.5, 0.25, 64), [1500, 384, 96, 24]),
    "2d_kernel0": (1500, 2, 0, 0, 0.0, 1.0, (48, 0.5, 0.25, 64), [1500, 384, 96, 24]),
    "1d_quadratic": (1200, 1, 3, 2, 0.05, 0.3, (40, 0.5, 0.25, 40), [1200, 320, 80, 20]),
    "3d_quadratic": (2500, 3, 3, 2, 0.05, 0.3, (80, 0.5, 0.125, 250), [2500, 320, 40]),
    "one_level": (60, 3, 3, 1, 0.05, 0.3, (48, 0.5, 0.25, 64), [60]),
}
ORDER = 5


def inputs(name):
    n, dim, kid, drift, nugget, br, prm, sizes = CASES[name]
    pts = W.cloud(n, dim, 100 + n + dim)
    st = InterpolantSettings(kid, dim, drift=drift, nugget=nugget, base_range=br, total_sill=1.0)
    rng = np.random.default_rng(n + 7 * dim)
    rgs = [np.concatenate([rng.standard_normal(n), np.zeros(st.basis_size)]) for _ in range(2)]
    return pts, st, DDMParams(*prm), sizes, rgs


def make_tree(pts, st, deterministic=True):
    # (the calibration inputs of the local solvers have sill 1 > range 0.3: past the reference builder's assertion)
    kp = F.KernelParams(F.KernelType(st.kernel_type), base_range=st.base_range, total_sill=st.total_sill, validate=False)
    return F.FmmTree(pts, ORDER, kp, True, True, deterministic=deterministic)


class Case:
    """A deterministic tree, its preconditioner, the decomposition, a DebugLevel per level on the level's own domains, and one
    trace -- taken after an apply on another residual, so that d_out and d_res hold stale values when the sweep begins."""

    def __init__(self, name, global_scaling=False, deterministic=True, levels=None):
        self.name = name
        self.pts, self.st, self.prm, self.sizes, (warm, self.rg) = inputs(name)
        self.n, self.basis = self.pts.shape[0], self.st.basis_size
        self.tree = make_tree(self.pts, self.st, deterministic)
        self.pre = SchwarzPreconditioner(self.tree, self.pts, self.st, self.prm, global_scaling=global_scaling)
        self.ddm = DDMTree(self.pts, self.prm).levels
        assert [len(lv.point_indices) for lv in self.ddm] == self.sizes == [len(self.pre.level_points(li))
                                                                          for li in range(self.pre.num_levels)]
        for li, lv in enumerate(self.ddm):
            assert np.array_equal(lv.point_indices, self.pre.level_points(li))
        nl = len(self.ddm)
        self.levels = levels or [DebugLevel(self.pts, W.level_domains(lv), self.st, solve_for_poly=(li + 1 == nl and self.basis > 0))
                                 for li, lv in enumerate(self.ddm)]
        self.ortho = self.pre.debug_ortho()
        # the coarse domain's special points: the first k of the hook level's reordered indices (a handle that chose others
        # fails the tail check: its sp_mono would not be the one restated)
        self.special = self.levels[-1].indices[0][:self.basis]
        coarse_pts = self.pts[self.ddm[-1].point_indices]
        self.scaling = W.extents_scaling(self.pts if global_scaling else coarse_pts)
        self.pre(warm)
        self.z, self.steps, self.initial = self.pre.debug_apply_trace(self.rg)

    def check(self, **kw):
        return W.check_trace(self.pts, self.st, self.ddm, self.levels, self.ortho, self.rg, self.z, self.steps, self.initial,
                             special=self.special, scaling=self.scaling, **kw)


_cases = {}


def case(name):
    if name not in _cases:
        _cases[name] = Case(name)
    return _cases[name]


@pytest.fixture(scope="module", autouse=True)
def _release_everything_at_the_end():
    yield
    _cases.clear()


def assert_positive(stats, kinds):
    for k in kinds:
        assert stats[k] is not None and stats[k] > 0, f"no {k} check saw a difference: it compares a value with itself?"


@pytest.mark.parametrize("name", ["3d_linear", "2d_kernel0", "1d_quadratic", "3d_quadratic"])
def test_every_part_of_every_record_with_a_basis(name):
    c = case(name)
    assert len(c.steps) == 2 * (len(c.sizes) - 1) and c.basis == {"3d_linear": 4, "2d_kernel0": 1, "1d_quadratic": 3,
                                                                 "3d_quadratic": 10}[name]
    assert c.levels[-1].k == [c.basis] and c.special.size == c.basis
    stats = c.check()
    print(f"{name}: largest error / bound per kind: {stats}")
    assert_positive(stats, ["residual", "projection", "writeback", "tail", "stale", "solve_rows", "writeback_rows"])
    if name == "3d_quadratic":      # level 0: 2500 rows in 1024 blocks of 3, the last one (row 2499 alone) short, 190 empty
        assert W.projection_steps(2500) == 1 + 8 + 833
    worst, measured = W.check_ortho(c.ortho, c.pre.monomial_matrix)
    print(f"{name}: ortho deviation / tolerance {worst:.3g} (float64 restatement off by {measured:.3g})")
    assert worst > 0


def test_no_drift_writes_back_bit_for_bit_without_projection_or_tail():
    c = case("3d_no_drift")
    assert c.basis == 0 and c.ortho is None and c.special.size == 0 and c.z.size == c.n
    stats = c.check()
    print(f"3d_no_drift: {stats}")
    assert stats["projection"] is None and stats["tail"] is None and stats["writeback"] is None
    assert all(s["proj"] is None and s["tail"] is None for s in c.steps)
    assert_positive(stats, ["residual", "solve_rows", "writeback_rows"])


def test_one_level_is_a_single_coarse_step_with_a_tail():
    c = case("one_level")
    assert len(c.steps) == 1
    s = c.steps[0]
    assert (s["level"], s["coarse"], s["have_sl"], s["add_poly"]) == (0, True, False, True) and s["tail"] is not None
    assert c.levels[0].k == [4]
    stats = c.check()
    print(f"one_level: {stats}")
    assert_positive(stats, ["tail", "solve_rows", "writeback_rows"])
    W.check_ortho(c.ortho, c.pre.monomial_matrix)


def test_global_scaling_coarse_coefficients_and_the_same_polynomial():
    d = case("3d_linear")
    g = Case("3d_linear", global_scaling=True, levels=d.levels)
    factor = d.levels[-1].factor()
    stats = g.check(coarse_factor=factor)
    print(f"3d_linear, global scaling: {stats}")
    assert_positive(stats, ["residual", "projection", "writeback", "tail", "coarse", "solve_rows"])
    # the first coarse visit reads the same residual in both handles (the fine levels do not depend on the scaling)
    coarse_rows = d.ddm[-1].point_indices
    assert W.same_bits(d.steps[1]["res"][coarse_rows], g.steps[1]["res"][coarse_rows])
    assert not np.array_equal(d.steps[-1]["tail"], g.steps[-1]["tail"])
    # both tails as one polynomial at the special points: the difference of the right-hand sides is bounded from the forward
    # bounds of the two coarse solves and the exact image of the difference of the residual inputs (reference, section 5)
    lv = d.levels[-1]
    same = W.check_tails_agree(lambda v: W.R.solve_forward(factor[0], lv.m[0], lv.k[0], lv.q[0], v), lv.indices[0], d.pts, d.st,
                               d.special, [(c.steps[-1], c.steps[-2], c.rg, c.scaling) for c in (d, g)])
    print(f"the two tails at the special points: {same}")
    assert same["ratio"] > 0


def test_the_trace_entry_refuses_too_few_steps():
    import ctypes
    from ferreus_rbf_rs_amd import _lib as L
    c = case("3d_linear")
    n, cap = c.n, len(c.steps) - 1
    z, info, initial = np.zeros(n + c.basis), np.zeros((cap, 5), dtype=np.int32), np.zeros((2, n))
    vectors, small, count = np.zeros((cap, 4, n)), np.zeros((cap, 32)), ctypes.c_int32(-1)
    rc = L.load().bbfmm_schwarz_debug_apply_trace(c.pre._h, c.rg.ctypes.data, z.ctypes.data, c.rg.size, cap, info.ctypes.data,
                                                  initial.ctypes.data, vectors.ctypes.data, small.ctypes.data, ctypes.byref(count))
    assert rc == L.BAD_ARGUMENT and not z.any() and not vectors.any()
    assert W.same_bits(c.pre(c.rg), c.z), "the refused call left the handle as it was"


@pytest.mark.parametrize("name", ["3d_linear", "2d_kernel0", "1d_quadratic", "3d_quadratic", "3d_no_drift"])
def test_the_partial_product_of_every_record(name):
    """y is the tree's product with the correction so far at the level's rows: a wrong subset id or row list shows here.
    Both entries gather the weights, run the upward pass, the downward pass and the leaf pass of a subset plan built by the same
    function from the same rows, and the handle is deterministic: the values are equal, not only within the 1e-11 of
    test_gpu_parity.py (the host entry adds w * 0, which can only turn a -0 into a +0: values are compared, not bits)."""
    c = case(name)
    worst, checked = 0.0, 0
    for i, s in enumerate(c.steps):
        if not s["have_sl"]:
            continue
        rows = c.pre.level_points(s["level"])
        ref = c.tree.fast_matrix_vector_product(c.steps[i - 1]["sl"], target_indices=rows)[rows]
        err = float(np.abs(s["y"] - ref).max() / np.abs(ref).max())
        worst, checked = max(worst, err), checked + 1
        assert err <= 1e-11, (name, i, err)
        assert np.array_equal(s["y"], ref), (name, i, err)
    print(f"{name}: {checked} partial products, largest relative difference {worst:.3g}")
    assert checked == len(c.steps) - 1


def test_apply_equals_trace_and_two_traces_are_bit_identical():
    c = case("3d_linear")
    assert W.same_bits(c.pre(c.rg), c.z)
    z2, steps2, initial2 = c.pre.debug_apply_trace(c.rg)
    assert W.same_bits(z2, c.z) and len(steps2) == len(c.steps)
    for a, b in zip(c.steps, steps2):
        for key in ("y", "out", "sl", "proj", "tail"):
            assert (a[key] is None) == (b[key] is None)
            if a[key] is not None:
                assert W.same_bits(a[key], b[key]), key
        if a["have_sl"]:     # (the other rows of d_res are those of the apply before: check_residual holds them to that)
            rows = c.ddm[a["level"]].point_indices
            assert W.same_bits(a["res"][rows], b["res"][rows])
    assert W.same_bits(initial2["out"], c.steps[-1]["out"]) and W.same_bits(initial2["res"], c.steps[-1]["res"])


def test_a_default_tree_passes_every_check_of_every_record():
    """f64 atomics in the partial products: y changes in its last bits from run to run, every step is still restated from the
    record's own y."""
    d = case("3d_linear")
    c = Case("3d_linear", deterministic=False, levels=d.levels)
    stats = c.check()
    print(f"3d_linear on a default tree: {stats}")
    assert_positive(stats, ["residual", "projection", "writeback", "tail", "solve_rows"])
    z2, steps2, initial2 = c.pre.debug_apply_trace(c.rg)
    W.check_trace(c.pts, c.st, c.ddm, c.levels, c.ortho, c.rg, z2, steps2, initial2, special=c.special, scaling=c.scaling)
    assert W.same_bits(initial2["out"], c.steps[-1]["out"]) and W.same_bits(initial2["res"], c.steps[-1]["res"])
    assert W.same_bits(steps2[0]["sl"], c.steps[0]["sl"]), "the first step has no product in it"


def test_the_per_thread_stride_loop_of_the_projection():
    """263,000 rows: 257 rows per block, the first size at which a thread of project_partial_kernel adds a second row.
    (Tree, preconditioner and trace take 0.2 s on an MI355X.)"""
    n = 263_000
    pts = W.cloud(n, 3, 5)
    st = InterpolantSettings(3, 3, drift=0, nugget=0.05, base_range=0.3, total_sill=1.0)
    t0 = time.perf_counter()
    tree = make_tree(pts, st)
    pre = SchwarzPreconditioner(tree, pts, st, DDMParams())
    rng = np.random.default_rng(8)
    rg = np.concatenate([rng.standard_normal(n), [0.0]])
    z, steps, initial = pre.debug_apply_trace(rg)
    print(f"n = {n}: tree, preconditioner and trace in {time.perf_counter() - t0:.1f} s")
    assert -(-n // W.PROJECT_BLOCKS) == 257 and W.projection_steps(n) == 2 + 8 + 1023
    rows = pre.level_points(0)
    assert np.array_equal(rows, np.arange(n))
    ortho = pre.debug_ortho()

    class _Level:
        def __init__(self, rows):
            self.point_indices = rows
    ddm = [_Level(pre.level_points(li)) for li in range(pre.num_levels)]
    W.check_order(steps, pre.num_levels, 1, z, n)
    stats = W.check_trace(pts, st, ddm, None, ortho, rg, z, steps, initial, only_level=0, order=False)
    print(f"n = {n}, level 0: {stats}")
    # (level 0 is the first step of a sweep: no product, its residual record is "d_res untouched", asserted by check_residual)
    assert stats["residual"] is None and not steps[0]["have_sl"]
    assert_positive(stats, ["projection", "writeback"])
