"""The local solvers of the Schwarz preconditioner (csrc/ddm_kernels.hip) on prescribed domains, through the debug hook
(bbfmm_ddm_debug_level_*), against the long-double restatement and the derived bounds of tests/ddm_local_reference.py: the
assembled Q^T A Q entry by entry, the factor through the exact residual A - L L^T, the substitutions through their backward
error, the fallback verdicts, the rows a solve leaves alone, and bitwise reproducibility -- at every block edge of the
kernels (tests/ddm_local_cases.py)."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import ddm_local_cases as C
import ddm_local_reference as R
from kernel_reference import LD, U


class Built:
    """A level, what the hook copies out of it, and one solve with all_points = 1 (shared by the tests of a case)."""

    def __init__(self, pts, doms, st, seed=1, solve=True):
        self.pts, self.doms, self.st = pts, doms, st
        self.level = C.make_level(pts, doms, st)
        self.assembled = self.level.assembled()
        self.factor = self.level.factor()
        self.values = np.random.default_rng(seed).standard_normal(pts.shape[0])
        self.sentinel = np.full(pts.shape[0], C.SENTINEL)
        self.out = self.level.solve(self.values, self.sentinel, True) if solve else None


def check_layout(b, expected_k=None):
    lv = b.level
    for i, (idx, mask) in enumerate(b.doms):
        assert sorted(lv.indices[i]) == sorted(idx), "the reordered indices are a permutation of the domain's"
        given = dict(zip(idx.tolist(), np.asarray(mask, bool).tolist()))
        assert [given[g] for g in lv.indices[i].tolist()] == lv.internal[i].tolist(), "the internal mask follows its points"
        assert lv.q[i].shape == (lv.k[i], lv.m[i]) and lv.m[i] == len(idx) - lv.k[i]
        if expected_k is not None:
            assert lv.k[i] == expected_k[i], (i, lv.k[i], expected_k[i])


# ---------------------------------------------------------------- the per-domain path, every block edge
@pytest.fixture(scope="module")
def flagship():
    pts, doms, st, ks = C.flagship()
    b = Built(pts, doms, st)
    check_layout(b, ks)
    assert not b.level.is_big and b.level.mode == [0] * len(doms) and b.level.n_fallback == 0
    assert tuple(b.level.m[:len(C.M_ALL)]) == C.M_ALL and b.level.m[len(C.M_ALL):] == [40, 50]
    return b


def test_assembly_every_entry_of_every_size(flagship):
    b = flagship
    worst = [C.check_assembly(b.level, b.pts, b.st, b.assembled, i) for i in range(len(b.doms))]
    print("assembly, |A_dev - A| / bound per domain:", np.round(worst, 3))
    assert max(worst) > 0
    # the domain with duplicated points: r2 = 0 off the diagonal
    x = C.domain_points(b.level, b.pts, len(b.doms) - 1)
    d2 = ((x[:, None, :] - x[None, :, :]) ** 2).sum(axis=2)
    assert (d2[np.triu_indices(x.shape[0], 1)] == 0).sum() >= 3


def test_factor_residual_at_every_size(flagship):
    b = flagship
    res = [C.check_factor(b.level, b.assembled, b.factor, i) for i in range(len(b.doms))]
    print("factor, |A - L L^T| / bound per domain:", np.round([r["ratio"] for r in res], 3),
          "kappa_blk", np.round([r["kappa_blk"] for r in res], 1))
    assert max(r["kappa_blk"] for r in res) < 100, "calibration inputs: well-conditioned diagonal blocks"


def test_solve_backward_error_and_untouched_rows(flagship):
    b = flagship
    lv = b.level
    n = b.pts.shape[0]
    res = [C.check_solve(lv, b.factor, b.values, b.out, i) for i in range(len(b.doms))]
    print("solve, backward error / bound per domain:", np.round([r["ratio"] for r in res], 3),
          "special rows:", np.round([r["ratio_special"] for r in res], 3))
    assert C.rows_written(lv, n, True).all() and not (b.out == C.SENTINEL).any()
    # all_points = 0: the internal rows get the same bits, every other row keeps the caller's
    part = lv.solve(b.values, b.sentinel, False)
    w = C.rows_written(lv, n, False)
    assert 0 < w.sum() < n
    assert C.same_bits(part[w], b.out[w])
    assert C.same_bits(part[~w], b.sentinel[~w])


@pytest.mark.parametrize("dim,drift,k", [(3, -1, 0), (3, 0, 1), (3, 2, 10), (1, 1, 2), (1, 2, 3), (2, 1, 3), (2, 2, 6)])
def test_every_polynomial_size(dim, drift, k):
    pts, doms, st, ks = C.sized(100 + 10 * dim + k, dim, drift, C.M_FEW, k)
    b = Built(pts, doms, st)
    check_layout(b, ks)
    assert b.level.mode == [0] * len(doms) and tuple(b.level.m) == C.M_FEW
    for i in range(len(doms)):
        C.check_assembly(b.level, pts, st, b.assembled, i)
        C.check_factor(b.level, b.assembled, b.factor, i)
        C.check_solve(b.level, b.factor, b.values, b.out, i)


@pytest.mark.parametrize("kid,drift,nugget,base_range", [(0, 0, 0.0, 1.0), (1, 1, 0.0, 1.0), (2, 1, 0.0, 1.0), (3, -1, 0.02, 0.3),
                                                         (4, 0, 0.02, 0.3), (5, 1, 0.02, 0.5), (6, 2, 0.02, 0.4)])
def test_every_kernel_id(kid, drift, nugget, base_range):
    """Linear, ThinPlateSpline and Cubic with their drift: Q^T A Q is badly conditioned (up to 1e9), the factor's bound is
    not -- it depends on the diagonal blocks."""
    k = {-1: 0, 0: 1, 1: 4, 2: 10}[drift]
    pts, doms, st, ks = C.sized(200 + kid, 3, drift, C.M_KERNELS, k, kid=kid, nugget=nugget, base_range=base_range,
                                total_sill=base_range)
    b = Built(pts, doms, st)
    check_layout(b, ks)
    assert b.level.mode == [0] * len(doms), "positive definite in long double (checked below): no fallback expected"
    for i in range(len(doms)):
        _, ok = R.ld_cholesky(C.reference_matrix(b.level, pts, st, i))
        assert ok
        C.check_assembly(b.level, pts, st, b.assembled, i)
        f = C.check_factor(b.level, b.assembled, b.factor, i)
        s = C.check_solve(b.level, b.factor, b.values, b.out, i)
        print(f"kernel {kid} m = {b.level.m[i]}: factor {f['ratio']:.3f} (kappa_blk {f['kappa_blk']:.3g}), solve {s['ratio']:.3f}")


def test_512_domains_take_the_narrow_column_split():
    pts, doms, st, ks = C.many_small()
    assert len(doms) == 512
    b = Built(pts, doms, st)
    check_layout(b, ks)
    assert b.level.mode == [0] * 512
    for i in list(range(0, 512, 3)) + [511]:
        C.check_assembly(b.level, pts, st, b.assembled, i)
        C.check_factor(b.level, b.assembled, b.factor, i)
        C.check_solve(b.level, b.factor, b.values, b.out, i)


def test_overlapping_domains_write_their_internal_rows_only():
    pts, doms, st = C.overlapping()
    b = Built(pts, doms, st, solve=False)
    check_layout(b)
    lv = b.level
    n = pts.shape[0]
    out = lv.solve(b.values, b.sentinel, False)
    w = C.rows_written(lv, n, False)
    assert w.sum() == 450 and C.same_bits(out[~w], b.sentinel[~w])
    for i in range(3):
        C.check_factor(lv, b.assembled, b.factor, i)
        idx, internal = lv.indices[i], lv.internal[i]
        ref, fwd = R.solve_forward(b.factor[i], lv.m[i], lv.k[i], lv.q[i], b.values[idx])
        err = np.abs(out[idx[internal]].astype(LD) - ref[internal])
        assert (err <= fwd[internal]).all(), float((err / fwd[internal]).max())
        assert float((err / fwd[internal]).max()) > 0


# ---------------------------------------------------------------- the fallback
def test_fallback_verdicts_inverses_and_solutions():
    pts, doms, st, tight = C.fallback()
    b = Built(pts, doms, st)
    check_layout(b, [1] * len(doms))
    lv = b.level
    verdict = []
    for i in range(len(doms)):
        a = C.reference_matrix(lv, pts, st, i)
        lam, _, margin = R.spectrum_margin(a.astype(np.float64))
        assert margin >= R.EIG_MARGIN, (i, margin)                 # the reference's verdict is not marginal
        _, ok = R.ld_cholesky(a)
        assert ok == (lam > 0)
        verdict.append(0 if ok else 1)
    assert verdict == [1 if t else 0 for t in tight], "the case mixes both kinds as designed"
    assert lv.mode == verdict and lv.n_fallback == sum(verdict) and not lv.lu_taken
    for i in range(len(doms)):
        C.check_assembly(lv, pts, st, b.assembled, i)
        if lv.mode[i] == 0:
            C.check_factor(lv, b.assembled, b.factor, i)
            C.check_solve(lv, b.factor, b.values, b.out, i)
            continue
        m, k, idx = lv.m[i], lv.k[i], lv.indices[i]
        a = C.reference_matrix(lv, pts, st, i)
        ratio, ainv, kappa = R.inverse_check(b.factor[i], a, m)
        rhs, _ = R._rhs(lv.q[i], k, b.values[idx])
        g = ainv @ rhs
        scale = float(np.linalg.norm(ainv.astype(np.float64), 2) * np.linalg.norm(rhs.astype(np.float64)))
        err = float(np.linalg.norm((b.out[idx[k:]].astype(LD) - g).astype(np.float64)))
        tol = (8 * m * kappa + m ** 1.5) * U * scale
        print(f"mode 1, m = {m}: inverse {ratio:.3g} of its bound, solution {err / tol:.3g} (kappa {kappa:.3g})")
        assert err <= tol
        lam_s = lv.q[i].astype(LD) @ b.out[idx[k:]].astype(LD)
        assert (np.abs(b.out[idx[:k]].astype(LD) - lam_s) <=
                R.gamma(-(-m // 256) + 9) * (np.abs(lv.q[i]) @ np.abs(b.out[idx[k:]]))).all()


def _rocsolver_loads():
    for name in ("librocsolver.so.0", "librocsolver.so", "/opt/rocm/lib/librocsolver.so"):
        try:
            ctypes.CDLL(name)
            return True
        except OSError:
            pass
    return False


def test_large_indefinite_domain_takes_the_pivoted_lu():
    if not _rocsolver_loads():
        pytest.skip("rocSOLVER cannot be loaded on this machine: the pivoted LU of a large domain is unavailable")
    m, k = 2113, 1
    pts = C.two_clusters(np.random.default_rng(77), m + k, 2e-6)
    doms = [(np.arange(m + k), np.ones(m + k, bool))]
    st = C.settings(drift=0, nugget=-0.05)
    b = Built(pts, doms, st)
    lv = b.level
    assert lv.is_big and lv.m == [m]
    a = C.reference_matrix(lv, pts, st, 0)
    lam, _, margin = R.spectrum_margin(a.astype(np.float64))
    assert margin >= R.EIG_MARGIN and lam < 0
    kappa = 1.0 / margin                                           # (symmetric: |lambda|_max / |lambda|_min)
    assert lv.lu_taken
    rows = R.big_rows(m)
    C.check_assembly(lv, pts, st, b.assembled, 0, rows=rows)
    assert C.same_bits(b.assembled[0], b.factor[0]), "the packed matrix is assembled again for the LU"
    idx = lv.indices[0]
    rhs, _ = R._rhs(lv.q[0], k, b.values[idx])
    g = R.refined_solve(a, rhs)
    err = float(np.linalg.norm((b.out[idx[k:]].astype(LD) - g).astype(np.float64)))
    tol = 8 * m * U * kappa * float(np.linalg.norm(g.astype(np.float64)))
    print(f"pivoted LU, m = {m}: error {err / tol:.3g} of the bound (kappa {kappa:.3g})")
    assert err <= tol


# ---------------------------------------------------------------- one large domain
@pytest.mark.parametrize("m,k", C.BIG_CASES)
def test_large_domain_path(m, k):
    pts, doms, st = C.big(m, k)
    b = Built(pts, doms, st)
    check_layout(b, [k])
    lv = b.level
    assert lv.is_big and lv.m == [m] and not lv.lu_taken and lv.mode == [0]
    rows = R.big_rows(m)
    a = C.check_assembly(lv, pts, st, b.assembled, 0, rows=rows)
    f = C.check_factor(lv, b.assembled, b.factor, 0, rows=rows)
    s = C.check_solve(lv, b.factor, b.values, b.out, 0)
    print(f"m = {m}, k = {k}: assembly {a:.3f}, factor {f['ratio']:.3f} (kappa_blk {f['kappa_blk']:.2f}), "
          f"solve {s['ratio']:.3g} (kappa_1024 {s['kappa_1024']:.1f}), special {s['ratio_special']:.3f}")
    assert f["kappa_blk"] < 100 and s["kappa_1024"] < 1e3, "calibration inputs"
    n = pts.shape[0]
    part = lv.solve(b.values, b.sentinel, False)
    w = C.rows_written(lv, n, False)
    assert 0 < w.sum() < n - 30
    assert C.same_bits(part[w], b.out[w]) and C.same_bits(part[~w], b.sentinel[~w])
    wa = C.rows_written(lv, n, True)
    assert wa.sum() == n - 30 and C.same_bits(b.out[~wa], b.sentinel[~wa])


# ---------------------------------------------------------------- determinism
@pytest.mark.parametrize("path", ["per_domain", "large"])
def test_two_builds_and_two_solves_give_the_same_bits(path):
    if path == "per_domain":
        pts, doms, st, _ = C.sized(7, 3, 1, (33, 65, 321, 385, 641), 4)
    else:
        pts, doms, st = C.big(2177, 4)
    a, b = Built(pts, doms, st), Built(pts, doms, st)
    assert a.level.is_big == (path == "large")
    for i in range(len(doms)):
        assert C.same_bits(a.assembled[i], b.assembled[i])
        assert C.same_bits(a.factor[i], b.factor[i])
    assert C.same_bits(a.out, b.out)
    assert C.same_bits(a.level.solve(a.values, a.sentinel, True), a.out)
    assert C.same_bits(a.level.solve(a.values, a.sentinel, False), b.level.solve(a.values, a.sentinel, False))
