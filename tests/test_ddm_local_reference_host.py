"""tests/ddm_local_reference.py without a GPU: the restatement agrees with oracle/ddm.py, float64 implementations of the same
operations (LAPACK's factor, a numpy restatement of the kernels' blocked algorithm with its explicit block inverses) pass
the checks, and each check rejects a defect of relative size 1e-12."""
import numpy as np
import pytest
import scipy.linalg as sla

import ddm_local_reference as R
from kernel_reference import LD, U
from oracle import bbfmm_oracle as O
from oracle import ddm as D


def calibration_matrix(m, seed=0, d=3, kid=3, base_range=0.3, nugget=0.05):
    """The calibration input of the bounds: uniform points in the unit cube, Spheroidal, range 0.3, nugget 0.05, no drift.
    Returns (points, float64 matrix as float64 host arithmetic assembles it, packed)."""
    x = R.on_grid(np.random.default_rng(1000 + m + seed).random((m, d)))
    a = np.array(O.kernel_matrix(kid, base_range, 1.0, x, x))
    a[np.diag_indices(m)] += nugget
    a = np.tril(a) + np.tril(a, -1).T
    return x, a, R.pack_lower(a)


def blocked_cholesky_f64(a, right_looking_panels=False):
    """The algorithm of ddm_cholesky_kernel in float64 numpy: 64-column blocks, the diagonal block factorised unblocked,
    its inverse formed column by column from the right, the rows below multiplied by that inverse."""
    a = np.tril(np.array(a, dtype=np.float64))
    m = a.shape[0]
    for jb in range(0, m, 64):
        nb = min(64, m - jb)
        j = slice(jb, jb + nb)
        if jb:
            a[jb:, j] -= a[jb:, :jb] @ a[j, :jb].T
        l11 = np.linalg.cholesky(np.tril(a[j, j]) + np.tril(a[j, j], -1).T)
        a[j, j] = l11
        if jb + nb >= m:
            break
        x = np.zeros((nb, nb))
        for c in range(nb - 1, -1, -1):
            dj = 1.0 / l11[c, c]
            x[c, c] = dj
            x[c + 1:, c] = -dj * (x[c + 1:, c + 1:] @ l11[c + 1:, c])
        a[jb + nb:, j] = a[jb + nb:, j] @ x.T
    return np.tril(a)


def test_pk_round_trips():
    for m in (1, 2, 7, 64, 65):
        idx = np.array([R.pk(r, c, m) for c in range(m) for r in range(c, m)])
        assert np.array_equal(idx, np.arange(m * (m + 1) // 2))          # column by column, no gaps
        a = np.tril(np.random.default_rng(m).standard_normal((m, m)))
        p = R.pack_lower(a)
        for r, c in ((0, 0), (m - 1, 0), (m - 1, m - 1), (m // 2, m // 3)):
            assert p[R.pk(r, c, m)] == a[r, c]
        assert np.array_equal(R.unpack_lower(p, m, np.float64), a)
        assert np.array_equal(R.unpack_symmetric(p, m, np.float64), a + np.tril(a, -1).T)


def test_gamma_and_rows():
    assert R.gamma(1) == pytest.approx(U, rel=1e-15) and R.gamma(1000) > 1000 * U
    rows = R.big_rows(2113)
    assert set(range(2113 - 128, 2113)) <= set(rows) and {0, 63, 64, 1023, 1024, 2047, 2048} <= set(rows)
    assert rows.size < 2113 // 8


# ---------------------------------------------------------------- against oracle/ddm.py
@pytest.mark.parametrize("kid,dim,drift,nugget,rng_,n", [(0, 3, 1, 0.0, 1.0, 70), (1, 2, None, 0.0, 1.0, 90),
                                                          (2, 3, None, 0.0, 1.0, 60), (3, 3, -1, 0.02, 0.3, 80),
                                                          (4, 3, 2, 0.05, 0.3, 75), (6, 1, 1, 0.01, 0.5, 40)])
def test_restatement_agrees_with_the_oracle_domain(kid, dim, drift, nugget, rng_, n):
    rng = np.random.default_rng(7 * kid + dim)
    pts = R.on_grid(rng.random((n + 20, dim)))
    st = D.InterpolantSettings(kid, dim, drift=drift, nugget=nugget, base_range=rng_, total_sill=rng_)
    dom = D.Domain(rng.permutation(n + 20)[:n])
    dom.internal_points_mask = [True] * n
    dom.factorise(pts, st, False)
    assert dom.chol is not None
    k = dom.n_special
    q = dom.q_top if k else np.zeros((0, n))
    m = n - k
    x = pts[np.asarray(dom.overlapping_point_indices)]
    a_ref, bound = R.assembly_reference(kid, rng_, rng_, nugget, x, k, q, where=0)
    # the oracle's float64 factor reproduces the long-double matrix: its assembly error (host budget) + textbook Cholesky
    lo = np.tril(dom.chol[0]).astype(LD)
    low = np.tril(np.ones((m, m), bool))
    err = np.abs(lo @ lo.T - a_ref)
    tol = bound + LD(R.gamma(m + 1)) * (np.abs(lo) @ np.abs(lo).T)
    assert (err[low] <= tol[low]).all(), float((err[low] / tol[low]).max())
    # and its solve is the long-double one within the forward bound
    v = rng.standard_normal(n + 20)
    coef, _ = dom.solve(v[:, None])
    ref, fwd = R.solve_forward(R.pack_lower(np.tril(dom.chol[0])), m, k, q, v[np.asarray(dom.overlapping_point_indices)])
    assert (np.abs(coef[:, 0].astype(LD) - ref) <= fwd).all()
    assert np.abs(coef[:, 0]).max() > 0


# ---------------------------------------------------------------- assembly
def _f64_assembly(kid, rng_, nugget, x, k, q):
    a = np.array(O.kernel_matrix(kid, rng_, rng_, x, x))
    a[np.diag_indices(x.shape[0])] += nugget
    if k == 0:
        return a, a
    a11, a12, a21, a22 = a[:k, :k], a[:k, k:], a[k:, :k], a[k:, k:]
    g = a12 + a11 @ q
    return a22 + q.T @ g + a21 @ q, a


@pytest.mark.parametrize("kid,dim,drift", [(0, 3, 0), (1, 2, 1), (2, 3, 2), (3, 3, 1), (5, 2, 2), (6, 3, -1)])
def test_assembly_check_passes_float64_and_sees_1e12(kid, dim, drift):
    rng = np.random.default_rng(40 + kid)
    n = 90
    pts = R.on_grid(rng.random((n, dim)))
    st = D.InterpolantSettings(kid, dim, drift=drift, nugget=0.03, base_range=0.4, total_sill=0.4)
    dom = D.Domain(np.arange(n))
    dom.internal_points_mask = [True] * n
    dom.factorise(pts, st, False)
    k = dom.n_special
    q = dom.q_top if k else np.zeros((0, n))
    m = n - k
    x = pts[np.asarray(dom.overlapping_point_indices)]
    a_ref, bound = R.assembly_reference(kid, 0.4, 0.4, 0.03, x, k, q, where=0)
    a64, full = _f64_assembly(kid, 0.4, 0.03, x, k, q)
    worst = R.assembly_check(R.pack_lower(a64), m, a_ref, bound)
    assert 0 < worst <= 1.0
    # a relative defect of 1e-12 in an entry is seen wherever cancellation between the terms of Q^T A Q has not already
    # taken those digits (bound < 1e-12 |A_ij|): most entries; for the cubic kernel with a quadratic drift a third of them
    rel = np.where(np.tril(np.ones((m, m), bool)), (bound / np.abs(a_ref)).astype(np.float64), np.inf)
    assert (rel < 1e-12).sum() >= (0.25 if kid == 2 else 0.75) * m * (m + 1) / 2
    order = np.argsort(rel, axis=None)
    sharp = int((rel < 0.5e-12).sum())
    for e in (order[0], order[sharp // 2], order[sharp - 1]):
        r, c = np.unravel_index(int(e), rel.shape)
        bad = a64.copy()
        bad[r, c] *= 1 + 1e-12
        with pytest.raises(AssertionError, match="assembly"):
            R.assembly_check(R.pack_lower(bad), m, a_ref, bound)
    if k:       # one term T_ai Q_aj of the polynomial part dropped from one entry
        bad = a64.copy()
        bad[m - 1, 1] -= full[0, k + m - 1] * q[0, 1]
        assert full[0, k + m - 1] * q[0, 1] != 0
        with pytest.raises(AssertionError, match="assembly"):
            R.assembly_check(R.pack_lower(bad), m, a_ref, bound)


# ---------------------------------------------------------------- factor
FACTOR_SIZES = (65, 321, 705)


@pytest.fixture(scope="module")
def calibration():
    return {m: calibration_matrix(m) for m in FACTOR_SIZES}


@pytest.mark.parametrize("m", FACTOR_SIZES)
def test_factor_check_passes_lapack_and_the_blocked_algorithm(calibration, m):
    _, a, ap = calibration[m]
    lap = R.factor_check(ap, R.pack_lower(np.linalg.cholesky(a)), m)
    blk = R.factor_check(ap, R.pack_lower(blocked_cholesky_f64(a)), m)
    print(f"m = {m}: LAPACK {lap['ratio']:.3f}, blocked with explicit inverses {blk['ratio']:.3f} of the bound; "
          f"kappa_blk {blk['kappa_blk']:.2f}, bound <= {blk['c_eff']:.0f} u |L||L^T|")
    assert lap["kappa_blk"] < 10          # the calibration inputs: well-conditioned diagonal blocks
    assert blk["c_eff"] < 40 * (m + 200)  # the derived bound stays a small multiple of the textbook one there


def test_factor_check_on_selected_rows_of_a_large_matrix():
    m = 2113
    _, a, ap = calibration_matrix(m)
    lo = blocked_cholesky_f64(a)
    rows = R.big_rows(m)
    res = R.factor_check(ap, R.pack_lower(lo), m, big=True, rows=rows)
    assert 0 < res["ratio"] <= 1.0
    last = np.arange(m - 8, m)                         # (the defects below are looked for in the last rows only)

    def ratio(bad):
        return R.factor_check(ap, R.pack_lower(bad), m, big=True, rows=last, check=False)["ratio"]

    bad = lo.copy()
    c = int(np.argmax(np.abs(lo[m - 5, :m - 5])))
    bad[m - 5, c] *= 1 + 1e-12           # in a selected row, the row's largest entry left of the diagonal: seen at 1e-12
    assert ratio(bad) > 1.0
    # in a row that is not selected a defect shows only through column 1500 of the later rows, one product among 1,500:
    # a dropped product L_rk L_ck of the update is seen there, a relative error of the entry from about 1e-9
    assert 1500 not in rows
    bad = lo.copy()
    bad[1500, 700] += lo[1500, 3] * lo[700, 3] / lo[700, 700]
    assert ratio(bad) > 1.0
    bad = lo.copy()
    bad[1500, 1500] *= 1 + 1e-9
    assert ratio(bad) > 1.0


@pytest.mark.parametrize("m", FACTOR_SIZES)
def test_factor_check_sees_small_defects(calibration, m):
    _, a, ap = calibration[m]
    lo = blocked_cholesky_f64(a)
    rng = np.random.default_rng(m)

    def ratio(bad):      # (the rows the defects below touch, not all of R again)
        return R.factor_check(ap, R.pack_lower(bad), m, rows=np.unique(touched), check=False)["ratio"]

    touched = [m // 2, m - 1, 48 if m == 65 else 128]
    assert ratio(lo) <= 1.0
    for _ in range(3):                                   # one entry off by 1e-12
        r = int(rng.integers(1, m))
        c = int(rng.integers(0, r))
        bad = lo.copy()
        bad[r, c] *= 1 + 1e-12
        touched.append(r)
        assert ratio(bad) > 1.0, (r, c)
    bad = lo.copy()                                      # the diagonal too
    bad[m // 2, m // 2] *= 1 + 1e-12
    assert ratio(bad) > 1.0
    # one product L_ik L_jk dropped from one entry of the update: (r, c) is then too large by L_rk L_ck / L_cc
    r, c, k = m - 1, m // 2, 3
    bad = lo.copy()
    bad[r, c] += lo[r, k] * lo[c, k] / lo[c, c]
    assert abs(lo[r, k] * lo[c, k]) > 0 and ratio(bad) > 1.0
    # ... and one doubled
    bad = lo.copy()
    bad[r, c] -= lo[r, k] * lo[c, k] / lo[c, c]
    assert ratio(bad) > 1.0
    # a 16 x 16 sub-tile stored transposed (below the diagonal blocks)
    bad = lo.copy()
    r0 = 48 if m == 65 else 128
    bad[r0:r0 + 16, 16:32] = lo[r0:r0 + 16, 16:32].T
    assert ratio(bad) > 1.0
    touched = np.arange(m)
    with pytest.raises(AssertionError, match="factor"):
        R.factor_check(ap, R.pack_lower(bad), m)


def test_factor_check_wants_exact_zeros_where_nothing_contributes():
    m = 70
    a = np.diag(np.arange(1.0, m + 1))                   # |L| |L^T| is zero off the diagonal
    lo = np.diag(np.sqrt(np.arange(1.0, m + 1)))
    assert R.factor_check(R.pack_lower(a), R.pack_lower(lo), m)["exact_zero_ok"]
    bad = a.copy()
    bad[5, 2] = 1e-300
    with pytest.raises(AssertionError, match="differs from 0"):
        R.factor_check(R.pack_lower(bad), R.pack_lower(lo), m)


def test_ld_cholesky_and_verdicts():
    _, a, _ = calibration_matrix(65)
    lo, ok = R.ld_cholesky(a)
    assert ok and float(np.abs(lo @ lo.T - np.tril(a).astype(LD))[np.tril_indices(65)].max()) < 1e-17
    lo2, ok2 = R.ld_cholesky(a - 0.2 * np.eye(65))       # pushed across zero
    lam, big, margin = R.spectrum_margin(a - 0.2 * np.eye(65))
    assert margin >= R.EIG_MARGIN and lam < 0 and not ok2


# ---------------------------------------------------------------- solve
def _blocked_solve_f64(lo, big):
    """The substitutions in float64: triangular solves per-domain, explicit inverses of 1024-blocks on the large path."""
    m = lo.shape[0]

    def run(rhs):
        if not big:
            return sla.solve_triangular(lo, sla.solve_triangular(lo, rhs, lower=True), lower=True, trans="T")
        y = rhs.copy()
        z = np.zeros(m)
        inv = {}
        for j0 in range(0, m, 1024):
            b = slice(j0, min(m, j0 + 1024))
            inv[j0] = sla.solve_triangular(lo[b, b], np.eye(b.stop - b.start), lower=True)
            z[b] = inv[j0] @ y[b]
            y[b.stop:] -= lo[b.stop:, b] @ z[b]
        g = np.zeros(m)
        for j0 in range(((m - 1) // 1024) * 1024, -1, -1024):
            b = slice(j0, min(m, j0 + 1024))
            g[b] = inv[j0].T @ z[b]
            z[:j0] -= lo[b, :j0].T @ g[b]
        return g
    return run


@pytest.mark.parametrize("m,k,big", [(65, 0, False), (321, 4, False), (705, 10, False), (2113, 4, True)])
def test_solve_check_passes_float64_and_sees_1e12(m, k, big):
    _, a, _ = calibration_matrix(m)
    lo = np.linalg.cholesky(a)
    rng = np.random.default_rng(m + k)
    q = rng.standard_normal((k, m))
    d = rng.standard_normal(k + m)
    rhs = (q.T @ d[:k] + d[k:]) if k else d
    g = _blocked_solve_f64(lo, big)(rhs)
    out = np.concatenate([q @ g, g])
    lp = R.pack_lower(lo)
    res = R.solve_check(lp, m, k, q, d, out, big=big)
    print(f"m = {m}, k = {k}, big = {big}: {res}")
    assert 0 < res["ratio"] <= 1.0
    i = int(np.argmax(np.abs(g)))
    bad = out.copy()
    # (the large path's bound carries gamma_1025 W2 of the 1024-blocks' explicit inverses: a defect is seen from 1e-10)
    bad[k + i] *= 1 + (1e-10 if big else 1e-12)
    assert R.solve_check(lp, m, k, q, d, bad, big=big, check=False)["ratio"] > 1.0
    with pytest.raises(AssertionError, match="solve"):
        R.solve_check(lp, m, k, q, d, bad, big=big)
    bad = out.copy()                                     # one column of the factor skipped in the forward sweep
    rhs2 = rhs.copy()
    z = sla.solve_triangular(lo, rhs2, lower=True)
    z[m - 1] += lo[m - 1, 2] * z[2] / lo[m - 1, m - 1]
    bad[k:] = sla.solve_triangular(lo, z, lower=True, trans="T")
    assert R.solve_check(lp, m, k, q, d, bad, big=big, check=False)["ratio"] > 1.0
    if k:
        bad = out.copy()
        bad[0] *= 1 + 1e-12
        assert R.solve_check(lp, m, k, q, d, bad, big=big, check=False)["ratio_special"] > 1.0


def test_forward_bound_and_inverse_check():
    m, k = 130, 4
    _, a, _ = calibration_matrix(m)
    lo = np.linalg.cholesky(a)
    rng = np.random.default_rng(3)
    q = rng.standard_normal((k, m))
    d = rng.standard_normal(k + m)
    g = sla.cho_solve((lo, True), q.T @ d[:k] + d[k:])
    ref, fwd = R.solve_forward(R.pack_lower(lo), m, k, q, d)
    out = np.concatenate([q @ g, g])
    assert (np.abs(out.astype(LD) - ref) <= fwd).all()
    out[k + 7] *= 1 + 1e-11
    assert not (np.abs(out.astype(LD) - ref) <= fwd).all()
    # the stored inverse of an indefinite matrix
    b = a - 0.2 * np.eye(m)
    assert R.spectrum_margin(b)[2] >= R.EIG_MARGIN
    inv = np.linalg.inv(b)
    inv = 0.5 * (inv + inv.T)
    ratio, x1, kappa = R.inverse_check(R.pack_lower(inv), b, m)
    assert ratio <= 1.0
    assert float(np.abs((x1 @ b.astype(LD)) - np.eye(m)).max()) < 1e-15 * kappa
    bad = inv.copy()
    bad[np.tril_indices(m)] *= 1 + 1e-9 * rng.standard_normal(m * (m + 1) // 2)
    assert R.inverse_check(R.pack_lower(bad), b, m, check=False)[0] > 1.0
    x = R.refined_solve(b, d[:m])
    assert float(np.abs(b.astype(LD) @ x - d[:m]).max()) < 1e-17 * kappa
