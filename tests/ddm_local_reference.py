"""The local solvers of the Schwarz preconditioner (csrc/ddm_kernels.hip) restated in extended precision, and the bounds
their outputs are held to.  A plain helper module (no tests), shared by test_ddm_local_reference_host.py (no GPU),
test_gpu_ddm_local.py and scripts/ddm_local_accuracy.py.  Q, the point order and k are INPUTS (the host polynomial part,
prepare_domain, is not under test): they come from the debug hook (ferreus_rbf_rs_amd.ddm.DebugLevel).

Everything that is compared is formed in numpy longdouble (64-bit significand, eps 1.08e-19); the BOUNDS are formed in
float64 where a matrix product is large (a bound needs three digits, not nineteen).  u = 2^-53, gamma_n = n u / (1 - n u).
All bounds are first order in u and COUNTED from the code path, as the pair-kernel tolerance was; none is fitted.

Storage.  A domain's reduced matrix and its factor are packed lower triangles, column by column: element (r, c), r >= c,
of an m x m matrix lies at pk(r, c, m) = c m - c (c - 1) / 2 + (r - c).

1. ASSEMBLY (ddm_prep_kernel, ddm_assemble_kernel)
       A_ij = phi_ij + nugget [i == j] + sum_a (Q_ai G_aj + T_ai Q_aj),   G = T + A11 Q,   T_aj = phi(s_a, x_j),
       A11 = phi(s, s) + nugget I          (s: the k special points, x: the m others)
   Test coordinates lie on a 2^-30 grid, so coordinate differences are exact and the squared distance carries the three
   squares and two sums: with the pointwise budget (a, b) of kernel_pointwise.py (|g_dev - g| <= u (a |g| + b |x g'|)) a
   device kernel value is off by at most  e(phi) = u (a |phi| + (b + 4) |x phi'|)  (4 as in test_gpu_pair_kernels.py).
   A term Q_ai A11_ab Q_bj passes the product A11 Q (1), up to k sums of the row of G (k), T + (.) (1), the product with
   Q_ai (1) and up to 2k sums into A_ij: 3k + 3 <= 4k + 2 roundings for k >= 1; T_ai Q_aj and phi_ij + nugget pass fewer.  So
       |A_dev - A|_ij <= e(phi_ij) + sum_a (|Q_ai| eG_aj + e(T_ai) |Q_aj|) + gamma_{4k+2} S_ij
       eG_aj = e(T_aj) + sum_b e(A11_ab) |Q_bj|
       S_ij  = |phi_ij| + |nugget| [i == j] + sum_a (|Q_ai| (|T_aj| + sum_b |A11_ab| |Q_bj|) + |T_ai| |Q_aj|)
   whatever the compiler contracts into FMAs.  Every entry of every domain is compared.

2. FACTOR (ddm_cholesky_kernel; big_diag / big_panel / big_syrk for one domain of more than 2048 rows)
   R = A - L L^T with A the device's OWN assembled matrix and L its factor, exact in long double.  The kernels are not
   textbook Cholesky.  For the block column J = [jb, jb + 64):
   (a) S = A[jb.., J] - sum_{k < jb} L[., k] L[J, k]^T on MFMA accumulators: a chain of jb FMAs in some order (gamma_jb on
       sum_{k<jb} |L_rk| |L_ck|) and the subtraction (u |S|).  Per-domain path: one subtraction.  Large path: the trailing
       matrix is updated once per 128-column panel, jb / 128 + 1 subtractions of partial sums that are at most
       2 (|L| |L^T|)_rc: 2 u (jb / 128 + 1) more.
   (b) the 64 x 64 diagonal block is factorised unblocked in LDS: |L11 L11^T - S11| <= gamma_65 |L11| |L11^T| (Higham,
       Accuracy and Stability of Numerical Algorithms, 2nd ed., Thm 10.3, any order of the sums).
       (a) + (b):  |R_rc| <= gamma_{jb+66} (|L| |L^T|)_rc for r, c in J, and the same term bounds step (a) below the block.
   (c) the rows below: L21 = fl(S21 X^T) with X the EXPLICIT inverse of L11, computed column by column from the right
       (X[j+1.., j] = -X[j+1.., j+1..] L11[j+1.., j] / l_jj, LAPACK's trti2 order; Higham section 14.2, method 2).  That
       recurrence is X L11 = I solved for X, so its LEFT residual is small, |X L11 - I| <= gamma_65 |X| |L11|; the panel
       needs the RIGHT one, F = L11 X - I = L11 (X L11 - I) L11^-1, |F| <= gamma_65 |L11| |X| |L11| |X|.  The product adds
       D with |D| <= gamma_64 |S21| |X^T|.  Then
           L21 L11^T - S21 = S21 F^T + D L11^T,    |S21| <= |L21| |L11^T| to first order,
           |R21| <= gamma_{jb+66 (+ ...)} (|L| |L^T|)_21 + |L21| (gamma_65 M2 + gamma_64 M1)^T,
           M1 = |L11| |X| |L11|,   M2 = M1 |X| |L11|          (64 x 64, formed in the test from the device's L11)
       M1 and M2 are what the explicit inverse costs: they grow with the condition of the diagonal BLOCK, not of A.  Had
       the panel been a triangular solve, M1 = M2 = |L11| and the whole bound gamma_{jb+66+129} |L| |L^T|.  A scalar form
       |R| <= c(m, kappa) u |L| |L^T| follows with kappa = max_{c >= k} M2_ck / |L11_ck|, c = m + 2 + 129 kappa, but one
       entry of L11 near zero makes that kappa huge for every entry of the block; the matrix form is evaluated instead.
       The first-order step drops terms of relative size gamma_65 kappa_blk^2; kappa_blk, the largest 2-norm condition
       number of the 64 x 64 diagonal blocks of the factor, is measured and asserted to be at most KAPPA_BLK_MAX = 1e5
       (7e-5), and the panel term carries a factor 1 + 2^-10 for it.
   Where (|L| |L^T|)_rc is exactly 0, R_rc must be exactly 0.  m <= ~700: all of R.  Large path: whole rows only -- the
   last 128, r mod 64 in {0, 63}, r mod 1024 in {0, 1023} (big_rows): a wrong L_rc shows in row r and in column r of every
   later row, so the last rows see every row above them.

3. SOLVE (ddm_solve_kernel; the big_blk_* kernels), for the device's factor L and its output gamma (rows of the
   non-special points) and lambda_s (rows of the special points):
       rhs = Q^T d_s + d_ns: k products and k sums, gamma_{k+1} (|Q^T| |d_s| + |d_ns|)   (k = 0: exact)
   Per-domain path: two substitutions in panels of 32.  Whatever the order of the sums, a substitution solves
   (L + dL) z = rhs with |dL| <= gamma_{m+1} |L| (Higham Thm 8.5), so
       |L L^T gamma - rhs| <= (2 gamma_{m+1} + gamma_{m+1}^2) |L| |L^T| |gamma|.
   Large path: blocks of 1024.  X = T^-1 of a diagonal block T comes from forward substitutions on unit vectors
   (big_block_inverse_kernel), |T X - I| <= gamma_1025 |T| |X|; z_B = fl(X y_B) adds gamma_1024 |X| |y_B|:
       |T z_B - y_B| <= 2 gamma_1025 W |z_B|,  W = |T| |X| |T|.
   The back sweep multiplies by X^T and needs the LEFT residual X T - I = X (T X - I) T:
       |T^T g_B - z_B| <= gamma_1025 (W2 + W)^T |g_B|,  W2 = W |X| |T|.
   A block's update of the entries still to be solved is a chain of at most 1024 FMAs in a fixed order and one
   subtraction, at most three times per entry, of partial sums below 2 |L| |z|: (gamma_1025 + 6 u) |L| |z|.  Together
       |L z - rhs| <= Kf |z|,  Kf = (gamma_1025 + 6 u) |L| + 2 gamma_1025 blockdiag(W)
       |L^T g - z| <= Kb |g|,  Kb = (gamma_1025 + 6 u) |L^T| + gamma_1025 blockdiag(W2 + W)^T
       |L L^T g - rhs| <= |L| Kb |g| + Kf |L^T| |g|
   -- the condition of the 1024 x 1024 diagonal blocks enters through W and W2 (kappa_1024 is reported with the result).
       lambda_s = Q gamma: a product, a chain of ceil(m / 256) sums per thread and an 8-level tree:
       |lambda_s - Q gamma| <= gamma_{ceil(m/256)+9} |Q| |gamma|.
   The scatter copies.  Rows the level does not write keep the caller's sentinel bit for bit.
   Where only some rows of gamma can be seen (all_points = 0), the backward bound b is turned into a forward one,
   |gamma - gamma_ref| <= |(L L^T)^-1| b, with gamma_ref the long-double substitution through the same L.

4. FALLBACK.  The device's verdict per domain (mode; for one large domain: the pivoted LU was taken) must equal "the
   long-double Cholesky of the long-double matrix fails".  The test matrices keep every eigenvalue at least EIG_MARGIN =
   1e-6 of the largest away from zero (asserted), so the verdict is not marginal: a perturbation of 1e-13 ||A|| cannot
   change it, and for the one large domain it is read off the float64 spectrum.
   mode 1 stores the inverse from Gauss-Jordan elimination with partial pivoting on the host (symmetrised).  Its forward
   error is normwise: ||Xhat - A^-1||_2 <= c_m u kappa_2(A) ||A^-1||_2 (Higham section 14.4, eq. 14.31), c_m a small
   multiple of m times the growth factor.  c_m = 8 m is used: every entry is the end of at most m eliminations of two
   roundings each, and growth factors above 4 are not met with partial pivoting on matrices of this kind (Higham section
   9.4).  The solve multiplies: ||gamma - A^-1 rhs||_2 <= (8 m kappa_2 + m^1.5) u ||A^-1||_2 ||rhs||_2.
   The pivoted LU of the large domain is backward stable with the same kind of constant:
   ||gamma - A^-1 rhs||_2 <= 8 m u kappa_2(A) ||gamma||_2; the reference solution is a float64 solve refined twice with
   long-double residuals (error kappa^2 u^2, far below the bound while kappa u << 1).
"""
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import kernel_pointwise as KP
import kernel_reference as KR
from kernel_reference import LD, U

CB = 64                  # block-column width of the factorisations
BB = 1024                # block width of the large path's substitutions
BIG_M = 2048             # one domain with more rows than this takes the multi-launch path
KAPPA_BLK_MAX = 1e5
EIG_MARGIN = 1e-6
GRID = 2.0 ** -30


def gamma(n):
    return n * U / (1.0 - n * U)


def on_grid(x):
    """Coordinates rounded to the 2^-30 grid (|x| < 2^20: differences and their squares are exact in long double)."""
    return np.round(np.asarray(x, dtype=np.float64) / GRID) * GRID


# ------------------------------------------------------------------ packed storage
def pk(r, c, m):
    return c * m - (c * (c - 1)) // 2 + (r - c)


def unpack_lower(packed, m, dtype=LD):
    """m x m, zero above the diagonal."""
    packed = np.asarray(packed)
    assert packed.shape == (m * (m + 1) // 2,)
    c, r = np.triu_indices(m)          # (c, r) runs column by column down the lower triangle
    out = np.zeros((m, m), dtype=dtype)
    out[r, c] = packed
    return out


def pack_lower(a):
    m = a.shape[0]
    c, r = np.triu_indices(m)
    return np.ascontiguousarray(a[r, c])


def unpack_symmetric(packed, m, dtype=LD):
    lo = unpack_lower(packed, m, dtype)
    return lo + np.tril(lo, -1).T


# ------------------------------------------------------------------ 1. assembly
def _pad3(x):
    x = np.atleast_2d(np.asarray(x, dtype=np.float64))
    return np.hstack([x, np.zeros((x.shape[0], 3 - x.shape[1]))]) if x.shape[1] < 3 else x


def _kernel_block(where, kid, base_range, total_sill, xa, xb):
    """(phi, |phi|, e(phi)) of the pairs xa x xb in long double."""
    p = KR.Params(kid, base_range, total_sill)
    dn = KR.Dense(kid, base_range, total_sill, xa, xb)
    a, b = KP.coefficients(where, p, "value", dn.r2)
    return dn.value, dn.abs_value, LD(U) * (a * dn.abs_value + (b + 4.0) * dn.abs_x_dvalue)


def assembly_reference(kid, base_range, total_sill, nugget, x, k, q, rows=None, where=1):
    """Q^T A Q of one domain and its per-entry bound.  x: the domain's points in its point order (special points first),
    q: k x m.  Returns (A, bound) as len(rows) x m long-double arrays (rows: all), entries above the diagonal included.
    where: 1 the device's kernel functions, 0 the host's (float64 libm)."""
    x = _pad3(x)
    s, xn = x[:k], x[k:]
    m = xn.shape[0]
    rows = np.arange(m) if rows is None else np.asarray(rows)
    nug = LD(np.float64(nugget))
    eye = (rows[:, None] == np.arange(m)[None, :])
    a, sabs, e = _kernel_block(where, kid, base_range, total_sill, xn[rows], xn)
    a = a + nug * eye
    sabs = sabs + abs(nug) * eye
    if k:
        ql = np.asarray(q, dtype=np.float64).astype(LD).reshape(k, m)
        aq = np.abs(ql)
        t, at, et = _kernel_block(where, kid, base_range, total_sill, s, xn)
        a11, aa11, ea11 = _kernel_block(where, kid, base_range, total_sill, s, s)
        a11 = a11 + nug * np.eye(k, dtype=LD)
        aa11 = aa11 + abs(nug) * np.eye(k, dtype=LD)
        g = t + a11 @ ql
        gabs = at + aa11 @ aq
        eg = et + ea11 @ aq
        a = a + ql[:, rows].T @ g + t[:, rows].T @ ql
        sabs = sabs + aq[:, rows].T @ gabs + at[:, rows].T @ aq
        e = e + aq[:, rows].T @ eg + et[:, rows].T @ aq
    return a, e + LD(gamma(4 * k + 2)) * sabs


def assembly_check(a_packed, m, a_ref, bound, rows=None):
    """Largest |A_dev - A| / bound over the lower triangle of the given rows; asserts it is at most 1."""
    rows = np.arange(m) if rows is None else np.asarray(rows)
    dev = unpack_lower(a_packed, m, np.float64)[rows].astype(LD)
    low = np.arange(m)[None, :] <= rows[:, None]
    err = np.abs(dev - a_ref)
    assert np.isfinite(dev[low]).all(), "assembled matrix is not finite"
    zero = low & (bound == 0)
    assert (err[zero] == 0).all(), "an entry with a zero bound differs"
    ok = low & (bound > 0)
    ratio = np.zeros(err.shape)
    ratio[ok] = (err[ok] / bound[ok]).astype(np.float64)
    i, j = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    worst = float(ratio[i, j])
    assert worst <= 1.0, f"assembly: |A_dev - A| = {worst:.3g} x bound at ({int(rows[i])}, {j}) of m = {m}"
    return worst


# ------------------------------------------------------------------ 2. factor
def ld_cholesky(a):
    """Left-looking Cholesky in long double of a symmetric matrix (lower triangle read).  Returns (L, ok); ok is False
    when a pivot is not positive (L is then meaningless)."""
    a = np.asarray(a, dtype=LD)
    m = a.shape[0]
    lo = np.zeros((m, m), dtype=LD)
    for j in range(m):
        v = a[j:, j] - lo[j:, :j] @ lo[j, :j]
        if not v[0] > 0:
            return lo, False
        lo[j:, j] = v / np.sqrt(v[0])
    return lo, True


def big_rows(m):
    """The rows of the large path whose residual is formed."""
    r = np.arange(m)
    keep = (r >= m - 128) | np.isin(r % CB, (0, CB - 1)) | np.isin(r % BB, (0, BB - 1))
    return r[keep]


def _tri_inv(t):
    import scipy.linalg as sla
    return sla.solve_triangular(t, np.eye(t.shape[0]), lower=True)


def factor_check(a_packed, l_packed, m, big=False, rows=None, check=True):
    """R = A - L L^T on the rows given (all) against the bound of section 2.  Returns dict(ratio, kappa_blk, c_eff,
    at): ratio = the largest |R| / bound, c_eff = the largest bound / (u |L| |L^T|), at = (r, c) of the largest ratio.
    check = False: measure only (the host tests that show a defect is seen)."""
    lo = unpack_lower(l_packed, m, LD)
    a = unpack_lower(a_packed, m, LD)
    l64 = lo.astype(np.float64)
    al = np.abs(l64)
    rows = np.arange(m) if rows is None else np.asarray(rows)

    def block_column(jb):
        nb = min(CB, m - jb)
        cols = np.arange(jb, jb + nb)
        rr = rows[rows >= jb]
        l11 = l64[np.ix_(cols, cols)]
        kappa = float(np.linalg.cond(l11))
        if rr.size == 0:
            return 0.0, (0, 0), 0.0, kappa, True
        kk = jb + nb
        res = np.abs(a[np.ix_(rr, cols)] - lo[rr, :kk] @ lo[cols, :kk].T)
        den = al[rr, :kk] @ al[cols, :kk].T
        steps = jb + CB + 2 + (2 * (jb // (2 * CB) + 1) if big else 0)
        bnd = gamma(steps) * den
        below = rr >= jb + nb
        if below.any():             # (nb = 64: the last block column has no rows below)
            x = np.abs(_tri_inv(l11))
            a11 = np.abs(l11)
            m1 = a11 @ x @ a11
            m2 = m1 @ x @ a11
            bnd[below] += (1.0 + 2.0 ** -10) * (al[np.ix_(rr[below], cols)] @ (gamma(CB + 1) * m2 + gamma(CB) * m1).T)
        low = cols[None, :] <= rr[:, None]
        zero = low & (den == 0)
        zero_ok = bool((res[zero] == 0).all())
        ok = low & (den > 0)
        if not ok.any():
            return 0.0, (0, 0), 0.0, kappa, zero_ok
        ratio = np.zeros(res.shape)
        ratio[ok] = (res[ok] / bnd[ok]).astype(np.float64)
        i, j = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
        return float(ratio[i, j]), (int(rr[i]), int(cols[j])), float((bnd[ok] / (U * den[ok])).max()), kappa, zero_ok

    # (numpy's long-double products run outside the interpreter lock: the block columns are formed side by side)
    with ThreadPoolExecutor(max_workers=16) as pool:
        parts = list(pool.map(block_column, range(0, m, CB)))
    worst, at = max((p[0], p[1]) for p in parts)
    c_eff = max(p[2] for p in parts)
    kappa_blk = max(p[3] for p in parts)
    exact_zero_ok = all(p[4] for p in parts)
    out = {"ratio": worst, "kappa_blk": kappa_blk, "c_eff": c_eff, "at": at, "exact_zero_ok": exact_zero_ok}
    if check:
        assert np.isfinite(l64).all(), "factor is not finite"
        assert kappa_blk <= KAPPA_BLK_MAX, f"kappa_blk = {kappa_blk:.3g}: outside the first-order analysis"
        assert exact_zero_ok, "R differs from 0 where |L| |L^T| is 0"
        assert worst <= 1.0, (f"factor: |A - L L^T| = {worst:.3g} x bound at {at} of m = {m} "
                              f"(kappa_blk = {kappa_blk:.3g}, bound <= {c_eff:.0f} u |L| |L^T|)")
    return out


# ------------------------------------------------------------------ 3. solve
def ld_cho_solve(lo, rhs):
    """(L L^T)^-1 rhs by long-double substitutions."""
    lo = np.asarray(lo, dtype=LD)
    m = lo.shape[0]
    z = np.array(rhs, dtype=LD)
    for j in range(m):
        z[j] = z[j] / lo[j, j]
        z[j + 1:] -= lo[j + 1:, j] * z[j]
    for j in range(m - 1, -1, -1):
        z[j] = z[j] / lo[j, j]
        z[:j] -= lo[j, :j] * z[j]
    return z


def _rhs(q, k, d):
    d = np.asarray(d, dtype=np.float64).astype(LD)
    if k == 0:
        return d, np.zeros(d.shape)
    ql = np.asarray(q, dtype=np.float64).astype(LD)
    rhs = ql.T @ d[:k] + d[k:]
    return rhs, (gamma(k + 1) * (np.abs(ql).T @ np.abs(d[:k]) + np.abs(d[k:]))).astype(np.float64)


def solve_residual_bound(l64, g_abs, big):
    """The bound of section 3 on |L L^T g - rhs| (without the rhs term) for |g| = g_abs, float64; and kappa_1024."""
    al = np.abs(l64)
    m = al.shape[0]
    v = al.T @ g_abs
    if not big:
        gm = gamma(m + 1)
        return (2 * gm + gm * gm) * (al @ v), 1.0
    c1, gb = gamma(BB + 1) + 6 * U, gamma(BB + 1)
    kb = c1 * v
    kf = c1 * (al @ v)
    kappa = 1.0
    for j0 in range(0, m, BB):
        blk = slice(j0, min(m, j0 + BB))
        t = l64[blk, blk]
        kappa = max(kappa, float(np.linalg.cond(t)))
        at, x = np.abs(t), np.abs(_tri_inv(t))
        w = at @ x @ at
        w2 = w @ x @ at
        kb[blk] += gb * ((w2 + w).T @ g_abs[blk])
        kf[blk] += 2 * gb * (w @ v[blk])
    return al @ kb + kf, kappa


def solve_check(l_packed, m, k, q, d, out, big=False, check=True):
    """d: the input values of the domain's points in its order; out: the device's output on them (all rows written).
    Returns dict(ratio, ratio_special, kappa_1024)."""
    lo = unpack_lower(l_packed, m, LD)
    out = np.asarray(out, dtype=np.float64)
    g = out[k:].astype(LD)
    rhs, e_rhs = _rhs(q, k, d)
    res = np.abs(lo @ (lo.T @ g) - rhs).astype(np.float64)
    bnd, kappa = solve_residual_bound(lo.astype(np.float64), np.abs(out[k:]), big)
    bnd = bnd + e_rhs
    ok = bnd > 0
    ratio = float((res[ok] / bnd[ok]).max()) if ok.any() else 0.0
    zero_ok = bool((res[~ok] == 0).all())
    rs = 0.0
    if k:
        ql = np.asarray(q, dtype=np.float64).astype(LD)
        es = np.abs(out[:k].astype(LD) - ql @ g).astype(np.float64)
        bs = gamma(-(-m // 256) + 9) * (np.abs(ql).astype(np.float64) @ np.abs(out[k:]))
        rs = float((es[bs > 0] / bs[bs > 0]).max()) if (bs > 0).any() else 0.0
        zero_ok &= bool((es[bs == 0] == 0).all())
    if check:
        assert np.isfinite(out).all(), "solution is not finite"
        assert zero_ok, "a residual with a zero bound is not zero"
        assert ratio <= 1.0, f"solve: |L L^T gamma - rhs| = {ratio:.3g} x bound (m = {m}, k = {k}, kappa_1024 = {kappa:.3g})"
        assert rs <= 1.0, f"solve: |lambda_s - Q gamma| = {rs:.3g} x bound (m = {m}, k = {k})"
    return {"ratio": ratio, "ratio_special": rs, "kappa_1024": kappa}


def solve_forward(l_packed, m, k, q, d):
    """(coefficients in the domain's point order, their forward bound) through the factor given: the long-double
    substitution and |(L L^T)^-1| times the backward bound of section 3 (per-domain path)."""
    lo = unpack_lower(l_packed, m, LD)
    rhs, e_rhs = _rhs(q, k, d)
    g = ld_cho_solve(lo, rhs)
    l64 = lo.astype(np.float64)
    g64 = np.abs(g).astype(np.float64)
    b, _ = solve_residual_bound(l64, g64, False)
    ainv = np.abs(np.linalg.inv(l64 @ l64.T))
    fg = ainv @ (b + e_rhs)
    if k == 0:
        return g, fg
    ql = np.asarray(q, dtype=np.float64).astype(LD)
    aq = np.abs(ql).astype(np.float64)
    lam = ql @ g
    fl = aq @ fg + gamma(-(-m // 256) + 9) * (aq @ g64)
    return np.concatenate([lam, g]), np.concatenate([fl, fg])


# ------------------------------------------------------------------ 4. fallback
def spectrum_margin(a_sym64):
    """(smallest eigenvalue, largest |eigenvalue|, smallest |eigenvalue| / largest) of a symmetric float64 matrix."""
    w = np.linalg.eigvalsh(a_sym64)
    big = float(np.abs(w).max())
    return float(w[0]), big, float(np.abs(w).min() / big)


def inverse_check(inv_packed, a_ref_sym, m, check=True):
    """The stored symmetric inverse of a mode-1 domain against the long-double matrix.  Returns ||Xhat - A^-1||_2 over its
    bound 8 m u kappa_2 ||A^-1||_2."""
    xh = unpack_symmetric(inv_packed, m, np.float64)
    a64 = np.asarray(a_ref_sym).astype(np.float64)
    # A^-1 to long double: float64 inverse and one Newton step X (2 I - A X) with the residual in long double
    x0 = np.linalg.inv(a64).astype(LD)
    al = np.asarray(a_ref_sym, dtype=LD)
    x1 = x0 @ (2 * np.eye(m, dtype=LD) - al @ x0)
    kappa = float(np.linalg.cond(a64))
    err = float(np.linalg.norm((xh.astype(LD) - x1).astype(np.float64), 2))
    ratio = err / (8 * m * U * kappa * float(np.linalg.norm(x1.astype(np.float64), 2)))
    if check:
        assert ratio <= 1.0, f"stored inverse: error {ratio:.3g} x bound (m = {m}, kappa = {kappa:.3g})"
    return ratio, x1, kappa


def refined_solve(a_sym, rhs, steps=2):
    """A^-1 rhs: a float64 solve refined with long-double residuals."""
    al = np.asarray(a_sym, dtype=LD)
    a64 = al.astype(np.float64)
    import scipy.linalg as sla
    lu = sla.lu_factor(a64)
    x = sla.lu_solve(lu, np.asarray(rhs).astype(np.float64)).astype(LD)
    for _ in range(steps):
        r = np.asarray(rhs, dtype=LD) - al @ x
        x = x + sla.lu_solve(lu, r.astype(np.float64)).astype(LD)
    return x
