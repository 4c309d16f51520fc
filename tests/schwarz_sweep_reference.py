"""The sweep of the Schwarz preconditioner between its levels (level_step() and the loop of the apply in csrc/schwarz.cpp, the
kernels of csrc/schwarz_kernels.hip) restated in numpy longdouble, one step from the device's own input, and the bounds each
part of a step is held to.  A plain helper module (no tests), shared by test_schwarz_sweep_reference_host.py (no GPU, a numpy
stand-in for the device) and test_gpu_schwarz_sweep.py.

A TRACE is what SchwarzPreconditioner.debug_apply_trace returns: after every level step the dict
    level, coarse, have_sl, add_poly, y (the partial product on the level's rows, None without have_sl), res, out, sl (N each),
    proj (fine levels with a basis, else None), tail (None unless the step produced one)
and `initial` = dict(res, out): the two vectors that persist between applies, as the sweep found them.  The state BEFORE step
i is state_before(steps, initial, i): the record before it, and sl = 0 at the start.  Every check reads the input of its part
from the device's own records, so no tolerance carries the accuracy of the FMM or the condition of a local system.

u = 2^-53, gamma_c = c u / (1 - c u).  Every bound is COUNTED from the code path; none is fitted.

1. RESIDUAL (residual_kernel).  On the level's rows r = rows[j]:  res[r] = rg[r] - y[j] - nugget sl[r].
   fl(rg - y) is off by at most u |rg - y|.  Then either fl(nugget sl) (u |nugget sl|) and a subtraction (u |res|), or one FMA
   (u |res|):  |res_dev - res| <= u (|rg - y| + |nugget sl| + |res_dev|)  with or without contraction.
   Every other row of d_res keeps the bits of the record before; without have_sl the solves read rg and d_res is untouched.

2. LOCAL SOLVES.  A DebugLevel (the product's own ddm_level_build / ddm_level_solve, pinned to long double by
   test_gpu_ddm_local.py) on the level's own domains solves the step's source (d_res, or rg without have_sl) into d_out of the
   record before: the result equals d_out of the record bit for bit, written and unwritten rows.  Under global_scaling the
   coarse domain's monomials differ, so do Q and the reduced matrix: there the coefficients are compared with what the
   default-scaling level gives for the same source, within the forward bound of ddm_local_reference.solve_forward.

3. PROJECTION (project_partial_kernel, project_final_kernel).  proj[b] = sum over the level's rows of ortho[r, b] out[r].
   Block i of the 1024 sums the rows [i per, (i + 1) per) of the level's row list, per = ceil(m / 1024): a thread adds
   t = ceil(per / 256) products to a zero (an inner product of t terms, gamma_t with or without FMAs), the 256 threads meet in
   an 8-level tree (8), and the partial sums of the nb = ceil(m / per) non-empty blocks are added in block order (nb - 1; the
   empty blocks add exact zeros):  |proj_dev - proj| <= gamma_{t + 8 + nb - 1} sum |ortho| |out|.
   Rows of d_out outside the level (stale values of earlier levels) do not enter the reference.

4. WRITE-BACK (add_rows_kernel, subtract_projection_kernel).  Coarse step, or no basis: sl[r] = fl(sl[r] + out[r]) on the
   level's rows -- one IEEE addition, compared bit for bit -- and the same bits elsewhere.  Fine level with a basis: on all N rows
   sl_after = (sl + out [level rows]) - sum_b ortho[., b] proj[b]: the addition (u |sl + out|), basis products summed in a
   chain (gamma_basis, one more for a contraction-free count), the subtraction (u |sl_after|):
       |sl_dev - sl_after| <= u (|sl + out| + |sl_dev|) + gamma_{basis + 1} sum_b |ortho| |proj|.

5. TAIL (host code of level_step, last coarse visit with a basis).  r_a = src[s_a] - sum_j A_special[a, j] c_j over the nc
   coarse points, s_a the k special points, c the device's d_out on the coarse points; sp_mono tail = r by Gaussian
   elimination with partial pivoting.  With the host's kernel values (pointwise budget (a, b) of kernel_pointwise.py, where =
   host, e(phi) = u (a |phi| + (b + 4) |x phi'|) as in ddm_local_reference) and the chain of nc subtractions,
       |r_dev - r| <= gamma_{nc + 1} (|src| + sum_j |A| |c|) + sum_j e(A_aj) |c_j|                            =: e_r
   and (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., Thm 9.5) (sp_mono + dA) tail = r_dev with
   ||dA||_inf <= k^2 gamma_{3k} rho ||sp_mono||_inf, rho the growth factor, measured by restating the elimination:
       |sp_mono tail - r|_a <= k^2 gamma_{3k} rho ||sp_mono||_inf ||tail||_inf + e_r[a].
   sp_mono: the monomials at the special points on (x - translation) / scale, translation and scale from the extents of the
   coarse domain's own points (default) or of all points (global_scaling), through the library's own evaluate_monomials.
   BOTH SCALINGS (check_tails_agree).  The two handles' tails describe one polynomial at the special points only as far as
   their right-hand sides agree, and those differ: the handles' records part after the first coarse visit (the coarse
   coefficients differ in their last bits, every later residual with them).  The difference of the right-hand sides is
   bounded from counted quantities.  With src_i the residual input of handle i's last coarse visit, x_i the long-double
   substitution through the default-scaling factor for src_i and f_i its forward bound (ddm_local_reference.solve_forward;
   |c_i - x_i| <= f_i is asserted for both handles),
       r_1 - r_2 = (src_1 - src_2)[s] - A_special (c_1 - c_2),
       |r_1 - r_2| <= |(src_1 - src_2)[s] - A_special (x_1 - x_2)| + |A_special| (f_1 + f_2),
   the first term being the exact image of the difference of the inputs.  So
       |sp_mono_1 tail_1 - sp_mono_2 tail_2| <= b_1 + b_2 + |A_special| (f_1 + f_2) + |(src_1 - src_2)[s] - A_special (x_1 - x_2)|
   with b_i the bound of the tail check above.  No term is read off the device's own right-hand sides.

6. ORTHO.  Modified Gram-Schmidt, twice, over the columns of monomial_matrix in their order, restated in long double.  No
   constant is derived for the product's float64 run; the deviation of a float64 numpy restatement of the same procedure from
   the long-double one is measured on the cloud at hand, and four times that is allowed.  The order of the sums belongs to the
   procedure: the product adds each block of 65,536 entries in a chain and the blocks in order, and so does the restatement
   (chained_dot); numpy's pairwise sums are ten times closer to long double than any such chain and would not measure it.
   Measured on the CPU, max |Q_f64 - Q_ld| (largest |Q| entry for scale), on the clouds of test_gpu_schwarz_sweep.py:
       3-D n = 1500 linear drift      (basis 4)    2.92e-16  (|Q| <= 0.0466)
       2-D n = 1500 constant drift    (basis 1)    2.92e-16  (|Q| = 0.0258)
       1-D n = 1200 quadratic drift   (basis 3)    2.37e-16  (|Q| <= 0.0647)
       3-D n = 2500 quadratic drift   (basis 10)   4.48e-16  (|Q| <= 0.0625)
       3-D n = 60   linear drift      (basis 4)    9.7e-17   (|Q| <= 0.251)
       3-D n = 263,000 constant drift (basis 1)    4.43e-16  (|Q| = 0.00195)
   (the second pass renormalises by sqrt(sum q^2), a chain of n roundings, which numpy's pairwise sum does not have: with
   the constant drift at n = 1500 the pairwise restatement is off by 2.0e-19 only, the chained one and the product by 2.92e-16).
   The product has so far been bit-identical to the chained restatement: the deviation is then exactly a quarter of the
   tolerance.  Orthonormality follows from the deviation: |Q^T Q - I| <= 2 sqrt(N) tol + 1e-17.

7. ORDER.  The records are (0, coarse), (1, coarse), ..., (levels - 2, coarse); add_poly on the last coarse visit only, have_sl
   false on the first step only; one level gives the single record (0 = coarse, have_sl false, add_poly).  A tail appears on
   the last coarse visit when there is a basis, nowhere else, and the last `basis` values of the result are it (or zeros).
"""
import numpy as np

import ddm_local_reference as R
from ddm_local_reference import gamma
from kernel_reference import LD, U

PROJECT_BLOCKS = 1024


def same_bits(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64).view(np.int64), np.asarray(b, dtype=np.float64).view(np.int64))


def worst_ratio(err, bound, what):
    """max err / bound; an entry whose bound is zero must be exact.  Asserts the ratio is at most 1."""
    err = np.asarray(err, dtype=LD).reshape(-1)
    bound = np.asarray(bound, dtype=LD).reshape(-1)
    assert np.isfinite(err.astype(np.float64)).all(), f"{what}: not finite"
    zero = bound == 0
    assert (err[zero] == 0).all(), f"{what}: an entry with a zero bound differs"
    if zero.all():
        return 0.0
    ratio = (err[~zero] / bound[~zero]).astype(np.float64)
    worst = float(ratio.max())
    assert worst <= 1.0, f"{what}: error = {worst:.3g} x bound at entry {int(np.flatnonzero(~zero)[int(np.argmax(ratio))])}"
    return worst


def state_before(steps, initial, i):
    """dict(res, out, sl) the step i starts from."""
    if i == 0:
        return {"res": initial["res"], "out": initial["out"], "sl": np.zeros_like(initial["out"])}
    return steps[i - 1]


def source(step, before, rg):
    """What the local solves of a step read."""
    return step["res"] if step["have_sl"] else np.asarray(rg, dtype=np.float64)[:before["sl"].size]


# ------------------------------------------------------------------ 1. residual
def check_residual(step, before, rg, rows, nugget):
    """Returns the largest error / bound on the level's rows (None without have_sl)."""
    n = before["sl"].size
    if not step["have_sl"]:
        assert step["y"] is None
        assert same_bits(step["res"], before["res"]), "residual: d_res was written although the product was skipped"
        return None
    rows = np.asarray(rows)
    y = np.asarray(step["y"], dtype=np.float64)
    assert y.shape == rows.shape
    rgl, sl = np.asarray(rg, dtype=np.float64)[:n][rows].astype(LD), before["sl"][rows].astype(LD)
    first = rgl - y.astype(LD)
    second = LD(np.float64(nugget)) * sl
    err = np.abs(step["res"][rows].astype(LD) - (first - second))
    bound = LD(U) * (np.abs(first) + np.abs(second) + np.abs(step["res"][rows].astype(LD)))
    worst = worst_ratio(err, bound, f"residual of level {step['level']}")
    other = np.ones(n, dtype=bool)
    other[rows] = False
    assert same_bits(step["res"][other], before["res"][other]), "residual: a row outside the level was written"
    return worst


# ------------------------------------------------------------------ 2. local solves
def level_domains(ddm_level):
    return [(np.asarray(dom.overlapping_point_indices), np.asarray(dom.internal_points_mask, dtype=bool))
            for dom in ddm_level.leaf_domains]


def check_local_solves(level, step, before, rg):
    """level: a DebugLevel (or a stand-in with its solve()) on the level's own domains, default scaling.  Bit for bit.
    Returns the number of rows the solve changed."""
    src = source(step, before, rg)
    out = level.solve(src, before["out"], bool(step["coarse"]))
    assert same_bits(out, step["out"]), (f"local solves of level {step['level']}: d_out differs from the level's own solvers in "
                                         f"{int((out.view(np.int64) != step['out'].view(np.int64)).sum())} rows")
    return int((before["out"].view(np.int64) != step["out"].view(np.int64)).sum())


def check_coarse_coefficients(level, factor, step, before, rg):
    """global_scaling: the coarse coefficients against the default-scaling level's long-double substitution for the same source,
    within its forward bound; rows outside the coarse domain keep their bits.  Returns the largest error / bound."""
    src = source(step, before, rg)
    idx = level.indices[0]
    ref, fwd = R.solve_forward(factor[0], level.m[0], level.k[0], level.q[0], src[idx])
    worst = worst_ratio(np.abs(step["out"][idx].astype(LD) - ref), fwd, "coarse coefficients under global scaling")
    other = np.ones(src.size, dtype=bool)
    other[idx] = False
    assert same_bits(step["out"][other], before["out"][other])
    return worst


# ------------------------------------------------------------------ 3. projection
def projection_steps(m, blocks=PROJECT_BLOCKS):
    per = -(-m // blocks)
    return -(-per // 256) + 8 + (-(-m // per) - 1)


def check_projection(step, ortho, rows):
    rows = np.asarray(rows)
    q = np.asarray(ortho, dtype=np.float64)[rows].astype(LD)
    v = step["out"][rows].astype(LD)
    ref = q.T @ v
    bound = LD(gamma(projection_steps(rows.size))) * (np.abs(q).T @ np.abs(v))
    return worst_ratio(np.abs(step["proj"].astype(LD) - ref), bound, f"projection of level {step['level']}")


def stale_rows(step, rows):
    """Rows of d_out outside the level that hold a non-zero value (the projection must not read them)."""
    other = np.ones(step["out"].size, dtype=bool)
    other[np.asarray(rows)] = False
    return int((step["out"][other] != 0).sum())


# ------------------------------------------------------------------ 4. write-back
def check_writeback(step, before, ortho, rows):
    """Returns the largest error / bound (fine level with a basis) or the number of rows changed (bit-for-bit paths)."""
    rows = np.asarray(rows)
    n = before["sl"].size
    added = before["sl"].copy()
    added[rows] = before["sl"][rows] + step["out"][rows]                 # one IEEE addition
    if step["coarse"] or ortho is None:
        assert step["proj"] is None
        assert same_bits(step["sl"], added), f"write-back of level {step['level']}: not sl + out on the level's rows, sl elsewhere"
        return int((added.view(np.int64) != before["sl"].view(np.int64)).sum())
    q = np.asarray(ortho, dtype=np.float64).astype(LD)
    exact = before["sl"].astype(LD)
    exact[rows] += step["out"][rows].astype(LD)
    p = step["proj"].astype(LD)
    ref = exact - q @ p
    bound = LD(U) * (np.abs(exact) + np.abs(step["sl"].astype(LD))) + LD(gamma(q.shape[1] + 1)) * (np.abs(q) @ np.abs(p))
    assert bound.shape == (n,)
    return worst_ratio(np.abs(step["sl"].astype(LD) - ref), bound, f"write-back of level {step['level']}")


# ------------------------------------------------------------------ 5. tail
def extents_scaling(x):
    """get_cheb_cube_scaling_factors: (translation, scale) of the points x (n x d), float64 as the product forms them."""
    x = np.atleast_2d(np.asarray(x, dtype=np.float64))
    lo, hi = x.min(axis=0), x.max(axis=0)
    sc = (hi - lo) / 2.0
    sc[sc == 0.0] = 1.0
    return (hi + lo) / 2.0, sc


def monomials(x, degree, translation, scale):
    """The library's evaluate_monomials (host code) at the points x (n x d): n x basis."""
    from ferreus_rbf_rs_amd import _lib as L
    x = np.asfortranarray(np.atleast_2d(np.asarray(x, dtype=np.float64)))
    n, d = x.shape
    k = degree + 1
    basis = {1: k, 2: k * (k + 1) // 2, 3: k * (k + 1) * (k + 2) // 6}[d]
    out = np.zeros((n, basis), order="F")
    tr = np.ascontiguousarray(translation, dtype=np.float64)
    sc = np.ascontiguousarray(scale, dtype=np.float64)
    rc = L.load().bbfmm_debug_evaluate_monomials(x.ctypes.data, n, d, n, degree, tr.ctypes.data, sc.ctypes.data, out.ctypes.data)
    assert rc == L.OK
    return out


def growth_factor(a):
    """Gaussian elimination with partial pivoting restated in float64: max |a_ij^(s)| over all stages / max |a_ij|."""
    a = np.array(a, dtype=np.float64)
    k = a.shape[0]
    top = big = np.abs(a).max()
    for c in range(k):
        p = c + int(np.argmax(np.abs(a[c:, c])))
        a[[c, p]] = a[[p, c]]
        for r in range(c + 1, k):
            a[r, c:] -= (a[r, c] / a[c, c]) * a[c, c:]
        big = max(big, np.abs(a[c + 1:, c + 1:]).max() if c + 1 < k else 0.0)
    return float(big / top)


def tail_residual(step, before, rg, points, st, special, coarse_points, scaling, nugget_diagonal=True):
    """(r in long double, e_r, sp_mono): the right-hand side of the tail's system restated from the device's d_out."""
    src = source(step, before, rg)
    special, cp = np.asarray(special), np.asarray(coarse_points)
    pts = np.atleast_2d(np.asarray(points, dtype=np.float64))
    a, aabs, ea = R._kernel_block(0, st.kernel_type, st.base_range, st.total_sill, R._pad3(pts[special]), R._pad3(pts[cp]))
    if nugget_diagonal:
        diag = special[:, None] == cp[None, :]
        a = a + LD(np.float64(st.nugget)) * diag
        aabs = aabs + abs(LD(np.float64(st.nugget))) * diag
    c = step["out"][cp].astype(LD)
    r = src[special].astype(LD) - a @ c
    e_r = LD(gamma(cp.size + 1)) * (np.abs(src[special].astype(LD)) + aabs @ np.abs(c)) + ea @ np.abs(c)
    sp_mono = monomials(pts[special], st.polynomial_degree, *scaling)
    return r, e_r, sp_mono


def check_tail(step, before, rg, points, st, special, coarse_points, scaling):
    """Returns (largest error / bound, the polynomial's values at the special points in long double, the bound per point)."""
    r, e_r, sp_mono = tail_residual(step, before, rg, points, st, special, coarse_points, scaling)
    k = sp_mono.shape[0]
    assert sp_mono.shape == (k, k) and step["tail"] is not None and step["tail"].shape == (k,)
    t = step["tail"].astype(LD)
    values = sp_mono.astype(LD) @ t
    rho = growth_factor(sp_mono)
    bound = LD(k * k * gamma(3 * k) * rho * np.abs(sp_mono).sum(axis=1).max() * np.abs(step["tail"]).max()) + e_r
    return worst_ratio(np.abs(values - r), bound, "tail"), values, bound


def check_tails_agree(forward, coarse_points, points, st, special, runs):
    """Both scalings.  forward(values on coarse_points) -> (coefficients in long double, their forward bound), through the
    default-scaling level of the coarse domain; coarse_points in that level's order; runs: per handle (last step, the record
    before it, rg, scaling).  Returns dict(ratio, rhs_difference, tail_bounds, coefficient_term, input_term): the largest
    difference / bound and the largest entry of |r_1 - r_2| and of the three parts of the bound."""
    cp, special = np.asarray(coarse_points), np.asarray(special)
    pts = np.atleast_2d(np.asarray(points, dtype=np.float64))
    a, aabs, _ = R._kernel_block(0, st.kernel_type, st.base_range, st.total_sill, R._pad3(pts[special]), R._pad3(pts[cp]))
    diag = special[:, None] == cp[None, :]
    a = a + LD(np.float64(st.nugget)) * diag
    aabs = aabs + abs(LD(np.float64(st.nugget))) * diag
    parts = []
    for step, before, rg, scaling in runs:
        src = source(step, before, rg)
        x, f = forward(src[cp])
        worst_ratio(np.abs(step["out"][cp].astype(LD) - x), f, "coarse coefficients of the last visit")
        _, values, bound = check_tail(step, before, rg, points, st, special, cp, scaling)
        r = tail_residual(step, before, rg, points, st, special, cp, scaling)[0]
        parts.append((values, bound, np.asarray(x, dtype=LD), np.asarray(f, dtype=LD), src[special].astype(LD), r))
    (v1, b1, x1, f1, s1, r1), (v2, b2, x2, f2, s2, r2) = parts
    coefficient_term = aabs @ (f1 + f2)
    input_term = np.abs((s1 - s2) - a @ (x1 - x2))
    ratio = worst_ratio(np.abs(v1 - v2), b1 + b2 + coefficient_term + input_term, "the two scalings describe one polynomial")
    top = lambda v: float(np.abs(v).max())
    return {"ratio": ratio, "rhs_difference": top(r1 - r2), "tail_bounds": top(b1 + b2), "coefficient_term": top(coefficient_term),
            "input_term": top(input_term)}


# ------------------------------------------------------------------ 6. ortho
ORTHO_BLOCK = 65536


def chained_dot(x, y):
    """The product's float64 dot: a chain over each block of 65,536 entries (cumsum adds in order), the blocks in order."""
    p = x * y
    total = np.float64(0.0)
    for lo in range(0, p.size, ORTHO_BLOCK):
        total = total + np.cumsum(p[lo:lo + ORTHO_BLOCK])[-1]
    return total


def mgs_twice(mono, dtype):
    """Modified Gram-Schmidt, twice, in the column order of the product (schwarz_create_impl).  float64: the sums are chains
    in the product's order; long double: numpy's own sums."""
    dot = chained_dot if dtype is np.float64 else (lambda x, y: x @ y)
    q = np.array(mono, dtype=dtype, order="F")
    for _ in range(2):
        for b in range(q.shape[1]):
            for c in range(b):
                q[:, b] -= dot(q[:, c], q[:, b]) * q[:, c]
            q[:, b] /= np.sqrt(dot(q[:, b], q[:, b]))
    return q


def ortho_tolerance(mono):
    """(Q in long double, measured max |Q_f64 - Q_ld|, the tolerance: four times that)."""
    q_ld = mgs_twice(mono, LD)
    measured = float(np.abs(mgs_twice(mono, np.float64).astype(LD) - q_ld).max())
    return q_ld, measured, 4.0 * measured


def check_ortho(ortho, mono):
    """Returns (largest deviation / tolerance, measured constant)."""
    q_ld, measured, tol = ortho_tolerance(mono)
    ortho = np.asarray(ortho, dtype=np.float64)
    assert ortho.shape == q_ld.shape
    n, basis = ortho.shape
    worst = worst_ratio(np.abs(ortho.astype(LD) - q_ld), np.full(ortho.shape, tol), "ortho")
    gram = ortho.astype(LD).T @ ortho.astype(LD)
    assert float(np.abs(gram - np.eye(basis)).max()) <= 2.0 * np.sqrt(n) * tol + 1e-17, "ortho is not orthonormal"
    return worst, measured


# ------------------------------------------------------------------ 7. order
def check_order(steps, num_levels, basis, result=None, n=None):
    coarse = num_levels - 1
    if coarse == 0:
        want = [(0, True, False, True)]
    else:
        want = []
        for i in range(coarse):
            want += [(i, False, i > 0, False), (coarse, True, True, i == coarse - 1)]
    got = [(s["level"], s["coarse"], s["have_sl"], s["add_poly"]) for s in steps]
    assert got == want, f"order of the sweep: {got} instead of {want}"
    for s in steps[:-1]:
        assert s["tail"] is None, f"a tail was produced on a visit that is not the last (level {s['level']})"
    last = steps[-1]
    assert (last["tail"] is not None) == (basis > 0), "the last coarse visit returns the tail exactly when there is a basis"
    if result is not None:
        assert result.size == n + basis
        assert same_bits(result[:n], last["sl"]), "the result is not the running correction of the last record"
        if basis:
            tail = np.zeros(basis)
            tail[basis - last["tail"].size:] = last["tail"]
            assert same_bits(result[n:], tail), "the last rows of the result are not the tail"


# ------------------------------------------------------------------ the whole trace
def cloud(n, dim, seed):
    """Uniform points of the unit cube on the 2^-30 grid."""
    return R.on_grid(np.random.default_rng(seed).random((n, dim)))


def check_trace(points, st, ddm_levels, levels, ortho, rg, z, steps, initial, special=None, scaling=None, coarse_factor=None,
                only_level=None, order=True):
    """Every check of a trace.  ddm_levels: DDMTree(points, params).levels.  levels: per level the object whose solve() restates
    the local solves (None: the local solves are not checked).  coarse_factor: given under global_scaling, the packed factor of
    levels[-1] (the default-scaling level of the coarse domain): the coarse steps are compared through their forward bound.
    special, scaling: the coarse domain's special points and the (translation, scale) of its monomials, for the tail.
    only_level: check the records of this level alone.  Returns the largest ratio (or count) per kind of check."""
    n = np.atleast_2d(points).shape[0]
    basis = 0 if ortho is None else ortho.shape[1]
    if order:
        check_order(steps, len(ddm_levels), basis, z, n)
    stats = {"residual": [], "projection": [], "writeback": [], "writeback_rows": [], "solve_rows": [], "coarse": [], "tail": [],
             "stale": []}
    for i, step in enumerate(steps):
        li = step["level"]
        if only_level is not None and li != only_level:
            continue
        before = state_before(steps, initial, i)
        rows = np.asarray(ddm_levels[li].point_indices)
        r = check_residual(step, before, rg, rows, st.nugget)
        if r is not None:
            stats["residual"].append(r)
        if levels is not None:
            if step["coarse"] and coarse_factor is not None:
                stats["coarse"].append(check_coarse_coefficients(levels[li], coarse_factor, step, before, rg))
            else:
                stats["solve_rows"].append(check_local_solves(levels[li], step, before, rg))
        if step["proj"] is not None:
            stats["projection"].append(check_projection(step, ortho, rows))
            if li >= 1:
                stats["stale"].append(stale_rows(step, rows))
        w = check_writeback(step, before, ortho, rows)
        stats["writeback" if step["proj"] is not None else "writeback_rows"].append(w)
        if step["tail"] is not None:
            stats["tail"].append(check_tail(step, before, rg, points, st, special, rows, scaling)[0])
    return {k: (max(v) if v else None) for k, v in stats.items()}
