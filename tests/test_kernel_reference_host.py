"""The long-double reference of tests/kernel_reference.py checked three ways without a GPU, and the host branch of
csrc/kernels.hpp (bbfmm_debug_kernel_values / bbfmm_debug_math with where = 0: libm and IEEE division, what assembles
the M2L operators) held pointwise to the budget of tests/kernel_pointwise.py."""
import numpy as np
import pytest

import ferreus_rbf_rs_amd as F
import kernel_pointwise as KP
import kernel_reference as KR
from kernel_reference import LD, U
from oracle import bbfmm_oracle as O

RANGES = {kid: (KR.SPHEROIDAL_RANGES if kid in KR.SPHEROIDAL else (1.0, 0.7)) for kid in KR.KERNEL_IDS}
CASES = [(kid, br) for kid in KR.KERNEL_IDS for br in RANGES[kid]]
SILL = 0.3          # total_sill <= base_range (KernelParamsBuilder::build)


def test_budget_entries_stay_under_64u():
    for where in (0, 1):
        for kid in KR.KERNEL_IDS:
            for path, (a, b) in KP.budget(where, kid).items():
                assert 0 < a <= KP.MAX_ENTRY and 0 <= b <= KP.MAX_ENTRY, (where, kid, path, a, b)
    assert KP.budget(1, 6)["value_far"][0] == 49.5      # the largest: Spheroidal9 far values


@pytest.mark.parametrize("kid,br", CASES)
def test_tables_are_mostly_in_the_measured_class(kid, br):
    """From the reference alone: at least 90 % of every kernel's table entries, per output, are checked by the relative
    measure (the rest -- overflow, underflow, the clamp region of bb_sqrt -- by their class)."""
    r2 = KR.table_for(kid, br)
    assert r2.size >= 200_000
    e = KR.evaluate(KR.Params(kid, br, SILL), r2)
    for path in ("value", "value_g", "factor"):
        assert KR.measured_class(e[path], r2).mean() >= 0.9, (kid, path)


def test_tables_hold_the_edges_the_rules_sit_on():
    t = KR.r2_table()
    for x in (0.0, 5e-324, KR.EPS, np.nextafter(KR.EPS, 0), np.nextafter(KR.EPS, 1), KR.EPS ** 2, np.nextafter(KR.EPS ** 2, 0),
              1.0, np.nextafter(1.0, 0), np.nextafter(1.0, 2), 1e-300, np.nextafter(1e-300, 0), 1e300, 4.0, 2.0 ** -199,
              2.0 ** -200 * (2 - 2.0 ** -52), 1000.0 ** 2):
        assert (t == x).any(), x
    for kid in KR.SPHEROIDAL:
        for br in KR.SPHEROIDAL_RANGES:
            p = KR.Params(kid, br, SILL)
            near = KR.spheroidal_near(p, KR.spheroidal_switch_table(kid, br))
            assert near[0] and not near[-1] and (np.diff(near.astype(int)) <= 0).all()      # both sides of the switch


@pytest.mark.parametrize("kid", KR.KERNEL_IDS)
def test_reference_against_mpmath(kid):
    """The same definitions once more, in 40-digit arithmetic, on a subset of the table: the long-double reference is good
    to a few units of 2^-64 -- 2^-57 (|g| + |x g'|) is asserted, 1/16 of the unit the device measure is expressed in."""
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 40
    br = RANGES[kid][1]
    p = KR.Params(kid, br, SILL)
    t = KR.table_for(kid, br)
    t = t[(t >= 2.0 ** -200) & (t <= 2.0 ** 200)]
    x = np.concatenate([t[:: max(1, t.size // 300)], KR.neighbours(1.0, 4), KR.neighbours(0.36787944117144233, 4)])
    if kid in KR.SPHEROIDAL:
        x = np.concatenate([x, KR.spheroidal_switch_table(kid, br)])
    if kid == 100:
        x = x[x * p.inv_br2 < 11000]            # exp stays inside the long-double range
    near = KR.spheroidal_near(p, x) if kid in KR.SPHEROIDAL else np.zeros(x.size, dtype=bool)
    g, xg, f, xf = KR.smooth(p, x.astype(LD), near if kid in KR.SPHEROIDAL else None)

    def exact(xi, is_near):
        X = xi if isinstance(xi, mp.mpf) else mp.mpf(float(xi))
        r = mp.sqrt(X)
        if kid == 0:
            return -r, -1 / r
        if kid == 1:
            return X * mp.log(r), 2 * mp.log(r) + 1
        if kid == 2:
            return r ** 3, 3 * r
        if kid in KR.SPHEROIDAL:
            if is_near:
                return mp.mpf(float(p.total_sill)) - mp.mpf(float(p.near_slope)) * r, -mp.mpf(float(p.near_slope)) / r
            tt, q = 1 + mp.mpf(float(p.s2)) * X, mp.mpf(p.pow) + mp.mpf(1) / 2
            return mp.mpf(float(p.far_coef)) * tt ** (-q), -2 * q * mp.mpf(float(p.s2)) * mp.mpf(float(p.far_coef)) * tt ** (-q - 1)
        if kid == 7:
            return 1 / r, -1 / r ** 3
        if kid == 8:
            return 1 / X, -2 / X ** 2
        if kid == 9:
            return 1 / X ** 2, -4 / X ** 3
        ib = mp.mpf(float(p.inv_br2))
        if kid == 100:
            return mp.exp(-X * ib), -2 * ib * mp.exp(-X * ib)
        return mp.sqrt(1 + X * ib), ib / mp.sqrt(1 + X * ib)

    tol = mp.mpf(2) ** -57
    for i in range(x.size):
        ge, fe = exact(x[i], near[i])
        # numpy prints a long double with all its digits
        gl, fl = mp.mpf(np.format_float_scientific(g[i], precision=25)), mp.mpf(np.format_float_scientific(f[i], precision=25))
        sg = abs(ge) + abs(mp.mpf(np.format_float_scientific(xg[i], precision=25)))
        sf = abs(fe) + abs(mp.mpf(np.format_float_scientific(xf[i], precision=25)))
        assert abs(gl - ge) <= tol * sg, (kid, "value", x[i])
        assert abs(fl - fe) <= tol * sf, (kid, "factor", x[i])
    # the sensitivities x g', x f' against a central difference of the mpmath definitions
    for i in range(0, x.size, 7):
        X, h = mp.mpf(float(x[i])), mp.mpf(float(x[i])) * mp.mpf(10) ** -12
        (g1, f1), (g0, f0) = exact(X + h, near[i]), exact(X - h, near[i])
        for got, num, scale in ((xg[i], X * (g1 - g0) / (2 * h), abs(g1)), (xf[i], X * (f1 - f0) / (2 * h), abs(f1))):
            got = mp.mpf(np.format_float_scientific(got, precision=25))
            assert abs(got - num) <= mp.mpf(10) ** -9 * (abs(num) + scale), (kid, x[i])


def test_zero_rules_of_the_reference_module():
    """Both sides of each rule, stated as numbers (what rbf_kernels.rs / non_rbf_kernels.rs return there)."""
    eps = KR.EPS
    below, above = np.nextafter(eps, 0), np.nextafter(eps, 1)
    for kid in KR.KERNEL_IDS:
        e = KR.evaluate(KR.Params(kid, 1.0, SILL), np.array([0.0, below, eps, above, eps * eps * (1 - eps), eps * eps]))
        if kid in KR.NO_GRAD_ZERO_RULE:
            assert (e["factor"] != 0).all()
        else:
            assert (e["factor"][:3] == 0).all() and e["factor"][3] != 0      # r2 <= eps: zero-filled gradient
        if kid in KR.VALUE_ZERO_RULE:
            assert e["value"][0] == 0 and e["value"][4] == 0 and e["value"][5] != 0    # |r| < eps  <=>  r2 < eps^2
            assert (e["value_g"][:3] == 0).all() and e["value_g"][3] != 0
        if kid == 0:
            assert e["value_g"][2] == -np.sqrt(LD(eps))
        if kid in KR.SPHEROIDAL:
            assert (e["value_g"] == e["value"]).all() and e["value"][0] == LD(np.float64(SILL))


@pytest.mark.parametrize("kid", KR.KERNEL_IDS)
def test_reference_against_the_oracle(kid):
    """The oracle (oracle/passes.c: f64, the host formulas) against the long-double sums, per row and right-hand side, to
    the bound the pair-kernel tests use with the host budget, and O.kernel_phi pointwise."""
    rng = np.random.default_rng(kid)
    d, n, m, K = 3, 300, 120, 3
    br = 0.7
    src = np.round(rng.random((n, d)) * 2 ** 30) / 2 ** 30
    tgt = np.vstack([src[:40], np.round(rng.random((m - 40, d)) * 2 ** 30) / 2 ** 30])
    w = rng.standard_normal((n, K))
    D = KR.Dense(kid, br, SILL, tgt, src)
    y, g = O.dense_sum(kid, br, SILL, tgt, src, w, with_grads=True)
    y0 = O.dense_sum(kid, br, SILL, tgt, src, w)
    ref0, s_phi, s_xd = D.sums(w)
    a, b = KP.sum_budget(0, kid, "value")
    assert (np.abs(y0.astype(LD) - ref0) <= LD(U) * ((a + 4 + n) * s_phi + (b + 4) * s_xd)).all()
    ref, gref, s_phi, s_xd, s_f, s_xf = D.grad_sums(w)
    a, b = KP.sum_budget(0, kid, "value_g")
    assert (np.abs(y.astype(LD) - ref) <= LD(U) * ((a + 4 + n) * s_phi + (b + 4) * s_xd)).all()
    a, b = KP.sum_budget(0, kid, "factor")
    got = g.reshape(m, K, d)                       # column k * d + axis
    assert (np.abs(got.astype(LD) - gref) <= LD(U) * ((a + 5 + n) * s_f + (b + 4) * s_xf)).all()
    # kernel_phi(r) = phi at f64(r * r): one more rounding of the argument
    r = np.concatenate([rng.random(200) * 3, [0.0, 1.0, 1e-20]])
    p = KR.Params(kid, br, SILL)
    e = KR.evaluate(p, r * r)
    a, b = KP.coefficients(0, p, "value", r * r)
    got = np.array([O.kernel_phi(kid, ri, br, SILL) for ri in r])
    assert (np.abs(got.astype(LD) - e["value"]) <= LD(U) * (a * np.abs(e["value"]) + b * np.abs(e["x_dvalue"]))).all()


@pytest.mark.parametrize("which", list(F.fmm_tree.DEBUG_MATH))
def test_host_primitives(which):
    KP.check_primitive(0, which, F.debug_math(0, which, KP.primitive_inputs(which)))


@pytest.mark.parametrize("kid,br", CASES)
def test_host_kernel_functions_pointwise(kid, br):
    KP.check_kernel(0, kid, br, SILL, F.debug_kernel_values(0, kid, br, SILL, KR.table_for(kid, br)))


def test_hooks_refuse_bad_arguments():
    from ferreus_rbf_rs_amd import _lib as L
    lib, x, o = L.load(), np.ones(4), np.zeros(4)
    assert lib.bbfmm_debug_kernel_values(0, 10, 1.0, 1.0, x.ctypes.data, 4, o.ctypes.data, o.ctypes.data, o.ctypes.data) == L.BAD_ARGUMENT
    assert lib.bbfmm_debug_kernel_values(2, 0, 1.0, 1.0, x.ctypes.data, 4, o.ctypes.data, o.ctypes.data, o.ctypes.data) == L.BAD_ARGUMENT
    assert lib.bbfmm_debug_kernel_values(0, 0, 1.0, 1.0, x.ctypes.data, 4, None, o.ctypes.data, o.ctypes.data) == L.BAD_ARGUMENT
    assert lib.bbfmm_debug_math(0, 4, x.ctypes.data, 4, o.ctypes.data, None) == L.BAD_ARGUMENT
    assert lib.bbfmm_debug_math(0, 0, x.ctypes.data, 4, o.ctypes.data, None) == L.OK and (o == 1).all()
