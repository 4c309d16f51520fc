"""The twelve kernel functions in extended precision (numpy longdouble, 64-bit significand), written from their
mathematical definitions -- phi(r) of ferreus_rbf_utils rbf_kernels.rs / non_rbf_kernels.rs, the ten-digit Spheroidal
constants of constants.rs, and the two extension kernels exp(-r^2 / range^2) and sqrt(1 + r^2 / range^2) -- as functions
of x = r^2, NOT from csrc/kernels.hpp or oracle/passes.c.  A plain helper module (no tests): what the pointwise and the
pair-kernel tests compare the product with.

Per kernel: g(x) = phi, the gradient factor f(x) = 2 dphi/dx (gradient = f * (target - source)), and x g'(x), x f'(x)
(the sensitivity to a relative perturbation of the argument, which the error measure of the tests needs).

What is emulated exactly, in f64, are the reference's DECISIONS (they are part of the definition of what it returns):
  value paths      f64(sqrt(r2)) < DBL_EPSILON -> 0          (ThinPlateSpline, Laplacian, OneOverR2, OneOverR4)
  gradient paths   r2 <= DBL_EPSILON -> factor 0, value -sqrt(r2) (Linear), eval_r2 (Spheroidal), 0 (the others)
  Spheroidal       f64(s2 * r2) <= ip2 -> near branch, with s2, ip2, near_slope, far_coef derived ONCE in f64 as
                   SpheroidalRbfKernel::new does (they are the kernel's parameters, not part of a pair's arithmetic)
  extension kernels: no zero rule; their parameter 1 / range^2 is derived once in f64.
"""
import functools

import numpy as np

LD = np.longdouble
assert np.finfo(LD).nmant >= 63, "the reference needs a long double with at least 64 significand bits"

U = 2.0 ** -53                 # unit roundoff of f64
EPS = 2.0 ** -52               # DBL_EPSILON
DBL_MIN = np.finfo(np.float64).tiny
KERNEL_IDS = (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 100, 101)
SPHEROIDAL = (3, 4, 5, 6)
VALUE_ZERO_RULE = (1, 7, 8, 9)
NO_GRAD_ZERO_RULE = (100, 101)
# constants.rs: inflexion_point, linear_slope, range_scaling, inv_y_intercept (orders 3, 5, 7, 9)
SPHEROIDAL_CONSTANTS = {
    3: (0.5000000000, 0.7500000000, 2.6798340586, 0.8734640537),
    4: (0.4082482905, 1.0206207262, 1.5822795750, 0.8575980168),
    5: (0.3535533906, 1.2374368671, 1.2008676644, 0.8494862533),
    6: (0.3162277660, 1.4230249471, 1.0000000000, 0.8445585690),
}


class Params:
    """The parameters a kernel object holds (f64, derived once)."""

    def __init__(self, kid, base_range=1.0, total_sill=1.0):
        self.kid, self.base_range, self.total_sill = kid, np.float64(base_range), np.float64(total_sill)
        if kid in SPHEROIDAL:
            ip, slope, scaling, inv_y = (np.float64(c) for c in SPHEROIDAL_CONSTANTS[kid])
            s = scaling / self.base_range
            self.s2, self.ip2 = s * s, ip * ip
            self.near_slope, self.far_coef = self.total_sill * slope * s, self.total_sill * inv_y
            self.pow = kid - 2                       # 1, 2, 3, 4 for the orders 3, 5, 7, 9
        self.inv_br2 = np.float64(1.0) / (self.base_range * self.base_range)


def spheroidal_near(p, r2):
    """The reference's branch decision, in f64."""
    return p.s2 * np.asarray(r2, dtype=np.float64) <= p.ip2


def _ipow(t, n):
    out = t.copy()
    for _ in range(n - 1):
        out = out * t
    return out


def smooth(p, x, near=None):
    """(g, x g', f, x f') in long double WITHOUT the zero rules, at x > 0 (long double array).  `near`: the Spheroidal
    branch per element (default: the reference's decision on f64(x))."""
    kid = p.kid
    x = np.asarray(x, dtype=LD)
    with np.errstate(all="ignore"):
        if kid == 0:      # -r
            r = np.sqrt(x)
            return -r, -r / 2, -1 / r, 1 / (2 * r)
        if kid == 1:      # r^2 ln r = x ln(x) / 2
            lx = np.log(x)
            return x * lx / 2, x * (lx + 1) / 2, lx + 1, np.ones_like(x)
        if kid == 2:      # r^3
            r = np.sqrt(x)
            return x * r, 1.5 * x * r, 3 * r, 1.5 * r
        if kid in SPHEROIDAL:
            if near is None:
                near = spheroidal_near(p, x.astype(np.float64))
            sill, slope, fc, s2 = LD(p.total_sill), LD(p.near_slope), LD(p.far_coef), LD(p.s2)
            r = np.sqrt(x)
            gn, xgn, fn, xfn = sill - slope * r, -slope * r / 2, -slope / r, slope / (2 * r)
            q = LD(p.pow) + LD(0.5)                    # phi = far_coef * t^-q, t = 1 + s2 x
            t = 1 + s2 * x
            tq = _ipow(t, p.pow) * np.sqrt(t)         # t^q
            gf = fc / tq
            xgf = -q * fc * s2 * x / (tq * t)
            ff = -2 * q * s2 * fc / (tq * t)
            xff = 2 * q * (q + 1) * s2 * s2 * fc * x / (tq * t * t)
            return np.where(near, gn, gf), np.where(near, xgn, xgf), np.where(near, fn, ff), np.where(near, xfn, xff)
        if kid == 7:      # 1 / r
            ir = 1 / np.sqrt(x)
            return ir, -ir / 2, -ir / x, 1.5 * ir / x
        if kid == 8:      # 1 / r^2
            return 1 / x, -1 / x, -2 / (x * x), 4 / (x * x)
        if kid == 9:      # 1 / r^4
            return 1 / (x * x), -2 / (x * x), -4 / (x * x * x), 12 / (x * x * x)
        ib = LD(p.inv_br2)
        if kid == 100:    # exp(-r^2 / range^2)
            g = np.exp(-x * ib)
            return g, -x * ib * g, -2 * ib * g, 2 * ib * ib * x * g
        if kid == 101:    # sqrt(1 + r^2 / range^2)
            g = np.sqrt(1 + x * ib)
            return g, x * ib / (2 * g), ib / g, -ib * ib * x / (2 * g * g * g)
    raise ValueError(kid)


def value_is_zero(kid, r2):
    """The value paths' rule on f64 r2."""
    r2 = np.asarray(r2, dtype=np.float64)
    if kid in VALUE_ZERO_RULE:
        return np.sqrt(r2) < EPS
    return np.zeros(r2.shape, dtype=bool)


def grad_is_zero(kid, r2):
    """The gradient paths' rule on f64 r2."""
    r2 = np.asarray(r2, dtype=np.float64)
    if kid in NO_GRAD_ZERO_RULE:
        return np.zeros(r2.shape, dtype=bool)
    return r2 <= EPS


def evaluate(p, r2, x=None):
    """What the reference returns for f64 squared distances r2, in long double, and the sensitivities:
    dict(value, x_dvalue, value_g, factor, x_dfactor).  `x`: the exact squared distance in long double where r2 is its
    rounding (the pair sums); the rules are always decided on r2."""
    r2 = np.asarray(r2, dtype=np.float64)
    x = r2.astype(LD) if x is None else np.asarray(x, dtype=LD)
    safe = np.where(x > 0, x, LD(1))
    near = spheroidal_near(p, r2) if p.kid in SPHEROIDAL else None
    g, xg, f, xf = smooth(p, safe, near)
    at0 = ~(x > 0)
    if at0.any():         # limits at x = 0 of the kernels that have one (the others are zeroed by a rule below)
        g0 = {0: 0, 1: 0, 2: 0, 100: 1, 101: 1}.get(p.kid, LD(p.total_sill) if p.kid in SPHEROIDAL else 0)
        f0 = {100: -2 * LD(p.inv_br2), 101: LD(p.inv_br2)}.get(p.kid, 0)
        g, xg, f, xf = np.where(at0, LD(g0), g), np.where(at0, LD(0), xg), np.where(at0, LD(f0), f), np.where(at0, LD(0), xf)
    vz, gz = value_is_zero(p.kid, r2), grad_is_zero(p.kid, r2)
    zero = LD(0)
    value = np.where(vz, zero, g)
    if p.kid == 0 or p.kid in SPHEROIDAL:
        value_g = g                                    # -sqrt(r2) / eval_r2(r2) also under the gradient rule
    else:
        value_g = np.where(gz, zero, g)
    return {"value": value, "x_dvalue": np.where(vz, zero, xg), "value_g": value_g,
            "x_dvalue_g": xg if (p.kid == 0 or p.kid in SPHEROIDAL) else np.where(gz, zero, xg),
            "factor": np.where(gz, zero, f), "x_dfactor": np.where(gz, zero, xf)}


# ------------------------------------------------------------------ dense sums
class Dense:
    """The m x n kernel matrices of one (kernel, targets, sources) in long double, computed once and shared: sums for any
    weights come from them.  Coordinates are f64; differences, squares and their sum are formed in long double (exact for
    coordinates on a 2^-30 grid), and the rules are decided on the f64 rounding of the squared distance."""

    def __init__(self, kid, base_range, total_sill, targets, sources):
        t = np.atleast_2d(np.asarray(targets, dtype=np.float64)).astype(LD)
        s = np.atleast_2d(np.asarray(sources, dtype=np.float64)).astype(LD)
        self.d = t.shape[1]
        self.diff = t[:, None, :] - s[None, :, :]                       # m x n x d
        x = (self.diff * self.diff).sum(axis=2)
        self.r2 = x.astype(np.float64)
        e = evaluate(Params(kid, base_range, total_sill), self.r2, x)
        self.value, self.value_g, self.factor = e["value"], e["value_g"], e["factor"]
        self.abs_value, self.abs_x_dvalue = np.abs(e["value"]), np.abs(e["x_dvalue"])
        self.abs_value_g, self.abs_x_dvalue_g = np.abs(e["value_g"]), np.abs(e["x_dvalue_g"])
        self.abs_x_dfactor = np.abs(e["x_dfactor"])

    def sums(self, weights):
        """y = Phi W and the absolute sums sum_j |w_j| |phi_ij|, sum_j |w_j| |r2 phi'_ij|: each m x K, long double."""
        w = _as_ld_matrix(weights)
        aw = np.abs(w)
        return self.value @ w, self.abs_value @ aw, self.abs_x_dvalue @ aw

    def grad_sums(self, weights):
        """The gradient paths: (values m x K, gradients m x K x d, sum |w||phi|, sum |w||r2 phi'|,
        sum_j |w_j| |f_ij| |dx_a| as m x K x d, sum_j |w_j| |r2 f'_ij| |dx_a| as m x K x d)."""
        w = _as_ld_matrix(weights)
        aw = np.abs(w)
        ad = np.abs(self.diff)
        g = np.stack([(self.factor * self.diff[:, :, a]) @ w for a in range(self.d)], axis=2)
        ga = np.stack([(np.abs(self.factor) * ad[:, :, a]) @ aw for a in range(self.d)], axis=2)
        gx = np.stack([(self.abs_x_dfactor * ad[:, :, a]) @ aw for a in range(self.d)], axis=2)
        return self.value_g @ w, g, self.abs_value_g @ aw, self.abs_x_dvalue_g @ aw, ga, gx


def _as_ld_matrix(weights):
    w = np.asarray(weights, dtype=np.float64)
    return (w[:, None] if w.ndim == 1 else w).astype(LD)


def dense_sum(kid, base_range, total_sill, targets, sources, weights, with_grads=False):
    """y = K(X_t, X_s) W in long double (and the gradients as m x K x d)."""
    D = Dense(kid, base_range, total_sill, targets, sources)
    if not with_grads:
        return D.sums(weights)[0]
    v, g = D.grad_sums(weights)[:2]
    return v, g


class PairSums:
    """Everything the exact-sum tests need for one (kernel, targets, sources, weights), computed once in chunks of target
    rows (the m x n long-double matrices are never held whole).  Value path: y, s_phi, s_xd (m x K); gradient path (the
    first grad_cols right-hand sides): yg, g (m x Kg x d), sg_phi, sg_xd, s_f, s_xf (m x Kg x d)."""

    def __init__(self, kid, base_range, total_sill, targets, sources, weights, grad_cols, chunk=256):
        t = np.atleast_2d(np.asarray(targets, dtype=np.float64))
        w = np.asarray(weights, dtype=np.float64)
        parts, gparts = [], []
        for lo in range(0, t.shape[0], chunk):
            D = Dense(kid, base_range, total_sill, t[lo:lo + chunk], sources)
            parts.append(D.sums(w))
            gparts.append(D.grad_sums(w[:, :grad_cols]))
        self.y, self.s_phi, self.s_xd = (np.concatenate(c) for c in zip(*parts))
        self.yg, self.g, self.sg_phi, self.sg_xd, self.s_f, self.s_xf = (np.concatenate(c) for c in zip(*gparts))
        self.n_src = np.atleast_2d(sources).shape[0]


# ------------------------------------------------------------------ the pointwise input tables
def neighbours(x0, half):
    """The 2 * half + 1 consecutive doubles centred on x0 > 0."""
    x0 = np.float64(x0)
    i0 = int(np.array([x0]).view(np.int64)[0])
    return np.arange(i0 - half, i0 + half + 1, dtype=np.int64).view(np.float64)


SPHEROIDAL_RANGES = (1.0, 0.3, 0.5, 50.0)


def spheroidal_switch_table(kid, base_range):
    """(e): the 17 doubles centred on ip^2 / s^2."""
    p = Params(kid, base_range, 1.0)
    return neighbours(p.ip2 / p.s2, 8)


@functools.lru_cache(maxsize=None)
def r2_table(hi_exp=200):
    """Sets (a)-(d) and (f)-(h) of squared distances, deterministic; the part above 1e-300 sorted apart from the clamp
    region.  hi_exp: the top of the log-uniform range of (a) (2^200; lower for the Gaussian, which underflows)."""
    rng = np.random.default_rng(20260117)
    n = 200_000
    a = np.ldexp(1.0 + rng.random(n), rng.integers(-200, hi_exp, n).astype(np.int32))                 # (a)
    k = np.arange(-200, 201)
    b = np.concatenate([np.ldexp(1.0, k), np.ldexp(1.0 + 2.0 ** -52, k), np.ldexp(2.0 - 2.0 ** -52, k)])  # (b)
    c = np.arange(1, 1001, dtype=np.float64) ** 2                                                     # (c)
    d = np.concatenate([neighbours(EPS, 8), neighbours(EPS * EPS, 8)])                                # (d)
    kk = np.arange(1, 53)
    f = np.concatenate([neighbours(1.0, 16), 1.0 + np.ldexp(1.0, -kk), 1.0 - np.ldexp(1.0, -kk)])     # (f)
    g = np.concatenate([[0.0, 5e-324, 1e-310], neighbours(1e-300, 2)])                               # (g)
    h = np.concatenate([10.0 ** np.arange(61, 301, 1.0), [1e300]])                                    # (h)
    out = np.concatenate([a, b, c, d, f, g, h])
    out.setflags(write=False)
    return out


def table_for(kid, base_range=1.0):
    """The r2 table of one kernel: the common sets, and for the Spheroidal kernels (e) for this base_range."""
    if kid == 100:   # exp(-x / range^2) underflows past x = 745 range^2: (a) stops at 2^9 range^2, (h) keeps the tail
        t = r2_table(int(np.floor(np.log2(base_range * base_range))) + 9)
    else:
        t = r2_table()
    if kid in SPHEROIDAL:
        t = np.concatenate([t, spheroidal_switch_table(kid, base_range)])
    return t


SQRT_CLAMP = 1e-300          # below it bb_sqrt clamps the argument of its seed: absolute error only
ABS_CLASS_TOL = 1e-150       # sqrt(1e-300)


RANGE_GUARD = 2.0 ** 900     # see measured_class


def measured_class(ref, r2):
    """True where the relative measure applies: the reference result is zero by a rule, or a finite normal f64 that lies
    in 2^-900 .. 2^900, and the argument is outside the clamp region of bb_sqrt.  The guard band: a result within 2^124 of
    either end of the f64 range is formed from an intermediate -- r2 r2 r2, t^(p + 1), r r r -- that has already left it
    (the reference's own f64 arithmetic returns 0 or inf there as well), so only the class is asserted there."""
    with np.errstate(all="ignore"):
        r64 = np.abs(np.asarray(ref).astype(np.float64))
    normal = np.isfinite(r64) & (r64 >= 1.0 / RANGE_GUARD) & (r64 <= RANGE_GUARD)
    return (normal | (np.asarray(ref) == 0)) & (np.asarray(r2) >= SQRT_CLAMP)


def ulps(dev, ref):
    """|dev - ref| in ulps of the correctly rounded reference result (normal range)."""
    ref = np.asarray(ref, dtype=LD)
    with np.errstate(all="ignore"):
        r64 = np.abs(ref.astype(np.float64))
        return (np.abs(np.asarray(dev, dtype=np.float64).astype(LD) - ref) / np.spacing(r64).astype(LD)).astype(np.float64)
