"""The error budget of the kernel functions of csrc/kernels.hpp and the pointwise check built on it, shared by
test_kernel_reference_host.py (where = 0, no GPU), test_gpu_kernel_pointwise.py (where = 1) and test_gpu_pair_kernels.py
(the per-row tolerance of the exact sums).  A plain helper module.

Measure, with u = 2^-53 and x = r2:    |g_dev - g_ref| <= u * (a |g_ref| + b |x g_ref'(x)|)
a counts the roundings applied to the result, b those applied to the argument before the transcendental step.  The pairs
(a, b) are COUNTED from the code path, not tuned: a correctly rounded operation counts 1 (relative error u), a primitive
twice its bound in ulps (1 ulp = 2u), and a count is multiplied by the power the quantity is raised to.

Primitive bounds (ulps of the correctly rounded result):
  bb_sqrt, bb_sqrt_rsqrt   2     the claim of kernels.hpp (v_rsq_f64 seed + one cubic step)
  bb_rcp                   1     v_rcp_f64 seed + two FMA Newton steps
  bb_log                   3.1   normal x.  s = (m - 1) * rcp(m + 1): m - 1 exact (Sterbenz), m + 1 one rounding (1u), rcp
                                 1 ulp (2u), the product 1u -> 4u on s and on t = 2s.  The series term t s^2 p is at most 1 %
                                 of t (s^2 <= 0.0295, p <= 0.34), so its ~13u of roundings add 0.13u, its truncation (1e-18)
                                 0.01u.  e = 0: hi = 0, result = t + lo2: one more rounding -> 5.2u.  e != 0: e * ln2_hi is
                                 exact; |result| >= ln 2 - ln sqrt 2 = 0.347 >= |t + lo2|, so the errors of t stay 4u relative
                                 to the result, and t + lo2 and hi + (..) each add at most 1u -> 6.2u = 3.1 ulp.
  exp, pow (device)        2     no accuracy statement for the OCML double-precision functions was found in the ROCm
                                 documentation installed with the toolchain (share/doc, the headers); 2 ulp is the fallback
  host: libm and IEEE operations count 0.5 ulp (1u) each.
"""
import numpy as np

import kernel_reference as KR
from kernel_reference import LD, U

SQ = 4.0      # bb_sqrt / bb_sqrt_rsqrt: 2 ulp
RC = 2.0      # bb_rcp: 1 ulp
LG = 6.2      # bb_log: 3.1 ulp
EX = 4.0      # exp / pow of the device library: 2 ulp
PRIMITIVE_ULPS = {"sqrt": 2.0, "sqrt_rsqrt": 2.0, "rsqrt": 2.0, "rcp": 1.0, "log": 3.1}
# host: libm / IEEE, 0.5 ulp each; 1 / sqrt(x) is two roundings, 2u relative, which is up to 2 ulp of a result just above a power of two
HOST_PRIMITIVE_ULPS = {"sqrt": 0.5, "sqrt_rsqrt": 0.5, "rsqrt": 2.0, "rcp": 0.5, "log": 0.5}
MAX_ENTRY = 64.0
# Relative bounds of the refinement steps themselves, in u, derived from the device code (tighter than the ulp claims above,
# which they imply: a relative error of k u is at most k ulp).  With y the seed, E = 1 - x y^2 (|E| <= 1.1e-7):
#   bb_sqrt        t = fl(x y) = x y (1 + d1); e = 1 - t y = E - d1 (one FMA, its rounding is u |e|); the result
#                  fl(t + (t e) p) = sqrt(x) (1 + d1 / 2) (1 + d2) (1 + 5 E^3 / 16): 1.5 u, the rest (roundings of p and t e,
#                  the cubic truncation) below 1e-6 u
#   bb_sqrt_rsqrt  r = fl(y + (y e) p) = x^-1/2 (1 - d1 / 2) (1 + d2): 1.5 u; s = fl(x r): 2.5 u
#   bb_rcp         after the first Newton step e = 1 - x y is a rounding-level quantity computed by one FMA; the second
#                  step's fl(y + y e) is one rounding of a value whose own error is e^2: 1 u
# A wrong coefficient of the cubic step (0.375 -> 0.37) adds up to 0.005 E^2 = 0.49 u: invisible to the 2 ulp claim, not to these.
REL_U = {"sqrt": 1.5001, "sqrt_rsqrt": 2.5001, "rsqrt": 1.5001, "rcp": 1.0001}


def _spheroidal(where, P):
    """P = 1..4 (orders 3..9), q = P + 1/2; phi = sill - slope sqrt(x) (near), far_coef t^-q with t = 1 + s2 x (far)."""
    q = P + 0.5
    if where == 1:
        return {
            # sq 2 ulp (4) and the product (1) act on slope sqrt(x) = 2 |x g'|: b = 10; the subtraction: a = 1
            "value_near": (1.0, 2 * (SQ + 1)),
            # fl(s2 x): exactly a relative perturbation of x (b = 1); fl(1 + .) is one of t, raised to q (a += q);
            # rs 2 ulp (4), rs2 = rs rs (2 * 4 + 1 = 9), rp = rs rs2^P (4 + P (9 + 1)), far_coef * rp (1)
            "value_far": (q + SQ + P * (2 * SQ + 2) + 1, 1.0),
            "factor_near": (SQ + 2, 0.0),             # sqrt (4), 1 / r (1), the product with near_slope (1)
            # t as above raised to q + 1 (a += q + 1, b = 1); pow 2 ulp (4); (-2p) s2, .. far_coef, the division (3)
            "factor_far": (q + 1 + EX + 3, 1.0),
        }
    return {
        "value_near": (1.0, 2 * 2.0),                 # sqrt (1) and the product (1) on slope sqrt(x) = 2 |x g'|; subtraction
        "value_far": (q + (P - 1) + 3, 1.0),          # t (q, b = 1); t^P (P - 1), sqrt (1), tp sqrt(t) (1), the division (1)
        "factor_near": (3.0, 0.0),                    # sqrt, 1 / r, the product
        "factor_far": (q + 1 + 1 + 3, 1.0),           # t (q + 1, b = 1), pow (1), two products and the division (3)
    }


def budget(where, kid):
    """{path: (a, b)} for the paths value / value_g / factor of kernel kid (Spheroidal: *_near and *_far)."""
    dev = where == 1
    if kid == 0:     # -sqrt(x); factor -1 / r
        s = SQ if dev else 1.0
        return {"value": (s, 0.0), "value_g": (s, 0.0), "factor": (s + 1, 0.0)}
    if kid == 1:
        if dev:
            # value 0.5 x log(x): log (6.2), one product (0.5 x is exact).  value_g x (0.5 log x): the same.
            # factor log(x) + 1: the error of log is 6.2u |ln x| <= 6.2u (|f| + 1) and x f' = 1: a = 6.2 + 1 (the addition), b = 6.2
            return {"value": (LG + 1, 0.0), "value_g": (LG + 1, 0.0), "factor": (LG + 1, LG)}
        # host: r = sqrt(x) carries 1u, so log(r) is off by u absolute (argument) + u |ln r| (its rounding).
        # value (r r) log r: r r (3), log (1), product (1) on g, and u x for the argument, x = 2 (x g' - g): a = 5 + 2, b = 2
        # value_g x log r: log (1), product (1), u x: a = 2 + 2, b = 2
        # factor 2 log r + 1: 2 (u + u |ln r|) = 2u + u |ln x| <= 3u + u |f|, the addition u |f|: a = 2, b = 3 (x f' = 1)
        return {"value": (7.0, 2.0), "value_g": (4.0, 2.0), "factor": (2.0, 3.0)}
    if kid == 2:     # r r r: 3 sqrt + 2; x r: sqrt + 1; 3 r: sqrt + 1
        s = SQ if dev else 1.0
        return {"value": (3 * s + 2, 0.0), "value_g": (s + 1, 0.0), "factor": (s + 1, 0.0)}
    if kid in KR.SPHEROIDAL:
        t = _spheroidal(where, kid - 2)
        return {"value_near": t["value_near"], "value_far": t["value_far"], "value_g_near": t["value_near"],
                "value_g_far": t["value_far"], "factor_near": t["factor_near"], "factor_far": t["factor_far"]}
    if kid == 7:
        if dev:      # value rs (2 ulp); value_g 1 / bb_sqrt (4 + 1); factor -(ir ir ir): 3 * 5 + 2
            return {"value": (SQ, 0.0), "value_g": (SQ + 1, 0.0), "factor": (3 * (SQ + 1) + 2, 0.0)}
        return {"value": (2.0, 0.0), "value_g": (2.0, 0.0), "factor": (8.0, 0.0)}     # sqrt, division; ir^3: 3 * 2 + 2
    if kid == 8:
        if dev:      # value bb_rcp (1 ulp); value_g 1 / x; factor -2 (1 / (x x)): product, division
            return {"value": (RC, 0.0), "value_g": (1.0, 0.0), "factor": (2.0, 0.0)}
        return {"value": (4.0, 0.0), "value_g": (1.0, 0.0), "factor": (2.0, 0.0)}     # value 1 / (r r): 2 sqrt + product + division
    if kid == 9:
        if dev:      # value q q, q = bb_rcp: 2 * 2 + 1; value_g 1 / (x x); factor -4 (1 / (x x x))
            return {"value": (2 * RC + 1, 0.0), "value_g": (2.0, 0.0), "factor": (3.0, 0.0)}
        return {"value": (8.0, 0.0), "value_g": (2.0, 0.0), "factor": (3.0, 0.0)}     # (r r) (r r): 2 * 3 + 1, division
    e = EX if dev else 1.0
    if kid == 100:   # exp(-(x ib)): the product perturbs the argument (b = 1), exp; factor (-2 ib) v: one more product
        return {"value": (e, 1.0), "value_g": (e, 1.0), "factor": (e + 1, 1.0)}
    if kid == 101:   # sqrt(1 + x ib): the product (b = 1), the addition raised to 1/2 (0.5), sqrt; factor ib / v: division
        s = SQ if dev else 1.0
        return {"value": (0.5 + s, 1.0), "value_g": (0.5 + s, 1.0), "factor": (0.5 + s + 1, 1.0)}
    raise ValueError(kid)


def sum_budget(where, kid, path):
    """(a, b) of a path for the pair sums: the larger of the branches."""
    bud = budget(where, kid)
    ent = [v for k, v in bud.items() if k == path or k in (path + "_near", path + "_far")]
    return max(a for a, _ in ent), max(b for _, b in ent)


def coefficients(where, p, path, r2):
    bud = budget(where, p.kid)
    if p.kid in KR.SPHEROIDAL:
        near = KR.spheroidal_near(p, r2)
        (an, bn), (af, bf) = bud[path + "_near"], bud[path + "_far"]
        return np.where(near, an, af), np.where(near, bn, bf)
    a, b = bud[path]
    return np.full(r2.shape, a), np.full(r2.shape, b)


def check_kernel(where, kid, base_range, total_sill, values, r2=None):
    """Asserts the three outputs of bbfmm_debug_kernel_values (`values` = (value, value_g, factor) at the table of the
    kernel, or at r2) against the reference; returns {path: (largest measure / bound, largest error in u |g_ref|)}."""
    p = KR.Params(kid, base_range, total_sill)
    r2 = KR.table_for(kid, base_range) if r2 is None else r2
    e = KR.evaluate(p, r2)
    out = {}
    for path, dev, xd in (("value", values[0], "x_dvalue"), ("value_g", values[1], "x_dvalue_g"), ("factor", values[2], "x_dfactor")):
        ref = e[path]
        dev = np.asarray(dev, dtype=np.float64)
        meas = KR.measured_class(ref, r2)
        # the class check.  Towards overflow: the same infinity, or (inside the guard band) a finite value that agrees to
        # 2^-40; towards underflow and in the clamp region of bb_sqrt: finite, absolute error at most sqrt(1e-300)
        with np.errstate(all="ignore"):
            r64 = ref.astype(np.float64)
            aerr = np.abs(dev.astype(LD) - ref)
        rest = ~meas
        big = rest & (np.abs(r64) > 1.0)
        inf = big & np.isinf(dev)
        assert np.array_equal(np.sign(dev[inf]), np.sign(r64[inf])), (kid, path, "overflow class")
        assert (aerr[big & ~inf] <= np.ldexp(np.abs(ref[big & ~inf]), -40)).all() and not np.isnan(dev[big]).any(), \
            (kid, path, "finite near the top of the range but wrong")
        assert not (inf & (np.abs(r64) <= KR.RANGE_GUARD)).any(), (kid, path, "infinite below the guard band")
        fin = rest & ~big
        assert np.isfinite(dev[fin]).all(), (kid, path, "finite class")
        assert (aerr[fin] <= KR.ABS_CLASS_TOL).all(), (kid, path, "absolute error outside the normal range", r2[fin][np.argmax(aerr[fin])])
        assert (dev[fin & (ref == 0)] == 0).all(), (kid, path, "exact zero expected (r2 = 0 or a zero rule)")
        # which side of a rule (they all sit at or below DBL_EPSILON): an exact zero on one side only is another decision
        low = meas & (r2 < 2.0 ** -40)
        assert np.array_equal(dev[low] == 0, ref[low] == 0), \
            (kid, path, "zero rule decided differently at r2 =", r2[low][(dev[low] == 0) != (ref[low] == 0)][:5])
        a, b = coefficients(where, p, path, r2)
        assert a.max() <= MAX_ENTRY and b.max() <= MAX_ENTRY
        den = LD(U) * (a * np.abs(ref) + b * np.abs(e[xd]))
        assert np.isfinite(dev[meas]).all(), (kid, path, "not finite in the measured class")
        ok = meas & (den > 0)
        ratio = (aerr[ok] / den[ok]).astype(np.float64)
        nz = meas & (ref != 0)
        rel = (aerr[nz] / (LD(U) * np.abs(ref[nz]))).astype(np.float64)
        i = int(np.argmax(ratio))
        out[path] = (float(ratio.max()), float(rel.max()))
        print(f"kernel {kid} range {base_range} where {where} {path}: measure / bound {ratio.max():.3f} at r2 = {r2[ok][i]!r} "
              f"(a, b = {a[ok][i]}, {b[ok][i]}); largest error {rel.max():.2f} u |g|; measured class {meas.mean():.4f}")
        assert ratio.max() <= 1.0, (kid, path, float(ratio.max()), r2[ok][i])
    return out


def primitive_inputs(which):
    t = KR.r2_table()
    if which in ("rcp", "log"):
        t = t[t >= 2.0 ** -1000]       # x > 0 and normal, 1 / x normal
    return t


def check_primitive(where, which, outs, x=None):
    """bb_sqrt / bb_sqrt_rsqrt / bb_rcp / bb_log against long double; returns the largest error in ulps (per output)."""
    x = primitive_inputs(which) if x is None else x
    bounds = PRIMITIVE_ULPS if where == 1 else HOST_PRIMITIVE_ULPS
    xl = x.astype(LD)
    res = {}
    with np.errstate(all="ignore"):
        refs = {"sqrt": [np.sqrt(xl)], "sqrt_rsqrt": [np.sqrt(xl), 1 / np.sqrt(xl)], "rcp": [1 / xl], "log": [np.log(xl)]}[which]
    outs = outs if isinstance(outs, tuple) else (outs,)
    for name, dev, ref in zip(("out", "out2"), outs, refs):
        bound = bounds["rsqrt" if name == "out2" else which]
        big = x >= KR.SQRT_CLAMP
        if which == "log":
            big &= x != 1.0
            assert (dev[x == 1.0] == 0).all()
        ul = KR.ulps(dev[big], ref[big])
        i = int(np.argmax(ul))
        nz = big & (ref != 0)
        rel = (np.abs(dev[nz].astype(LD) - ref[nz]) / (LD(U) * np.abs(ref[nz]))).astype(np.float64)
        res[name] = float(ul.max())
        res[name + "_rel_u"] = float(rel.max())
        print(f"{which} {name} where {where}: largest error {ul.max():.3f} ulp at x = {x[big][i]!r} (bound {bound}); "
              f"{rel.max():.4f} u relative at x = {x[nz][int(np.argmax(rel))]!r}")
        assert ul.max() <= bound, (which, name, float(ul.max()), x[big][i])
        if where == 1 and which != "log":
            key = "rsqrt" if name == "out2" else which
            assert rel.max() <= REL_U[key], (which, name, "relative error in u", float(rel.max()), REL_U[key])
        if name == "out" and which.startswith("sqrt"):        # the clamp region: exact zero at 0, absolute error below
            small = ~big
            assert (dev[x == 0] == 0).all()
            assert np.isfinite(dev[small]).all()
            assert (np.abs(dev[small].astype(LD) - ref[small]) <= KR.ABS_CLASS_TOL).all()
    return res
