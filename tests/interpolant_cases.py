"""Inputs and checks shared by tests/test_interpolant_host.py and the GPU tests of ferreus_rbf_rs_amd.rbf."""
import numpy as np

import interpolant_restatement as IR
from ferreus_rbf_rs_amd import rbf as RBF

TREND3 = (87.0, 255.0, 25.0, 4.0, 2.0, 1.0)           # the reference's isosurface_trend_linear example


def terms_case(d, degree, k, m=1000, seed=0):
    """world targets away from the origin, a random polynomial, translation / scale and an affine map"""
    rng = np.random.default_rng(1000 * d + 10 * (degree + 1) + k + seed)
    x = 50.0 + 20.0 * rng.random((m, d))
    nb = IR.basis_size(d, degree)
    lam = rng.standard_normal((nb, k)) if nb else None
    tr, sc = 55.0 + rng.random(d), 8.0 + 4.0 * rng.random(d)
    B = rng.standard_normal((d, d)) + 2.0 * np.eye(d)
    b = 10.0 * rng.standard_normal(d)
    terms = RBF.FieldTerms(d, degree, lam, tr, sc, B, b).with_columns(k)
    values = rng.standard_normal((m, k))
    grad = rng.standard_normal((m, k * d))
    return terms, x, values, grad, (lam, tr, sc, B, b)


def check_terms_against_numpy(terms, x, values, grad, parts, where):
    """contract 1 against the restatement: |delta| <= 1e-13 (|value added to| + sum_j |m_j lambda_j|) per entry (at most 10
    terms of at most 4 roundings each and the running sum: under 50 * 2^-53 = 6e-15)"""
    lam, tr, sc, B, b = parts
    d, k = terms.d, terms.k
    y = RBF.affine_points(terms, x, where)
    ref = x @ B + b
    assert (np.abs(y - ref) <= 1e-13 * (np.abs(x) @ np.abs(B) + np.abs(b))).all()
    g = RBF.trend_gradients(terms, grad, where)
    bound = np.abs(grad).reshape(-1, k, d) @ np.abs(B.T)
    assert (np.abs(g - IR.trend_gradients(grad, B, k)) <= 1e-13 * bound.reshape(g.shape)).all()
    if lam is None:
        v, g2 = RBF.polynomial_terms(terms, x, values, grad, where)
        assert np.array_equal(v, values) and np.array_equal(g2, grad)        # degree -1 adds nothing
        return y, g, v, g2
    v, g2 = RBF.polynomial_terms(terms, x, values, grad, where)
    pv, pg, va, ga = IR.polynomial(x, terms.degree, lam, tr, sc)
    assert (np.abs(v - (values + pv)) <= 1e-13 * (np.abs(values) + va)).all()
    assert (np.abs(g2 - (grad + pg)) <= 1e-13 * (np.abs(grad) + ga)).all()
    assert np.array_equal(RBF.polynomial_terms(terms, x, values, None, where), v)     # the values do not depend on the gradients
    return y, g, v, g2


def planted_duplicates(d=3, tol=2.0 ** -10, seed=5):
    """5,000 uniform points in the unit cube with, appended in index order: 300 exact copies, 300 copies displaced by
    0.5 tol, 300 by 1.5 tol, 100 chains a, b, c with |a - b|, |b - c| <= tol < |a - c|, 50 pairs astride a grid-cell
    boundary (cells of side about tol from the cloud's minimum corner, the origin) and one pair exactly tol apart along one axis.
    Returns (points, tol, expectations) with expectations = {index: kept?} for the planted points whose fate is known
    by construction."""
    rng = np.random.default_rng(seed)
    base = rng.random((5000, d))
    base[0] = 0.0                                        # the minimum corner is the origin: cell boundaries at multiples of tol
    expect = {}
    blocks = [base]
    n = len(base)

    def add(points, fates):
        nonlocal n
        blocks.append(points)
        for q, kept in enumerate(fates):
            if kept is not None:
                expect[n + q] = kept
        n += len(points)

    def direction(m):
        v = rng.standard_normal((m, d))
        return v / np.abs(v).max(axis=1, keepdims=True)   # infinity norm 1

    src = rng.choice(np.arange(1, 5000), 900, replace=False)
    add(base[src[:300]].copy(), [False] * 300)
    add(base[src[300:600]] + 0.5 * tol * direction(300), [None] * 300)   # (dropped unless their original was: the greedy decides)
    add(base[src[600:]] + 1.5 * tol * direction(300), [None] * 300)
    a = 2.0 + rng.random((100, d))                         # chains far from everything else and from each other
    a[:, 0] = 2.0 + 0.01 * np.arange(100)
    e0 = np.zeros(d)
    e0[0] = 1.0
    chain = np.empty((300, d))
    chain[0::3], chain[1::3], chain[2::3] = a, a + 0.75 * tol * e0, a + 1.5 * tol * e0
    add(chain, [True, False, True] * 100)
    p = 4.0 + rng.random((50, d))
    p[:, 0] = 4.0 + tol * (64 * np.arange(50) + 10)        # on a cell boundary along x
    pair = np.empty((100, d))
    pair[0::2], pair[1::2] = p - 0.25 * tol * e0, p + 0.25 * tol * e0
    add(pair, [True, False] * 50)
    q = np.full((1, d), 6.0)
    add(np.vstack([q, q + tol * e0]), [True, False])       # exactly tol apart (a power of two: the difference is exact): dropped
    pts = np.vstack(blocks)
    assert (pts[n - 1] - pts[n - 2])[0] == tol
    return pts, tol, expect


def check_duplicates(points, tol, where, expect=None):
    keep = RBF.remove_duplicates(points, tol, where)
    ref = IR.greedy_duplicates(points, tol)
    assert keep.dtype == np.int64 and np.array_equal(keep, ref), (len(keep), len(ref))
    if expect:
        kept = set(keep.tolist())
        wrong = [i for i, want in expect.items() if (i in kept) != want]
        assert not wrong, wrong[:10]
    return keep
