"""The device side of csrc/interpolant_terms.hip: the three per-target kernels against the host functions (one
__host__ __device__ definition, so bit for bit) and the numpy restatement, duplicate removal on the device against the
host path and the brute-force greedy, and bbfmm_evaluate_interpolant against the plain entry points."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import interpolant_cases as C
import interpolant_restatement as IR
import ferreus_rbf_rs_amd as F
from ferreus_rbf_rs_amd import rbf as RBF

HOST, DEVICE = 0, 1


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


# ---------------------------------------------------------------- contract 1
@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("degree", [-1, 0, 1, 2])
@pytest.mark.parametrize("d", [1, 2, 3])
def test_terms_on_the_device_equal_the_host_bit_for_bit(d, degree, k):
    """affine_points, polynomial_terms and trend_gradients: both sides compile the same function under fp contract(off) and
    divide by IEEE division, so every entry is the same double.  1,000 targets is no multiple of the block."""
    terms, x, values, grad, parts = C.terms_case(d, degree, k)
    host = C.check_terms_against_numpy(terms, x, values, grad, parts, HOST)
    dev = C.check_terms_against_numpy(terms, x, values, grad, parts, DEVICE)
    for h, v in zip(host, dev):
        assert same_bits(h, v)


def test_terms_over_more_than_one_grid_stride():
    terms, x, values, grad, parts = C.terms_case(3, 2, 1, m=256 * 4096 + 77)
    v = RBF.polynomial_terms(terms, x, values, None, DEVICE)
    assert same_bits(v, RBF.polynomial_terms(terms, x, values, None, HOST))


# ---------------------------------------------------------------- contract 3
@pytest.mark.parametrize("d", [3, 2])
def test_device_duplicate_removal_equals_host_and_greedy(d):
    pts, tol, expect = C.planted_duplicates(d)
    keep = C.check_duplicates(pts, tol, DEVICE, expect)
    assert np.array_equal(keep, RBF.remove_duplicates(pts, tol, HOST))


def test_device_duplicate_removal_edge_cases():
    pts, tol, _ = C.planted_duplicates(3)
    one_cell = pts[:6000] * 1e-3                             # 6,000 points inside one grid cell
    assert np.abs(one_cell).max() < 0.05
    C.check_duplicates(one_cell, 0.05, DEVICE)
    assert len(C.check_duplicates(pts, 0.0, DEVICE)) == len(pts) - 300
    assert RBF.remove_duplicates(pts[:1], tol, DEVICE).tolist() == [0]
    assert RBF.remove_duplicates(np.tile(pts[:1], (700, 1)), 0.0, DEVICE).tolist() == [0]
    line = np.cumsum(np.full(300, 0.75))[:, None] * np.ones((1, 3))   # a chain resolves one link per round
    keep, rounds = RBF.remove_duplicates(line, 1.0, DEVICE, return_rounds=True)
    assert keep.tolist() == list(range(0, 300, 2)) and rounds >= 150
    rng = np.random.default_rng(3)
    far = 1.0e6 + rng.random((2000, 3))                      # a tolerance far below the extent: cells larger than tol
    C.check_duplicates(np.vstack([far, far[:50] + 1e-13]), 1e-12, DEVICE)
    shuffled = pts[rng.permutation(len(pts))]                # the result follows the index order, not the positions
    C.check_duplicates(shuffled, tol, DEVICE)


# ---------------------------------------------------------------- contract 4
@pytest.fixture(scope="module")
def linear_tree():
    rng = np.random.default_rng(11)
    pts = rng.random((3000, 3))
    w = rng.standard_normal((3000, 2))
    x = 0.02 + 0.96 * rng.random((2000, 3))
    ext = [-0.5, -0.5, -0.5, 1.5, 1.5, 1.5]
    # deterministic: two runs of one pass on a default handle differ in their last bits themselves (f64 atomics)
    tree = F.FmmTree(pts, 5, F.KernelParams(F.KernelType.LinearRbf), True, False, extents=ext, deterministic=True)
    return tree, pts, w, x


@pytest.mark.parametrize("k", [1, 2])
def test_evaluate_interpolant_without_terms_is_the_plain_entry_point(linear_tree, k):
    tree, pts, w, x = linear_tree
    w = np.asfortranarray(w[:, :k])
    tree.set_weights(w)
    assert same_bits(RBF.evaluate_interpolant(tree, RBF.FULL, w, x), tree.evaluate(w, x))
    v, g = RBF.evaluate_interpolant(tree, RBF.FULL, w, x, RBF.FieldTerms(3).with_columns(k), True)
    pv, pg = tree.evaluate_with_gradients(w, x)
    assert same_bits(v, pv) and same_bits(g, pg)
    tree.set_local_coefficients(w)
    assert same_bits(RBF.evaluate_interpolant(tree, RBF.LEAVES, w, x), tree.evaluate_leaves(w, x))
    v, g = RBF.evaluate_interpolant(tree, RBF.LEAVES, w, x, None, True)
    pv, pg = tree.evaluate_leaves_with_gradients(w, x)
    assert same_bits(v, pv) and same_bits(g, pg)


@pytest.mark.parametrize("mode", [RBF.FULL, RBF.LEAVES])
@pytest.mark.parametrize("k", [1, 2])
def test_evaluate_interpolant_with_terms(linear_tree, k, mode):
    """plain evaluate at the numpy-transformed targets plus the numpy polynomial, to contract 1's bound plus 1e-12 max|f|
    (two batchings of one leaf pass): the transformed targets differ in their last bit"""
    tree, pts, w, x = linear_tree
    w = np.asfortranarray(w[:, :k])
    rng = np.random.default_rng(k)
    lam = rng.standard_normal((10, k))
    tr, sc = np.array([0.5, 0.4, 0.6]), np.array([0.5, 0.7, 0.45])
    a, _ = RBF.global_trend_transform(3, (20.0, 40.0, 10.0, 1.2, 1.0, 0.9), [0.5, 0.5, 0.5])
    B, b = a[:3, :3], a[3, :3]
    terms = RBF.FieldTerms(3, 2, lam, tr, sc, B, b)
    tree.set_weights(w)
    if mode == RBF.LEAVES:
        tree.set_local_coefficients(w)
    v, g = RBF.evaluate_interpolant(tree, mode, w, x, terms, True)
    xt = np.asfortranarray(x @ B + b)
    pv, pg = (tree.evaluate_with_gradients if mode == RBF.FULL else tree.evaluate_leaves_with_gradients)(w, xt)
    qv, qg, va, ga = IR.polynomial(x, 2, lam, tr, sc)
    tg = IR.trend_gradients(pg, B, k)
    assert (np.abs(v - (pv + qv)) <= 1e-13 * (np.abs(pv) + va) + 1e-12 * np.abs(pv).max()).all()
    assert (np.abs(g - (tg + qg)) <= 1e-13 * (np.abs(tg) + ga) + 1e-12 * np.abs(pg).max() * np.abs(B).sum()).all()
    assert same_bits(RBF.evaluate_interpolant(tree, mode, w, x, terms), v)            # values alone: the same values


def test_evaluate_interpolant_adds_the_nugget_at_the_sources(linear_tree):
    tree, pts, w, x = linear_tree
    w = np.asfortranarray(w[:, :1])
    tree.set_weights(w)
    v = RBF.evaluate_interpolant(tree, RBF.FULL, w, pts, RBF.FieldTerms(3), False, 0.25)
    assert same_bits(v, tree.evaluate(w, pts) + w * 0.25)
    with pytest.raises(ValueError, match="nugget"):                                        # not the sources: its own message
        RBF.evaluate_interpolant(tree, RBF.FULL, w, x, RBF.FieldTerms(3), False, 0.25)
    with pytest.raises(ValueError, match="bad terms"):
        RBF.evaluate_interpolant(tree, RBF.FULL, w, x, RBF.FieldTerms(2))
