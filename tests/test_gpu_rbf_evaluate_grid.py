"""RBFInterpolator.evaluate_grid and tensor targets of evaluate_targets[_with_gradients] against the numpy path of
evaluate_targets at the same nodes."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import interpolant_cases as C
import interpolant_restatement as IR
from evaluate_grid_restatement import grid_coords, rotation_z
from ferreus_rbf_rs_amd import rbf as RBF

K, D = RBF.RBFKernelType, RBF.Drift
ORIGIN, SPACING, SHAPE = [1.6, 0.7, 0.6], [0.3, 0.25, 0.2], [12, 10, 9]
AXES = rotation_z(30.0)                              # x in [0.47, 4.46], y in [0.7, 4.3], z in [0.6, 2.2]


@pytest.fixture(scope="module")
def fit():
    """1,500 signed distances of a sphere (below naive_solve_threshold: one dense solve), a linear drift, two value
    columns and the global trend of the reference's example"""
    rng = np.random.default_rng(9)
    pts = rng.uniform(0.5, 5.5, (1500, 3))
    r = np.linalg.norm(pts - 3.0, axis=1)
    vals = np.stack([r - 1.8, np.sin(pts[:, 0]) + 0.3 * pts[:, 2]], axis=1)
    st = RBF.InterpolantSettings(K.Linear, drift=D.Linear)
    return RBF.RBFInterpolator(pts, vals, st, RBF.Params(K.Linear, deterministic=True), RBF.GlobalTrend.three(*C.TREND3))


def bounds(fit, x):
    """per entry: 1e-13 (|kernel sum| + sum_j |m_j lambda_j|) + 1e-12 max|kernel sum| for the values, and the same with the
    trend's chain rule for the gradients (the bar of test_gpu_isosurface_terms.py and test_gpu_rbf_interpolator.py)"""
    gt, k = fit.global_trend, fit.source_values.shape[1]
    kv, kg = fit._evaluator.evaluate_leaves_with_gradients(None, np.asfortranarray(x @ gt.B + gt.b))
    _, _, va, ga = IR.polynomial(x, fit.settings.polynomial_degree, fit.coefficients.poly_coefficients, fit.translation_factor,
                                 fit.scale_factor)
    tg = IR.trend_gradients(kg, gt.B, k)
    return (1e-13 * (np.abs(kv) + va) + 1e-12 * np.abs(kv).max(), 1e-13 * (np.abs(tg) + ga) + 1e-12 * np.abs(kg).max() * np.abs(gt.B).sum())


def test_grid_without_an_evaluator_raises(fit):
    assert fit._evaluator is None
    with pytest.raises(ValueError):
        fit.evaluate_grid(ORIGIN, SPACING, SHAPE)


def test_grid_and_tensor_targets_against_evaluate_targets(fit):
    import torch
    fit.build_evaluator([-1.0, -1.0, -1.0, 7.0, 7.0, 7.0])
    steps = np.asarray(SPACING)[:, None] * AXES
    x = np.asfortranarray(grid_coords(ORIGIN, steps, SHAPE))
    ref_v, ref_g = fit.evaluate_targets_with_gradients(x)
    assert ref_v.shape == (len(x), 2) and ref_g.shape == (len(x), 6)
    bv, bg = bounds(fit, x)
    v, g, stats = fit.evaluate_grid(ORIGIN, SPACING, SHAPE, axes=AXES, gradients=True, max_job_targets=16, return_stats=True)
    assert v.shape == (*SHAPE, 2) and g.shape == (*SHAPE, 2, 3) and stats["nodes"] == len(x) and stats["largest_job"] <= 16
    ev, eg = np.abs(v.reshape(-1, 2) - ref_v), np.abs(g.reshape(-1, 6) - ref_g)
    print(f"evaluate_grid against evaluate_targets: values {ev.max():.3g} (smallest bound {bv.min():.3g}), "
          f"gradients {eg.max():.3g} (smallest bound {bg.min():.3g})")
    assert (ev <= bv).all() and (eg <= bg).all()
    assert (np.abs(fit.evaluate_grid(ORIGIN, SPACING, SHAPE, axes=AXES).reshape(-1, 2) - fit.evaluate_targets(x)) <= bv).all()
    # axis-aligned by default, one spacing for every axis
    va = fit.evaluate_grid([1.0, 1.0, 1.0], 0.4, [5, 4, 3])
    xa = np.asfortranarray(grid_coords([1.0, 1.0, 1.0], 0.4 * np.eye(3), [5, 4, 3]))
    assert (np.abs(va.reshape(-1, 2) - fit.evaluate_targets(xa)) <= bounds(fit, xa)[0]).all()
    # tensors on the evaluator's device come back as tensors
    xt = torch.from_numpy(np.ascontiguousarray(x)).to(f"cuda:{fit._evaluator.device()}")
    tv = fit.evaluate_targets(xt)
    tv2, tg = fit.evaluate_targets_with_gradients(xt)
    assert isinstance(tv, torch.Tensor) and tv.is_cuda and tv.shape == ref_v.shape and tg.shape == ref_g.shape
    assert (np.abs(tv.cpu().numpy() - ref_v) <= bv).all() and (np.abs(tv2.cpu().numpy() - ref_v) <= bv).all()
    assert (np.abs(tg.cpu().numpy() - ref_g) <= bg).all()
    assert isinstance(fit.evaluate_targets(x), np.ndarray)                   # numpy input keeps its path
