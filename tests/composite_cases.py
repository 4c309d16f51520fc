"""The clouds, fits and evaluator trees the composite-field tests share (built once per process), and the place their
measured figures go."""
import functools
import json
import os

import numpy as np

import interpolant_cases as C
import ferreus_rbf_rs_amd as F
from ferreus_rbf_rs_amd import rbf as RBF

K, D = RBF.RBFKernelType, RBF.Drift
EXT = [0.0, 0.0, 0.0, 6.0, 6.0, 6.0]
RES = 0.3                                             # 45 x 33 x 33 nodes in the box of E
CENTRE, RADIUS = np.array([3.0, 3.0, 3.0]), 1.8


def sdf(p):
    return np.linalg.norm(p - CENTRE, axis=1) - RADIUS


def topography(uv):
    return 3.4 + 0.5 * np.sin(0.9 * uv[:, 0]) * np.cos(0.7 * uv[:, 1])


def same_mesh(a, b):
    return a[0].shape == b[0].shape and np.array_equal(a[1], b[1]) and np.array_equal(a[0].view(np.uint64), b[0].view(np.uint64))


def cloud(seed, n, d):
    """non-uniform: half the points uniform in [0.5, 5.5]^d, half in a tight cluster, so the adaptive tree has leaves on
    several levels (W lists) and, with the evaluator's padding, empty regions"""
    rng = np.random.default_rng(seed)
    a = rng.uniform(0.5, 5.5, (n // 2, d))
    b = np.clip(rng.normal(size=(n - n // 2, d)) * 0.3 + np.array([2.2, 3.9, 3.6])[:d], 0.5, 5.5)
    return np.concatenate([a, b])


def evaluator_extents(fit, axes, extents=EXT, resolution=RES):
    """the union of the source and isosurface extents +- 10 resolutions on the given axes, in world coordinates"""
    pts = fit.source_points
    ext = np.asarray(extents, dtype=np.float64)
    lo, hi = ext[:3][list(axes)], ext[3:][list(axes)]
    return np.concatenate([np.minimum(pts.min(0), lo) - 10.0 * resolution, np.maximum(pts.max(0), hi) + 10.0 * resolution])


def evaluator(fit, axes, extents=EXT, resolution=RES, column=0):
    """the tree RBFInterpolator.build_isosurfaces makes (rbf.rs:990-1000) on the given axes of the extents, by hand"""
    d = len(axes)
    ev = evaluator_extents(fit, axes, extents, resolution)
    if fit.global_trend is not None:
        corners = np.array([[ev[j + d] if (i >> j) & 1 else ev[j] for j in range(d)] for i in range(1 << d)])
        ct = fit.global_trend.transform_points(corners, 0)
        ev = np.concatenate([ct.min(0), ct.max(0)])
    t = F.FmmTree(fit._tpoints, fit.params.fmm_params.interpolation_order, fit.settings.kernel_params(), True, False, extents=list(ev),
                  params=fit.params.fmm_params.to_tree(), deterministic=True)
    w = np.asfortranarray(fit.coefficients.point_coefficients[:, column:column + 1])
    t.set_weights(w)
    t.set_local_coefficients(w)
    return t


@functools.lru_cache(maxsize=None)
def model():
    """(fit, tree): 3,000 signed distances of a sphere, Linear kernel, quadratic drift and the reference example's trend"""
    pts = cloud(5, 3000, 3)
    fit = RBF.RBFInterpolator(pts, sdf(pts), RBF.InterpolantSettings(K.Linear, drift=D.Quadratic), RBF.Params(K.Linear, deterministic=True),
                              RBF.GlobalTrend.three(*C.TREND3))
    tree = evaluator(fit, (0, 1, 2))
    s = tree.stats()
    assert s.depth >= 2 and s.n_w > 0 and s.n_leaves > 8
    return fit, tree


@functools.lru_cache(maxsize=None)
def plain():
    """(points, tree, level): a tree over the 3-D cloud in world coordinates with random weights and no terms at all; its
    kernel sum's median over the points as a level that has a surface"""
    pts = cloud(5, 3000, 3)
    ev = np.concatenate([np.minimum(pts.min(0), EXT[:3]) - 10.0 * RES, np.maximum(pts.max(0), EXT[3:]) + 10.0 * RES])
    t = F.FmmTree(pts, 7, F.KernelParams(F.FmmKernelType.LinearRbf), True, False, extents=list(ev), deterministic=True)
    w = np.asfortranarray(np.random.default_rng(9).normal(size=(len(pts), 1)))
    t.set_weights(w)
    t.set_local_coefficients(w)
    return pts, t, float(np.median(t.evaluate_leaves(None, np.asfortranarray(pts))[:, 0]))


@functools.lru_cache(maxsize=None)
def topo():
    """(fit, tree): 2,000 heights of a 2-D topography, Linear kernel with a linear drift"""
    uv = cloud(6, 2000, 2)
    fit = RBF.RBFInterpolator(uv, topography(uv), RBF.InterpolantSettings(K.Linear, drift=D.Linear), RBF.Params(K.Linear, deterministic=True))
    tree = evaluator(fit, (0, 1))        # EXT is a cube: the same square serves every axis
    s = tree.stats()
    assert s.d == 2 and s.depth >= 2 and s.n_w > 0
    return fit, tree


WHAT = ("figures the tests of composite fields print (tests/composite_cases.py record): errors of a HEIGHT operand's lattice field and "
        "gradients against the host-target evaluate_leaves of the same handle (bounds from 1e-12 max|g|, the standing bound of two "
        "batchings of one leaf pass), and the largest vertex difference between evaluate_targets as a callable and the FieldExpr of "
        "the same model (bound 1e-12 max|f| / min|grad f|); lattice 45 x 33 x 33 nodes, MI355X")


@functools.lru_cache(maxsize=None)
def topo_trend():
    """(fit, tree): the same heights with a linear drift and a 2-D global trend (rotated 30 degrees, ratio 2)"""
    uv = cloud(6, 2000, 2)
    fit = RBF.RBFInterpolator(uv, topography(uv), RBF.InterpolantSettings(K.Linear, drift=D.Linear), RBF.Params(K.Linear, deterministic=True),
                              RBF.GlobalTrend.two(30.0, 2.0, 1.0))
    tree = evaluator(fit, (0, 1))
    assert fit.terms(1).B is not None and tree.stats().d == 2
    return fit, tree


def record(name, value, bound):
    """print a measured figure, and put it into the JSON file COMPOSITE_FIELD_ACCURACY_JSON names, if any (the layout of
    profiles/composite_field_accuracy.json)"""
    print(f"{name}: measured {value:.3g}, bound {bound:.3g}")
    path = os.environ.get("COMPOSITE_FIELD_ACCURACY_JSON")
    if not path:
        return
    data = {"what": WHAT, "figures": {}}
    if os.path.exists(path):
        with open(path) as f:
            data = json.load(f)
    data["figures"][name] = {"measured": float(value), "bound": float(bound)}
    with open(path, "w") as f:
        json.dump(data, f, indent=1, sort_keys=True)
        f.write("\n")
