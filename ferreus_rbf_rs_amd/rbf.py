"""ferreus_rbf::RBFInterpolator (ferreus_rbf/src/rbf.rs:304-1172) over the pieces of this package: one object that fits,
evaluates and meshes.  The names and signatures mirror py_ferreus_rbf (ferreus_rbf.pyi, interpolant_config, config,
progress, isosurfacing), so the reference's example scripts run with only their imports changed.

The facade is glue: the tree, the Schwarz preconditioner, the solvers, the evaluators and the isosurfacer are the
existing entry points.  What it adds on the device is in csrc/interpolant_terms.{hpp,hip}: the global trend's affine map
of the targets, the polynomial part with its gradient, the trend's chain rule on gradients, and duplicate removal.
DESIGN.md "The interpolant around the tree" has the contracts, the arithmetic order and the differences from the reference.

Not implemented (NotImplementedError): boundary closure (ClosePositive / CloseNegative), save_model / load_model.
"""
from __future__ import annotations

import ctypes
import enum
import time
from typing import Callable, List, Optional, Union

import numpy as np

from . import _lib as L
from . import ddm as _ddm
from . import solvers as _solvers
from .fmm_tree import FmmParams as _TreeFmmParams
from .fmm_tree import FmmTree, KernelParams, KernelType, M2LCompressionType, SpheroidalOrder

__all__ = ["RBFInterpolator", "GlobalTrend", "InterpolantSettings", "RBFKernelType", "SpheroidalOrder", "Drift", "FittingAccuracy",
           "FittingAccuracyType", "Params", "FmmParams", "DDMParams", "Solvers", "FmmCompressionType", "Coefficients", "Mesh",
           "BoundaryClosure", "ClusterMethod", "Progress", "DuplicatesRemoved", "SolverIteration", "SurfacingProgress", "Message", "FieldTerms",
           "global_trend_transform", "duplicate_cutoff_distance", "remove_duplicates", "affine_points", "polynomial_terms",
           "trend_gradients", "evaluate_interpolant", "default_drift", "default_fmm_interpolation_order"]


# ------------------------------------------------------------------------------------------------ interpolant_config
class Drift(enum.Enum):
    """interpolant_config.rs:24-33"""
    None_ = 0
    Constant = 1
    Linear = 2
    Quadratic = 3

    @property
    def degree(self) -> int:
        return self.value - 1


class RBFKernelType(enum.Enum):
    """interpolant_config.rs:35-42"""
    Linear = 0
    ThinPlateSpline = 1
    Cubic = 2
    Spheroidal = 3


class FittingAccuracyType(enum.Enum):
    """interpolant_config.rs:54-63 (the reference's numbering; solvers.FittingAccuracyType has the ABI's)"""
    Relative = 0
    Absolute = 1


def default_drift(kernel_type: RBFKernelType) -> Drift:
    """get_min_drift, interpolant_config.rs:44-52: the default and the least drift of each kernel"""
    return {RBFKernelType.Linear: Drift.Constant, RBFKernelType.ThinPlateSpline: Drift.Linear, RBFKernelType.Cubic: Drift.Linear,
            RBFKernelType.Spheroidal: Drift.None_}[RBFKernelType(kernel_type)]


def default_fmm_interpolation_order(kernel_type: RBFKernelType) -> int:
    """get_default_fmm_interpolation_order, config.rs:200-207"""
    return {RBFKernelType.Linear: 7, RBFKernelType.ThinPlateSpline: 9, RBFKernelType.Cubic: 11}.get(RBFKernelType(kernel_type), 7)


class FittingAccuracy:
    """interpolant_config.rs:80-92"""

    def __init__(self, tolerance: float = 1e-6, tolerance_type: FittingAccuracyType = FittingAccuracyType.Relative):
        self.tolerance = float(tolerance)
        self.tolerance_type = FittingAccuracyType(tolerance_type)

    def to_solver(self) -> _solvers.FittingAccuracy:
        return _solvers.FittingAccuracy(self.tolerance, _solvers.FittingAccuracyType[self.tolerance_type.name])


class InterpolantSettings:
    """InterpolantSettings (interpolant_config.rs:118-190).  to_ddm(d) is the ddm.InterpolantSettings the solver reads."""

    def __init__(self, kernel_type: RBFKernelType, spheroidal_order: Optional[SpheroidalOrder] = None, drift: Optional[Drift] = None,
                 nugget: Optional[float] = None, base_range: Optional[float] = None, total_sill: Optional[float] = None,
                 fitting_accuracy: Optional[FittingAccuracy] = None):
        self.kernel_type = RBFKernelType(kernel_type)
        self.spheroidal_order = SpheroidalOrder.Three if spheroidal_order is None else SpheroidalOrder(spheroidal_order)
        least = default_drift(self.kernel_type)
        self.drift = least if drift is None else Drift(drift)
        if self.drift.value < least.value:
            raise ValueError(f"Min degree for kernel: {least.degree}")                       # interpolant_config.rs:173
        self.nugget = 0.0 if nugget is None else float(nugget)
        self.base_range = 1.0 if base_range is None else float(base_range)
        self.total_sill = 1.0 if total_sill is None else float(total_sill)
        self.fitting_accuracy = fitting_accuracy or FittingAccuracy()

    @property
    def polynomial_degree(self) -> int:
        return self.drift.degree

    @property
    def kernel_id(self) -> KernelType:
        if self.kernel_type is RBFKernelType.Spheroidal:
            return {3: KernelType.Spheroidal3Rbf, 5: KernelType.Spheroidal5Rbf, 7: KernelType.Spheroidal7Rbf,
                    9: KernelType.Spheroidal9Rbf}[self.spheroidal_order.value]
        return {RBFKernelType.Linear: KernelType.LinearRbf, RBFKernelType.ThinPlateSpline: KernelType.ThinPlateSplineRbf,
                RBFKernelType.Cubic: KernelType.CubicRbf}[self.kernel_type]

    def kernel_params(self) -> KernelParams:
        return KernelParams(self.kernel_id, base_range=self.base_range, total_sill=self.total_sill)

    def to_ddm(self, dimensions: int) -> _ddm.InterpolantSettings:
        return _ddm.InterpolantSettings(int(self.kernel_id), dimensions, self.polynomial_degree, self.nugget, self.base_range,
                                        self.total_sill)

    def _c(self) -> L.Interpolant:
        return L.Interpolant(int(self.kernel_id), self.polynomial_degree, self.nugget, self.base_range, self.total_sill, 0)


# ------------------------------------------------------------------------------------------------ config
class Solvers(enum.Enum):
    DDM = 0
    FGMRES = 1


class FmmCompressionType(enum.Enum):
    None_ = 0
    SVD = 1
    ACA = 2


class DDMParams:
    """config.rs:42-69; defaults 1024, 0.5, 0.125, 4096"""

    def __init__(self, leaf_threshold: int = 1024, overlap_quota: float = 0.5, coarse_ratio: float = 0.125,
                 coarse_threshold: int = 4096):
        self.leaf_threshold, self.overlap_quota = int(leaf_threshold), float(overlap_quota)
        self.coarse_ratio, self.coarse_threshold = float(coarse_ratio), int(coarse_threshold)

    def to_ddm(self) -> _ddm.DDMParams:
        return _ddm.DDMParams(self.leaf_threshold, self.overlap_quota, self.coarse_ratio, self.coarse_threshold)


class FmmParams:
    """config.rs:209-252"""

    def __init__(self, interpolation_order: int, max_points_per_cell: int = 256,
                 compression_type: FmmCompressionType = FmmCompressionType.ACA, epsilon: Optional[float] = None,
                 eval_chunk_size: int = 1024):
        self.interpolation_order = int(interpolation_order)
        self.max_points_per_cell = int(max_points_per_cell)
        self.compression_type = FmmCompressionType(compression_type)
        self.epsilon = 10.0 ** -self.interpolation_order if epsilon is None else float(epsilon)
        self.eval_chunk_size = int(eval_chunk_size)

    def to_tree(self) -> _TreeFmmParams:
        return _TreeFmmParams(self.max_points_per_cell, M2LCompressionType[self.compression_type.name], self.epsilon,
                              self.eval_chunk_size)


class Params:
    """Params (config.rs:96-190).  Beyond the reference: deterministic (BBFMM_FLAG_DETERMINISTIC on the trees) and
    ddm_params = "reference" (the default: DDMParams' defaults) | "for_points" (ddm.DDMParams.for_points(n), DESIGN.md
    section 9) besides a DDMParams; solver_vectors = "host" (the default) | "device": where the iterative solver keeps its
    vectors (solvers.fgmres / schwarz_ddm_solver, vectors=)."""

    def __init__(self, kernel_type: RBFKernelType, solver_type: Optional[Solvers] = None,
                 ddm_params: Union[None, str, DDMParams] = None, fmm_params: Optional[FmmParams] = None,
                 naive_solve_threshold: Optional[int] = None, test_unique: Optional[bool] = None, deterministic: bool = False,
                 solver_vectors: str = "host"):
        self.kernel_type = RBFKernelType(kernel_type)
        self.solver_type = Solvers.FGMRES if solver_type is None else Solvers(solver_type)
        if isinstance(ddm_params, str) and ddm_params not in ("reference", "for_points"):
            raise ValueError('ddm_params must be a DDMParams, "reference" or "for_points"')
        self.ddm_params = "reference" if ddm_params is None else ddm_params
        self.fmm_params = fmm_params or FmmParams(default_fmm_interpolation_order(self.kernel_type))
        self.naive_solve_threshold = 4096 if naive_solve_threshold is None else int(naive_solve_threshold)
        self.test_unique = True if test_unique is None else bool(test_unique)
        self.deterministic = bool(deterministic)
        if solver_vectors not in ("host", "device"):
            raise ValueError('solver_vectors must be "host" or "device"')
        self.solver_vectors = solver_vectors

    def ddm_for(self, n: int) -> _ddm.DDMParams:
        if self.ddm_params == "reference":
            return _ddm.DDMParams()
        if self.ddm_params == "for_points":
            return _ddm.DDMParams.for_points(n)
        return self.ddm_params.to_ddm() if isinstance(self.ddm_params, DDMParams) else self.ddm_params


# ------------------------------------------------------------------------------------------------ progress
class DuplicatesRemoved:
    def __init__(self, num_duplicates: int):
        self.num_duplicates = int(num_duplicates)


class SolverIteration:
    def __init__(self, iter: int, residual: float, progress: float):  # noqa: A002 -- the reference's field name
        self.iter, self.residual, self.progress = int(iter), float(residual), float(progress)


class SurfacingProgress:
    def __init__(self, isovalue: float, stage: str, progress: float):
        self.isovalue, self.stage, self.progress = float(isovalue), str(stage), float(progress)


class Message:
    def __init__(self, message: str):
        self.message = str(message)


ProgressEvent = Union[SolverIteration, DuplicatesRemoved, SurfacingProgress, Message]


class Progress:
    """progress/__init__.pyi: events go to `callback`"""

    def __init__(self, callback: Optional[Callable[[ProgressEvent], None]] = None):
        self.callback = callback

    def emit(self, event) -> None:
        if self.callback is not None:
            self.callback(event)


# ------------------------------------------------------------------------------------------------ isosurfacing
class BoundaryClosure(enum.Enum):
    None_ = 0
    ClosePositive = 1
    CloseNegative = 2


class ClusterMethod(enum.Enum):
    """ferreus_rmt's ClusterMethod; the string options "none", "average" and "curvature" keep working everywhere"""
    None_ = 0
    Average = 1
    CurvatureWeighted = 2


class Mesh:
    """isosurfacing.Mesh: vertices (n, 3) float64, facets (m, 3) vertex ids"""

    def __init__(self, vertices, facets, stats=None):
        self._vertices = np.ascontiguousarray(vertices, dtype=np.float64)
        self._facets = np.ascontiguousarray(facets, dtype=np.int64)
        self.stats = stats

    @property
    def vertices(self) -> np.ndarray:
        return self._vertices

    @property
    def facets(self) -> np.ndarray:
        return self._facets

    def save_obj(self, path: str, name: str) -> None:
        """Wavefront OBJ: one object `name`, `v x y z` lines, then `f a b c` with 1-based ids"""
        with open(path, "w") as f:
            f.write(f"o {name}\n")
            for v in self._vertices:
                f.write(f"v {float(v[0])!r} {float(v[1])!r} {float(v[2])!r}\n")
            for t in self._facets:
                f.write(f"f {int(t[0]) + 1} {int(t[1]) + 1} {int(t[2]) + 1}\n")


# ------------------------------------------------------------------------------------------------ the device terms
def _cols(a, name, cols=None):
    arr = np.asarray(a, dtype=np.float64)
    if arr.ndim == 1:
        arr = arr[:, None]
    if arr.ndim != 2 or (cols is not None and arr.shape[1] != cols):
        raise ValueError(f"{name}: expected a 2-D array" + (f" with {cols} columns" if cols is not None else "") + f", got {arr.shape}")
    return np.asfortranarray(arr)


def basis_size(d: int, degree: int) -> int:
    k = degree + 1
    return 0 if k <= 0 else {1: k, 2: k * (k + 1) // 2, 3: k * (k + 1) * (k + 2) // 6}[d]


class FieldTerms:
    """What an interpolant adds to its kernel sum (bbfmm_interpolant_terms): the polynomial `coefficients` (basis_size x k,
    monomials 1 | s_a | s_a s_b with a <= b of s = (x - translation) / scale, x the WORLD point) and a global trend's
    affine map x' = x B + b of the points the tree is asked at.  Accepted as `drift=` by FmmTree.build_isosurfaces."""

    def __init__(self, d: int, degree: int = -1, coefficients=None, translation=None, scale=None, B=None, b=None):
        self.d, self.degree = int(d), int(degree)
        if not 1 <= self.d <= 3 or not -1 <= self.degree <= 2:
            raise ValueError("FieldTerms: d = 1..3, degree = -1..2")
        nb = basis_size(self.d, self.degree)
        self.coefficients = None
        self.k = 1
        if nb:
            c = _cols(coefficients, "coefficients")
            if c.shape[0] != nb:
                raise ValueError(f"coefficients must have {nb} rows, got {c.shape[0]}")
            self.coefficients, self.k = c, c.shape[1]
        self.translation = np.zeros(3)
        self.scale = np.ones(3)
        if translation is not None:
            self.translation[:self.d] = np.asarray(translation, dtype=np.float64).reshape(-1)[:self.d]
        if scale is not None:
            self.scale[:self.d] = np.asarray(scale, dtype=np.float64).reshape(-1)[:self.d]
        if (B is None) != (b is None):
            raise ValueError("FieldTerms: B and b come together")
        self.B = None if B is None else np.ascontiguousarray(np.asarray(B, dtype=np.float64).reshape(self.d, self.d))
        self.b = None if b is None else np.ascontiguousarray(np.asarray(b, dtype=np.float64).reshape(self.d))

    def with_columns(self, k: int) -> "FieldTerms":
        """the same terms for k value columns when there is no polynomial"""
        if self.coefficients is None:
            self.k = int(k)
        return self

    def _c(self) -> L.InterpolantTerms:
        t = L.InterpolantTerms()
        t.size = ctypes.sizeof(L.InterpolantTerms)
        t.d, t.polynomial_degree, t.k = self.d, self.degree, self.k
        t.has_affine = 0 if self.B is None else 1
        if self.coefficients is not None:
            t.coefficients = self.coefficients.ctypes.data
            t.ld_coefficients = self.coefficients.shape[0]
        for a in range(3):
            t.translation[a], t.scale[a] = self.translation[a], self.scale[a]
        if self.B is not None:
            for q, v in enumerate(self.B.reshape(-1)):
                t.B[q] = v
            for a in range(self.d):
                t.b[a] = self.b[a]
        return t


def _check(rc, what):
    if rc == L.DEVICE_ERROR:
        raise RuntimeError(f"{what} failed on the device (status {rc})")
    if rc != L.OK:
        raise ValueError(f"{what}: bad argument (status {rc})")


def affine_points(terms: FieldTerms, x, where: int = 1) -> np.ndarray:
    """x B + b (global_trend.rs:266-272) on the host (where = 0) or the device (1)"""
    x = _cols(x, "x", terms.d)
    out = np.zeros_like(x, order="F")
    m = x.shape[0]
    c = terms._c()
    _check(L.load().bbfmm_debug_interpolant_terms(where, 0, ctypes.byref(c), x.ctypes.data, m, max(m, 1), out.ctypes.data, max(m, 1),
                                                  None, 0, None, 0), "affine_points")
    return out


def polynomial_terms(terms: FieldTerms, x, values, grad=None, where: int = 1):
    """values + polynomial at the world points x, and with grad (m x k d) grad + its gradient; returns copies"""
    x = _cols(x, "x", terms.d)
    m = x.shape[0]
    v = np.array(_cols(values, "values", terms.k), order="F")
    g = None if grad is None else np.array(_cols(grad, "grad", terms.k * terms.d), order="F")
    if v.shape[0] != m or (g is not None and g.shape[0] != m):
        raise ValueError("one row per target")
    c = terms._c()
    _check(L.load().bbfmm_debug_interpolant_terms(where, 1, ctypes.byref(c), x.ctypes.data, m, max(m, 1), None, 0, v.ctypes.data,
                                                  max(m, 1), None if g is None else g.ctypes.data, max(m, 1)), "polynomial_terms")
    return v if g is None else (v, g)


def trend_gradients(terms: FieldTerms, grad, where: int = 1) -> np.ndarray:
    """grad B^T per target and column (rbf.rs:1272-1298); returns a copy"""
    g = np.array(_cols(grad, "grad", terms.k * terms.d), order="F")
    m = g.shape[0]
    c = terms._c()
    _check(L.load().bbfmm_debug_interpolant_terms(where, 2, ctypes.byref(c), None, m, max(m, 1), None, 0, None, 0, g.ctypes.data,
                                                  max(m, 1)), "trend_gradients")
    return g


def global_trend_transform(d: int, params, center):
    """(affine, inverse), each (d + 1, d + 1) for row-vector points [x 1] @ affine (bbfmm_global_trend_transform)"""
    p = np.ascontiguousarray(np.asarray(params, dtype=np.float64).reshape(-1))
    c = np.ascontiguousarray(np.asarray(center, dtype=np.float64).reshape(-1))
    if p.size != {1: 1, 2: 3, 3: 6}.get(int(d), -1) or c.size != d:
        raise ValueError("global_trend_transform: d = 1, 2, 3 with 1, 3, 6 parameters and a centre of d coordinates")
    a, inv = np.zeros((d + 1, d + 1)), np.zeros((d + 1, d + 1))
    _check(L.load().bbfmm_global_trend_transform(int(d), p.ctypes.data, c.ctypes.data, a.ctypes.data, inv.ctypes.data),
           "global_trend_transform")
    return a, inv


def duplicate_cutoff_distance(settings: InterpolantSettings, h_ref: float) -> float:
    """duplicate_cutoff_distance (rbf.rs:1391-1415)"""
    out = ctypes.c_double(0.0)
    st = settings._c()
    _check(L.load().bbfmm_duplicate_cutoff_distance(ctypes.byref(st), float(h_ref), ctypes.byref(out)), "duplicate_cutoff_distance")
    return out.value


def remove_duplicates(points, tol: float, where: int = 1, return_rounds: bool = False):
    """The kept indices of remove_duplicates (rbf.rs:1430-1467) at tolerance tol: i is kept iff no kept j < i lies within tol
    in the infinity norm (inclusive).  where = 0: the host, 1: the device."""
    x = _cols(points, "points")
    n, d = x.shape
    keep = np.zeros(max(n, 1), dtype=np.int64)
    nk, rounds = ctypes.c_int64(0), ctypes.c_int64(0)
    _check(L.load().bbfmm_remove_duplicates(x.ctypes.data, n, d, max(n, 1), float(tol), int(where), keep.ctypes.data, ctypes.byref(nk),
                                            ctypes.byref(rounds)), "remove_duplicates")
    out = keep[:nk.value].copy()
    return (out, rounds.value) if return_rounds else out


FULL, LEAVES = 0, 1


def evaluate_interpolant(tree: FmmTree, mode: int, weights, targets, terms: Optional[FieldTerms] = None, with_gradients: bool = False,
                         nugget: float = 0.0):
    """_evaluate (rbf.rs:1180-1270) in one call (bbfmm_evaluate_interpolant): values, or (values, gradients).  weights None
    in Leaves mode uses the weights resident on the device."""
    x = tree._targets(targets)
    m = x.shape[0]
    if weights is None:
        wp, rows, k = None, tree.n_points, tree._nrhs
    else:
        w = _cols(weights, "weights")
        wp, rows, k = w.ctypes.data, w.shape[0], w.shape[1]
    out = np.zeros((m, k), order="F")
    g = np.zeros((m, k * tree.dim), order="F") if with_gradients else None
    bad = ctypes.c_int64(-1)
    c = None if terms is None else terms.with_columns(k)._c()
    rc = tree._lib.bbfmm_evaluate_interpolant(tree._h, int(mode), int(with_gradients), wp, rows, k, rows, x.ctypes.data, m, max(m, 1),
                                              None if c is None else ctypes.byref(c), float(nugget), out.ctypes.data, max(m, 1),
                                              None if g is None else g.ctypes.data, max(m, 1), ctypes.byref(bad))
    tree._raise(rc, bad, mode == LEAVES)
    return (out, g) if with_gradients else out


# ------------------------------------------------------------------------------------------------ the global trend
class GlobalTrend:
    """GlobalTrend (global_trend.rs:35-126): angles in degrees"""

    def __init__(self, dimensions: int, params):
        self.dimensions = int(dimensions)
        self.params = [float(v) for v in params]

    @classmethod
    def one(cls, major_ratio: float) -> "GlobalTrend":
        return cls(1, [major_ratio])

    @classmethod
    def two(cls, rotation_angle: float, major_ratio: float, minor_ratio: float) -> "GlobalTrend":
        return cls(2, [rotation_angle, major_ratio, minor_ratio])

    @classmethod
    def three(cls, dip: float, dip_direction: float, pitch: float, major_ratio: float, semi_major_ratio: float,
              minor_ratio: float) -> "GlobalTrend":
        return cls(3, [dip, dip_direction, pitch, major_ratio, semi_major_ratio, minor_ratio])

    def transform(self, center) -> "GlobalTrendTransform":
        return GlobalTrendTransform(self, center)


class GlobalTrendTransform:
    """GlobalTrendTransform (global_trend.rs:128-287): affine, inverse; B, b with x' = x B + b"""

    def __init__(self, trend: GlobalTrend, center):
        d = trend.dimensions
        self.affine, self.inverse = global_trend_transform(d, trend.params, center)
        self.B, self.b = self.affine[:d, :d].copy(), self.affine[d, :d].copy()
        self._fwd = FieldTerms(d, B=self.B, b=self.b)
        self._inv = FieldTerms(d, B=self.inverse[:d, :d], b=self.inverse[d, :d])

    def transform_points(self, x, where: int = 1) -> np.ndarray:
        return affine_points(self._fwd, x, where)

    def inverse_transform_points(self, x, where: int = 1) -> np.ndarray:
        return affine_points(self._inv, x, where)


# ------------------------------------------------------------------------------------------------ the interpolator
class Coefficients:
    def __init__(self, point_coefficients, poly_coefficients):
        self._point, self._poly = point_coefficients, poly_coefficients

    @property
    def point_coefficients(self) -> np.ndarray:
        return self._point

    @property
    def poly_coefficients(self) -> Optional[np.ndarray]:
        return self._poly


def _extents_of(x) -> np.ndarray:
    return np.concatenate([x.min(axis=0), x.max(axis=0)])


class RBFInterpolator:
    """RBFInterpolator::new / setup_and_solve (rbf.rs:317-582).  After construction: coefficients, source_points (world
    coordinates, after duplicate removal), source_values, residual_histories (one list of (iteration, residual) per value
    column; empty on the naive path), stage_seconds."""

    def __init__(self, points, values, interpolant_settings: InterpolantSettings, params: Optional[Params] = None,
                 global_trend: Optional[GlobalTrend] = None, progress_callback: Optional[Progress] = None):
        t_start = time.perf_counter()
        pts = np.array(_cols(points, "points"), order="F")
        vals = np.array(_cols(values, "values"), order="F")
        n, d = pts.shape
        if not 1 <= d <= 3:
            raise ValueError(f"Unsupported number of dimensions: {d}")
        if vals.shape[0] != n:
            raise ValueError("values must hold one row per point")
        self.settings = interpolant_settings
        self.params = params or Params(interpolant_settings.kernel_type)
        self.progress = progress_callback
        self.stage_seconds = {}
        self._evaluator = None
        st = interpolant_settings
        if self.params.test_unique:                                                        # rbf.rs:341-359
            t0 = time.perf_counter()
            ext = _extents_of(pts)
            tol = duplicate_cutoff_distance(st, float(np.abs(ext[d:] - ext[:d]).max()))
            keep = remove_duplicates(pts, tol, 1)
            if len(keep) != n:
                self._emit(DuplicatesRemoved(n - len(keep)))
                pts, vals = np.asfortranarray(pts[keep]), np.asfortranarray(vals[keep])
                n = len(keep)
            self.duplicate_tolerance = tol
            self.stage_seconds["remove_duplicates"] = time.perf_counter() - t0
        self._points, self._values = pts, vals
        t0 = time.perf_counter()
        self.global_trend = None
        self._tpoints = pts
        if global_trend is not None:                                                       # rbf.rs:361-370
            if global_trend.dimensions != d:
                raise ValueError(f"a {global_trend.dimensions}-D global trend for {d}-D points")
            center = pts.sum(axis=0) / n                                                   # get_center, rbf.rs:1300-1305
            self.global_trend = global_trend.transform(center)
            self._tpoints = self.global_trend.transform_points(pts)
        self.dimensions = d
        self.basis_size = basis_size(d, st.polynomial_degree)
        self.translation_factor, self.scale_factor = np.zeros(d), np.ones(d)
        if self.basis_size:                                                                # get_cheb_cube_scaling_factors of the transformed points
            lo, hi = self._tpoints.min(axis=0), self._tpoints.max(axis=0)
            self.translation_factor, self.scale_factor = (hi + lo) / 2.0, (hi - lo) / 2.0
            self.scale_factor[self.scale_factor == 0.0] = 1.0
        self.stage_seconds["trend_and_setup"] = time.perf_counter() - t0
        self.residual_histories: List[list] = []
        self._solve()
        self.stage_seconds["total"] = time.perf_counter() - t_start
        self._emit(Message(f"Took {self.stage_seconds['total']:.3f} s to solve RBF for {n} points using the following settings:\n"
                           f"Kernel: {st.kernel_type.name}, Polynomial degree: {st.polynomial_degree}\n"
                           f"Fitting accuracy: {st.fitting_accuracy.tolerance}, Tolerance type: {st.fitting_accuracy.tolerance_type.name}"))

    # ---- plumbing
    def _emit(self, event) -> None:
        if self.progress is not None:
            self.progress.emit(event)

    def _monomial_points(self):
        return None if self.global_trend is None else self._points

    def _tree(self, adaptive: bool, sparse: bool, extents) -> FmmTree:
        """_setup_fmmtree (rbf.rs:594-631): the transformed points; given extents go through their 8 transformed corners"""
        d = self.dimensions
        ext = None
        if extents is not None:
            ext = np.asarray(extents, dtype=np.float64).reshape(-1)
            if self.global_trend is not None:
                corners = np.array([[ext[j + d] if (i >> j) & 1 else ext[j] for j in range(d)] for i in range(1 << d)])
                ext = _extents_of(self.global_trend.transform_points(corners, 0))
        return FmmTree(self._tpoints, self.params.fmm_params.interpolation_order, self.settings.kernel_params(), adaptive, sparse,
                       extents=None if ext is None else list(ext), params=self.params.fmm_params.to_tree(), deterministic=self.params.deterministic)

    def terms(self, k: Optional[int] = None) -> FieldTerms:
        """the interpolant's terms besides the kernel sum, for k value columns (all of them by default)"""
        poly = self._coefficients.poly_coefficients
        gt = self.global_trend
        if poly is not None and k is not None and k != poly.shape[1]:
            poly = poly[:, :k]
        t = FieldTerms(self.dimensions, self.settings.polynomial_degree if self.basis_size else -1, poly, self.translation_factor,
                       self.scale_factor, None if gt is None else gt.B, None if gt is None else gt.b)
        return t.with_columns(self._values.shape[1] if k is None else k)

    # ---- the fit
    def _solve(self) -> None:
        t0 = time.perf_counter()
        n, k = self._values.shape
        st, d = self.settings, self.dimensions
        sd = st.to_ddm(d)
        if n < self.params.naive_solve_threshold:                                          # rbf.rs:423-454
            point, poly = self._naive_solve(sd)
        else:
            tree = FmmTree(self._tpoints, self.params.fmm_params.interpolation_order, st.kernel_params(), True, True,
                           params=self.params.fmm_params.to_tree(), deterministic=self.params.deterministic)
            pre = _ddm.SchwarzPreconditioner(tree, self._tpoints, sd, self.params.ddm_for(n), monomial_points=self._monomial_points())
            self.stage_seconds["solver_setup"] = time.perf_counter() - t0
            t0 = time.perf_counter()
            m = self.basis_size
            op = _solvers.RbfSystemOperator(tree, m, pre.monomial_matrix, st.nugget)
            tol = st.fitting_accuracy.to_solver()
            point = np.zeros((n, k), order="F")
            poly = np.zeros((m, k), order="F") if m else None

            def on_iteration(it, res, progress):
                self._emit(SolverIteration(it, res, progress))

            for c in range(k):                                                             # rbf.rs:536-574
                rhs = np.concatenate([self._values[:, c], np.zeros(m)])
                if self.params.solver_type is Solvers.FGMRES:
                    x, hist = _solvers.fgmres(op, rhs, pre, None, 20, 5, tol, on_iteration, vectors=self.params.solver_vectors)
                else:
                    x, hist = _solvers.schwarz_ddm_solver(op, rhs, pre, 100, tol, on_iteration, vectors=self.params.solver_vectors)
                self.residual_histories.append(hist)
                point[:, c] = x[:n]
                if m:
                    poly[:, c] = x[n:]
            pre.close()
        self._coefficients = Coefficients(point, poly)
        self.stage_seconds["solve"] = time.perf_counter() - t0

    def _naive_solve(self, sd):
        """One all-internal domain factorised with solve_for_poly (Domain::factorise / solve, domain.rs:153-470)."""
        from .fmm_tree import debug_kernel_values
        n, k = self._values.shape
        st, m = self.settings, self.basis_size
        level = _ddm.DebugLevel(self._tpoints, [(np.arange(n), np.ones(n, dtype=bool))], sd, solve_for_poly=True,
                                monomial_points=self._monomial_points())
        try:
            point = np.zeros((n, k), order="F")
            for c in range(k):
                point[:, c] = level.solve(self._values[:, c], np.zeros(n), True)
            if not m:
                return point, None
            ks = level.k[0]
            if ks != m:
                raise ValueError(f"the polynomial basis is not unisolvent on these points (rank {ks} of {m}): lower the drift")
            sp = level.indices[0][:ks]                                                     # the special points (domain.rs:214-224)
        finally:
            level.close()
        # the polynomial tail from the special points' rows of the system (domain.rs:352-355, 440-470):
        # P_s lambda = f_s - (A c)_s, P_s the monomials at the special points
        mono = np.zeros((ks, m), order="F")
        world = np.asfortranarray(self._points[sp])
        tr = np.ascontiguousarray(self.translation_factor)
        sc = np.ascontiguousarray(self.scale_factor)
        _check(L.load().bbfmm_debug_evaluate_monomials(world.ctypes.data, ks, self.dimensions, ks, st.polynomial_degree, tr.ctypes.data,
                                                       sc.ctypes.data, mono.ctypes.data), "evaluate_monomials")
        diff = self._tpoints[sp][:, None, :] - self._tpoints[None, :, :]
        a_rows = debug_kernel_values(0, int(st.kernel_id), st.base_range, st.total_sill, (diff * diff).sum(axis=2))[0].reshape(ks, n)
        a_rows[np.arange(ks), sp] += st.nugget
        poly = np.asfortranarray(np.linalg.solve(mono, self._values[sp] - a_rows @ point))
        return point, poly

    # ---- properties
    @property
    def source_points(self) -> np.ndarray:
        return self._points

    @property
    def source_values(self) -> np.ndarray:
        return self._values

    @property
    def coefficients(self) -> Coefficients:
        return self._coefficients

    # ---- evaluation
    def _targets(self, targets) -> np.ndarray:
        return _cols(targets, "targets", self.dimensions)

    def _one_shot(self, targets, with_gradients):
        x = self._targets(targets)                                                         # rbf.rs:633-757
        src, tgt = _extents_of(self._points), _extents_of(x)
        d = self.dimensions
        ext = np.concatenate([np.minimum(src[:d], tgt[:d]), np.maximum(src[d:], tgt[d:])])
        tree = self._tree(True, False, ext)
        w = self._coefficients.point_coefficients
        tree.set_weights(w)
        return evaluate_interpolant(tree, FULL, w, x, self.terms(), with_gradients)

    def evaluate(self, targets) -> np.ndarray:
        return self._one_shot(targets, False)

    def evaluate_with_gradients(self, targets):
        return self._one_shot(targets, True)

    def evaluate_at_source(self, add_nugget: Optional[bool] = False) -> np.ndarray:
        tree = self._tree(True, True, None)                                                # rbf.rs:766-791
        w = self._coefficients.point_coefficients
        tree.set_weights(w)
        return evaluate_interpolant(tree, FULL, w, self._points, self.terms(), False, self.settings.nugget if add_nugget else 0.0)

    def build_evaluator(self, extents=None) -> None:
        tree = self._tree(True, False, extents)                                            # rbf.rs:793-804
        w = self._coefficients.point_coefficients
        tree.set_weights(w)
        tree.set_local_coefficients(w)
        self._evaluator = tree

    def _leaves(self, targets, with_gradients):
        if self._evaluator is None:
            raise ValueError("build_evaluator must be called first")
        return evaluate_interpolant(self._evaluator, LEAVES, self._coefficients.point_coefficients, self._targets(targets), self.terms(),
                                    with_gradients)

    @staticmethod
    def _is_tensor(x) -> bool:
        return type(x).__module__.split(".")[0] == "torch"

    def _leaves_device(self, targets, with_gradients):
        """torch tensors on the evaluator's device: FmmTree.evaluate_device, tensors back (gradients as (m, K d))"""
        if self._evaluator is None:
            raise ValueError("build_evaluator must be called first")
        out = self._evaluator.evaluate_device(targets, gradients=with_gradients, terms=self.terms())
        if not with_gradients:
            return out
        v, g = out
        m, k, d = g.shape
        return v, g.as_strided((m, k * d), (1, max(m, 1)), g.storage_offset())

    def evaluate_targets(self, targets):
        if self._is_tensor(targets):
            return self._leaves_device(targets, False)
        return self._leaves(targets, False)

    def evaluate_targets_with_gradients(self, targets):
        if self._is_tensor(targets):
            return self._leaves_device(targets, True)
        return self._leaves(targets, True)

    def evaluate_grid(self, origin, spacing, shape, *, axes=None, gradients=False, out="numpy", **options):
        """The interpolant on a regular grid (a block model, a section, a volume): node (i0, i1, i2) lies at origin +
        sum_j i_j spacing[j] axes[j]; axes (d, d), row j the direction of index j, defaults to the identity.  Uses the tree
        of build_evaluator.  Values (*shape, K) and with gradients (*shape, K, d); options: those of FmmTree.evaluate_grid
        (batch_bytes, batch_independent, max_job_targets, return_stats)."""
        if self._evaluator is None:
            raise ValueError("build_evaluator must be called first")
        d = self.dimensions
        spacing = np.asarray(spacing, dtype=np.float64).reshape(-1)
        if spacing.size == 1:
            spacing = np.repeat(spacing, d)
        axes = np.eye(d) if axes is None else np.asarray(axes, dtype=np.float64).reshape(d, d)
        if spacing.size != d:
            raise ValueError(f"spacing: one value, or one per axis ({d})")
        return self._evaluator.evaluate_grid(origin, spacing[:, None] * axes, shape, gradients=gradients, terms=self.terms(), out=out,
                                             **options)

    # ---- isosurfaces
    def build_isosurfaces(self, extents, resolution: float, isovalues, boundary_closure: Optional[BoundaryClosure] = None, *,
                          cluster="curvature", follow="surface", seeds=None, finish="clipped", self_intersections="rollback",
                          return_stats=False, return_field=False, batch_bytes: int = 0):
        """build_isosurfaces (rbf.rs:980-1069) on the device extractor; the keywords override its options
        (FmmTree.build_isosurfaces); finish="close_positive" / "close_negative" close the mesh on the faces of the extents.
        The first value column is meshed."""
        closure = BoundaryClosure.None_ if boundary_closure is None else BoundaryClosure(boundary_closure)
        if closure is not BoundaryClosure.None_:
            raise NotImplementedError(f"boundary_closure=BoundaryClosure.{closure.name} is not mapped onto the closure yet: pass "
                                      f"finish={'close_positive' if closure is BoundaryClosure.ClosePositive else 'close_negative'!r} instead")
        if self.dimensions != 3:
            raise ValueError("Only supported for 3D isosurfacing")
        ext = np.asarray(extents, dtype=np.float64).reshape(-1)
        src = _extents_of(self._points)
        ev = np.concatenate([np.minimum(src[:3], ext[:3]) - 10.0 * resolution, np.maximum(src[3:], ext[3:]) + 10.0 * resolution])
        tree = self._tree(True, False, ev)
        w = np.asfortranarray(self._coefficients.point_coefficients[:, :1])
        tree.set_weights(w)
        tree.set_local_coefficients(w)
        isovalues = [float(v) for v in np.atleast_1d(isovalues)]
        for v in isovalues:
            self._emit(SurfacingProgress(v, "started", 0.0))
        terms = self.terms(1)
        drift = terms if (terms.coefficients is not None or terms.B is not None) else None
        out = tree.build_isosurfaces(ext, float(resolution), isovalues, drift=drift, return_field=return_field, batch_bytes=batch_bytes,
                                     cluster=cluster, return_stats=return_stats, finish=finish, self_intersections=self_intersections,
                                     follow=follow, seeds=(self._points if seeds is None else seeds) if follow == "surface" else None)
        meshes, field = out if return_field else (out, None)
        result = [Mesh(m[0], m[1], m[2] if return_stats else None) for m in meshes]
        for v in isovalues:
            self._emit(SurfacingProgress(v, "finished", 1.0))
        return (result, field) if return_field else result

    def build_isosurface(self, extents, resolution: float, isovalue: float, boundary_closure: Optional[BoundaryClosure] = None,
                         **options):
        out = self.build_isosurfaces(extents, resolution, [isovalue], boundary_closure, **options)
        if options.get("return_field"):
            return out[0][0], out[1]
        return out[0]

    # ---- persistence: the reference's serde layout cannot be checked here
    def save_model(self, path: str) -> None:
        raise NotImplementedError("save_model is not implemented: the reference's model file layout is not reproduced here")

    @staticmethod
    def load_model(path: str, progress_callback: Optional[Progress] = None) -> "RBFInterpolator":
        raise NotImplementedError("load_model is not implemented: the reference's model file layout is not reproduced here")
