"""Python host-side mirror of the reference's evaluator API over the C ABI.

Mirrors the only existing foreign-language binding of the seam, `py_ferreus_bbfmm`
(py_ferreus_bbfmm/src/python_bindings.rs:66-390): same class names, constructor
arguments, method names, array conventions and error behaviour, so the parity
tests read like the reference's examples.  All compute goes through
libferreus_bbfmm_hip.so (HIP kernels); nothing here computes potentials.
"""
from __future__ import annotations

import ctypes
import enum
from typing import Optional

import numpy as np

from . import _lib as L


class KernelType(enum.IntEnum):
    """ferreus_rbf_utils::KernelType (ferreus_rbf_utils/src/utils.rs:558-571)."""
    LinearRbf = 0
    ThinPlateSplineRbf = 1
    CubicRbf = 2
    Spheroidal3Rbf = 3
    Spheroidal5Rbf = 4
    Spheroidal7Rbf = 5
    Spheroidal9Rbf = 6
    Laplacian = 7
    OneOverR2 = 8
    OneOverR4 = 9
    # extension kernels of this repository (not in the reference)
    GaussianExt = 100
    MultiquadricExt = 101


class FmmKernelType(enum.Enum):
    """py_ferreus_bbfmm FmmKernelType (python_bindings.rs:66-76) + the two extensions."""
    LinearRbf = "LinearRbf"
    ThinPlateSplineRbf = "ThinPlateSplineRbf"
    CubicRbf = "CubicRbf"
    SpheroidalRbf = "SpheroidalRbf"
    Laplacian = "Laplacian"
    OneOverR2 = "OneOverR2"
    OneOverR4 = "OneOverR4"
    GaussianExt = "GaussianExt"
    MultiquadricExt = "MultiquadricExt"


class SpheroidalOrder(enum.Enum):
    """python_bindings.rs:78-85"""
    Three = 3
    Five = 5
    Seven = 7
    Nine = 9


class M2LCompressionType(enum.IntEnum):
    """ferreus_bbfmm::M2LCompressionType (bbfmm.rs:62-73; python name None_)."""
    None_ = 0
    SVD = 1
    ACA = 2


class FmmParams:
    """FmmParams (bbfmm.rs:77-104; python_bindings.rs:106-131)."""

    def __init__(self, max_points_per_cell: int, compression_type: M2LCompressionType,
                 epsilon: float, eval_chunk_size: int):
        self.max_points_per_cell = int(max_points_per_cell)
        self.compression_type = M2LCompressionType(compression_type)
        self.epsilon = float(epsilon)
        self.eval_chunk_size = int(eval_chunk_size)

    @staticmethod
    def new_defaults(interpolation_order: int) -> "FmmParams":
        p = L.Params()
        L.load().bbfmm_params_defaults(interpolation_order, ctypes.byref(p))
        return FmmParams(p.max_points_per_cell, M2LCompressionType(p.compression_type), p.epsilon,
                         p.eval_chunk_size)

    def _c(self) -> L.Params:
        return L.Params(self.max_points_per_cell, int(self.compression_type), self.epsilon,
                        self.eval_chunk_size)


class KernelParams:
    """KernelParams (kernel_helpers.rs:17-79; python_bindings.rs:133-188)."""

    def __init__(self, kernel_type, *, spheroidal_order: Optional[SpheroidalOrder] = None,
                 base_range: Optional[float] = None, total_sill: Optional[float] = None, validate: bool = True):
        """validate=False: skip the reference builder's assertion total_sill <= base_range.  The library itself takes any
        sill (it only scales the kernel); the calibration inputs of the local-solver tests have sill 1 and range 0.3."""
        if isinstance(kernel_type, KernelType):
            kt = kernel_type
        else:
            kernel_type = FmmKernelType(kernel_type)
            if kernel_type is FmmKernelType.SpheroidalRbf:
                order = spheroidal_order if spheroidal_order is not None else SpheroidalOrder.Three
                kt = {3: KernelType.Spheroidal3Rbf, 5: KernelType.Spheroidal5Rbf,
                      7: KernelType.Spheroidal7Rbf, 9: KernelType.Spheroidal9Rbf}[
                    SpheroidalOrder(order).value]
            else:
                kt = KernelType[kernel_type.name]
        self.kernel_type = kt
        self.base_range = 1.0 if base_range is None else float(base_range)     # builder defaults,
        self.total_sill = 1.0 if total_sill is None else float(total_sill)     # kernel_helpers.rs:25-31
        # KernelParamsBuilder::build asserts (kernel_helpers.rs:69-70)
        assert self.base_range > 0.0
        assert self.total_sill <= self.base_range or not validate


class FmmError(ValueError):
    """FmmError (bbfmm.rs:20-45); the PyO3 binding raises ValueError with these messages."""


class CallbackFailed(FmmError):
    """BBFMM_CALLBACK_FAILED: a caller's field callback returned nonzero (bbfmm_isosurfaces_from_function_opts)"""


class PointOutsideTree(FmmError):
    def __init__(self, point_index: int, leaf: bool = False):
        what = "FMM leaf evaluation failed" if leaf else "FMM evaluation failed"
        super().__init__(f"{what}: target point at row {point_index} lies outside the tree extents")
        self.point_index = point_index


class KernelDoesNotSupportGradients(FmmError):
    def __init__(self):
        super().__init__("FMM evaluation failed: gradient evaluation requested but kernel does "
                         "not support gradients")


def _as_f64_2d(a, name):
    """numpy_to_matref (python_bindings.rs:20-36): 1-D or 2-D float64."""
    arr = np.asarray(a)
    if arr.dtype != np.float64 or arr.ndim not in (1, 2):
        raise TypeError(f"Expected a 1D/2D float64 array for {name}")
    if arr.ndim == 1:
        arr = arr[:, None]
    return np.asfortranarray(arr)


class FmmTree:
    """ferreus_rbf_utils::FmmTree (utils.rs:383-494) / py FmmTree (python_bindings.rs:191-390)."""

    def __init__(self, source_points, interpolation_order: int, kernel_params: KernelParams,
                 adaptive_tree: bool, sparse: bool, *, extents=None,
                 params: Optional[FmmParams] = None, host_only: bool = False,
                 m2l_shared_basis: bool = False, direct_small_w_leaves: bool = False, deterministic: bool = False,
                 devices=None):
        """m2l_shared_basis: BBFMM_FLAG_M2L_SHARED_BASIS, an extension beyond the reference (off by default):
        the M2L stages run in one orthonormal basis per level, cut at params.epsilon.
        direct_small_w_leaves: BBFMM_FLAG_DIRECT_SMALL_W_LEAVES, likewise an extension: W-list leaves with no
        more points than nodes are summed directly instead of through M2P / P2L.
        deterministic: BBFMM_FLAG_DETERMINISTIC -- fixed summation order everywhere (no f64 atomics), bitwise
        reproducible results from run to run like the reference's.
        devices: HIP device ids of a handle that spans several devices of this process (bbfmm_create_on_devices): the
        matvec entry points run partitioned over them, nothing else changes for the caller.  An id may repeat (logical
        parts on one device).  None: the current device -- or the list in FERREUS_BBFMM_DEVICES, which is how the
        unchanged Rust caller is switched."""
        lib = L.load()
        pts = _as_f64_2d(source_points, "source_points")
        n, d = pts.shape
        ext = None
        if extents is not None:
            ext = np.ascontiguousarray(np.asarray(extents, dtype=np.float64).reshape(-1))
            d = len(ext) // 2                       # bbfmm.rs:291
        cpar = params._c() if params is not None else None
        h = ctypes.c_void_p()
        flags = ((L.FLAG_HOST_ONLY if host_only else 0) |
                 (L.FLAG_M2L_SHARED_BASIS if m2l_shared_basis else 0) |
                 (L.FLAG_DIRECT_SMALL_W_LEAVES if direct_small_w_leaves else 0) |
                 (L.FLAG_DETERMINISTIC if deterministic else 0))
        args = (pts.ctypes.data, n, d, n, int(interpolation_order),
                int(kernel_params.kernel_type), kernel_params.base_range,
                kernel_params.total_sill, int(bool(adaptive_tree)), int(bool(sparse)),
                ext.ctypes.data if ext is not None else None,
                ctypes.byref(cpar) if cpar is not None else None, flags)
        if devices is None:
            rc = lib.bbfmm_create(*args, ctypes.byref(h))
        else:
            dev = np.ascontiguousarray(np.asarray(devices, dtype=np.int32).reshape(-1))
            rc = lib.bbfmm_create_on_devices(*args, dev.ctypes.data, len(dev), ctypes.byref(h))
        self._h = h
        self._lib = lib
        if rc != L.OK:
            msg = lib.bbfmm_last_error(h).decode() if h else "bbfmm_create failed"
            if h:
                lib.bbfmm_destroy(h)
                self._h = None
            if rc == L.DEVICE_ERROR:
                raise RuntimeError(msg)
            raise ValueError(msg)              # the reference panics
        self.interpolation_order = int(interpolation_order)
        self.kernel_params = kernel_params
        self.adaptive_tree = bool(adaptive_tree)
        self.sparse = bool(sparse)
        self.n_points = n
        self.dim = d
        self.deterministic = bool(deterministic)
        self._nrhs = 0
        self._compressed = params is None or params.compression_type != M2LCompressionType.None_

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            self._lib.bbfmm_destroy(h)
            self._h = None

    # -- errors
    def _raise(self, rc, bad=None, leaf=False):
        if rc == L.OK:
            return
        msg = self._lib.bbfmm_last_error(self._h).decode()
        if rc == L.POINT_OUTSIDE_TREE:
            raise PointOutsideTree(int(bad.value), leaf)
        if rc == L.KERNEL_NO_GRADIENTS:
            raise KernelDoesNotSupportGradients()
        if rc == L.DEVICE_ERROR:
            raise RuntimeError(msg)
        raise ValueError(msg)

    # -- API
    def set_weights(self, weights) -> None:
        w = _as_f64_2d(weights, "weights")
        self._raise(self._lib.bbfmm_set_weights(self._h, w.ctypes.data, w.shape[0], w.shape[1],
                                                w.shape[0]))
        self._nrhs = w.shape[1]

    def set_local_coefficients(self, weights) -> None:
        w = _as_f64_2d(weights, "weights")
        self._raise(self._lib.bbfmm_set_local_coefficients(self._h, w.ctypes.data, w.shape[0],
                                                           w.shape[1], w.shape[0]))
        self._nrhs = w.shape[1]           # (the column count may also have been fixed by a matvec on the C side)

    def _targets(self, target_points):
        """m x d column-major targets; the C ABI takes a pointer and reads d columns, so the column count is checked here
        (the reference's faer views panic on a missing column; found by the ASan run of scripts/sanitize_host.sh)."""
        x = _as_f64_2d(target_points, "target_points")
        if x.shape[1] != self.dim:
            raise ValueError(f"target_points must have {self.dim} columns, got {x.shape[1]}")
        return x

    def _eval(self, fn, weights, target_points, grads, leaf):
        x = self._targets(target_points)
        if weights is None and leaf:
            # leaves-only calls may reuse the weights resident on the device (header: bbfmm_evaluate_leaves)
            wp, rows, k = None, self.n_points, self._nrhs
        else:
            w = _as_f64_2d(weights, "weights")
            wp, rows, k = w.ctypes.data, w.shape[0], w.shape[1]
        m = x.shape[0]
        out = np.zeros((m, k), order="F")
        bad = ctypes.c_int64(-1)
        if grads:
            g = np.zeros((m, k * self.dim), order="F")
            rc = fn(self._h, wp, rows, k, rows, x.ctypes.data, m, max(m, 1),
                    out.ctypes.data, max(m, 1), g.ctypes.data, max(m, 1), ctypes.byref(bad))
            self._raise(rc, bad, leaf)
            return out, g
        rc = fn(self._h, wp, rows, k, rows, x.ctypes.data, m, max(m, 1),
                out.ctypes.data, max(m, 1), ctypes.byref(bad))
        self._raise(rc, bad, leaf)
        return out

    def evaluate(self, weights, target_points):
        return self._eval(self._lib.bbfmm_evaluate, weights, target_points, False, False)

    def evaluate_with_gradients(self, weights, target_points):
        return self._eval(self._lib.bbfmm_evaluate_with_gradients, weights, target_points, True, False)

    def evaluate_leaves(self, weights, target_points):
        return self._eval(self._lib.bbfmm_evaluate_leaves, weights, target_points, False, True)

    def evaluate_leaves_with_gradients(self, weights, target_points):
        return self._eval(self._lib.bbfmm_evaluate_leaves_with_gradients, weights, target_points,
                          True, True)

    # -- device-resident targets and regular grids (bbfmm_evaluate_device, bbfmm_evaluate_grid)
    def _evaluate_options(self, batch_independent, max_job_targets, batch_bytes=0, outputs_on_device=False):
        return L.EvaluateOptions(ctypes.sizeof(L.EvaluateOptions), -1 if batch_independent is None else int(bool(batch_independent)),
                                 -1 if max_job_targets is None else int(max_job_targets), int(batch_bytes), int(bool(outputs_on_device)))

    def _terms_c(self, terms):
        return None if terms is None else terms.with_columns(self._nrhs)._c()

    def _torch_device(self):
        import torch
        return torch.device("cuda", self.device())

    @staticmethod
    def _torch_columns(m, cols, device):
        """(m, cols) float64 with column-major storage, the layout of the C ABI"""
        import torch
        return torch.empty((cols, max(m, 1)), dtype=torch.float64, device=device)[:, :m].t()

    def evaluate_device(self, x, *, gradients=False, terms=None, batch_independent=None, max_job_targets=None):
        """Leaves mode (set_local_coefficients first) at targets that live on the tree's device: x a float64 torch tensor
        (m, d), or a tuple of d contiguous columns of m.  The SoA copy is made by torch, nothing touches the host.  Returns
        a tensor (m, K) for the K weight columns and, with gradients, also (m, K, d); both are views of the column-major
        result.  terms: rbf.FieldTerms of an interpolant (global trend before the pass, polynomial and trend gradients
        behind it).  batch_independent: None is the tree's deterministic flag.  max_job_targets: jobs of the leaf pass
        hold at most this many targets (0: one job per leaf, None: the library's default)."""
        import torch
        dev, d, k = self._torch_device(), self.dim, self._nrhs
        if k < 1:
            raise ValueError("set_local_coefficients must be called first")
        if isinstance(x, (tuple, list)):
            if len(x) != d:
                raise ValueError(f"expected {d} coordinate columns, got {len(x)}")
            soa = torch.stack([torch.as_tensor(c).reshape(-1) for c in x])
        else:
            if x.ndim != 2 or x.shape[1] != d:
                raise ValueError(f"target_points must be (m, {d}), got {tuple(x.shape)}")
            soa = x.t()
        if soa.dtype != torch.float64 or soa.device != dev:
            raise TypeError(f"device targets must be float64 tensors on {dev}")
        soa = soa.contiguous()
        m = soa.shape[1]
        vals = self._torch_columns(m, k, dev)
        grad = self._torch_columns(m, k * d, dev) if gradients else None
        torch.cuda.synchronize(dev)                  # the tree's passes run on its own stream
        bad = ctypes.c_int64(-1)
        opts = self._evaluate_options(batch_independent, max_job_targets)
        c = self._terms_c(terms)
        rc = self._lib.bbfmm_evaluate_device(self._h, int(bool(gradients)), soa.data_ptr() if m else None, m, max(m, 1),
                                             None if c is None else ctypes.byref(c), vals.data_ptr(), max(m, 1),
                                             grad.data_ptr() if grad is not None else None, max(m, 1), ctypes.byref(opts),
                                             ctypes.byref(bad))
        self._raise(rc, bad, True)
        if not gradients:
            return vals
        return vals, torch.as_strided(grad, (m, k, d), (1, d * max(m, 1), max(m, 1)), grad.storage_offset())

    def last_grid_stats(self) -> dict:
        """nodes, slabs, leaf_runs, jobs, largest_job, w_jobs of the last evaluate_grid"""
        s = np.zeros(8, dtype=np.int64)
        self._raise(self._lib.bbfmm_evaluate_grid_stats(self._h, s.ctypes.data))
        return dict(zip(L.GRID_STATS, (int(v) for v in s)))

    def _grid(self, origin, steps, shape):
        d = self.dim
        origin = np.asarray(origin, dtype=np.float64).reshape(-1)
        steps = np.asarray(steps, dtype=np.float64)
        shape = [int(n) for n in np.asarray(shape).reshape(-1)]
        if origin.size != d or steps.shape != (d, d) or len(shape) != d or min(shape) < 0:
            raise ValueError(f"a grid of a {d}-D tree needs an origin of {d} coordinates, ({d}, {d}) steps and {d} counts >= 0")
        return make_grid(origin, steps, shape), shape

    def evaluate_grid(self, origin, steps, shape, *, gradients=False, terms=None, out="numpy", batch_bytes=0,
                      batch_independent=None, max_job_targets=None, return_stats=False):
        """Leaves mode at the nodes of a regular grid: node (i0, i1, i2) lies at origin + i0 steps[0] + i1 steps[1] +
        i2 steps[2] (row j of `steps` is the world step of index j; a rotated block model is a non-diagonal `steps`).  The
        coordinates are made on the device slab by slab (batch_bytes of device memory each, 0: the default) and never
        exist on the host.  Returns values of shape (*shape, K) and, with gradients, (*shape, K, d): views of the
        column-major result, numpy arrays or (out="torch") tensors on the tree's device.  return_stats: also
        last_grid_stats().  The other options are those of evaluate_device."""
        if out not in ("numpy", "torch"):
            raise ValueError('out is "numpy" or "torch"')
        d, k = self.dim, self._nrhs
        if k < 1:
            raise ValueError("set_local_coefficients must be called first")
        g, shape = self._grid(origin, steps, shape)
        m = int(np.prod(shape))
        ld = max(m, 1)
        if out == "torch":
            import torch
            dev = self._torch_device()
            vals = self._torch_columns(m, k, dev)
            grad = self._torch_columns(m, k * d, dev) if gradients else None
            torch.cuda.synchronize(dev)
            vp, gp = vals.data_ptr(), (grad.data_ptr() if gradients else None)
        else:
            vals = np.zeros((m, k), order="F")
            grad = np.zeros((m, k * d), order="F") if gradients else None
            vp, gp = vals.ctypes.data, (grad.ctypes.data if gradients else None)
        bad = ctypes.c_int64(-1)
        opts = self._evaluate_options(batch_independent, max_job_targets, batch_bytes, out == "torch")
        c = self._terms_c(terms)
        rc = self._lib.bbfmm_evaluate_grid(self._h, int(bool(gradients)), ctypes.byref(g), None if c is None else ctypes.byref(c),
                                           vp, ld, gp, ld, ctypes.byref(opts), ctypes.byref(bad))
        self._raise(rc, bad, True)
        # row r = C order of the indices, column-major columns: (*shape, K) and (*shape, K, d) without a copy
        row = [int(np.prod(shape[j + 1:])) for j in range(d)]
        if out == "torch":
            import torch
            res = [torch.as_strided(vals, (*shape, k), (*row, ld), vals.storage_offset())]
            if gradients:
                res.append(torch.as_strided(grad, (*shape, k, d), (*row, d * ld, ld), grad.storage_offset()))
        else:
            as_strided = np.lib.stride_tricks.as_strided
            res = [as_strided(vals, (*shape, k), tuple(8 * s for s in (*row, ld)))]
            if gradients:
                res.append(as_strided(grad, (*shape, k, d), tuple(8 * s for s in (*row, d * ld, ld))))
        if return_stats:
            res.append(self.last_grid_stats())
        return res[0] if len(res) == 1 else tuple(res)

    # -- isosurfaces (isosurface.py)
    def build_isosurfaces(self, extents, resolution, isovalues, *, drift=None, return_field=False, batch_bytes=0,
                          cluster="none", return_stats=False, finish="raw", self_intersections="ignore", follow="dense",
                          seeds=None):
        """RBFInterpolator::build_isosurfaces (ferreus_rbf/src/rbf.rs:980-) on the device, one field evaluation for all
        isovalues: a list of (vertices (n, 3) f64, facets (m, 3) int64), the marching-tetrahedra mesh of ferreus_rmt
        (isosurface.rs:489-) over every sample point of the extraction domain.  finish: "raw" (the default) is that mesh
        before clipping and cleaning, two lattice cells past the extents on every side; "clipped" runs the reference's
        clip_mesh_to_aabb and clean_mesh on the device before the download (isosurface.rs:1009-1021), its finished mesh
        for BoundaryClosure::None; "close_positive" / "close_negative" then close that mesh on the six faces of the
        extents (BoundaryClosure::ClosePositive / CloseNegative; see isosurface.py; stats under "closure").  cluster: "none" (the default) is ClusterMethod::None, one vertex per crossed lattice edge; "average"
        is ClusterMethod::Average, the intersections near a sample point merged into their mean where the topology
        tests allow it, with the predicted-edge and non-manifold rollbacks (isosurface.rs:715-930); its
        self-intersection rollback (isosurface.rs:932-1007) runs with self_intersections="rollback" ("ignore", the
        default, leaves it out; see isosurface.py); the lattice field then stays on the device (40 bytes per node of the lattice
        box), and a lattice that does not fit is refused before any work; "curvature" is ClusterMethod::CurvatureWeighted,
        the same clusters placed at the mean weighted by the curvature estimate of every crossed edge
        (curvature_weighting.rs; 48 bytes per node; vertices agree with a host computation to rounding, not bit for bit).
        return_stats: (vertices, facets, stats) per
        isovalue, stats the clustering counts of isosurface.STATS and of the rollback passes, with cluster="curvature"
        under "curvature" the counts of isosurface.CURVATURE_STATS, and with finish="clipped"
        under "finish" the counts of isosurface.FINISH_STATS, with self_intersections="rollback" under
        "self_intersections" those of isosurface.INTERSECTION_STATS.  Needs set_local_coefficients (one column) first, like
        evaluate_leaves, and a tree whose extents hold the lattice (the reference pads its evaluator by 10 resolutions,
        rbf.rs:992-998; a node outside raises PointOutsideTree before any work).  drift: None, [a, b0, b1, b2] or
        (a, [b0, b1, b2]) added to the field as a + b . x (isosurface.affine_drift folds the reference's Constant /
        Linear drift with its translation and scale).  return_field: also the lattice field, shape
        isosurface.lattice_info(extents, resolution)["shape"], NaN off the evaluated nodes.  batch_bytes: device memory
        for one batch of k-planes (0: the default); the meshes do not depend on it.  follow: "dense" (the default)
        evaluates every node of the extraction domain; "surface" only the bricks of lattice nodes a wavefront reaches
        from `seeds` ((n, 3) points, None: the source points, rbf.rs:1049) after they were projected onto the level set,
        as the reference follows the surface (see isosurface.py); a component no seed reaches is then absent, the
        returned field NaN where it was not evaluated, and the stats hold isosurface.FOLLOW_STATS under "follow"."""
        from . import isosurface as I
        return I.build_isosurfaces(self, extents, resolution, isovalues, drift=drift, return_field=return_field,
                                   batch_bytes=batch_bytes, cluster=cluster, return_stats=return_stats, finish=finish,
                                   self_intersections=self_intersections, follow=follow, seeds=seeds)

    def build_isosurface(self, extents, resolution, isovalue, *, drift=None, return_field=False, batch_bytes=0,
                         cluster="none", return_stats=False, finish="raw", self_intersections="ignore", follow="dense",
                         seeds=None):
        """RBFInterpolator::build_isosurface (rbf.rs:954-) at one isovalue: (vertices, facets), then the stats when
        return_stats, then the lattice field when return_field; see build_isosurfaces."""
        out = self.build_isosurfaces(extents, resolution, [isovalue], drift=drift, return_field=return_field,
                                     batch_bytes=batch_bytes, cluster=cluster, return_stats=return_stats, finish=finish,
                                     self_intersections=self_intersections, follow=follow, seeds=seeds)
        if return_field:
            meshes, field = out
            return (*meshes[0], field)
        return out[0]

    def source_points(self):
        out = np.zeros((self.n_points, self.dim), order="F")
        self._raise(self._lib.bbfmm_source_points(self._h, out.ctypes.data, self.n_points))
        return out

    # -- the FGMRES matvec (ferreus_rbf/src/rbf.rs:1338-1379)
    def fast_matrix_vector_product(self, weights, basis_size=0, target_indices=None,
                                   polynomial_matrix=None, nugget=0.0):
        w = np.ascontiguousarray(np.asarray(weights, dtype=np.float64).reshape(-1))
        res = np.zeros_like(w)
        idx = None
        if target_indices is not None:
            idx = np.ascontiguousarray(np.asarray(target_indices, dtype=np.int64))
        poly = None
        if polynomial_matrix is not None:
            poly = np.asfortranarray(np.asarray(polynomial_matrix, dtype=np.float64))
        rc = self._lib.bbfmm_fast_matrix_vector_product(
            self._h, w.ctypes.data, len(w), int(basis_size),
            idx.ctypes.data if idx is not None else None, len(idx) if idx is not None else 0,
            poly.ctypes.data if poly is not None else None,
            poly.shape[0] if poly is not None else 0, float(nugget), res.ctypes.data)
        self._raise(rc)
        self._nrhs = 1
        return res

    def prepare_target_subset(self, target_indices) -> None:
        """bbfmm_prepare_target_subset: build and cache the plan of a later partial product ahead of time."""
        idx = np.ascontiguousarray(np.asarray(target_indices, dtype=np.int64))
        self._raise(self._lib.bbfmm_prepare_target_subset(self._h, idx.ctypes.data, len(idx)))

    # -- device-resident matvec (what bench.py times); d_w / d_out are device pointers
    def matvec_device(self, d_w_ptr: int, ldw: int, k: int, d_out_ptr: int, ldo: int, sync=True):
        self._raise(self._lib.bbfmm_matvec_device(self._h, d_w_ptr, ldw, k, d_out_ptr, ldo,
                                                  int(sync)))
        self._nrhs = int(k)

    def stream(self) -> int:
        return int(self._lib.bbfmm_stream(self._h) or 0)

    # -- one handle over several devices (bbfmm_create_on_devices / FERREUS_BBFMM_DEVICES)
    def device_count(self) -> int:
        """Parts of the handle (1: an ordinary handle on one device)."""
        return int(self._lib.bbfmm_device_count(self._h))

    def part_device(self, part: int = 0) -> int:
        """HIP device of a part (part 0: the handle's own device, where device-resident vectors live)."""
        return int(self._lib.bbfmm_part_device(self._h, int(part)))

    def device(self) -> int:
        return self.part_device(0)

    def group_bounds(self) -> np.ndarray:
        """parts + 1 offsets into the tree's sorted points: part g owns [bounds[g], bounds[g + 1])."""
        b = np.zeros(self.device_count() + 1, dtype=np.int64)
        self._raise(self._lib.bbfmm_group_bounds(self._h, b.ctypes.data))
        return b

    def part_phase_ms(self, part: int):
        ms = np.zeros(L.N_PHASES)
        cnt = np.zeros(L.N_PHASES, dtype=np.int64)
        self._raise(self._lib.bbfmm_get_part_phase_ms(self._h, int(part), ms.ctypes.data, cnt.ctypes.data))
        return dict(zip(L.PHASE_NAMES, ms.tolist())), dict(zip(L.PHASE_NAMES, cnt.tolist()))

    def set_partition(self, rank: int, world: int):
        self._raise(self._lib.bbfmm_set_partition(self._h, rank, world))

    def partition_rows(self) -> np.ndarray:
        n = self._lib.bbfmm_partition_row_count(self._h)
        rows = np.zeros(n, dtype=np.int64)
        self._raise(self._lib.bbfmm_partition_rows(self._h, rows.ctypes.data))
        return rows

    def partition_coarse_count(self) -> int:
        """Doubles per right-hand side of the coarse multipoles a partition exchanges (0: none)."""
        return int(self._lib.bbfmm_partition_coarse_count(self._h))

    def matvec_partition_upward(self, d_w: int, ldw: int, k: int, d_coarse: int, comm_stream: int = 0):
        """First half of the partitioned matvec (device pointers): this rank's share of the upward pass; packs
        k x partition_coarse_count() partial coarse multipoles into d_coarse for the all-reduce, then queues the near
        field.  comm_stream: the HIP stream (pointer) the all-reduce will be issued on (0: ordered by the caller)."""
        self._raise(self._lib.bbfmm_matvec_partition_upward(self._h, d_w, ldw, k, d_coarse or None, comm_stream or None))

    def matvec_partition_finish(self, d_coarse: int, d_out: int, ldo: int, sync: bool = True, comm_stream: int = 0):
        """Second half: d_coarse summed over the ranks; downward + leaf pass of the owned targets."""
        self._raise(self._lib.bbfmm_matvec_partition_finish(self._h, d_coarse or None, d_out, ldo, int(sync), comm_stream or None))

    def partition_world(self) -> int:
        """Parts of the handle's partition (1: none set)."""
        return int(self._lib.bbfmm_partition_world(self._h))

    def partition_rank(self) -> int:
        """The part of its partition this handle owns."""
        return int(self._lib.bbfmm_partition_rank(self._h))

    def partition_bounds(self) -> np.ndarray:
        """world + 1 offsets into the tree's sorted points: part r owns bounds[r] .. bounds[r + 1) (the same on every
        rank of a `set_partition(rank, world)`)."""
        world = self.partition_world()
        b = np.zeros(world + 1, dtype=np.int64)
        self._raise(self._lib.bbfmm_partition_bounds(self._h, world, b.ctypes.data))
        return b

    def matvec_partition_finish_sorted(self, d_coarse: int, d_seg: int, ld: int, comm_stream: int = 0):
        """Second half with the owned potentials left in sorted order: k rows of d_seg (stride ld), the block a rank
        sends to the all-gather (asynchronous on the handle's stream)."""
        self._raise(self._lib.bbfmm_matvec_partition_finish_sorted(self._h, d_coarse or None, d_seg, ld, comm_stream or None))

    def partition_scatter(self, d_all: int, first_part: int, n_parts: int, m_max: int, k: int, d_out: int, ldo: int):
        """Gathered blocks d_all[n_parts][k][m_max] of parts first_part .. first_part + n_parts -> their rows of d_out."""
        self._raise(self._lib.bbfmm_partition_scatter(self._h, d_all, first_part, n_parts, m_max, k, d_out, ldo))

    def debug_partition_upward_counts(self):
        """(counts, reads, info): the rank's upward plan walked with point counts (see the header)."""
        c = self.stats().n_cells
        counts = np.zeros(c, dtype=np.int64)
        reads = np.zeros(c, dtype=np.uint8)
        info = np.zeros(4, dtype=np.int64)
        self._raise(self._lib.bbfmm_debug_partition_upward_counts(self._h, counts.ctypes.data, reads.ctypes.data,
                                                                 info.ctypes.data))
        return counts, reads, info

    def set_profiling(self, on: bool):
        self._lib.bbfmm_set_profiling(self._h, int(on))

    def phase_ms(self, reset=False, counts=False):
        """Accumulated per-phase device milliseconds (and interval counts) since the last reset."""
        ms = (ctypes.c_double * L.N_PHASES)()
        cnt = (ctypes.c_int64 * L.N_PHASES)()
        self._lib.bbfmm_get_phase_ms(self._h, ms, cnt)
        if reset:
            self._lib.bbfmm_reset_phase_ms(self._h)
        d = dict(zip(L.PHASE_NAMES, list(ms)))
        if counts:
            return d, dict(zip(L.PHASE_NAMES, list(cnt)))
        return d

    # -- introspection
    def stats(self) -> L.TreeStats:
        s = L.TreeStats()
        self._raise(self._lib.bbfmm_get_tree_stats(self._h, ctypes.byref(s)))
        return s

    def last_evaluate_at_sources(self) -> bool:
        """True when the last evaluate() found its targets to be the source points (bit for bit, row for row) and
        ran the resident-target path of the matvec (include/ferreus_bbfmm_hip.h, bbfmm_last_evaluate_at_sources)."""
        return int(self._lib.bbfmm_last_evaluate_at_sources(self._h)) == 1

    def debug_rows_of_sources(self, target_points):
        """Source rows of targets that are rows of the sources (bit for bit), or None when one of them is no source point."""
        x = self._targets(target_points)
        rows = np.zeros(x.shape[0], dtype=np.int64)
        ok = self._lib.bbfmm_debug_rows_of_sources(self._h, x.ctypes.data, x.shape[0], max(x.shape[0], 1), rows.ctypes.data)
        return rows if ok else None

    def last_evaluate_path(self) -> int:
        """0: the general path; 1: targets = the sources (resident target set; partitioned over the parts of a device group);
        2: targets = rows of the sources (cached plan of the index set); 3: arbitrary targets sharded over the parts of a
        device group -- bbfmm_last_evaluate_at_sources"""
        return int(self._lib.bbfmm_last_evaluate_at_sources(self._h))

    def debug_targets_are_sources(self, target_points) -> bool:
        """The host-side comparison bbfmm_evaluate runs on m == N targets (bit for bit, row for row)."""
        x = self._targets(target_points)
        return bool(self._lib.bbfmm_debug_targets_are_sources(self._h, x.ctypes.data, x.shape[0], max(x.shape[0], 1)))

    def tree_built_on_device(self) -> bool:
        return bool(self._lib.bbfmm_tree_built_on_device(self._h))

    def cells(self):
        s = self.stats()
        keys = np.zeros(s.n_cells, dtype=np.uint64)
        leaf = np.zeros(s.n_cells, dtype=np.uint8)
        self._raise(self._lib.bbfmm_get_cells(self._h, keys.ctypes.data, leaf.ctypes.data))
        return keys, leaf

    def leaf_sources(self):
        s = self.stats()
        ptr = np.zeros(s.n_cells + 1, dtype=np.int64)
        idx = np.zeros(max(s.n_points, 1), dtype=np.int64)
        self._raise(self._lib.bbfmm_get_leaf_sources(self._h, ptr.ctypes.data, idx.ctypes.data))
        return ptr, idx[:ptr[-1]]

    def interaction_list(self, which: str):
        s = self.stats()
        n = ctypes.c_int64(0)
        self._raise(self._lib.bbfmm_get_list(self._h, which.encode()[0:1], None, None, ctypes.byref(n)))
        ptr = np.zeros(s.n_cells + 1, dtype=np.int64)
        idx = np.zeros(max(n.value, 1), dtype=np.int32)
        self._raise(self._lib.bbfmm_get_list(self._h, which.encode()[0:1], ptr.ctypes.data,
                                             idx.ctypes.data, ctypes.byref(n)))
        return ptr, idx[:n.value]

    def m2l_ranks(self):
        s = self.stats()
        nref = ctypes.c_int32(0)
        self._raise(self._lib.bbfmm_get_m2l_ranks(self._h, None, ctypes.byref(nref)))
        ranks = np.zeros((s.depth + 1, nref.value), dtype=np.int32)
        self._raise(self._lib.bbfmm_get_m2l_ranks(self._h, ranks.ctypes.data, ctypes.byref(nref)))
        return ranks

    def m2l_operator(self, level: int, ref: int):
        n = self.stats().n_nodes
        out = np.zeros((n, n), order="F")
        self._raise(self._lib.bbfmm_get_m2l_operator(self._h, level, ref, out.ctypes.data))
        return out

    def m2l_factors(self, level: int, ref: int):
        """(U [n x r], Vt [r x n] or None) of one reference operator."""
        n = self.stats().n_nodes
        r = int(self.m2l_ranks()[level, ref])
        u = np.zeros((n, r), order="F")
        compressed = r < n or self._compressed
        vt = np.zeros((r, n), order="F") if compressed else None
        self._raise(self._lib.bbfmm_get_m2l_factors(self._h, level, ref, u.ctypes.data,
                                                    vt.ctypes.data if vt is not None else None))
        return u, vt

    def permutation_tables(self):
        n = self.stats().n_nodes
        nperm = ctypes.c_int32(0)
        self._raise(self._lib.bbfmm_get_permutation_tables(self._h, ctypes.byref(nperm), None, None,
                                                           None, None))
        nvec = 7 ** self.dim
        perm = np.zeros((nperm.value, n), dtype=np.int32)
        inv = np.zeros((nperm.value, n), dtype=np.int32)
        pl = np.zeros(nvec, dtype=np.int32)
        rl = np.zeros(nvec, dtype=np.int32)
        self._raise(self._lib.bbfmm_get_permutation_tables(
            self._h, ctypes.byref(nperm), perm.ctypes.data, inv.ctypes.data, pl.ctypes.data,
            rl.ctypes.data))
        return perm, inv, pl, rl

    def points_to_leaves(self, x):
        x = self._targets(x)
        m = x.shape[0]
        cells = np.zeros(max(m, 1), dtype=np.int32)
        bad = ctypes.c_int64(-1)
        rc = self._lib.bbfmm_points_to_leaves(self._h, x.ctypes.data, m, max(m, 1),
                                              cells.ctypes.data, ctypes.byref(bad))
        self._raise(rc, bad)
        return cells[:m]

    def debug_dense_m2m(self, child_index: int):
        n = self.stats().n_nodes
        out = np.zeros((n, n), order="F")
        self._raise(self._lib.bbfmm_debug_dense_m2m(self._h, child_index, out.ctypes.data))
        return out

    def debug_m2l_variants(self):
        """(number of stage-1 boundary variants, source cells that use one)"""
        nv, nc = ctypes.c_int64(), ctypes.c_int64()
        self._raise(self._lib.bbfmm_debug_m2l_variants(self._h, ctypes.byref(nv), ctypes.byref(nc)))
        return nv.value, nc.value

    def debug_m2l_pairs(self, stage=1):
        """(pairs_on, operators): per stage-1 operator a dict with level, octant, kind (0: class, 1: boundary variant
        or group operator), pairs (the vectors t whose product also serves Rt) and singles, as tuples of components.
        stage=2: the same for the stage-2 operators, the target lists of the classes (kind 0)."""
        fn = self._lib.bbfmm_debug_m2l_pairs if stage == 1 else self._lib.bbfmm_debug_m2l_pairs_stage2
        n, on = ctypes.c_int64(), ctypes.c_int32()
        self._raise(fn(self._h, None, 0, ctypes.byref(n), ctypes.byref(on)))
        buf = np.zeros(max(n.value, 1), dtype=np.int32)
        self._raise(fn(self._h, buf.ctypes.data, n.value, ctypes.byref(n), ctypes.byref(on)))
        d, ops, i = self.dim, [], 0
        while i < n.value:
            level, octant, kind, ne = (int(v) for v in buf[i:i + 4])
            ent = buf[i + 4:i + 4 + ne * (d + 1)].reshape(ne, d + 1)
            ops.append({"level": level, "octant": octant, "kind": kind,
                        "pairs": [tuple(int(x) for x in e[1:]) for e in ent if e[0] == 1],
                        "singles": [tuple(int(x) for x in e[1:]) for e in ent if e[0] == 0]})
            i += 4 + ne * (d + 1)
        return bool(on.value), ops

    def debug_m2l_pairs_axes(self, stage=1):
        """(info, operators) of stage 1 with both kinds of pairs.  info: axes in force (0: no pairs) and the executed work
        (column blocks x contraction steps over the level classes) of the one-axis and the two-axis layout.  Per operator:
        level, octant, kind, pad_cols (columns left empty to keep the kinds apart), yb0, block_kinds (per column block 0:
        x order, 1: y order), and x_pairs (listed by the member with t0 > 0), y_pairs (t1 > 0), singles as dicts
        vector -> (first, last) column block of its columns ((-1, -1): rank 0).
        stage=2: the target lists of the classes.  info as above with the work as contraction steps x column groups.  Per
        class: level, octant, kp (length of A), kpy (the y boundary: offset in A of the first y leader, kp without y
        pairs), k_pad, pad (entries of A left empty before kpy), and x_pairs, y_pairs (listed by their leaders), singles
        as dicts vector -> (slot offset, partner's slot offset or -1, rank)."""
        if stage == 2:
            fn = self._lib.bbfmm_debug_m2l_pairs_axes_stage2
            n = ctypes.c_int64()
            self._raise(fn(self._h, None, 0, ctypes.byref(n)))
            buf = np.zeros(max(n.value, 1), dtype=np.int32)
            self._raise(fn(self._h, buf.ctypes.data, n.value, ctypes.byref(n)))
            info = {"axes": int(buf[0]), "work_x": int(buf[1]), "work_xy": int(buf[2])}
            d, ops, i = self.dim, [], 3
            while i < n.value:
                level, octant, kp, kpy, k_pad, pad, ne = (int(v) for v in buf[i:i + 7])
                ent = buf[i + 7:i + 7 + ne * (d + 4)].reshape(ne, d + 4)
                by_kind = [{tuple(int(x) for x in e[4:]): (int(e[1]), int(e[2]), int(e[3])) for e in ent if e[0] == k}
                           for k in range(3)]
                ops.append({"level": level, "octant": octant, "kp": kp, "kpy": kpy, "k_pad": k_pad, "pad": pad,
                            "singles": by_kind[0], "x_pairs": by_kind[1], "y_pairs": by_kind[2]})
                i += 7 + ne * (d + 4)
            return info, ops
        fn = self._lib.bbfmm_debug_m2l_pairs_axes
        n = ctypes.c_int64()
        self._raise(fn(self._h, None, 0, ctypes.byref(n)))
        buf = np.zeros(max(n.value, 1), dtype=np.int32)
        self._raise(fn(self._h, buf.ctypes.data, n.value, ctypes.byref(n)))
        info = {"axes": int(buf[0]), "work_x": int(buf[1]), "work_xy": int(buf[2])}
        d, ops, i = self.dim, [], 3
        while i < n.value:
            level, octant, kind, pad_cols, yb0, n_blk, ne = (int(v) for v in buf[i:i + 7])
            kinds = [int(v) for v in buf[i + 7:i + 7 + n_blk]]
            ent = buf[i + 7 + n_blk:i + 7 + n_blk + ne * (d + 3)].reshape(ne, d + 3)
            by_kind = [{tuple(int(x) for x in e[3:]): (int(e[1]), int(e[2])) for e in ent if e[0] == k} for k in range(3)]
            ops.append({"level": level, "octant": octant, "kind": kind, "pad_cols": pad_cols, "yb0": yb0, "block_kinds": kinds,
                        "singles": by_kind[0], "x_pairs": by_kind[1], "y_pairs": by_kind[2]})
            i += 7 + n_blk + ne * (d + 3)
        return info, ops

    M2L_DIGEST_FAMILIES = ("scalars", "partners_orbits", "class_lists", "class_rows", "class_cells", "tiles1", "tiles2", "batches")

    def debug_m2l_table_digests(self):
        """(digests, flops_level) of a host_only handle: one 64-bit FNV-1a digest per family of the integer M2L tables, as a
        dict family -> hex string in the order of M2L_DIGEST_FAMILIES (csrc/fmm_tree.hpp lists what each family holds), and
        the M2L flop count of every level, which is a sum in a fixed order and is compared as a value."""
        n, nl = ctypes.c_int32(), ctypes.c_int32()
        self._raise(self._lib.bbfmm_debug_m2l_table_digests(self._h, None, 0, ctypes.byref(n), None, 0, ctypes.byref(nl)))
        assert n.value == len(self.M2L_DIGEST_FAMILIES)
        dig, fl = np.zeros(n.value, dtype=np.uint64), np.zeros(max(nl.value, 1))
        self._raise(self._lib.bbfmm_debug_m2l_table_digests(self._h, dig.ctypes.data, n.value, ctypes.byref(n), fl.ctypes.data,
                                                            nl.value, ctypes.byref(nl)))
        return {k: f"{int(v):016x}" for k, v in zip(self.M2L_DIGEST_FAMILIES, dig)}, [float(v) for v in fl[:nl.value]]

    def debug_m2l_s2_plan(self) -> tuple:
        """(ga, gb, ce, co, ya, yb): the kernel instance stage 2 runs in the parity basis -- column groups per chunk of the
        x-even and x-odd half, chunks per half, and with two axes the y-even groups of a chunk (0, 0 with one axis).  All
        zeros without stage-2 pairs.  The plan is made on the host: host_only handles answer too."""
        out = (ctypes.c_int32 * 6)()
        self._raise(self._lib.bbfmm_debug_m2l_s2_plan(self._h, out))
        return tuple(int(v) for v in out)

    WX_JOB_FIELDS = ("n_w_jobs", "n_wx_jobs", "n_wxl_jobs", "max_rows_wx", "max_rows_wxl", "max_cells_wx", "max_cells_wxl",
                     "max_cells_w")

    def debug_wx_jobs(self) -> dict:
        """The W / X jobs of the resident target set (targets = sources): the number of M2P jobs, of chunk jobs and of
        whole-leaf jobs of the fused M2P + P2L pass, the largest row count of a chunk job and of a whole-leaf job, the largest
        W-cell count of a chunk job, of a whole-leaf job and of an M2P job.  Planned on the host: host_only handles answer."""
        out = (ctypes.c_int32 * 8)()
        self._raise(self._lib.bbfmm_debug_wx_jobs(self._h, out))
        return {k: int(v) for k, v in zip(self.WX_JOB_FIELDS, out)}

    def debug_m2l_s2_last_ksplit(self) -> int:
        """Parts into which this handle's most recent parity-basis stage-2 launch split the contraction (0: none yet)."""
        ks = ctypes.c_int32()
        self._raise(self._lib.bbfmm_debug_m2l_s2_last_ksplit(self._h, ctypes.byref(ks)))
        return ks.value

    def debug_leaf_runs(self) -> dict:
        """The leaf passes over runs of leaves (BBFMM_LEAF_PASSES) of this handle: its mask, the runs of the resident target
        set's job list, the jobs outside every run, and all its jobs."""
        c = (ctypes.c_int32 * 4)()
        self._raise(self._lib.bbfmm_debug_leaf_runs(self._h, c))
        return {"mask": c[0], "runs": c[1], "rest": c[2], "jobs": c[3]}

    def debug_group_state(self) -> dict:
        """What a device group holds and has queued (bbfmm_debug_group_state): parts, whether BBFMM_GROUP_OWN_COPIES was set when
        the handle was created, the owner of every part's copy of the weights, the weight mirrors the primary holds now, and
        counted since creation: mirror pieces, peer copies, plain device copies between parts, waits for another part's copy,
        columns of device-resident weights copied to other parts; whether the runtime refused a peer copy within one device.
        A plain handle reports one part and zeros."""
        parts = self.device_count()
        c = (ctypes.c_int64 * (9 + parts))()
        self._raise(self._lib.bbfmm_debug_group_state(self._h, c, len(c)))
        keys = ("parts", "own_copies", "live_mirrors", "mirror_pieces", "peer_copies", "plain_copies", "weight_waits", "weights_in",
                "self_peer_refused")
        st = {k: int(v) for k, v in zip(keys, c[:9])}
        st["own_copies"], st["self_peer_refused"] = bool(st["own_copies"]), bool(st["self_peer_refused"])
        st["owners"] = [int(v) for v in c[9:9 + parts]]
        return st

    def debug_get_coefficients(self, which: str, k: int) -> np.ndarray:
        s = self.stats()
        n = s.n_nodes
        if which in ("P", "p"):  # Mp: the multipoles in stage 1's parity basis, whole rows with their pads
            ln = ctypes.c_int32(0)
            self._raise(self._lib.bbfmm_debug_m2l_parity_len(self._h, ctypes.byref(ln)))
            n = ln.value
        out = np.zeros((k, s.n_cells, n))
        self._raise(self._lib.bbfmm_debug_get_coefficients(self._h, which.encode()[0:1], k,
                                                           out.ctypes.data))
        return out

    def debug_apply_m2l_tables_host(self, M: np.ndarray) -> np.ndarray:
        M = np.ascontiguousarray(M, dtype=np.float64)
        Lc = np.zeros_like(M)
        self._raise(self._lib.bbfmm_debug_apply_m2l_tables_host(self._h, M.ctypes.data,
                                                                Lc.ctypes.data))
        return Lc


def make_grid(origin, steps, shape) -> L.Grid:
    """bbfmm_grid of a d-D grid: origin (d,), steps (d, d) with row j the world step of index j, shape (d,)"""
    origin = np.asarray(origin, dtype=np.float64).reshape(-1)
    d = origin.size
    steps = np.asarray(steps, dtype=np.float64)
    shape = [int(n) for n in np.asarray(shape).reshape(-1)]
    if not 1 <= d <= 3 or steps.shape != (d, d) or len(shape) != d:
        raise ValueError("a d-D grid needs an origin of d coordinates, (d, d) steps and d counts, d = 1..3")
    g = L.Grid()
    g.size, g.d = ctypes.sizeof(L.Grid), d
    for a in range(3):
        g.shape[a] = shape[a] if a < d else 1
    for j in range(d):
        g.origin[j] = origin[j]
        for a in range(d):
            g.steps[3 * j + a] = steps[j, a]
    return g


def debug_grid_coords(where: int, origin, steps, shape, r0: int, n: int) -> np.ndarray:
    """Rows [r0, r0 + n) of the grid (C order) as an (n, d) column-major array, through the one definition of
    csrc/evaluate_grid.hpp: where = 0 the host loop (no device needed), where = 1 the kernel."""
    g = make_grid(origin, steps, shape)
    out = np.zeros((n, g.d), order="F")
    rc = L.load().bbfmm_debug_grid_coords(int(where), ctypes.byref(g), int(r0), int(n), out.ctypes.data, max(n, 1))
    if rc != L.OK:
        raise (RuntimeError if rc == L.DEVICE_ERROR else ValueError)(f"bbfmm_debug_grid_coords failed with status {rc}")
    return out


def debug_split_runs(where: int, tgt_begin, tgt_end, job_cell, cap: int):
    """(begin, end, cell) of the jobs the runs are cut into with at most cap targets each (csrc/targets.hpp): where = 0
    the host loop, where = 1 the count / scan / fill kernels."""
    tb = np.ascontiguousarray(tgt_begin, dtype=np.int32)
    te = np.ascontiguousarray(tgt_end, dtype=np.int32)
    jc = np.ascontiguousarray(job_cell, dtype=np.int32)
    if not tb.shape == te.shape == jc.shape or tb.ndim != 1:
        raise ValueError("one begin, end and cell per run")
    lib, n, nj = L.load(), tb.size, ctypes.c_int64(0)

    def check(rc):
        if rc != L.OK:
            raise (RuntimeError if rc == L.DEVICE_ERROR else ValueError)(f"bbfmm_debug_split_runs failed with status {rc}")

    check(lib.bbfmm_debug_split_runs(int(where), tb.ctypes.data, te.ctypes.data, jc.ctypes.data, n, int(cap), None, None, None, 0,
                                     ctypes.byref(nj)))
    ob, oe, oc = (np.zeros(max(nj.value, 1), dtype=np.int32) for _ in range(3))
    check(lib.bbfmm_debug_split_runs(int(where), tb.ctypes.data, te.ctypes.data, jc.ctypes.data, n, int(cap), ob.ctypes.data,
                                     oe.ctypes.data, oc.ctypes.data, nj.value, ctypes.byref(nj)))
    return ob[:nj.value], oe[:nj.value], oc[:nj.value]


def fp64_valu_selftest():
    """(chip-wide v_fma_f64 TFLOP/s, shader clock in MHz during the run) on the current device."""
    tf, mhz = ctypes.c_double(0), ctypes.c_double(0)
    if L.load().bbfmm_fp64_valu_selftest(ctypes.byref(tf), ctypes.byref(mhz)) != L.OK:
        raise RuntimeError("the FP64 VALU microbenchmark needs a HIP device")
    return tf.value, mhz.value


def mfma_f64_selftest():
    """(measured FP64 MFMA TFLOP/s, lane-layout mismatches) on the current device."""
    tf = ctypes.c_double(0)
    errs = ctypes.c_int32(-1)
    info = (ctypes.c_double * 6)()
    rc = L.load().bbfmm_mfma_f64_selftest(ctypes.byref(tf), ctypes.byref(errs), info)
    if rc != L.OK:
        raise RuntimeError("MFMA self-test needs a HIP device")
    mfma_f64_selftest.info = dict(zip(["cycles_per_mfma_lone_wave", "clock_mhz_lone_wave",
                                       "cycles_per_mfma_per_simd_busy", "clock_mhz_busy",
                                       "tflops_1wave_per_simd", "tflops_2waves_per_simd"], list(info)))
    return tf.value, errs.value


def debug_kernel_values(where: int, kernel_id: int, base_range: float, total_sill: float, r2):
    """(value, value of the gradient path, gradient factor) of kernel `kernel_id` at each squared distance of r2, through
    the functions of csrc/kernels.hpp: where = 0 the host branch (no device needed), where = 1 the device branch."""
    x = np.ascontiguousarray(r2, dtype=np.float64).ravel()
    v, vg, f = np.empty_like(x), np.empty_like(x), np.empty_like(x)
    rc = L.load().bbfmm_debug_kernel_values(where, kernel_id, float(base_range), float(total_sill), x.ctypes.data, x.size,
                                            v.ctypes.data, vg.ctypes.data, f.ctypes.data)
    if rc != L.OK:
        raise RuntimeError(f"bbfmm_debug_kernel_values failed with status {rc}")
    return v, vg, f


DEBUG_MATH = {"sqrt": 0, "sqrt_rsqrt": 1, "rcp": 2, "log": 3}


def debug_math(where: int, which: str, x):
    """bb_sqrt / bb_sqrt_rsqrt / bb_rcp / bb_log of csrc/kernels.hpp element by element (where as in debug_kernel_values);
    "sqrt_rsqrt" returns the pair (sqrt, 1 / sqrt)."""
    x = np.ascontiguousarray(x, dtype=np.float64).ravel()
    out, out2 = np.empty_like(x), np.empty_like(x)
    rc = L.load().bbfmm_debug_math(where, DEBUG_MATH[which], x.ctypes.data, x.size, out.ctypes.data,
                                   out2.ctypes.data if which == "sqrt_rsqrt" else None)
    if rc != L.OK:
        raise RuntimeError(f"bbfmm_debug_math failed with status {rc}")
    return (out, out2) if which == "sqrt_rsqrt" else out
