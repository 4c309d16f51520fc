"""MI355X-native BBFMM matvec for ferreus_rbf_rs's RBF solve hot path.

`FmmTree` mirrors ferreus_rbf_utils::FmmTree / py_ferreus_bbfmm.FmmTree; all passes run
as HIP kernels behind the C ABI in include/ferreus_bbfmm_hip.h.
"""
from .fmm_tree import (FmmError, FmmKernelType, FmmParams, FmmTree, KernelDoesNotSupportGradients,
                       KernelParams, KernelType, M2LCompressionType, PointOutsideTree,
                       SpheroidalOrder, mfma_f64_selftest, fp64_valu_selftest,
                       debug_kernel_values, debug_math)

from . import solvers  # noqa: E402  (FGMRES / Schwarz drivers, iterative_solvers.rs)
from . import rbf  # noqa: E402  (RBFInterpolator: fit, evaluate and mesh in one object, rbf.rs)
from . import rmt  # noqa: E402  (isosurfaces of any field: composite interpolants and callables, py_ferreus_rmt)
from .isosurface import (clip_mesh, close_mesh, isosurface_from_values, isosurfaces_from_values,  # noqa: E402
                         mesh_self_intersections, triangle_pair)

__all__ = ["solvers", "rbf", "rmt", "FmmTree", "FmmParams", "KernelParams", "KernelType", "FmmKernelType",
           "SpheroidalOrder", "M2LCompressionType", "FmmError", "PointOutsideTree",
           "KernelDoesNotSupportGradients", "mfma_f64_selftest", "fp64_valu_selftest", "debug_kernel_values", "debug_math",
           "isosurface_from_values", "isosurfaces_from_values", "clip_mesh", "close_mesh", "mesh_self_intersections",
           "triangle_pair"]
