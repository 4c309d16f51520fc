"""py_ferreus_rmt / ferreus_rbf.isosurfacing: isosurfaces of any field (ferreus_rmt::build_isosurface, isosurface.rs:488-540;
python_bindings.rs:258-282, 378-400).  `surface_fn` is one of two things:

* a `FieldExpr`, built from `field`, `height_field`, `affine`, `box`, `maximum`, `minimum`, unary minus, `+ / - float` and
  `* float`: interpolants combined on the device by a postfix program (bbfmm_isosurfaces_from_fields_opts; DESIGN.md
  "Composite fields"), with no Python in the loop;
* any callable `f(targets (m, 3)) -> (m,) or (m, 1)`, with `gradient_fn(targets) -> (values, (m, 3))`: every batch of
  lattice nodes crosses the host and Python (bbfmm_isosurfaces_from_function_opts), as in the reference.

    clipped = rmt.maximum(rmt.field(model) - 20.0, rmt.height_field(topo, axis=2))      # isosurface_linear_topo
    mesh = rmt.build_isosurface(seed_points, extents, 5.0, 0.0, clipped)
    mesh2 = rmt.build_isosurface(seed_points, extents, 10.0, 0.0, model.evaluate_targets,  # isosurface_linear_rmt
                                 gradient_fn=model.evaluate_targets_with_gradients)

Boundary closure other than BoundaryClosure.None_ raises NotImplementedError (see `box`).
"""
from __future__ import annotations

import ctypes
from typing import Callable, Optional, Sequence, Union

import numpy as np

from . import _lib as L
from . import isosurface as _iso
from .fmm_tree import CallbackFailed
from .rbf import BoundaryClosure, ClusterMethod, Mesh, Progress, RBFInterpolator, SurfacingProgress, FieldTerms, _extents_of

__all__ = ["FieldExpr", "field", "height_field", "affine", "box", "maximum", "minimum", "build_isosurface", "build_isosurfaces",
           "compile_expr", "BoundOperand", "isosurfaces_from_fields", "evaluate_fields", "CallbackFailed", "MAX_OPERANDS", "MAX_PROGRAM", "MAX_STACK"]

MAX_OPERANDS, MAX_PROGRAM, MAX_STACK = 8, 64, 8
_CLUSTER = {ClusterMethod.None_: "none", ClusterMethod.Average: "average", ClusterMethod.CurvatureWeighted: "curvature"}


class _Operand:
    def __init__(self, kind, source=None, axis=2, column=0, coefficients=None, scale=1.0, offset=0.0):
        self.kind, self.source, self.axis, self.column = kind, source, int(axis), int(column)
        self.coefficients = coefficients
        self.scale, self.offset = float(scale), float(offset)

    def moved(self, scale, offset):
        return _Operand(self.kind, self.source, self.axis, self.column, self.coefficients, scale, offset)


def _number(c, what):
    if isinstance(c, FieldExpr) or not np.isscalar(c) or isinstance(c, (bool, np.bool_, complex, str, bytes)):
        raise ValueError(f"{what} takes a real number, got {type(c).__name__} (combine fields with rmt.maximum / rmt.minimum)")
    c = float(c)
    if not np.isfinite(c):
        raise ValueError(f"{what} takes a finite number")
    return c


class FieldExpr:
    """A field over world points: one operand pushed as scale * v + offset, or max / min / neg of expressions."""

    def __init__(self, op, *args):
        self.op, self.args = op, args          # "operand" (_Operand,), "max" / "min" (a, b), "neg" (a,)

    def _leaf(self, what):
        if self.op != "operand":
            raise ValueError(f"{what} a combined expression is not supported: only an operand's own scale and offset and unary "
                             "minus are expressible (apply it to the operands instead)")
        return self.args[0]

    def __neg__(self):
        return FieldExpr("neg", self)

    def __add__(self, c):
        c, o = _number(c, "+"), self._leaf("an offset on")
        return FieldExpr("operand", o.moved(o.scale, o.offset + c))

    __radd__ = __add__

    def __sub__(self, c):
        c, o = _number(c, "-"), self._leaf("an offset on")
        return FieldExpr("operand", o.moved(o.scale, o.offset - c))

    def __rsub__(self, c):                   # c - (scale * v + offset): the operand with scale -scale and offset c - offset
        c, o = _number(c, "-"), self._leaf("an offset on")
        return FieldExpr("operand", o.moved(-o.scale, c - o.offset))

    def __mul__(self, c):
        c, o = _number(c, "*"), self._leaf("a scale on")
        return FieldExpr("operand", o.moved(o.scale * c, o.offset * c))

    __rmul__ = __mul__


def field(rbfi: RBFInterpolator, column: int = 0) -> FieldExpr:
    """The 3-D interpolant `rbfi` (its kernel sum, polynomial and global trend), value column `column`."""
    if not isinstance(rbfi, RBFInterpolator) or rbfi.dimensions != 3:
        raise ValueError("rmt.field takes a 3-D RBFInterpolator")
    if not 0 <= int(column) < rbfi.source_values.shape[1]:
        raise ValueError(f"column {column} of {rbfi.source_values.shape[1]}")
    return FieldExpr("operand", _Operand(L.FIELD_MODEL, rbfi, column=column))


def height_field(rbfi2d: RBFInterpolator, axis: int = 2, column: int = 0) -> FieldExpr:
    """x[axis] - g(u, v): (u, v) the other two coordinates in ascending axis order, g the 2-D interpolant `rbfi2d`.
    Negative below the surface g, so `maximum(model, height_field(topo))` cuts the model off above the topography."""
    if not isinstance(rbfi2d, RBFInterpolator) or rbfi2d.dimensions != 2:
        raise ValueError("rmt.height_field takes a 2-D RBFInterpolator")
    if int(axis) not in (0, 1, 2):
        raise ValueError("axis must be 0, 1 or 2")
    if not 0 <= int(column) < rbfi2d.source_values.shape[1]:
        raise ValueError(f"column {column} of {rbfi2d.source_values.shape[1]}")
    return FieldExpr("operand", _Operand(L.FIELD_HEIGHT, rbfi2d, axis=axis, column=column))


def affine(c0: float, c: Sequence[float]) -> FieldExpr:
    """c0 + c[0] x0 + c[1] x1 + c[2] x2, summed left to right."""
    co = np.concatenate([[float(c0)], np.asarray(c, dtype=np.float64).reshape(-1)])
    if co.shape != (4,) or not np.all(np.isfinite(co)):
        raise ValueError("rmt.affine takes c0 and three finite coefficients")
    return FieldExpr("operand", _Operand(L.FIELD_AFFINE, coefficients=co))


def _fold(op, exprs):
    if len(exprs) == 1 and not isinstance(exprs[0], FieldExpr):
        exprs = tuple(exprs[0])
    if len(exprs) < 1 or not all(isinstance(e, FieldExpr) for e in exprs):
        raise ValueError(f"rmt.{op}imum takes FieldExpr arguments")
    out = exprs[0]
    for e in exprs[1:]:
        out = FieldExpr(op, out, e)
    return out


def maximum(*exprs) -> FieldExpr:
    """max of the arguments, folded left: max(max(a, b), c).  Of two equal values the earlier one is kept."""
    return _fold("max", exprs)


def minimum(*exprs) -> FieldExpr:
    return _fold("min", exprs)


def box(extents) -> FieldExpr:
    """The maximum of the six affines lo_a - x_a, x_a - hi_a (a = 0, 1, 2 in that order): negative inside the box.
    `maximum(expr, rmt.box(extents))` with a box strictly inside the extraction extents yields a closed mesh, the way the
    topography example closes its model at the topography: the surface of `expr` inside the box and the box's faces where
    `expr` is negative.  It is the level set of a max, so it is bevelled within one lattice cell of the box's rim and
    edges; it is not the reference's planar cap (BoundaryClosure.ClosePositive / CloseNegative, not implemented)."""
    e = _iso._ext(extents)
    if not np.all(np.isfinite(e)) or not np.all(e[:3] <= e[3:]):
        raise ValueError("box: finite extents with min <= max")
    planes = []
    for a in range(3):
        unit = np.zeros(3)
        unit[a] = 1.0
        planes.append(affine(e[a], -unit))
        planes.append(affine(-e[3 + a], unit))
    return maximum(*planes)


def compile_expr(expr: FieldExpr):
    """(operands, program): the _Operand leaves in order of first push and the postfix codes."""
    if not isinstance(expr, FieldExpr):
        raise ValueError("a FieldExpr is needed")
    operands, program = [], []
    codes = {"max": L.FIELD_OP_MAX, "min": L.FIELD_OP_MIN, "neg": L.FIELD_OP_NEG}
    depth = [0, 0]

    def walk(e):
        if e.op == "operand":
            program.append(len(operands))
            operands.append(e.args[0])
            depth[0] += 1
            depth[1] = max(depth)
            return
        for a in e.args:
            walk(a)
        program.append(codes[e.op])
        depth[0] -= len(e.args) - 1

    walk(expr)
    if len(operands) > MAX_OPERANDS:
        raise ValueError(f"the expression has {len(operands)} operands, at most {MAX_OPERANDS} are supported")
    if len(program) > MAX_PROGRAM:
        raise ValueError(f"the expression compiles to {len(program)} codes, at most {MAX_PROGRAM} are supported")
    if depth[1] > MAX_STACK:
        raise ValueError(f"the expression needs a stack of {depth[1]}, at most {MAX_STACK} is supported (fold it to the left)")
    return operands, program


def _column_terms(rbfi: RBFInterpolator, column: int) -> Optional[FieldTerms]:
    poly, gt = rbfi.coefficients.poly_coefficients, rbfi.global_trend
    if poly is None and gt is None:
        return None
    return FieldTerms(rbfi.dimensions, rbfi.settings.polynomial_degree if rbfi.basis_size else -1,
                      None if poly is None else np.asfortranarray(poly[:, column:column + 1]), rbfi.translation_factor, rbfi.scale_factor,
                      None if gt is None else gt.B, None if gt is None else gt.b)


def _evaluator(o: _Operand, ext: np.ndarray, resolution: float):
    """The evaluator tree of one operand, as RBFInterpolator.build_isosurfaces makes it (rbf.rs:990-998): the union of the
    source and isosurface extents +- 10 resolutions, for a height field on its two in-plane axes."""
    rbfi = o.source
    axes = [0, 1, 2] if o.kind == L.FIELD_MODEL else [a for a in range(3) if a != o.axis]
    d = len(axes)
    src = _extents_of(rbfi.source_points)
    lo, hi = ext[:3][axes], ext[3:][axes]
    ev = np.concatenate([np.minimum(src[:d], lo) - 10.0 * resolution, np.maximum(src[d:], hi) + 10.0 * resolution])
    tree = rbfi._tree(True, False, ev)
    w = np.asfortranarray(rbfi.coefficients.point_coefficients[:, o.column:o.column + 1])
    tree.set_weights(w)
    tree.set_local_coefficients(w)
    return tree, _column_terms(rbfi, o.column)


class BoundOperand:
    """One bbfmm_field_operand over a tree that is ready (set_local_coefficients, one column): kind L.FIELD_MODEL (a d = 3
    FmmTree), L.FIELD_HEIGHT (d = 2, with `axis`) or L.FIELD_AFFINE (`coefficients` [c0, c1, c2, c3], no tree); `terms` the
    rbf.FieldTerms of the tree's interpolant or None."""

    def __init__(self, kind, tree=None, terms=None, axis=2, scale=1.0, offset=0.0, coefficients=None):
        self.kind, self.tree, self.terms, self.axis = int(kind), tree, terms, int(axis)
        self.scale, self.offset = float(scale), float(offset)
        self.coefficients = None if coefficients is None else np.asarray(coefficients, dtype=np.float64).reshape(4)


def _bind(o: _Operand, ext, resolution) -> BoundOperand:
    if o.kind == L.FIELD_AFFINE:
        return BoundOperand(o.kind, scale=o.scale, offset=o.offset, coefficients=o.coefficients)
    tree, terms = _evaluator(o, ext, resolution)
    return BoundOperand(o.kind, tree, terms, o.axis, o.scale, o.offset)


def _c_operands(operands):
    """(ctypes array, objects to keep alive, device of the first tree or None)"""
    arr = (L.FieldOperand * max(len(operands), 1))()
    keep, device = [], None
    for q, o in enumerate(operands):
        c = arr[q]
        c.size = ctypes.sizeof(L.FieldOperand)
        c.kind, c.axis, c.scale, c.offset = o.kind, o.axis, o.scale, o.offset
        if o.coefficients is not None:
            for a in range(4):
                c.affine[a] = o.coefficients[a]
        if o.tree is not None:
            c.handle = o.tree._h
            if device is None:
                device = o.tree.device()
        if o.terms is not None:
            ct = o.terms._c()
            keep += [o.terms, ct]
            c.terms = ctypes.addressof(ct)
    return arr, keep, device


def isosurfaces_from_fields(operands, program, extents, resolution, isovalues, *, cluster="none", finish="raw",
                            self_intersections="ignore", follow="dense", seeds=None, return_stats=False, return_field=False,
                            batch_bytes: int = 0):
    """bbfmm_isosurfaces_from_fields_opts on BoundOperands and a postfix program (codes >= 0: push that operand,
    L.FIELD_OP_MAX / _MIN / _NEG), with the options and the return value of isosurface.build_isosurfaces: a list of
    (vertices, facets[, stats]) per isovalue, and the lattice field with return_field."""
    lib = L.load()
    cm, fin, isect = _iso._cluster(cluster), _iso._finish(finish), _iso._self_intersections(self_intersections)
    fol, sd = _iso._follow(follow), _iso._seeds(seeds)
    if fol and sd is None:
        raise ValueError("follow='surface' of a composite field needs seeds")
    ext, iso = _iso._ext(extents), _iso._isovalues(isovalues)
    opts = _iso._options(cm, fin, batch_bytes, isect, fol, sd if fol else None)
    arr, keep, device = _c_operands(operands)
    prog = np.ascontiguousarray(program, dtype=np.int32)
    field_t = info = None
    if return_field:
        import torch
        info = _iso.lattice_info(ext, resolution)
        dev = torch.device(f"cuda:{device if device is not None else torch.cuda.current_device()}")
        field_t = torch.full((int(np.prod(info["shape"])),), float("nan"), dtype=torch.float64, device=dev)
        torch.cuda.synchronize(dev)
    res = ctypes.c_void_p()
    rc = lib.bbfmm_isosurfaces_from_fields_opts(arr, len(operands), prog.ctypes.data, len(prog), ext.ctypes.data, float(resolution),
                                                iso.ctypes.data, len(iso), field_t.data_ptr() if field_t is not None else None,
                                                ctypes.addressof(opts), ctypes.byref(res))
    del keep
    try:
        if rc != L.OK:
            _iso._raise(rc, lib.bbfmm_isosurface_error(res).decode() if res else "isosurface extraction failed")
        meshes = _iso._meshes(lib, res, return_stats, fin, isect, fol, cm)
    finally:
        if res:
            lib.bbfmm_isosurface_destroy(res)
    if return_field:
        return meshes, field_t.cpu().numpy().reshape(info["shape"])
    return meshes


def evaluate_fields(operands, program, points, with_gradients: bool = False):
    """The composite field of BoundOperands and a postfix program at `points` ((m, 3) world points), through the device path
    the extraction takes (bbfmm_debug_evaluate_fields): values (m,), and with_gradients also the gradients (m, 3)."""
    lib = L.load()
    x = np.asarray(points, dtype=np.float64)
    if x.ndim != 2 or x.shape[1] != 3:
        raise ValueError(f"points must have shape (m, 3), got {x.shape}")
    x = np.asfortranarray(x)
    m = len(x)
    arr, keep, _ = _c_operands(operands)
    prog = np.ascontiguousarray(program, dtype=np.int32)
    values = np.zeros(m)
    grad = np.zeros((m, 3), order="F") if with_gradients else None
    rc = lib.bbfmm_debug_evaluate_fields(arr, len(operands), prog.ctypes.data, len(prog), x.ctypes.data, m, max(m, 1), values.ctypes.data,
                                         grad.ctypes.data if grad is not None else None, max(m, 1))
    del keep
    if rc != L.OK:
        h = next((o.tree._h for o in operands if o.tree is not None), None)
        _iso._raise(rc, lib.bbfmm_last_error(h).decode() if h else "evaluate_fields: bad operands or program")
    return (values, np.ascontiguousarray(grad)) if with_gradients else values


def _values_of(out, m, what):
    a = np.asarray(out)
    if a.dtype == object or not (np.issubdtype(a.dtype, np.floating) or np.issubdtype(a.dtype, np.integer)):
        raise ValueError(f"{what} must return real numbers, got dtype {a.dtype}")
    if a.shape not in ((m,), (m, 1)):
        raise ValueError(f"{what} must return {m} values of shape ({m},) or ({m}, 1), got {a.shape}")
    return a.reshape(m).astype(np.float64, copy=False)


def _trampolines(surface_fn, gradient_fn, caught):
    """The two C callbacks; an exception inside a callable is stored in `caught` and reported as a failure."""

    def targets(x, m, ldx):
        return np.ascontiguousarray(np.ctypeslib.as_array(x, shape=(3, ldx))[:, :m].T)

    def on_field(x, m, ldx, values, user):
        try:
            np.ctypeslib.as_array(values, shape=(m,))[:] = _values_of(surface_fn(targets(x, m, ldx)), m, "surface_fn")
            return 0
        except BaseException as e:  # noqa: BLE001 -- re-raised by the caller of the C entry
            caught.append(e)
            return 1

    def on_gradient(x, m, ldx, values, gradients, ldg, user):
        try:
            out = gradient_fn(targets(x, m, ldx))
            if not isinstance(out, (tuple, list)) or len(out) != 2:
                raise ValueError("gradient_fn must return (values, gradients)")
            np.ctypeslib.as_array(values, shape=(m,))[:] = _values_of(out[0], m, "gradient_fn")
            g = np.asarray(out[1])
            if g.shape == (m, 1, 3):
                g = g.reshape(m, 3)
            if g.shape != (m, 3) or not np.issubdtype(g.dtype, np.floating):
                raise ValueError(f"gradient_fn must return float gradients of shape ({m}, 3), got {g.shape} {g.dtype}")
            np.ctypeslib.as_array(gradients, shape=(3, ldg))[:, :m] = g.T
            return 0
        except BaseException as e:  # noqa: BLE001
            caught.append(e)
            return 1

    return L.FIELD_FN(on_field), (L.GRADIENT_FN(on_gradient) if gradient_fn is not None else None)


def build_isosurfaces(seed_points, extents, resolution: float, isovalues, isosurface_fn: Union[FieldExpr, Callable], *,
                      gradient_fn: Optional[Callable] = None, cluster_method: Optional[ClusterMethod] = ClusterMethod.CurvatureWeighted,
                      boundary_closure: Optional[BoundaryClosure] = BoundaryClosure.None_, progress_callback: Optional[Progress] = None,
                      follow="surface", finish="clipped", self_intersections="rollback", return_stats=False, return_field=False,
                      batch_bytes: int = 0):
    """One rbf.Mesh per isovalue of `isosurface_fn`, a FieldExpr or a callable (see the module), followed from
    `seed_points` ((n, 3) world points).  The keywords past progress_callback are those of
    RBFInterpolator.build_isosurfaces with its defaults (finish="close_positive" / "close_negative": the mesh closed on the
    faces of the extents); return_field needs a FieldExpr.  `gradient_fn` is used by the seed
    projection of a callable and ignored for a FieldExpr, which has its own gradient."""
    closure = BoundaryClosure.None_ if boundary_closure is None else BoundaryClosure(boundary_closure)
    if closure is not BoundaryClosure.None_:
        raise NotImplementedError(f"boundary_closure=BoundaryClosure.{closure.name} is not mapped onto the closure yet: pass "
                                  f"finish={'close_positive' if closure is BoundaryClosure.ClosePositive else 'close_negative'!r} instead")
    method = ClusterMethod.CurvatureWeighted if cluster_method is None else ClusterMethod(cluster_method)
    lib = L.load()
    cm, fin, isect = _iso._cluster(_CLUSTER[method]), _iso._finish(finish), _iso._self_intersections(self_intersections)
    fol = _iso._follow(follow)
    sd = _iso._seeds(seed_points)
    if fol and sd is None:
        raise ValueError("follow='surface' needs seed_points")
    ext, iso = _iso._ext(extents), _iso._isovalues(isovalues)
    resolution = float(resolution)
    progress = progress_callback
    for v in iso:
        if progress is not None:
            progress.emit(SurfacingProgress(float(v), "started", 0.0))
    field = None
    if isinstance(isosurface_fn, FieldExpr):
        operands, program = compile_expr(isosurface_fn)
        bound = [_bind(o, ext, resolution) for o in operands]
        out = isosurfaces_from_fields(bound, program, ext, resolution, iso, cluster=_CLUSTER[method], finish=finish,
                                      self_intersections=self_intersections, follow=follow, seeds=sd if fol else None,
                                      return_stats=return_stats, return_field=return_field, batch_bytes=batch_bytes)
        meshes, field = out if return_field else (out, None)
    elif callable(isosurface_fn):
        if return_field:
            raise ValueError("return_field needs a FieldExpr")
        if gradient_fn is not None and not callable(gradient_fn):
            raise ValueError("gradient_fn must be callable")
        caught = []
        opts = _iso._options(cm, fin, batch_bytes, isect, fol, sd if fol else None)
        f, g = _trampolines(isosurface_fn, gradient_fn, caught)
        res = ctypes.c_void_p()
        rc = lib.bbfmm_isosurfaces_from_function_opts(f, g, None, ext.ctypes.data, resolution, iso.ctypes.data, len(iso),
                                                      ctypes.addressof(opts), ctypes.byref(res))
        try:
            if caught:
                raise caught[0]
            if rc != L.OK:
                _iso._raise(rc, lib.bbfmm_isosurface_error(res).decode() if res else "isosurface extraction failed")
            meshes = _iso._meshes(lib, res, return_stats, fin, isect, fol, cm)
        finally:
            if res:
                lib.bbfmm_isosurface_destroy(res)
    else:
        raise ValueError("surface_fn must be a rmt.FieldExpr or a callable")
    result = [Mesh(m[0], m[1], m[2] if return_stats else None) for m in meshes]
    for v in iso:
        if progress is not None:
            progress.emit(SurfacingProgress(float(v), "finished", 1.0))
    return (result, field) if return_field else result


def build_isosurface(seed_points, extents, resolution: float, isovalue: float, surface_fn: Union[FieldExpr, Callable], **options):
    """build_isosurfaces for one isovalue: the Mesh (and the field with return_field)."""
    out = build_isosurfaces(seed_points, extents, resolution, [isovalue], surface_fn, **options)
    if options.get("return_field"):
        return out[0][0], out[1]
    return out[0]
