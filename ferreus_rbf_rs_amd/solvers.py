"""Iterative solvers of ferreus_rbf behind the C ABI (ferreus_rbf/src/iterative_solvers.rs).

`fgmres` / `schwarz_ddm_solver` take Python callables for the operator and the right
preconditioner exactly like the reference takes closures; `RbfSystemOperator` is the
reference's `IterativeSolver::matvec` (rbf.rs:105-117) on the device tree, bound natively (no
Python in the matvec path).  Everything computes in libferreus_bbfmm_hip.so.

`vectors="device"` runs the same drivers with every vector in device memory (bbfmm_fgmres_device,
bbfmm_schwarz_ddm_solver_device; DESIGN.md, "Device-resident solvers"): the operators are then the native wrappers'
device twins or callables on torch tensors, and `b` / `x0` may be torch tensors on the device.
"""
from __future__ import annotations

import ctypes
import enum
from typing import Callable, List, Optional, Tuple

import numpy as np

from . import _lib as L


class FittingAccuracyType(enum.IntEnum):
    """interpolant_config.rs:54-63"""
    Absolute = L.ACCURACY_ABSOLUTE
    Relative = L.ACCURACY_RELATIVE


class FittingAccuracy:
    """interpolant_config.rs:80-92 (defaults 1e-6, Relative)."""

    def __init__(self, tolerance: float = 1e-6,
                 tolerance_type: FittingAccuracyType = FittingAccuracyType.Relative):
        self.tolerance = float(tolerance)
        self.tolerance_type = FittingAccuracyType(tolerance_type)


def givens_rotation(f: float, g: float) -> Tuple[float, float, float]:
    """iterative_solvers.rs:185-227"""
    c, s, r = ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
    L.load().bbfmm_givens_rotation(f, g, ctypes.byref(c), ctypes.byref(s), ctypes.byref(r))
    return c.value, s.value, r.value


class _Operator:
    """(function pointer, user pointer) pair for a bbfmm_apply_fn; keeps its referents alive."""

    def __init__(self, fn_ptr, user_ptr, keep):
        self.fn_ptr, self.user_ptr, self._keep = fn_ptr, user_ptr, keep


def _wrap_callable(f: Callable[[np.ndarray], np.ndarray]) -> _Operator:
    err: List[BaseException] = []

    def tramp(_user, x, y, n):
        try:
            xa = np.ctypeslib.as_array(x, shape=(n,))
            out = np.asarray(f(xa), dtype=np.float64).reshape(-1)
            if out.size != n:
                raise ValueError(f"operator returned {out.size} values for a vector of {n}")
            np.ctypeslib.as_array(y, shape=(n,))[:] = out
            return L.OK
        except BaseException as e:  # noqa: BLE001 -- must not unwind through C
            err.append(e)
            return L.BAD_ARGUMENT

    cb = L.APPLY_FN(tramp)
    op = _Operator(ctypes.cast(cb, ctypes.c_void_p), None, (cb, err))
    op.errors = err
    return op


class RbfSystemOperator:
    """IterativeSolver::matvec (rbf.rs:105-117): y = fast_matrix_vector_product(tree, x, basis_size,
    all sources, monomial_matrix, nugget) with the native entry point as the callback."""

    def __init__(self, tree, basis_size: int = 0, monomial_matrix=None, nugget: float = 0.0):
        self.tree = tree
        self.n = tree.n_points + int(basis_size)
        self._poly = None if monomial_matrix is None else np.asfortranarray(monomial_matrix, dtype=np.float64)
        self._sys = L.RbfSystem(tree._h, int(basis_size),
                                None if self._poly is None else self._poly.ctypes.data,
                                0 if self._poly is None else self._poly.shape[0], float(nugget))
        lib = L.load()
        self._op = _Operator(ctypes.cast(lib.bbfmm_rbf_system_apply, ctypes.c_void_p),
                             ctypes.cast(ctypes.pointer(self._sys), ctypes.c_void_p), (self._sys, self._poly, tree))
        self._op.errors = []
        self._basis_size, self._nugget = int(basis_size), float(nugget)
        self._dev = None                     # bbfmm_rbf_system_device*, created by the first device solve or apply
        self._dop_cache = None

    def __call__(self, x):
        x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1)
        y = np.zeros_like(x)
        rc = L.load().bbfmm_rbf_system_apply(self._op.user_ptr, x.ctypes.data, y.ctypes.data, x.size)
        if rc != L.OK:
            raise RuntimeError(f"bbfmm_rbf_system_apply failed with status {rc}")
        return y

    @property
    def _dop(self) -> "_Operator":
        """The device twin (bbfmm_rbf_system_apply_device): the monomial matrix goes to the device once."""
        if self._dop_cache is None:
            lib = L.load()
            h = ctypes.c_void_p()
            rc = lib.bbfmm_rbf_system_device_create(self.tree._h, self._basis_size,
                                                    None if self._poly is None else self._poly.ctypes.data,
                                                    0 if self._poly is None else self._poly.shape[0], self._nugget,
                                                    ctypes.byref(h))
            if rc != L.OK:
                msg = lib.bbfmm_last_error(self.tree._h)
                raise RuntimeError(f"bbfmm_rbf_system_device_create failed with status {rc}: {(msg or b'').decode()}")
            self._dev, self._lib = h, lib
            self._dop_cache = _Operator(ctypes.cast(lib.bbfmm_rbf_system_apply_device, ctypes.c_void_p), h, (self.tree,))
            self._dop_cache.errors = []
        return self._dop_cache

    def apply_device(self, x):
        """y = A x for a float64 torch tensor on the tree's device; returns a tensor there (nothing crosses the bus)."""
        return _apply_native_device(self._dop, self.tree, x, "bbfmm_rbf_system_apply_device")

    def close(self) -> None:
        """Release the device copy of the monomial matrix now (also done when the last reference goes)."""
        if getattr(self, "_dev", None):
            self._lib.bbfmm_rbf_system_device_destroy(self._dev)
            self._dev = self._dop_cache = None

    def __del__(self):
        self.close()


def _apply_native_device(dop, tree, x, what):
    import torch
    dev = torch.device("cuda", tree.device())
    if not (isinstance(x, torch.Tensor) and x.device == dev and x.dtype == torch.float64):
        raise TypeError(f"{what}: a float64 torch tensor on {dev} is expected")
    x = x.contiguous().reshape(-1)
    y = torch.empty_like(x)
    torch.cuda.synchronize(dev)               # x was written on torch's streams, the operator runs on the tree's
    fn = ctypes.cast(dop.fn_ptr, L.APPLY_DEVICE_FN)
    rc = fn(dop.user_ptr, x.data_ptr(), y.data_ptr(), x.numel(), tree.stream())
    torch.cuda.synchronize(dev)
    if rc != L.OK:
        raise RuntimeError(f"{what} failed with status {rc}")
    return y


class _DevicePointer:
    """n doubles at a device address as the CUDA array interface describes them: torch wraps them without a copy."""

    def __init__(self, ptr: int, n: int):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": "<f8", "data": (ptr, False), "version": 2, "strides": None}


def _wrap_device_callable(f, device) -> _Operator:
    """A callable on torch tensors as a bbfmm_apply_device_fn.  The tensors it is handed WRAP the solver's device
    vectors (no copy); it runs with `stream` as torch's current stream, so its work is ordered with the solver's; its
    result is copied into the solver's output vector on that stream.  Exceptions are kept and re-raised by the solver
    call once the C driver has returned."""
    import torch
    err: List[BaseException] = []

    def tramp(_user, x, y, n, stream):
        try:
            with torch.cuda.device(device), torch.cuda.stream(torch.cuda.ExternalStream(stream, device=device)):
                xt = torch.as_tensor(_DevicePointer(x, n), device=device)
                yt = torch.as_tensor(_DevicePointer(y, n), device=device)
                out = f(xt)
                if not isinstance(out, torch.Tensor):
                    raise TypeError("a device operator returns a torch tensor")
                if out.numel() != n:
                    raise ValueError(f"operator returned {out.numel()} values for a vector of {n}")
                yt.copy_(out.reshape(-1))
            return L.OK
        except BaseException as e:  # noqa: BLE001 -- must not unwind through C
            err.append(e)
            return L.BAD_ARGUMENT

    cb = L.APPLY_DEVICE_FN(tramp)
    op = _Operator(ctypes.cast(cb, ctypes.c_void_p), None, (cb, err))
    op.errors = err
    return op


_SIDE_STREAMS = {}


def _solver_stream(device):
    """The stream of a solve without native operators: torch's current stream of the device, unless that is the null
    stream, which the drivers refuse (kernels of the library and torch's own on it were measured not to stay in order:
    DESIGN.md section 16); then one side stream per device, created once."""
    import torch
    cur = torch.cuda.current_stream(device)
    if cur.cuda_stream:
        return cur
    if device not in _SIDE_STREAMS:
        _SIDE_STREAMS[device] = torch.cuda.Stream(device)
    return _SIDE_STREAMS[device]


def _native_tree(f):
    if isinstance(f, RbfSystemOperator):
        return f.tree
    return getattr(f, "_tree", None) if isinstance(getattr(f, "_dop", None), _Operator) else None


def _run_device(entry_name, a, m, b, x0, args_tail, callback):
    """The device drivers: b / x0 numpy -> uploaded once, x downloaded once and returned as numpy; b a torch tensor on
    the device -> x comes back as a tensor there."""
    import torch
    lib = L.load()
    tree = _native_tree(a) or _native_tree(m)
    as_tensor = isinstance(b, torch.Tensor)
    if tree is not None:
        device = torch.device("cuda", tree.device())
    elif as_tensor:
        device = b.device
    else:
        device = torch.device("cuda", torch.cuda.current_device())
    if device.type != "cuda":
        raise ValueError('vectors="device" needs tensors on the device')

    def to_device(v):
        if v is None:
            return None
        if isinstance(v, torch.Tensor):
            if v.device != device:
                raise ValueError(f"the vectors must live on {device}, the operators' device")
            return v.to(torch.float64).contiguous().reshape(-1)
        return torch.from_numpy(np.ascontiguousarray(v, dtype=np.float64).reshape(-1)).to(device)

    bt, x0t = to_device(b), to_device(x0)
    n = bt.numel()
    if x0t is not None and x0t.numel() != n:
        raise ValueError("x0 must have the length of b")

    def as_op(f):
        if f is None:
            return None
        if _native_tree(f) is not None:
            return f._dop
        return _wrap_device_callable(f, device)

    ao, mo = as_op(a), as_op(m)
    # native operators work on their tree's stream; callables alone on torch's current stream of the device
    keep_stream = None if tree is not None else _solver_stream(device)
    stream = tree.stream() if tree is not None else int(keep_stream.cuda_stream)
    hist: List[Tuple[int, float]] = []

    def on_iter(_user, it, res, progress):
        hist.append((int(it), float(res)))
        if callback is not None:
            callback(int(it), float(res), float(progress))

    cb = L.ITERATION_FN(on_iter)
    xt = torch.empty(n, dtype=torch.float64, device=device)
    iters, res = ctypes.c_int64(0), ctypes.c_double(0.0)
    torch.cuda.synchronize(device)            # b, x0 are in place before the solver's stream reads them
    rc = getattr(lib, entry_name)(n, ao.fn_ptr, ao.user_ptr, bt.data_ptr(), None if mo is None else mo.fn_ptr,
                                  None if mo is None else mo.user_ptr, *args_tail(x0t), cb, None, xt.data_ptr(),
                                  ctypes.byref(iters), ctypes.byref(res), stream)
    torch.cuda.synchronize(device)
    for op in (ao, mo):
        if op is not None and getattr(op, "errors", None):
            e = op.errors[0]
            del op.errors[:]
            raise e
    if rc != L.OK:
        msg = lib.bbfmm_last_error(tree._h).decode() if tree is not None else ""
        raise RuntimeError(f"{entry_name} failed with status {rc}" + (f": {msg}" if msg else ""))
    return (xt if as_tensor else xt.cpu().numpy()), hist


def _as_operator(f) -> Optional[_Operator]:
    if f is None:
        return None
    if isinstance(f, RbfSystemOperator) or isinstance(getattr(f, "_op", None), _Operator):
        return f._op                      # natively bound operators (system matvec, Schwarz preconditioner)
    return _wrap_callable(f)


def _run(entry, n, a, m, args_mid, callback):
    hist: List[Tuple[int, float]] = []

    def on_iter(_user, it, res, progress):
        hist.append((int(it), float(res)))
        if callback is not None:
            callback(int(it), float(res), float(progress))

    cb = L.ITERATION_FN(on_iter)
    x = np.zeros(n)
    iters, res = ctypes.c_int64(0), ctypes.c_double(0.0)
    rc = entry(n, a.fn_ptr, a.user_ptr, *args_mid(m), cb, None, x.ctypes.data, ctypes.byref(iters),
               ctypes.byref(res))
    for op in (a, m):
        if op is not None and getattr(op, "errors", None):
            raise op.errors[0]
    if rc != L.OK:
        raise RuntimeError(f"solver failed with status {rc}")
    return x, hist


def fgmres(a, b, m=None, x0=None, max_outer_iterations: int = 20, max_inner_iterations: int = 5,
           tolerance: Optional[FittingAccuracy] = None, callback=None, vectors: str = "host"):
    """fgmres (iterative_solvers.rs:38-172).  a, m: callables on 1-D float64 arrays (or a
    RbfSystemOperator).  Returns (x, [(iteration, residual), ...]).
    vectors="device": every vector stays on the device (bbfmm_fgmres_device); a, m: RbfSystemOperator,
    ddm.SchwarzPreconditioner or callables on 1-D float64 torch tensors; b, x0: numpy arrays (x returned as numpy) or
    torch tensors on the device (x returned as a tensor there)."""
    tol = tolerance or FittingAccuracy()
    if vectors not in ("host", "device"):
        raise ValueError('vectors must be "host" or "device"')
    if vectors == "device":
        def tail(x0t):
            return (None if x0t is None else x0t.data_ptr(), int(max_outer_iterations), int(max_inner_iterations),
                    int(tol.tolerance_type), tol.tolerance)
        return _run_device("bbfmm_fgmres_device", a, m, b, x0, tail, callback)
    b = np.ascontiguousarray(b, dtype=np.float64).reshape(-1)
    x0a = None if x0 is None else np.ascontiguousarray(x0, dtype=np.float64).reshape(-1)
    ao, mo = _as_operator(a), _as_operator(m)
    lib = L.load()

    def mid(mo_):
        return (b.ctypes.data, None if mo_ is None else mo_.fn_ptr, None if mo_ is None else mo_.user_ptr,
                None if x0a is None else x0a.ctypes.data, int(max_outer_iterations), int(max_inner_iterations),
                int(tol.tolerance_type), tol.tolerance)

    return _run(lib.bbfmm_fgmres, b.size, ao, mo, mid, callback)


def schwarz_ddm_solver(matvec, rhs, m=None, max_iterations: int = 100,
                       tolerance: Optional[FittingAccuracy] = None, callback=None, vectors: str = "host"):
    """schwarz_ddm_solver (iterative_solvers.rs:229-281).  vectors="device": as in fgmres
    (bbfmm_schwarz_ddm_solver_device)."""
    tol = tolerance or FittingAccuracy()
    if vectors not in ("host", "device"):
        raise ValueError('vectors must be "host" or "device"')
    if vectors == "device":
        def tail(_x0t):
            return (int(max_iterations), int(tol.tolerance_type), tol.tolerance)
        return _run_device("bbfmm_schwarz_ddm_solver_device", matvec, m, rhs, None, tail, callback)
    rhs = np.ascontiguousarray(rhs, dtype=np.float64).reshape(-1)
    ao, mo = _as_operator(matvec), _as_operator(m)
    lib = L.load()

    def mid(mo_):
        return (rhs.ctypes.data, None if mo_ is None else mo_.fn_ptr, None if mo_ is None else mo_.user_ptr,
                int(max_iterations), int(tol.tolerance_type), tol.tolerance)

    return _run(lib.bbfmm_schwarz_ddm_solver, rhs.size, ao, mo, mid, callback)
