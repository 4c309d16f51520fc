"""The device-resident solvers' C ABI, as far as it answers without a GPU: the entries are declared, exported and bound,
bad arguments come back as BBFMM_BAD_ARGUMENT before anything touches a device, and a host-only handle is refused
with a message."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from ferreus_rbf_rs_amd import _lib as L

NEW = ["bbfmm_fgmres_device", "bbfmm_schwarz_ddm_solver_device", "bbfmm_rbf_system_device_create",
       "bbfmm_rbf_system_device_destroy", "bbfmm_rbf_system_apply_device", "bbfmm_schwarz_apply_device",
       "bbfmm_debug_solver_vector_op"]


def test_new_entries_are_declared_exported_and_bound():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ferreus_bbfmm_hip.h")).read(), flags=re.S)
    lib = ctypes.CDLL(L.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, text), f"{name} is not declared in the header"
        assert name in L.SIGNATURES and hasattr(lib, name), name
    assert "bbfmm_apply_device_fn" in text
    L.load()


def test_header_cites_the_reference_lines_the_entries_replace():
    text = open(os.path.join(ROOT, "include", "ferreus_bbfmm_hip.h")).read()
    section = text[text.index("iterative solvers, vectors on the device"):]
    for cite in ("iterative_solvers.rs:38-281", "rbf.rs:105-117"):
        assert cite in section
    at = text.index("int bbfmm_schwarz_apply_device(")
    assert "schwarz.rs:32-82" in text[at - 1000:at]


@L.APPLY_DEVICE_FN
def _never(_user, _x, _y, _n, _stream):       # an operator the bad-argument cases must not reach
    raise AssertionError("the driver called the operator")


OPERATOR = ctypes.cast(_never, ctypes.c_void_p)
PTR = ctypes.c_void_p(0x1000)                 # stands for a device vector: never read, the checks come first
STREAM = ctypes.c_void_p(0x2000)              # stands for a created stream: never used, the checks come first
REL, ABS = L.ACCURACY_RELATIVE, L.ACCURACY_ABSOLUTE


def _fgmres(n=10, a=OPERATOR, b=PTR, x=PTR, outer=20, inner=5, ttype=REL, stream=STREAM):
    it, res = ctypes.c_int64(-1), ctypes.c_double(-1.0)
    return L.load().bbfmm_fgmres_device(n, a, None, b, None, None, None, outer, inner, ttype, 1e-6, None, None, x,
                                        ctypes.byref(it), ctypes.byref(res), stream)


def _schwarz(n=10, a=OPERATOR, b=PTR, x=PTR, iters=100, ttype=REL, stream=STREAM):
    it, res = ctypes.c_int64(-1), ctypes.c_double(-1.0)
    return L.load().bbfmm_schwarz_ddm_solver_device(n, a, None, b, OPERATOR, None, iters, ttype, 1e-6, None, None, x,
                                                    ctypes.byref(it), ctypes.byref(res), stream)


@pytest.mark.parametrize("kwargs", [dict(n=0), dict(n=-3), dict(a=None), dict(b=None), dict(x=None), dict(inner=0),
                                    dict(outer=-1), dict(ttype=2), dict(ttype=-1), dict(stream=None)])
def test_fgmres_device_bad_arguments(kwargs):
    assert _fgmres(**kwargs) == L.BAD_ARGUMENT


@pytest.mark.parametrize("kwargs", [dict(n=0), dict(a=None), dict(b=None), dict(x=None), dict(iters=-1), dict(ttype=7),
                                    dict(stream=None)])
def test_schwarz_ddm_solver_device_bad_arguments(kwargs):
    assert _schwarz(**kwargs) == L.BAD_ARGUMENT


def test_native_operators_without_their_object_are_bad_arguments():
    lib = L.load()
    native = ctypes.cast(lib.bbfmm_rbf_system_apply_device, ctypes.c_void_p)
    assert _fgmres(a=native) == L.BAD_ARGUMENT                       # user == NULL
    assert lib.bbfmm_rbf_system_apply_device(None, PTR, PTR, 10, None) == L.BAD_ARGUMENT
    assert lib.bbfmm_schwarz_apply_device(None, PTR, PTR, 10, None) == L.BAD_ARGUMENT


def test_vector_hook_bad_arguments():
    lib = L.load()
    a = np.ones(4)
    out, sc = np.zeros(4), np.zeros(2)
    call = lib.bbfmm_debug_solver_vector_op
    assert call(9, 0, 4, a.ctypes.data, a.ctypes.data, None, 1.0, 0, None, 0, out.ctypes.data, sc.ctypes.data) == L.BAD_ARGUMENT
    assert call(0, 0, 0, a.ctypes.data, a.ctypes.data, None, 1.0, 0, None, 0, out.ctypes.data, sc.ctypes.data) == L.BAD_ARGUMENT
    assert call(0, 0, 4, a.ctypes.data, None, None, 1.0, 0, None, 0, out.ctypes.data, sc.ctypes.data) == L.BAD_ARGUMENT
    assert call(1, 5, 4, a.ctypes.data, None, None, 1.0, 0, None, 0, out.ctypes.data, sc.ctypes.data) == L.BAD_ARGUMENT
    assert call(6, 3, 4, a.ctypes.data, a.ctypes.data, None, 1.0, 0, None, 0, out.ctypes.data, None) == L.BAD_ARGUMENT


def test_system_operator_on_a_host_only_handle_is_refused_with_a_message():
    import ferreus_rbf_rs_amd as F
    from ferreus_rbf_rs_amd import solvers as S
    pts = np.random.default_rng(0).random((500, 3))
    tree = F.FmmTree(pts, 5, F.KernelParams(F.FmmKernelType.LinearRbf), True, True, host_only=True)
    lib = L.load()
    h = ctypes.c_void_p()
    poly = np.asfortranarray(np.ones((500, 4)))
    rc = lib.bbfmm_rbf_system_device_create(tree._h, 4, poly.ctypes.data, 500, 0.1, ctypes.byref(h))
    assert rc == L.DEVICE_ERROR and not h.value
    message = lib.bbfmm_last_error(tree._h)
    assert message and b"HOST_ONLY" in message
    # bad arguments of the constructor itself
    assert lib.bbfmm_rbf_system_device_create(None, 0, None, 0, 0.0, ctypes.byref(h)) == L.BAD_ARGUMENT
    assert lib.bbfmm_rbf_system_device_create(tree._h, -1, None, 0, 0.0, ctypes.byref(h)) == L.BAD_ARGUMENT
    assert lib.bbfmm_rbf_system_device_create(tree._h, 0, None, 0, 0.0, None) == L.BAD_ARGUMENT
    # and through Python: the device solve raises with that message, the host entry's own refusal is as before
    op = S.RbfSystemOperator(tree, 4, poly, 0.1)
    with pytest.raises(RuntimeError, match="HOST_ONLY"):
        op._dop


def test_python_arguments():
    from ferreus_rbf_rs_amd import rbf, solvers as S
    with pytest.raises(ValueError):
        S.fgmres(lambda v: v, np.ones(3), vectors="gpu")
    with pytest.raises(ValueError):
        S.schwarz_ddm_solver(lambda v: v, np.ones(3), vectors="")
    assert rbf.Params(rbf.RBFKernelType.Linear).solver_vectors == "host"
    assert rbf.Params(rbf.RBFKernelType.Linear, solver_vectors="device").solver_vectors == "device"
    with pytest.raises(ValueError):
        rbf.Params(rbf.RBFKernelType.Linear, solver_vectors="pinned")
