"""The argument checks of the isosurface, field and evaluate entry points of the C ABI: the status and the exact text
of bbfmm_last_error / bbfmm_isosurface_error for every bad argument the entries refuse before any device work, through
_lib's ctypes signatures on host-only handles (no GPU)."""
import ctypes

import numpy as np
import pytest

from ferreus_rbf_rs_amd import _lib as L
from ferreus_rbf_rs_amd import fmm_tree as T

HOST_ONLY = "handle was created with BBFMM_FLAG_HOST_ONLY"
FOLLOW_SURFACE = 1
MAX_OPERANDS = 8          # kFieldMaxOperands (field_program.hpp)

EXTENTS = np.array([0.1, 0.1, 0.1, 0.9, 0.9, 0.9])
INVERTED = np.array([0.1, 0.9, 0.1, 0.9, 0.1, 0.9])
ISO = np.array([0.5])
NAN = float("nan")


@pytest.fixture(scope="module")
def lib():
    return L.load()


@pytest.fixture(scope="module")
def trees():
    """Host-only handles over 200 random points: d = 3 and d = 2."""
    rng = np.random.default_rng(5)
    kp = T.KernelParams(T.FmmKernelType.LinearRbf)
    return {d: T.FmmTree(rng.random((200, d)), 4, kp, True, True, host_only=True) for d in (3, 2)}


@pytest.fixture(scope="module")
def h3(trees):
    return trees[3]._h


@pytest.fixture(scope="module")
def h2(trees):
    return trees[2]._h


def ptr(a):
    return None if a is None else a.ctypes.data


def last_error(lib, h):
    return lib.bbfmm_last_error(h).decode()


def iso_options(**kw):
    o = L.IsosurfaceOptions()
    o.size = ctypes.sizeof(L.IsosurfaceOptions)
    for name, v in kw.items():
        setattr(o, name, v)
    return o


class Result:
    """The bbfmm_isosurface_result an entry publishes through *out; destroyed with the object."""

    def __init__(self, lib):
        self.lib = lib
        self.p = ctypes.c_void_p(0xdead)      # every entry with an `out` overwrites it, with NULL or a result

    def error(self):
        return self.lib.bbfmm_isosurface_error(self.p).decode()

    def __del__(self):
        if self.p and self.p.value != 0xdead:
            self.lib.bbfmm_isosurface_destroy(self.p)


# ---- bbfmm_build_isosurfaces_opts: the message is the handle's, *out is NULL
def build_opts(lib, h, *, extents=EXTENTS, isovalues=ISO, n_iso=None, drift=None, options=None, out=True):
    r = Result(lib)
    rc = lib.bbfmm_build_isosurfaces_opts(h, ptr(extents), 0.1, ptr(isovalues), len(isovalues) if n_iso is None else n_iso,
                                          ptr(drift), None, None if options is None else ctypes.byref(options),
                                          ctypes.byref(r.p) if out else None)
    if out:
        assert not r.p, "no result is published on a failure"
    return rc, last_error(lib, h)


SEEDS = np.zeros((3, 5))
BUILD_CASES = {
    "null out": (dict(out=False), L.BAD_ARGUMENT, "isosurface: out must not be null"),
    "options size": (dict(options=iso_options(size=4)), L.BAD_ARGUMENT,
                     "isosurface: options->size must be sizeof(bbfmm_isosurface_options)"),
    "cluster": (dict(options=iso_options(cluster_method=99)), L.BAD_ARGUMENT, "isosurface: unknown cluster method 99"),
    "finish": (dict(options=iso_options(finish=99)), L.BAD_ARGUMENT, "isosurface: unknown finish 99"),
    "self intersections": (dict(options=iso_options(self_intersections=99)), L.BAD_ARGUMENT,
                           "isosurface: unknown self-intersection handling 99"),
    "follow": (dict(options=iso_options(follow=7)), L.BAD_ARGUMENT, "isosurface: unknown follow mode 7"),
    "seeds ld": (dict(options=iso_options(follow=FOLLOW_SURFACE, seeds=SEEDS.ctypes.data, n_seeds=5, seeds_ld=3)), L.BAD_ARGUMENT,
                 "isosurface: seeds must hold n_seeds >= 0 points with seeds_ld >= n_seeds"),
    "isovalue": (dict(isovalues=np.array([0.5, NAN])), L.BAD_ARGUMENT, "isosurface: isovalues must be finite"),
    "no isovalues": (dict(n_iso=0), L.BAD_ARGUMENT, "isosurface: at least one isovalue is needed"),
    "drift": (dict(drift=np.array([0.0, 1.0, NAN, 0.0])), L.BAD_ARGUMENT, "isosurface: drift must be finite"),
    "host only": (dict(), L.DEVICE_ERROR, HOST_ONLY),
    "host only with options": (dict(options=iso_options(cluster_method=1, finish=1)), L.DEVICE_ERROR, HOST_ONLY),
}


@pytest.mark.parametrize("case", sorted(BUILD_CASES))
def test_build_isosurfaces_opts(lib, h3, case):
    kw, rc, text = BUILD_CASES[case]
    assert build_opts(lib, h3, **kw) == (rc, text)


def test_build_isosurfaces_opts_needs_three_dimensions(lib, h2):
    assert build_opts(lib, h2) == (L.BAD_ARGUMENT, "isosurface: only supported for 3D (d = 3)")


def test_build_isosurfaces_opts_null_handle(lib):
    r = Result(lib)
    assert lib.bbfmm_build_isosurfaces_opts(None, ptr(EXTENTS), 0.1, ptr(ISO), 1, None, None, None, ctypes.byref(r.p)) == L.BAD_ARGUMENT
    assert last_error(lib, None) == "null handle"


# ---- the entries that own their result: the message is the result's and, with a handle, the handle's too
def from_values(lib, h, *, values, options=None):
    r = Result(lib)
    rc = lib.bbfmm_isosurfaces_from_values_opts(h, ptr(values), ptr(EXTENTS), 0.1, ptr(ISO), 1,
                                                None if options is None else ctypes.byref(options), ctypes.byref(r.p))
    assert r.p and lib.bbfmm_isosurface_count(r.p) == 0
    if h:
        assert last_error(lib, h) == r.error()
    return rc, r.error()


@pytest.mark.parametrize("with_handle", [False, True])
def test_isosurfaces_from_values_opts(lib, h3, with_handle):
    h = h3 if with_handle else None
    values = np.zeros(8)          # never read: the checks come first
    assert from_values(lib, h, values=None) == (L.BAD_ARGUMENT, "isosurface: values must not be null")
    assert from_values(lib, h, values=values, options=iso_options(follow=FOLLOW_SURFACE)) == (
        L.BAD_ARGUMENT, "isosurface: follow=surface of a caller's values needs seeds")
    if with_handle:
        assert from_values(lib, h, values=values) == (L.DEVICE_ERROR, HOST_ONLY)


def test_isosurfaces_from_values_opts_options_size(lib, h3):
    r = Result(lib)
    o = iso_options(size=4)
    assert lib.bbfmm_isosurfaces_from_values_opts(h3, ptr(np.zeros(8)), ptr(EXTENTS), 0.1, ptr(ISO), 1, ctypes.byref(o),
                                                  ctypes.byref(r.p)) == L.BAD_ARGUMENT
    assert not r.p and last_error(lib, h3) == "isosurface: options->size must be sizeof(bbfmm_isosurface_options)"


TRIANGLE = np.array([[0.2, 0.2, 0.2], [0.8, 0.2, 0.2], [0.2, 0.8, 0.2]])
FACET = np.array([[0, 1, 2]], dtype=np.int64)


def mesh_entry(lib, name, h, vertices, n_vertices, facets, extents):
    r = Result(lib)
    f = getattr(lib, name)
    if name == "bbfmm_isosurface_close_mesh":
        rc = f(h, ptr(vertices), n_vertices, ptr(facets), len(facets), ptr(extents), 0.1, 2, ctypes.byref(r.p))
    else:
        rc = f(h, ptr(vertices), n_vertices, ptr(facets), len(facets), ptr(extents), ctypes.byref(r.p))
    assert r.p and lib.bbfmm_isosurface_count(r.p) == 0
    if h:
        assert last_error(lib, h) == r.error()
    return rc, r.error()


MESH_ENTRIES = ["bbfmm_isosurface_finish_mesh", "bbfmm_isosurface_self_intersections", "bbfmm_isosurface_close_mesh"]


@pytest.mark.parametrize("with_handle", [False, True])
@pytest.mark.parametrize("name", MESH_ENTRIES)
def test_mesh_entries(lib, h3, name, with_handle):
    h = h3 if with_handle else None
    bad_facet = np.array([[0, 1, 5]], dtype=np.int64)
    assert mesh_entry(lib, name, h, TRIANGLE, 3, bad_facet, EXTENTS) == (L.BAD_ARGUMENT, "isosurface: facet 0 names vertex 5 of 3")
    assert mesh_entry(lib, name, h, None, 3, FACET, EXTENTS) == (L.BAD_ARGUMENT, "isosurface: vertices and facets must not be null")
    assert mesh_entry(lib, name, h, TRIANGLE, 3, FACET, INVERTED) == (L.BAD_ARGUMENT, "isosurface: inverted extents (max < min on axis 1)")
    if name != "bbfmm_isosurface_self_intersections":     # the detector's box is optional
        assert mesh_entry(lib, name, h, TRIANGLE, 3, FACET, None) == (L.BAD_ARGUMENT, "isosurface: extents must not be null")
    if with_handle:
        assert mesh_entry(lib, name, h, TRIANGLE, 3, FACET, EXTENTS) == (L.DEVICE_ERROR, HOST_ONLY)


def test_self_intersections_refuses_a_vertex_that_is_not_finite(lib, h3):
    v = TRIANGLE.copy()
    v[1, 2] = NAN
    for h in (None, h3):
        assert mesh_entry(lib, "bbfmm_isosurface_self_intersections", h, v, 3, FACET, None) == (
            L.BAD_ARGUMENT, "isosurface: vertex 1 is not finite")


# ---- composite fields
def operand(**kw):
    o = L.FieldOperand()
    o.size = ctypes.sizeof(L.FieldOperand)
    o.kind = L.FIELD_AFFINE
    o.scale = 1.0
    for name, v in kw.items():
        setattr(o, name, v)
    return o


def operand_cases(h3, h2):
    """name -> (operands, n_operands, text, the handle debug_evaluate_fields leaves the text in or None)"""
    at = "isosurface: operand 0: "
    one = lambda **kw: ((L.FieldOperand * 1)(operand(**kw)), 1)   # noqa: E731
    many = (L.FieldOperand * (MAX_OPERANDS + 1))(*[operand() for _ in range(MAX_OPERANDS + 1)])
    return {
        "no operands": (many, 0, "isosurface: 0 operands (1 .. 8)", None),
        "too many operands": (many, MAX_OPERANDS + 1, "isosurface: 9 operands (1 .. 8)", None),
        "size": (*one(size=8), at + "size must be sizeof(bbfmm_field_operand)", None),
        "kind": (*one(kind=9), at + "unknown kind 9", None),
        "scale": (*one(scale=float("inf")), at + "scale and offset must be finite", None),
        "affine with a handle": (*one(handle=h3.value), at + "an affine operand takes no handle and no terms", None),
        "model without a handle": (*one(kind=L.FIELD_MODEL), at + "a handle is needed", None),
        "model of a plane": (*one(kind=L.FIELD_MODEL, handle=h2.value), at + "a model operand needs a handle with d = 3, got d = 2", h2),
        "height axis": (*one(kind=L.FIELD_HEIGHT, handle=h2.value, axis=3), at + "axis must be 0, 1 or 2, got 3", h2),
        "host only": (*one(kind=L.FIELD_MODEL, handle=h3.value), at + HOST_ONLY, h3),
        "host only height": (*one(kind=L.FIELD_HEIGHT, handle=h2.value, axis=2), at + HOST_ONLY, h2),
    }


OPERAND_CASES = ["no operands", "too many operands", "size", "kind", "scale", "affine with a handle", "model without a handle",
                 "model of a plane", "height axis", "host only", "host only height"]
PROGRAM = np.array([0], dtype=np.int32)


def from_fields(lib, ops, n, options=None):
    r = Result(lib)
    rc = lib.bbfmm_isosurfaces_from_fields_opts(ops, n, ptr(PROGRAM), 1, ptr(EXTENTS), 0.1, ptr(ISO), 1, None,
                                                None if options is None else ctypes.byref(options), ctypes.byref(r.p))
    assert r.p and lib.bbfmm_isosurface_count(r.p) == 0
    return rc, r.error()


@pytest.mark.parametrize("case", OPERAND_CASES)
def test_isosurfaces_from_fields_opts_operands(lib, h3, h2, case):
    ops, n, text, _ = operand_cases(h3, h2)[case]
    assert from_fields(lib, ops, n) == (L.BAD_ARGUMENT, text)


def test_isosurfaces_from_fields_opts_takes_no_terms(lib, h3, h2):
    terms = L.InterpolantTerms()
    ops, n, _, _ = operand_cases(h3, h2)["kind"]      # the options are looked at first
    assert from_fields(lib, ops, n, iso_options(terms=ctypes.addressof(terms))) == (
        L.BAD_ARGUMENT, "isosurface: options->terms must be NULL here (terms belong to operands)")
    assert from_fields(lib, ops, n, iso_options(size=4)) == (
        L.BAD_ARGUMENT, "isosurface: options->size must be sizeof(bbfmm_isosurface_options)")
    assert lib.bbfmm_isosurfaces_from_fields_opts(ops, n, ptr(PROGRAM), 1, ptr(EXTENTS), 0.1, ptr(ISO), 1, None, None, None) == L.BAD_ARGUMENT


@pytest.mark.parametrize("case", OPERAND_CASES)
def test_debug_evaluate_fields_operands(lib, h3, h2, case):
    ops, n, text, h = operand_cases(h3, h2)[case]
    x, v = np.zeros((3, 4)), np.zeros(4)
    if h:      # the message goes to the first operand's handle, when the operands got that far
        assert build_opts(lib, h)[1] != text      # another message is left behind first
    assert lib.bbfmm_debug_evaluate_fields(ops, n, ptr(PROGRAM), 1, ptr(x), 4, 4, ptr(v), None, 0) == L.BAD_ARGUMENT
    if h:
        assert last_error(lib, h) == text


def test_isosurfaces_from_function_opts_null_callback(lib):
    r = Result(lib)
    assert lib.bbfmm_isosurfaces_from_function_opts(None, None, None, ptr(EXTENTS), 0.1, ptr(ISO), 1, None, ctypes.byref(r.p)) == L.BAD_ARGUMENT
    assert r.p and r.error() == "isosurface: the field callback must not be null"
    assert lib.bbfmm_isosurfaces_from_function_opts(None, None, None, ptr(EXTENTS), 0.1, ptr(ISO), 1, None, None) == L.BAD_ARGUMENT


# ---- bbfmm_evaluate_device, bbfmm_evaluate_grid
def eval_options(**kw):
    o = L.EvaluateOptions()
    o.size = ctypes.sizeof(L.EvaluateOptions)
    o.batch_independent = o.max_job_targets = -1
    for name, v in kw.items():
        setattr(o, name, v)
    return o


def grid(d):
    g = L.Grid()
    g.size = ctypes.sizeof(L.Grid)
    g.d = d
    for a in range(d):
        g.shape[a] = 3
        g.origin[a] = 0.2
        g.steps[4 * a] = 0.1
    return g


def evaluate_device(lib, h, *, gradients=0, terms=None, options=None):
    bad = ctypes.c_int64(-1)
    # (the device pointers are never followed: every case ends at a check)
    rc = lib.bbfmm_evaluate_device(h, gradients, 0x1000, 4, 4, None if terms is None else ctypes.byref(terms), 0x1000, 4, None, 4,
                                   None if options is None else ctypes.byref(options), ctypes.byref(bad))
    return rc, last_error(lib, h)


def evaluate_grid(lib, h, *, d=3, terms=None, options=None):
    bad = ctypes.c_int64(-1)
    g, out = grid(d), np.zeros(27)
    rc = lib.bbfmm_evaluate_grid(h, 0, ctypes.byref(g), None if terms is None else ctypes.byref(terms), ptr(out), 27, None, 0,
                                 None if options is None else ctypes.byref(options), ctypes.byref(bad))
    return rc, last_error(lib, h)


OPTIONS_SIZE = "evaluate: options->size must be sizeof(bbfmm_evaluate_options)"
OPTIONS_RANGE = "evaluate: batch_independent is -1, 0 or 1 and max_job_targets -1, 0 or a positive count"
BAD_TERMS = "bad terms (size, d, k, degree -1 .. 2, coefficients, scale != 0)"


@pytest.mark.parametrize("entry", [evaluate_device, evaluate_grid])
def test_evaluate_device_and_grid_options(lib, h3, entry):
    name = entry.__name__
    assert entry(lib, h3, options=eval_options(size=4)) == (L.BAD_ARGUMENT, OPTIONS_SIZE)
    assert entry(lib, h3, options=eval_options(batch_independent=2)) == (L.BAD_ARGUMENT, OPTIONS_RANGE)
    assert entry(lib, h3, options=eval_options(max_job_targets=-2)) == (L.BAD_ARGUMENT, OPTIONS_RANGE)
    assert entry(lib, h3, terms=L.InterpolantTerms()) == (L.BAD_ARGUMENT, f"{name}: {BAD_TERMS}")      # size = 0
    assert entry(lib, h3) == (L.DEVICE_ERROR, HOST_ONLY)
    assert entry(lib, h3, options=eval_options(batch_independent=1, max_job_targets=64)) == (L.DEVICE_ERROR, HOST_ONLY)


def test_evaluate_device_gradients_need_their_array(lib, h3):
    assert evaluate_device(lib, h3, gradients=1) == (L.BAD_ARGUMENT, "evaluate_device: gradients need their array")


def test_evaluate_grid_of_another_dimension(lib, h3, h2):
    text = "evaluate_grid: bad grid (size, d of the tree, shape >= 0, finite origin and steps)"
    assert evaluate_grid(lib, h3, d=2) == (L.BAD_ARGUMENT, text)
    assert evaluate_grid(lib, h2, d=3) == (L.BAD_ARGUMENT, text)
    assert evaluate_grid(lib, h2, d=2) == (L.DEVICE_ERROR, HOST_ONLY)


def test_evaluate_device_and_grid_null_handle(lib):
    assert lib.bbfmm_evaluate_device(None, 0, None, 0, 1, None, None, 1, None, 1, None, None) == L.BAD_ARGUMENT
    g = grid(3)
    assert lib.bbfmm_evaluate_grid(None, 0, ctypes.byref(g), None, None, 1, None, 1, None, None) == L.BAD_ARGUMENT


# ---- the getters of a result
GETTERS = {      # name -> the arguments after (result, i)
    "bbfmm_isosurface_stats": 1, "bbfmm_isosurface_finish_stats": 1, "bbfmm_isosurface_closure_stats": 1,
    "bbfmm_isosurface_follow_stats": 1, "bbfmm_isosurface_follow_times": 1, "bbfmm_isosurface_intersection_stats": 1,
    "bbfmm_isosurface_curvature_stats": 1, "bbfmm_isosurface_follow_bricks": 2, "bbfmm_isosurface_intersection_ids": 2,
    "bbfmm_isosurface_size": 2, "bbfmm_isosurface_copy": 2,
}


@pytest.mark.parametrize("name", sorted(GETTERS))
def test_result_getters_refuse_what_is_not_there(lib, name):
    r = Result(lib)
    assert lib.bbfmm_isosurfaces_from_values_opts(None, None, ptr(EXTENTS), 0.1, ptr(ISO), 1, None, ctypes.byref(r.p)) == L.BAD_ARGUMENT
    count = lib.bbfmm_isosurface_count(r.p)
    assert count == 0 and lib.bbfmm_isosurface_count(None) == -1
    out = [np.full(64, -7, dtype=np.int64) for _ in range(GETTERS[name])]
    f = getattr(lib, name)
    for res, i in ((None, 0), (r.p, -1), (r.p, count)):
        assert f(res, i, *[ptr(o) for o in out]) == L.BAD_ARGUMENT
        assert all((o == -7).all() for o in out)      # nothing was written
    assert lib.bbfmm_isosurface_error(None) == b"null result"
