"""rmt.build_isosurface of a Python callable (bbfmm_isosurfaces_from_function_opts): a numpy sphere against
isosurfaces_from_values of the same function on the restatement's node coordinates, which also pins the coordinates
handed to the callback; following the surface with an analytic gradient and with central differences; an interpolant's
evaluate_targets as the callable against the FieldExpr of the same model; exceptions, shapes and device memory."""
import gc

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import composite_cases as CC
import isosurface_restatement as R
import ferreus_rbf_rs_amd as F
from ferreus_rbf_rs_amd import rmt

EXT, RES, same_mesh = CC.EXT, CC.RES, CC.same_mesh
RAW = dict(cluster_method=rmt.ClusterMethod.None_, finish="raw", self_intersections="ignore")
C0, C1, C2, RAD = 3.1, 2.9, 3.05, 1.7


def sphere(x):
    d0, d1, d2 = x[:, 0] - C0, x[:, 1] - C1, x[:, 2] - C2           # (every value from its own row: the same in every batch)
    return np.sqrt(d0 * d0 + d1 * d1 + d2 * d2) - RAD


def sphere_with_gradient(x):
    d = x - [C0, C1, C2]
    r = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])
    return r - RAD, d / r[:, None]


def as_pair(mesh):
    return mesh.vertices, mesh.facets


@pytest.fixture(scope="module")
def dense_sphere():
    calls = []

    def fn(x):
        assert x.dtype == np.float64 and x.ndim == 2 and x.shape[1] == 3 and x.flags.c_contiguous
        calls.append(len(x))
        return sphere(x)

    mesh = rmt.build_isosurface(None, EXT, RES, 0.0, fn, follow="dense", **RAW)
    return mesh, calls


def test_dense_mesh_of_a_callable_is_the_mesh_of_its_values_on_the_lattice(dense_sphere):
    mesh, calls = dense_sphere
    lat = R.Lattice(EXT, RES)
    assert sum(calls) == int(lat.inE.sum())                          # every node of E once
    values = sphere(lat.world(lat.node_ijk().reshape(-1, 3))).reshape(lat.shape)
    assert len(mesh.facets) > 500 and same_mesh(as_pair(mesh), F.isosurface_from_values(values, EXT, RES, 0.0))
    assert R.directed_edges_once(mesh.facets) and R.euler_characteristic(mesh.vertices, mesh.facets) == 2
    column = rmt.build_isosurface(None, EXT, RES, 0.0, lambda x: sphere(x)[:, None], follow="dense", **RAW)     # (m, 1) is accepted
    assert same_mesh(as_pair(mesh), as_pair(column))


@pytest.mark.parametrize("gradient_fn", [sphere_with_gradient, None])
def test_following_a_callable_from_seeds_is_the_dense_mesh(dense_sphere, gradient_fn):
    rng = np.random.default_rng(3)
    u = rng.normal(size=(40, 3))
    seeds = [C0, C1, C2] + (RAD + 0.4) * u / np.linalg.norm(u, axis=1)[:, None]      # off the sphere: the projection moves them
    mesh = rmt.build_isosurface(seeds, EXT, RES, 0.0, sphere, gradient_fn=gradient_fn, follow="surface", return_stats=True, **RAW)
    st = mesh.stats["follow"]
    assert st["newton_steps"] >= 1 and 0 < st["nodes_evaluated"] < st["nodes"]
    assert same_mesh(as_pair(mesh), as_pair(dense_sphere[0]))


def test_evaluate_targets_as_the_callable_agrees_with_the_field_expression():
    fit = CC.model()[0]
    ext = np.asarray(EXT)
    pts = fit.source_points
    fit.build_evaluator(np.concatenate([np.minimum(pts.min(0), ext[:3]) - 10.0 * RES, np.maximum(pts.max(0), ext[3:]) + 10.0 * RES]))
    by_expr, field = rmt.build_isosurface(None, EXT, RES, 0.0, rmt.field(fit), follow="dense", return_field=True, **RAW)
    by_call = rmt.build_isosurface(None, EXT, RES, 0.0, fit.evaluate_targets, follow="dense", **RAW)
    assert len(by_expr.facets) > 500 and np.array_equal(by_expr.facets, by_call.facets)
    _, grad = fit.evaluate_targets_with_gradients(by_expr.vertices)
    gmin = float(np.linalg.norm(np.asarray(grad).reshape(len(by_expr.vertices), 3), axis=1).min())
    err, bound = float(np.abs(by_expr.vertices - by_call.vertices).max()), 1e-12 * float(np.nanmax(np.abs(field))) / gmin
    CC.record("callable_against_field_expression_max_vertex_difference", err, bound)
    assert err <= bound
    # with the interpolant's own gradients the followed surface is the same set of facets
    followed = rmt.build_isosurface(pts, EXT, RES, 0.0, fit.evaluate_targets, gradient_fn=fit.evaluate_targets_with_gradients,
                                    follow="surface", **RAW)
    assert np.array_equal(followed.facets, by_call.facets)


def test_exception_in_the_callable_comes_out_and_leaves_nothing_behind():
    """The callable is the interpolant's own evaluate_targets, so its evaluator handle is in use inside the callback when
    the second call raises: the exception comes out, the same interpolant and the same callable give afterwards what they
    gave before, and no device memory stays behind."""
    import torch
    fit = CC.model()[0]
    ext = np.asarray(EXT)
    pts = fit.source_points
    fit.build_evaluator(np.concatenate([np.minimum(pts.min(0), ext[:3]) - 10.0 * RES, np.maximum(pts.max(0), ext[3:]) + 10.0 * RES]))
    small = dict(follow="dense", batch_bytes=1 << 20, **RAW)
    probe = np.random.default_rng(4).uniform(1.0, 5.0, (300, 3))

    def free_bytes():
        gc.collect()
        torch.cuda.synchronize()
        return torch.cuda.mem_get_info()[0]

    calls, fail_at = [], [0]

    class Boom(RuntimeError):
        pass

    def model_values(x):
        calls.append(len(x))
        values = fit.evaluate_targets(x)                             # the handle is used inside the callback
        if len(calls) == fail_at[0]:
            raise Boom("second call")
        return values

    values_before = fit.evaluate_targets(probe)
    first = rmt.build_isosurface(None, EXT, RES, 0.0, model_values, **small)
    assert len(first.facets) > 500 and len(calls) > 2                # several batches: the callable is called more than once
    before = free_bytes()
    del calls[:]
    fail_at[0] = 2
    with pytest.raises(Boom, match="second call"):
        rmt.build_isosurface(None, EXT, RES, 0.0, model_values, **small)
    assert len(calls) == 2
    fail_at[0] = 0
    assert np.array_equal(fit.evaluate_targets(probe).view(np.uint64), values_before.view(np.uint64))
    again = rmt.build_isosurface(None, EXT, RES, 0.0, model_values, **small)
    assert same_mesh(as_pair(first), as_pair(again))
    after = free_bytes()
    print("free device memory before and after:", before, after)
    assert after >= before


def test_callback_status_without_an_exception_is_callback_failed():
    import ctypes
    from ferreus_rbf_rs_amd import _lib as L
    from ferreus_rbf_rs_amd import isosurface as ISO
    lib, res = L.load(), ctypes.c_void_p()
    ext, iso = np.array(EXT), np.array([0.0])
    status_three = L.FIELD_FN(lambda x, m, ldx, v, user: 3)
    rc = lib.bbfmm_isosurfaces_from_function_opts(status_three, None, None, ext.ctypes.data, RES, iso.ctypes.data, 1, None, ctypes.byref(res))
    msg = lib.bbfmm_isosurface_error(res).decode()
    assert lib.bbfmm_isosurface_count(res) == 0
    lib.bbfmm_isosurface_destroy(res)
    assert rc == L.CALLBACK_FAILED and "callback returned 3" in msg
    with pytest.raises(rmt.CallbackFailed, match="callback returned 3"):
        ISO._raise(rc, msg)
    assert issubclass(rmt.CallbackFailed, F.FmmError)


@pytest.mark.parametrize("bad", [lambda x: sphere(x)[:-1], lambda x: np.zeros((len(x), 2)), lambda x: sphere(x).astype(complex),
                                 lambda x: None])
def test_wrong_shape_or_dtype_is_a_value_error(bad):
    with pytest.raises(ValueError):
        rmt.build_isosurface(None, EXT, RES, 0.0, bad, follow="dense", **RAW)


def test_wrong_gradient_shape_is_a_value_error():
    seeds = np.array([[C0 + RAD, C1, C2]])
    with pytest.raises(ValueError):
        rmt.build_isosurface(seeds, EXT, RES, 0.0, sphere, gradient_fn=lambda x: (sphere(x), np.zeros((len(x), 2))), follow="surface", **RAW)
    with pytest.raises(ValueError):
        rmt.build_isosurface(seeds, EXT, RES, 0.0, sphere, gradient_fn=lambda x: sphere(x), follow="surface", **RAW)
