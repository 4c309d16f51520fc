"""The lattice field of the isosurfacer with an interpolant's terms (bbfmm_isosurface_options.terms): a polynomial of any
degree at the world nodes and a global trend's map of the points the tree is asked at -- the returned field against
evaluate_leaves at the numpy-transformed nodes plus the numpy polynomial, the extractor's own properties on that field
(dense mesh = isosurfaces_from_values of it, follow = dense), the 4-value drift unchanged, and
RBFInterpolator.build_isosurface against the same call assembled by hand."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import interpolant_cases as C
import interpolant_restatement as IR
import isosurface_restatement as R
import ferreus_rbf_rs_amd as F
from ferreus_rbf_rs_amd import rbf as RBF

K, D = RBF.RBFKernelType, RBF.Drift
EXT = [0.0, 0.0, 0.0, 6.0, 6.0, 6.0]
RES = 0.15                                            # about 40 lattice nodes along each axis


def sdf(p):
    return np.linalg.norm(p - [3.0, 3.0, 3.0], axis=1) - 1.8


def same_mesh(a, b):
    return a[0].shape == b[0].shape and np.array_equal(a[1], b[1]) and np.array_equal(a[0].view(np.uint64), b[0].view(np.uint64))


def evaluator(fit, extents, resolution):
    """the tree RBFInterpolator.build_isosurfaces makes (rbf.rs:990-1000), assembled by hand"""
    pts = fit.source_points
    ext = np.asarray(extents, dtype=np.float64)
    ev = np.concatenate([np.minimum(pts.min(0), ext[:3]) - 10.0 * resolution, np.maximum(pts.max(0), ext[3:]) + 10.0 * resolution])
    if fit.global_trend is not None:
        corners = np.array([[ev[j + 3] if (i >> j) & 1 else ev[j] for j in range(3)] for i in range(8)])
        ct = fit.global_trend.transform_points(corners, 0)
        ev = np.concatenate([ct.min(0), ct.max(0)])
    t = F.FmmTree(fit._tpoints, fit.params.fmm_params.interpolation_order, fit.settings.kernel_params(), True, False, extents=list(ev),
                  params=fit.params.fmm_params.to_tree(), deterministic=True)
    w = np.asfortranarray(fit.coefficients.point_coefficients[:, :1])
    t.set_weights(w)
    t.set_local_coefficients(w)
    return t


@pytest.fixture(scope="module")
def quadratic_trend_fit():
    """3,000 signed distances of a sphere, Linear kernel with a quadratic drift and the reference example's trend"""
    rng = np.random.default_rng(5)
    pts = rng.uniform(0.5, 5.5, (3000, 3))
    st = RBF.InterpolantSettings(K.Linear, drift=D.Quadratic)
    fit = RBF.RBFInterpolator(pts, sdf(pts), st, RBF.Params(K.Linear, deterministic=True), RBF.GlobalTrend.three(*C.TREND3))
    return fit, evaluator(fit, EXT, RES)


@pytest.mark.parametrize("isovalues", [[0.0], [0.0, -0.4]])
def test_lattice_field_with_quadratic_terms_and_a_trend(quadratic_trend_fit, isovalues):
    fit, tree = quadratic_trend_fit
    terms = fit.terms(1)
    assert terms.degree == 2 and terms.B is not None
    meshes, field = tree.build_isosurfaces(EXT, RES, isovalues, drift=terms, return_field=True)
    lat = R.Lattice(EXT, RES)
    assert field.shape == lat.shape and np.array_equal(np.isnan(field), ~lat.inE)
    nodes = lat.e_nodes()
    w = lat.world(nodes)
    kv = tree.evaluate_leaves(None, np.asfortranarray(w @ fit.global_trend.B + fit.global_trend.b))[:, 0]
    pv, _, va, _ = IR.polynomial(w, 2, fit.coefficients.poly_coefficients, fit.translation_factor, fit.scale_factor)
    got = field[tuple((nodes - lat.lo)[:, ::-1].T)]
    assert (np.abs(got - (kv + pv[:, 0])) <= 1e-13 * (np.abs(kv) + va[:, 0]) + 1e-12 * np.abs(kv).max()).all()
    inside = np.linalg.norm(w - 3.0, axis=1) < 2.4                       # within the data: it is the fitted function, a sphere's distance
    assert float(np.abs(got - sdf(w))[inside].max()) < 0.2
    again = F.isosurfaces_from_values(field, EXT, RES, isovalues)
    for m, a in zip(meshes, again):
        assert len(m[1]) > 1000 and same_mesh(m, a)                      # the extractor's property: the mesh of the returned field
    assert R.directed_edges_once(meshes[0][1]) and R.euler_characteristic(*meshes[0]) == 2
    # following the surface from the data points (world coordinates): the Newton step sees the polynomial's gradient and B^T.
    # As without terms ("Following the surface", contract 5): the same decisions at every node, values equal to the
    # standing figure of two batchings of one leaf pass, and the mesh is the mesh of the returned field.
    followed, ffield = tree.build_isosurfaces(EXT, RES, isovalues, drift=terms, follow="surface", seeds=fit.source_points,
                                              return_stats=True, return_field=True)
    known = np.isfinite(ffield)
    scale = float(np.nanmax(np.abs(field)))
    err = float(np.abs(ffield[known] - field[known]).max())
    print(f"follow against dense with terms: max field difference {err:.3g}, the bar 1e-12 max|f| = {1e-12 * scale:.3g}")
    assert known.any() and not known[~lat.inE].any() and err <= 1e-12 * scale
    for iso, m, fm in zip(isovalues, meshes, followed):
        assert not (np.abs(field[lat.inE] - iso + 1e-9) < 1e-12 * scale).any()      # the isovalue decides every node the same way
        assert np.array_equal(m[1], fm[1]) and m[0].shape == fm[0].shape
        assert 0 < fm[2]["follow"]["nodes_evaluated"] < fm[2]["follow"]["nodes"]
        assert fm[2]["follow"]["newton_steps"] >= 1
    if len(isovalues) == 1:
        assert same_mesh(followed[0][:2], F.isosurface_from_values(ffield, EXT, RES, isovalues[0]))
    with pytest.raises(F.FmmError):
        tree.build_isosurfaces(EXT, RES, isovalues, drift=terms, follow="surface")      # a trend needs world seeds
    with pytest.raises(F.PointOutsideTree):
        tree.build_isosurfaces([-40.0, 0.0, 0.0, 6.0, 6.0, 6.0], RES, isovalues, drift=terms)   # the transformed corners are tested


def test_follow_with_terms_is_the_dense_mesh_bit_for_bit(quadratic_trend_fit):
    """Contract 7, last clause: follow="surface" on a one-component surface that the seeds reach gives the dense mesh bit for
    bit.  The dense pass batches the lattice by k-planes and the wavefront by bricks, and the tree's default leaf pass sizes
    its near-field and M2P jobs to the number of targets a leaf has in the call, which leaves 3e-16 between two batchings
    (DESIGN.md "Batching"; without terms the followed mesh agrees with the dense one to that figure, contract 5 of
    "Following the surface").  The field with terms asks the tree with batch_independent set (a fixed split of every leaf's
    targets), so on a deterministic handle each node's value is the same double in both passes."""
    fit, tree = quadratic_trend_fit
    terms = fit.terms(1)
    (dense,) = tree.build_isosurfaces(EXT, RES, [0.0], drift=terms)
    (followed,) = tree.build_isosurfaces(EXT, RES, [0.0], drift=terms, follow="surface", seeds=fit.source_points)
    print("facets equal:", np.array_equal(dense[1], followed[1]), "largest vertex difference:",
          float(np.abs(dense[0] - followed[0]).max()) if dense[0].shape == followed[0].shape else "shapes differ")
    assert same_mesh(dense, followed)


def test_affine_drift_is_unchanged_and_agrees_with_linear_terms(quadratic_trend_fit):
    fit, tree = quadratic_trend_fit
    drift = [0.25, 0.01, -0.02, 0.03]
    (m1,), f1 = tree.build_isosurfaces(EXT, RES, [0.0], drift=drift, return_field=True)
    (m2,), f2 = tree.build_isosurfaces(EXT, RES, [0.0], drift=(0.25, [0.01, -0.02, 0.03]), return_field=True)
    assert same_mesh(m1, m2) and np.array_equal(np.nan_to_num(f1), np.nan_to_num(f2))
    assert same_mesh(m1, F.isosurface_from_values(f1, EXT, RES, 0.0))
    (_,), f0 = tree.build_isosurfaces(EXT, RES, [0.0], return_field=True)
    lat = R.Lattice(EXT, RES)
    nodes = lat.e_nodes()
    sel = tuple((nodes - lat.lo)[:, ::-1].T)
    w = lat.world(nodes)
    dd = drift[0] + w @ np.array(drift[1:])
    assert float(np.abs(f1[sel] - (f0[sel] + dd)).max()) <= 1e-12 * float(np.abs(f0[sel] + dd).max())
    # the same drift as Linear terms (translation 0, scale 1) and no trend
    terms = RBF.FieldTerms(3, 1, np.array(drift)[:, None])
    (_,), f3 = tree.build_isosurfaces(EXT, RES, [0.0], drift=terms, return_field=True)
    assert float(np.abs(f3[sel] - f1[sel]).max()) <= 1e-13 * float((np.abs(f0[sel]) + np.abs(drift[0]) + np.abs(w) @ np.abs(drift[1:])).max())
    with pytest.raises(ValueError):
        tree.build_isosurfaces(EXT, RES, [0.0], drift=[1.0, 2.0, 3.0])
    with pytest.raises(ValueError):
        tree.build_isosurfaces(EXT, RES, [0.0], drift=RBF.FieldTerms(2, 1, np.zeros((3, 1))))


def test_both_drift_and_terms_are_refused_by_the_abi(quadratic_trend_fit):
    import ctypes
    from ferreus_rbf_rs_amd import _lib as L
    fit, tree = quadratic_trend_fit
    terms = fit.terms(1)._c()
    opts = L.IsosurfaceOptions(ctypes.sizeof(L.IsosurfaceOptions))
    opts.terms = ctypes.addressof(terms)
    ext, iso, drift = np.array(EXT), np.array([0.0]), np.array([0.0, 0.0, 0.0, 0.0])
    res = ctypes.c_void_p()
    rc = tree._lib.bbfmm_build_isosurfaces_opts(tree._h, ext.ctypes.data, RES, iso.ctypes.data, 1, drift.ctypes.data, None,
                                                ctypes.addressof(opts), ctypes.byref(res))
    assert rc == L.BAD_ARGUMENT and not res
    opts.size = L.IsosurfaceOptions.terms.offset                     # an older caller's struct: the terms are not read
    rc = tree._lib.bbfmm_build_isosurfaces_opts(tree._h, ext.ctypes.data, RES, iso.ctypes.data, 1, drift.ctypes.data, None,
                                                ctypes.addressof(opts), ctypes.byref(res))
    assert rc == L.OK
    tree._lib.bbfmm_isosurface_destroy(res)


def test_build_isosurface_of_the_interpolator_equals_the_call_by_hand():
    """2,000 signed distances of a sphere and a second, larger one that leaves the extents (so the clip runs)"""
    rng = np.random.default_rng(8)
    pts = rng.uniform(0.5, 5.5, (2000, 3))
    events = []
    fit = RBF.RBFInterpolator(pts, sdf(pts), RBF.InterpolantSettings(K.Linear), RBF.Params(K.Linear, deterministic=True),
                              progress_callback=RBF.Progress(events.append))
    ext = [0.0, 0.0, 0.0, 6.0, 6.0, 6.0]
    for extents, iso in ((ext, 0.0), ([0.0, 0.0, 0.0, 6.0, 6.0, 3.4], 0.3)):
        mesh = fit.build_isosurface(np.array(extents), 0.2, iso)
        tree = evaluator(fit, extents, 0.2)
        v, f = tree.build_isosurface(extents, 0.2, iso, drift=fit.terms(1), cluster="curvature", follow="surface", seeds=fit.source_points,
                                     finish="clipped", self_intersections="rollback")
        assert isinstance(mesh, RBF.Mesh) and len(mesh.facets) > 300
        assert np.array_equal(mesh.facets, f)
        assert float(np.abs(mesh.vertices - v).max()) <= 200 * 1e-15 * 0.2          # the curvature mode's documented bar
        assert float(np.abs(np.linalg.norm(mesh.vertices - 3.0, axis=1) - (1.8 + iso)).max()) < 0.1
    assert float(mesh.vertices[:, 2].max()) <= 3.4 + 1e-9                           # clipped to the extents
    stages = [e.stage for e in events if isinstance(e, RBF.SurfacingProgress)]
    assert stages == ["started", "finished"] * 2
    dense = fit.build_isosurface(np.array(ext), 0.2, 0.0, follow="dense", cluster="none", finish="raw", self_intersections="ignore")
    assert len(dense.facets) > len(fit.build_isosurface(np.array(ext), 0.2, 0.0).facets)      # the keyword overrides reach the extractor
    flat = RBF.RBFInterpolator(pts[:, :2], sdf(pts), RBF.InterpolantSettings(K.ThinPlateSpline))
    with pytest.raises(ValueError):
        flat.build_isosurface([0, 0, 6, 6], 0.2, 0.0)
