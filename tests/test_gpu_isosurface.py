"""Isosurface extraction on the RMT lattice on the device, against the numpy restatement of the contract
(tests/isosurface_restatement.py; DESIGN.md "Isosurfaces on the RMT lattice")."""
import os

import numpy as np
import pytest

from conftest import ROOT
import isosurface_restatement as R
from oracle import bbfmm_oracle as O

pytestmark = pytest.mark.gpu


def _same_mesh(got, want, extents):
    (v, f), (vr, fr) = got, want
    scale = float(np.abs(np.asarray(extents)).max())
    assert f.dtype == np.int64 and v.dtype == np.float64
    assert np.array_equal(f, fr)
    assert v.shape == vr.shape
    assert float(np.abs(v - vr).max(initial=0.0)) <= 1e-12 * scale


def _analytic(name, w):
    if name == "sphere":
        return np.linalg.norm(w - [3.0, 3.0, 3.0], axis=-1) - 2.0
    if name == "torus":
        return np.hypot(np.hypot(w[..., 0] - 3.0, w[..., 1] - 3.0) - 1.8, w[..., 2] - 3.0) - 0.7
    a = np.linalg.norm(w - [1.7, 3.0, 3.0], axis=-1) - 1.1
    b = np.linalg.norm(w - [4.4, 3.0, 3.1], axis=-1) - 1.0
    return np.minimum(a, b)


EULER = {"sphere": 2, "torus": 0, "two_spheres": 4}
EXT = [0.0, 0.0, 0.0, 6.0, 6.0, 6.0]


@pytest.mark.parametrize("name", ["sphere", "torus", "two_spheres"])
def test_caller_field_equals_the_restatement(name):
    import ferreus_rbf_rs_amd as F
    r = 0.08
    lat = R.Lattice(EXT, r)
    field = _analytic(name, lat.world(lat.node_ijk()))
    field[~lat.inE] = 12345.0                     # ignored off E
    v, f = F.isosurface_from_values(field, EXT, r, 0.0)
    _same_mesh((v, f), R.extract(lat, field, 0.0), EXT)
    assert len(f) > 1000
    assert R.directed_edges_once(f)
    assert R.euler_characteristic(v, f) == EULER[name]
    assert len(np.unique(f)) == len(v)             # every vertex is used (closed surfaces inside the domain)
    vol = R.enclosed_volume(v, f)                  # > 0: normals point towards positive g
    if name == "sphere":
        assert abs(vol - 4.0 / 3.0 * np.pi * 8.0) < 0.01 * 4.0 / 3.0 * np.pi * 8.0, vol
    assert vol > 0


def test_nan_patches_skip_their_tetrahedra_as_the_restatement_does():
    import ferreus_rbf_rs_amd as F
    r = 0.1
    lat = R.Lattice(EXT, r)
    field = _analytic("sphere", lat.world(lat.node_ijk()))
    nk, nj, ni = lat.shape
    field[nk // 2 - 3:nk // 2 + 2, :nj // 2, :] = np.nan
    field[:, nj // 3, ni // 2 + 4] = np.inf
    want = R.extract(lat, field, 0.0)
    got = F.isosurface_from_values(field, EXT, r, 0.0)
    _same_mesh(got, want, EXT)
    assert not R.directed_edges_once(got[1])       # the holes are there
    # several isovalues and a tiny batch budget give the same meshes, bit for bit
    many = F.isosurfaces_from_values(field, EXT, r, [0.0, -0.5, 0.3], batch_bytes=1)
    for iso, m in zip([0.0, -0.5, 0.3], many):
        one = F.isosurface_from_values(field, EXT, r, iso)
        assert np.array_equal(m[0], one[0]) and np.array_equal(m[1], one[1])
    _same_mesh(many[1], R.extract(lat, field, -0.5), EXT)


# ---- the FMM field: a small RBF fit
KID, BR, SILL = O.KERNEL_IDS["Spheroidal3Rbf"], 3.0, 1.0


@pytest.fixture(scope="module")
def fit():
    rng = np.random.default_rng(5)
    n = 2000
    pts = rng.uniform(0.5, 5.5, (n, 3))
    vals = np.linalg.norm(pts - [3.0, 3.0, 3.0], axis=1) - 1.8
    A = O.kernel_matrix(KID, BR, SILL, pts, pts)
    coef = np.linalg.solve(A + 1e-8 * np.eye(n), vals)[:, None]
    return pts, coef


def _tree(pts, coef, r, **kw):
    import ferreus_rbf_rs_amd as F
    pad = 10.0 * r                                  # the reference's evaluator padding (rbf.rs:992-998)
    ext = list(pts.min(0) - pad) + list(pts.max(0) + pad)
    t = F.FmmTree(pts, 7, F.KernelParams(F.KernelType(KID), base_range=BR, total_sill=SILL), True, False,
                  extents=ext, **kw)
    t.set_weights(coef)
    t.set_local_coefficients(coef)
    return t


def test_fmm_field_mesh_and_vertices(fit):
    pts, coef = fit
    r = 0.12
    ext = list(pts.min(0)) + list(pts.max(0))
    t = _tree(pts, coef, r)
    v, f, field = t.build_isosurface(ext, r, 0.0, return_field=True)
    lat = R.Lattice(ext, r)
    assert field.shape == lat.shape
    assert np.array_equal(np.isnan(field), ~lat.inE)
    nodes = lat.e_nodes()
    want = t.evaluate_leaves(None, lat.world(nodes))[:, 0]
    got = field[tuple((nodes - lat.lo)[:, ::-1].T)]
    assert float(np.abs(got - want).max() / np.abs(want).max()) <= 1e-12
    _same_mesh((v, f), R.extract(lat, field, 0.0), ext)
    assert len(f) > 1000 and R.directed_edges_once(f) and R.euler_characteristic(v, f) == 2
    # the interpolant at the vertices: within the linear-interpolation error of the lattice spacing
    fv = t.evaluate_leaves(None, v)[:, 0]
    assert float(np.abs(fv).max()) < 0.25 * r, float(np.abs(fv).max())
    # an affine drift is added on the device
    drift = (0.25, np.array([0.01, -0.02, 0.03]))
    _, _, field_d = t.build_isosurface(ext, r, 0.0, drift=drift, return_field=True)
    w = lat.world(nodes)
    dd = drift[0] + w @ drift[1]
    got_d = field_d[tuple((nodes - lat.lo)[:, ::-1].T)]
    assert float(np.abs(got_d - (got + dd)).max()) <= 1e-12 * float(np.abs(got + dd).max())


def test_outside_the_tree_is_refused_before_any_work(fit):
    import ferreus_rbf_rs_amd as F
    pts, coef = fit
    t = _tree(pts, coef, 0.5)
    with pytest.raises(F.PointOutsideTree):
        t.build_isosurface([-50.0, 0.0, 0.0, 6.0, 6.0, 6.0], 0.5, 0.0)
    t.build_isosurface(list(pts.min(0)) + list(pts.max(0)), 0.5, 0.0)    # the handle still works


def test_invariances_bitwise(fit):
    pts, coef = fit
    r = 0.15
    ext = list(pts.min(0)) + list(pts.max(0))
    isos = [0.0, -0.6, 0.4]
    t = _tree(pts, coef, r, deterministic=True)
    many = t.build_isosurfaces(ext, r, isos)
    for iso, m in zip(isos, many):
        one = t.build_isosurface(ext, r, iso)
        assert np.array_equal(m[0], one[0]) and np.array_equal(m[1], one[1])
    tiny = t.build_isosurfaces(ext, r, isos, batch_bytes=1)
    again = t.build_isosurfaces(ext, r, isos)
    t2 = _tree(pts, coef, r, deterministic=True)
    other = t2.build_isosurfaces(ext, r, isos)
    g = _tree(pts, coef, r, deterministic=True, devices=[0, 0])
    assert g.device_count() == 2
    grp = g.build_isosurfaces(ext, r, isos)
    for ms in (tiny, again, other, grp):
        for a, b in zip(many, ms):
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.mark.timeout(1800)
def test_albatite_spheroidal_example_at_resolution_5():
    """examples/isosurface_spheroidal.rs: Spheroidal order 3, range 50, sill 10, fitted on the device as
    test_albatite.py fits it, meshed at resolution 5 over the data's extents at isovalue 0."""
    import ferreus_rbf_rs_amd as F
    from ferreus_rbf_rs_amd import solvers as S
    from ferreus_rbf_rs_amd.ddm import DDMParams, InterpolantSettings, SchwarzPreconditioner
    z = np.load(os.path.join(ROOT, "tests", "golden", "albatite_SD_points.npz"))
    rows = z["rows"]
    pts, vals = np.ascontiguousarray(rows[:, :3]), rows[:, 3].copy()
    kid, br, sill = O.KERNEL_IDS["Spheroidal3Rbf"], 50.0, 10.0
    kp = F.KernelParams(F.KernelType(kid), base_range=br, total_sill=sill)
    tree = F.FmmTree(pts, 7, kp, True, True)
    st = InterpolantSettings(kid, 3, None, 0.0, br, sill)
    pre = SchwarzPreconditioner(tree, pts, st, DDMParams())
    op = S.RbfSystemOperator(tree, 0, pre.monomial_matrix, 0.0)
    x, hist = S.fgmres(op, vals.copy(), pre, None, 20, 5, S.FittingAccuracy(0.01, S.FittingAccuracyType.Absolute))
    assert float(hist[-1][1]) < 0.01
    res = 5.0
    ext = np.concatenate([pts.min(0), pts.max(0)])
    eext = list(ext[:3] - 10 * res) + list(ext[3:] + 10 * res)
    te = F.FmmTree(pts, 7, kp, True, False, extents=eext)
    coef = x[:, None].copy()
    te.set_weights(coef)
    te.set_local_coefficients(coef)
    # (not a deterministic tree: a mesh is checked against the restatement run on the field of the same call)
    v, f, field = te.build_isosurface(ext, res, 0.0, return_field=True)
    lat = R.Lattice(ext, res)
    _same_mesh((v, f), R.extract(lat, field, 0.0), ext)
    assert len(f) > 10000
