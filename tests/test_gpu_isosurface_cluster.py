"""Clustered isosurface extraction (cluster="average") on the device, against the numpy restatement of its contract
(tests/isosurface_cluster_restatement.py; DESIGN.md "Isosurfaces on the RMT lattice", vertex clustering).

Throughout: facets array_equal to the restatement's, vertices within 1e-12 * max|extents| (they are expected to be
bit-equal), and the returned counts equal to the restatement's."""
import numpy as np
import pytest

import isosurface_restatement as R
import isosurface_cluster_restatement as C
from test_gpu_isosurface import BR, EULER, EXT, KID, SILL, _analytic, _same_mesh, _tree, fit  # noqa: F401  (fit: a fixture)

pytestmark = pytest.mark.gpu


def _same_as_restatement(got, lat, field, iso, extents):
    v, f, stats = got
    want = C.extract(lat, field, iso)
    print("device", len(v), len(f), stats)
    print("restatement", len(want["vertices"]), len(want["facets"]), want["stats"])
    _same_mesh((v, f), (want["vertices"], want["facets"]), extents)
    assert stats == want["stats"]
    return want


def _noisy_sphere(amp, seed, r):
    lat = R.Lattice(EXT, r)
    field = _analytic("sphere", lat.world(lat.node_ijk())) + amp * np.random.default_rng(seed).standard_normal(lat.shape)
    return lat, field


@pytest.mark.parametrize("name", ["sphere", "torus", "two_spheres"])
def test_caller_field_equals_the_restatement(name):
    import ferreus_rbf_rs_amd as F
    r = 0.08
    lat = R.Lattice(EXT, r)
    field = _analytic(name, lat.world(lat.node_ijk()))
    field[~lat.inE] = 12345.0                     # ignored off E
    v, f, stats = F.isosurface_from_values(field, EXT, r, 0.0, cluster="average", return_stats=True)
    _same_as_restatement((v, f, stats), lat, field, 0.0, EXT)
    vr, fr = F.isosurface_from_values(field, EXT, r, 0.0, cluster="none")
    assert R.directed_edges_once(f)
    assert R.euler_characteristic(v, f) == EULER[name] == R.euler_characteristic(vr, fr)
    assert R.enclosed_volume(v, f) > 0
    assert 0 < len(v) < len(vr) and 0 < len(f) < len(fr)
    # fewer slivers than the raw mesh of the same field: the share of triangles whose smallest angle is below the raw
    # mesh's 10th percentile
    raw, clustered = C.min_angles(vr, fr), C.min_angles(v, f)
    q = np.percentile(raw, 10)
    print("share below the raw 10th percentile", float(np.degrees(q)), (raw < q).mean(), (clustered < q).mean())
    assert (clustered < q).mean() < (raw < q).mean()


def test_every_topology_case_and_pass_a():
    """The sphere with 0.05 * standard_normal noise per node at resolution 0.1: all five cases and pass A occur."""
    import ferreus_rbf_rs_amd as F
    lat, field = _noisy_sphere(0.05, 1, 0.1)
    got = F.isosurface_from_values(field, EXT, 0.1, 0.0, cluster="average", return_stats=True)
    _same_as_restatement(got, lat, field, 0.0, EXT)
    stats = got[2]
    for name in ("closed", "multi_hole", "flat_hole", "multi_surface", "simple"):
        assert stats[name] > 0, name
    assert stats["over_used_a"] > 0 and stats["split_a"] > 0


def test_pass_b_rolls_sample_points_back():
    """The same sphere with 0.15 * standard_normal noise: mesh edges with more than 2 faces survive pass A, pass B rolls
    their sample points back, and none is left."""
    import ferreus_rbf_rs_amd as F
    lat, field = _noisy_sphere(0.15, 1, 0.1)
    got = F.isosurface_from_values(field, EXT, 0.1, 0.0, cluster="average", return_stats=True)
    _same_as_restatement(got, lat, field, 0.0, EXT)
    v, f, stats = got
    assert stats["split_a"] > 0
    assert sum(stats["rolled_b"]) > 0 and stats["over_used_b"][0] > 0
    assert len(C.over_used(f)[0]) == 0


def test_open_surface_leaves_the_shell_of_the_domain_unclustered():
    """A sphere that leaves the extents: the sample points on the outer shell of E miss neighbours (incomplete) and keep
    one vertex per edge, as the restatement does."""
    import ferreus_rbf_rs_amd as F
    r = 0.15
    lat = R.Lattice(EXT, r)
    field = np.linalg.norm(lat.world(lat.node_ijk()) - [3.0, 3.0, 3.0], axis=-1) - 3.6
    got = F.isosurface_from_values(field, EXT, r, 0.0, cluster="average", return_stats=True)
    _same_as_restatement(got, lat, field, 0.0, EXT)
    assert got[2]["incomplete"] > 0 and got[2]["simple"] > 0
    assert not R.directed_edges_once(got[1])


def test_nan_patches_and_several_isovalues():
    import ferreus_rbf_rs_amd as F
    r = 0.1
    lat = R.Lattice(EXT, r)
    field = _analytic("sphere", lat.world(lat.node_ijk()))
    nk, nj, ni = lat.shape
    field[nk // 2 - 3:nk // 2 + 2, :nj // 2, :] = np.nan
    field[:, nj // 3, ni // 2 + 4] = np.inf
    got = F.isosurface_from_values(field, EXT, r, 0.0, cluster="average", return_stats=True)
    _same_as_restatement(got, lat, field, 0.0, EXT)
    assert not R.directed_edges_once(got[1])       # the holes are there
    isos = [0.0, -0.5, 0.3]
    many = F.isosurfaces_from_values(field, EXT, r, isos, batch_bytes=1, cluster="average", return_stats=True)
    for iso, m in zip(isos, many):
        one = F.isosurface_from_values(field, EXT, r, iso, cluster="average", return_stats=True)
        assert np.array_equal(m[0], one[0]) and np.array_equal(m[1], one[1]) and m[2] == one[2]
    _same_as_restatement(many[1], lat, field, -0.5, EXT)


def test_cluster_none_is_the_mesh_without_the_keyword():
    import ferreus_rbf_rs_amd as F
    lat, field = _noisy_sphere(0.05, 1, 0.1)
    plain = F.isosurface_from_values(field, EXT, 0.1, 0.0)
    none = F.isosurface_from_values(field, EXT, 0.1, 0.0, cluster="none", return_stats=True)
    assert np.array_equal(plain[0], none[0]) and np.array_equal(plain[1], none[1])
    assert C.stats_vector(none[2]).sum() == 0
    _same_mesh(plain, R.extract(lat, field, 0.0), EXT)


def test_fmm_field_equals_the_restatement(fit):
    pts, coef = fit
    r = 0.12
    ext = list(pts.min(0)) + list(pts.max(0))
    t = _tree(pts, coef, r)
    v, f, stats, field = t.build_isosurface(ext, r, 0.0, cluster="average", return_stats=True, return_field=True)
    lat = R.Lattice(ext, r)
    assert field.shape == lat.shape
    _same_as_restatement((v, f, stats), lat, field, 0.0, ext)
    assert len(f) > 1000 and R.directed_edges_once(f) and R.euler_characteristic(v, f) == 2
    vr, fr = t.build_isosurface(ext, r, 0.0)
    assert len(v) < len(vr) and len(f) < len(fr)
    _same_mesh((vr, fr), R.extract(lat, field, 0.0), ext)


def test_a_lattice_that_does_not_fit_is_refused_before_any_work(fit):
    """40 bytes per node of a 3e10-node box is over a terabyte: refused with a message, and the handle still works."""
    import ferreus_rbf_rs_amd as F
    pts, coef = fit
    big = [0.0, 0.0, 0.0, 100.0, 100.0, 100.0]
    t = F.FmmTree(pts, 7, F.KernelParams(F.KernelType(KID), base_range=BR, total_sill=SILL), True, False,
                  extents=[-10.0, -10.0, -10.0, 110.0, 110.0, 110.0])
    t.set_weights(coef)
    t.set_local_coefficients(coef)
    with pytest.raises(F.FmmError, match="cluster=average keeps 40 bytes per node"):
        t.build_isosurface(big, 0.05, 0.0, cluster="average")
    v, f = t.build_isosurface(list(pts.min(0)) + list(pts.max(0)), 0.5, 0.0, cluster="average")
    assert len(f) > 0


def test_invariances_bitwise(fit):
    pts, coef = fit
    r = 0.15
    ext = list(pts.min(0)) + list(pts.max(0))
    isos = [0.0, -0.6, 0.4]
    kw = dict(cluster="average", return_stats=True)
    t = _tree(pts, coef, r, deterministic=True)
    many = t.build_isosurfaces(ext, r, isos, **kw)
    for iso, m in zip(isos, many):
        one = t.build_isosurface(ext, r, iso, **kw)
        assert np.array_equal(m[0], one[0]) and np.array_equal(m[1], one[1]) and m[2] == one[2]
    tiny = t.build_isosurfaces(ext, r, isos, batch_bytes=1, **kw)
    again = t.build_isosurfaces(ext, r, isos, **kw)
    t2 = _tree(pts, coef, r, deterministic=True)
    other = t2.build_isosurfaces(ext, r, isos, **kw)
    g = _tree(pts, coef, r, deterministic=True, devices=[0, 0])
    assert g.device_count() == 2
    grp = g.build_isosurfaces(ext, r, isos, **kw)
    for ms in (tiny, again, other, grp):
        for a, b in zip(many, ms):
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]
    assert len(many[0][1]) > 500
    # and "none" on the same handle is the mesh without the keyword
    plain, none = t.build_isosurfaces(ext, r, isos), t.build_isosurfaces(ext, r, isos, cluster="none")
    for a, b in zip(plain, none):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
