"""Curvature-weighted clusters (cluster="curvature") on the device, against the numpy restatement of their contract
(tests/isosurface_curvature_restatement.py; DESIGN.md "Curvature-weighted clusters").

Facets, vertex counts and counts are compared exactly: the weights change positions only.  Vertices are compared within
a bar that comes from the restatement alone: G_v is the largest |v64 - v80| / r over the vertex coordinates between the
restatement in float64 and in long double, the bar 200 * max(G_v, 1e-15) * r per coordinate (the gap is about half an
ulp per operation, the device's trigonometric functions are a few ulp where the host's are one; 200 leaves some 50
times over that, and a wrong constant, branch or table row moves a vertex by 1e-6 * r or more).  The inputs must be
well conditioned: G_v <= 1e-13 and the same fallback edges in both precisions, or the test fails.

Measured on an MI355X (largest device gap in units of the bar): profiles/isosurface_curvature_accuracy.json."""
import functools

import numpy as np
import pytest

import isosurface_restatement as R
import isosurface_cluster_restatement as C
import isosurface_curvature_restatement as K
import isosurface_finish_restatement as FR
import isosurface_intersect_restatement as X
from test_gpu_isosurface import BR, EXT, KID, SILL, _tree, fit  # noqa: F401  (fit: a fixture)
from test_gpu_isosurface_cluster import _noisy_sphere
from test_isosurface_intersect_host import small_noisy_sphere

pytestmark = pytest.mark.gpu

CURV = dict(cluster="curvature", return_stats=True)
CLUSTER_KEYS = list(C.CASE_NAMES) + ["over_used_a", "split_a", "rolled_b", "over_used_b"]


def _conditions(lat, field, iso):
    """The restatement in both precisions with the conditions on the inputs asserted: (bar per coordinate, float64
    result)."""
    gv, gw, a, b = K.gaps(lat, field, iso)
    print("restatement: G_v", gv, "G_w", gw, a["curvature"])
    assert gv <= 1e-13
    assert np.array_equal(a["fallback"], b["fallback"])
    return K.bars(gv, gw, lat.resolution)[0], a


def _within(v, want, bar, what=""):
    assert v.dtype == np.float64 and v.shape == want.shape
    worst = float(np.abs(v - want).max(initial=0.0))
    print(what, "largest vertex gap", worst, "=", worst / bar, "bars")
    assert worst <= bar


def _same_as_restatement(got, want, bar, what=""):
    v, f, stats = got
    print("device", len(v), len(f), stats["curvature"])
    assert f.dtype == np.int64 and np.array_equal(f, want["facets"])
    _within(v, want["vertices"], bar, what)
    assert stats["curvature"] == want["curvature"]
    assert {k: stats[k] for k in CLUSTER_KEYS} == want["stats"]


def _positions_only(got, field, ext, r, iso=0.0):
    """The facets, the vertex count and the 16 clustering counts are the device's own with cluster="average"."""
    import ferreus_rbf_rs_amd as F
    va, fa, sa = F.isosurface_from_values(field, ext, r, iso, cluster="average", return_stats=True)
    assert np.array_equal(got[1], fa) and len(got[0]) == len(va)
    assert {k: got[2][k] for k in CLUSTER_KEYS} == sa and "curvature" not in sa
    return va


@functools.lru_cache(maxsize=None)
def analytic_case(name):
    lat = R.Lattice(K.EXT2, K.R2)
    field = K.analytic(name, lat.world(lat.node_ijk()))
    bar, want = _conditions(lat, field, 0.0)
    return lat, field, bar, want


@pytest.mark.parametrize("name", K.FIELDS)
def test_caller_field_equals_the_restatement(name):
    import ferreus_rbf_rs_amd as F
    lat, field, bar, want = analytic_case(name)
    field = field.copy()
    field[~lat.inE] = 12345.0                     # ignored off E
    got = F.isosurface_from_values(field, K.EXT2, K.R2, 0.0, **CURV)
    _same_as_restatement(got, want, bar, name)
    va = _positions_only(got, field, K.EXT2, K.R2)
    assert got[2]["curvature"]["edges"] > 500
    if name != "sphere":                          # (the closed sphere has its whole stencil nearly everywhere)
        assert got[2]["curvature"]["edge_fallbacks"] > 40
    if name != "plane":
        assert np.abs(got[0] - va).max() > 1e-3 * K.R2          # not the mean


@pytest.mark.parametrize("amp", [0.05, 0.15])
def test_every_topology_case_and_both_passes(amp):
    """The noisy spheres of the clustered tests: all five cases and pass A (0.05), pass B (0.15); the weights survive the
    re-marches."""
    import ferreus_rbf_rs_amd as F
    lat, field = _noisy_sphere(amp, 1, 0.1)
    bar, want = _conditions(lat, field, 0.0)
    got = F.isosurface_from_values(field, EXT, 0.1, 0.0, **CURV)
    _same_as_restatement(got, want, bar)
    _positions_only(got, field, EXT, 0.1)
    stats = got[2]
    assert stats["over_used_a"] > 0 and stats["split_a"] > 0
    if amp == 0.05:
        for name in ("closed", "multi_hole", "flat_hole", "multi_surface", "simple"):
            assert stats[name] > 0, name
    else:
        assert sum(stats["rolled_b"]) > 0


def test_nan_patches_and_two_isovalues():
    import ferreus_rbf_rs_amd as F
    lat, field, _, _ = analytic_case("sheet")
    field = field.copy()
    nk, nj, ni = lat.shape
    field[nk // 2 - 1:nk // 2 + 1, :nj // 2, :ni // 2] = np.nan
    field[:, nj // 3, ni // 2 + 3] = np.inf
    isos = [0.0, 0.07]
    many = F.isosurfaces_from_values(field, K.EXT2, K.R2, isos, batch_bytes=1, **CURV)
    for iso, m in zip(isos, many):
        one = F.isosurface_from_values(field, K.EXT2, K.R2, iso, **CURV)
        assert np.array_equal(m[0], one[0]) and np.array_equal(m[1], one[1]) and m[2] == one[2]
        bar, want = _conditions(lat, field, iso)
        _same_as_restatement(m, want, bar, f"isovalue {iso}")
    clean = analytic_case("sheet")[3]["curvature"]
    assert many[0][2]["curvature"]["edge_fallbacks"] > clean["edge_fallbacks"] - (clean["edges"] - many[0][2]["curvature"]["edges"])


def test_clipped_and_cleaned():
    import ferreus_rbf_rs_amd as F
    for name in ("sheet", "plane"):
        lat, field, bar, want = analytic_case(name)
        v, f, stats = F.isosurface_from_values(field, K.EXT2, K.R2, 0.0, finish="clipped", **CURV)
        wv, wf, wstats = FR.finish(want["vertices"], want["facets"], K.EXT2)
        assert np.array_equal(f, wf) and stats["finish"] == wstats
        _within(v, wv, bar + FR.bbox_eps(K.EXT2), name)
        assert stats["curvature"] == want["curvature"] and stats["finish"]["straddling"] > 0


def test_self_intersection_rollback():
    """The chain of the restatement: the two passes, the detector on the curvature-weighted vertices, one rollback.  The
    two precisions of the restatement must flag the same triangles.  They do not count the same pairs of overlapping
    boxes, though (227,682 against 231,640 on this field): a cluster of one edge is (w * p) * (1 / w), an ulp off p, and
    the boxes of triangles that meet in a lattice plane touch or miss each other by that ulp.  So the counts on which the
    two precisions agree are compared with the restatement's, and every count of the detector with the detector's
    restatement on the very vertices the device started from (its own mesh with "ignore")."""
    import ferreus_rbf_rs_amd as F
    lat, field, _ = small_noisy_sphere()
    bar, _ = _conditions(lat, field, 0.0)
    want = K.extract_rollback(lat, field, 0.0, EXT)
    far = K.extract_rollback(lat, field, 0.0, EXT, np.longdouble)
    assert np.array_equal(want["ids"], far["ids"]) and len(want["ids"]) > 0
    stable = [k for k in X.STAT_NAMES if want["self_intersections"][k] == far["self_intersections"][k]]
    print("restatement", want["self_intersections"], "long double", far["self_intersections"])
    assert {"true_pairs", "triangles", "cluster_vertices", "rolled_back"} <= set(stable)
    got = F.isosurface_from_values(field, EXT, 0.2, 0.0, self_intersections="rollback", **CURV)
    counts = got[2]["self_intersections"]
    print("device", counts)
    assert {k: counts[k] for k in stable} == {k: want["self_intersections"][k] for k in stable}
    _same_as_restatement(got, want, bar)
    assert counts["rolled_back"] > 0
    before = F.isosurface_from_values(field, EXT, 0.2, 0.0, **CURV)
    assert np.array_equal(before[1], want["before"][1])
    _within(before[0], want["before"][0], bar, "before the rollback")
    ids, detector, _ = X.detect(before[0], before[1], EXT)
    assert np.array_equal(ids, want["ids"]) and [counts[k] for k in X.STAT_NAMES[:5]] == detector


def test_fmm_field_and_following_the_surface(fit):
    import ferreus_rbf_rs_amd as F
    pts, coef = fit
    r = 0.15
    ext = list(pts.min(0)) + list(pts.max(0))
    t = _tree(pts, coef, r)
    v, f, stats, field = t.build_isosurface(ext, r, 0.0, return_field=True, **CURV)
    lat = R.Lattice(ext, r)
    assert field.shape == lat.shape
    bar, want = _conditions(lat, field, 0.0)
    _same_as_restatement((v, f, stats), want, bar, "tree")
    assert len(f) > 500 and R.directed_edges_once(f)
    # follow="surface" from the source points: the dense extraction of the field it evaluated, bit for bit, and the
    # whole component
    vs, fs, ss, field_s = t.build_isosurface(ext, r, 0.0, return_field=True, follow="surface", **CURV)
    dense = F.isosurface_from_values(field_s, ext, r, 0.0, **CURV)
    assert np.array_equal(vs, dense[0]) and np.array_equal(fs, dense[1]) and ss["curvature"] == dense[2]["curvature"]
    assert np.array_equal(fs, f) and ss["curvature"] == stats["curvature"]
    assert 0 < ss["follow"]["nodes_evaluated"] < ss["follow"]["nodes"]
    # a caller's values: the reached component is the dense one bit for bit
    lat2, sphere, _, _ = analytic_case("sphere")
    a = F.isosurface_from_values(sphere, K.EXT2, K.R2, 0.0, **CURV)
    b = F.isosurface_from_values(sphere, K.EXT2, K.R2, 0.0, follow="surface", seeds=[[1.0, 1.0, 1.8]], **CURV)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2]["curvature"] == b[2]["curvature"]


def test_invariances_bitwise(fit):
    pts, coef = fit
    r = 0.2
    ext = list(pts.min(0)) + list(pts.max(0))
    isos = [0.0, -0.6, 0.4]
    drift = [0.05, 0.01, -0.02, 0.015]
    kw = dict(drift=drift, **CURV)
    t = _tree(pts, coef, r, deterministic=True)
    many = t.build_isosurfaces(ext, r, isos, **kw)
    for iso, m in zip(isos, many):
        one = t.build_isosurface(ext, r, iso, **kw)
        assert np.array_equal(m[0], one[0]) and np.array_equal(m[1], one[1]) and m[2] == one[2]
    tiny = t.build_isosurfaces(ext, r, isos, batch_bytes=1, **kw)
    g = _tree(pts, coef, r, deterministic=True, devices=[0, 0])
    assert g.device_count() == 2
    grp = g.build_isosurfaces(ext, r, isos, **kw)
    for ms in (tiny, grp):
        for a, b in zip(many, ms):
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]
    assert len(many[0][1]) > 300 and many[0][2]["curvature"]["edges"] > many[0][2]["curvature"]["clusters"] > 0
    # the drift moves the surface
    plain = t.build_isosurface(ext, r, 0.0, **CURV)
    assert len(plain[1]) != len(many[0][1]) or not np.array_equal(plain[0], many[0][0])


def test_a_lattice_that_does_not_fit_is_refused_before_any_work(fit):
    """48 bytes per node of a 3e10-node box is over a terabyte: refused with the figure of this mode, and the handle still
    works."""
    import ferreus_rbf_rs_amd as F
    pts, coef = fit
    big = [0.0, 0.0, 0.0, 100.0, 100.0, 100.0]
    t = F.FmmTree(pts, 7, F.KernelParams(F.KernelType(KID), base_range=BR, total_sill=SILL), True, False,
                  extents=[-10.0, -10.0, -10.0, 110.0, 110.0, 110.0])
    t.set_weights(coef)
    t.set_local_coefficients(coef)
    with pytest.raises(F.FmmError, match="cluster=curvature keeps 48 bytes per node"):
        t.build_isosurface(big, 0.05, 0.0, cluster="curvature")
    v, f, st = t.build_isosurface(list(pts.min(0)) + list(pts.max(0)), 0.5, 0.0, **CURV)
    assert len(f) > 0 and st["curvature"]["clusters"] == len(v)


def test_unknown_method_is_refused():
    import ferreus_rbf_rs_amd as F
    lat, field, _, _ = analytic_case("sphere")
    with pytest.raises(ValueError, match="cluster must be one of"):
        F.isosurface_from_values(field, K.EXT2, K.R2, 0.0, cluster="curved")
