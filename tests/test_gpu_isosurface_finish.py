"""Clip and clean of isosurface meshes on the device (finish="clipped") against the numpy restatement of the contract
(tests/isosurface_finish_restatement.py; DESIGN.md "Isosurfaces on the RMT lattice", clip and clean).

Throughout: facets array_equal to the restatement's, vertices within 1e-12 * max|extents| (they are expected to be
bit-equal), and the finish counts equal to the restatement's.  The lattice meshes used here satisfy the condition of
tests/test_isosurface_finish_host.py under which the contract's weld is the reference's greedy one."""
import ctypes

import numpy as np
import pytest

import isosurface_restatement as R
import isosurface_cluster_restatement as C
import isosurface_finish_restatement as FR
from test_gpu_isosurface import _same_mesh, _tree, fit  # noqa: F401  (fit: a fixture)

pytestmark = pytest.mark.gpu

EXT, RES = FR.EXT, FR.RES


def _raw_restatement(lat, field, iso, cluster):
    if cluster == "none":
        return R.extract(lat, field, iso)
    out = C.extract(lat, field, iso)
    return out["vertices"], out["facets"]


def _edges_with_one_face(f):
    e = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), 1)
    u, n = np.unique(e, axis=0, return_counts=True)
    return u[n == 1]


def _check_properties(v, f, ext):
    lo, hi = np.asarray(ext[:3]), np.asarray(ext[3:])
    assert (v >= lo).all() and (v <= hi).all()             # inside, and what was made on a plane is exactly on it
    assert len(np.unique(f)) == len(v) and f.min(initial=0) == 0 and f.max(initial=-1) == len(v) - 1
    assert len(np.unique(np.sort(f, 1), axis=0)) == len(f)
    assert (f[:, 0] != f[:, 1]).all() and (f[:, 1] != f[:, 2]).all() and (f[:, 0] != f[:, 2]).all()
    open_edges = _edges_with_one_face(f)
    on_face = np.concatenate([v == lo, v == hi], 1)        # (n, 6): the faces a vertex lies on
    assert on_face[open_edges[:, 0]].any(1).all() and on_face[open_edges[:, 1]].any(1).all()
    return open_edges


@pytest.mark.parametrize("cluster", ["none", "average"])
@pytest.mark.parametrize("name", FR.FIELDS)
def test_caller_field_equals_the_restatement(name, cluster):
    import ferreus_rbf_rs_amd as F
    lat, field = FR.lattice_field(name)
    v, f, stats = F.isosurface_from_values(field, EXT, RES, 0.0, cluster=cluster, finish="clipped", return_stats=True)
    wv, wf, wstats = FR.finish(*_raw_restatement(lat, field, 0.0, cluster), EXT)
    print("device", len(v), len(f), stats["finish"])
    print("restatement", len(wv), len(wf), wstats)
    _same_mesh((v, f), (wv, wf), EXT)
    assert stats["finish"] == wstats
    assert stats["finish"]["straddling"] > 0 and stats["finish"]["outside"] > 0 and stats["finish"]["weld_loose"] == 0
    open_edges = _check_properties(v, f, EXT)
    assert len(open_edges) > 0                            # the surface leaves the box: it ends on its faces
    raw = F.isosurface_from_values(field, EXT, RES, 0.0, cluster=cluster)
    assert len(f) < len(raw[1])
    lo, hi = np.asarray(EXT[:3]), np.asarray(EXT[3:])
    assert (raw[0] < lo).any() or (raw[0] > hi).any()      # the raw mesh runs past the extents


@pytest.mark.parametrize("cluster", ["none", "average"])
def test_a_sphere_inside_the_extents_keeps_its_mesh(cluster):
    import ferreus_rbf_rs_amd as F
    lat = R.Lattice(EXT, RES)
    field = np.linalg.norm(lat.world(lat.node_ijk()) - [3.0, 3.0, 3.0], axis=-1) - 2.0
    rv, rf = F.isosurface_from_values(field, EXT, RES, 0.0, cluster=cluster)
    v, f, stats = F.isosurface_from_values(field, EXT, RES, 0.0, cluster=cluster, finish="clipped", return_stats=True)
    wv, wf, wstats = FR.finish(rv, rf, EXT)
    _same_mesh((v, f), (wv, wf), EXT)
    assert stats["finish"] == wstats
    assert stats["finish"]["straddling"] == 0 and stats["finish"]["outside"] == 0
    assert len(f) == len(rf) and len(v) == len(np.unique(rf))
    assert R.directed_edges_once(f) and R.euler_characteristic(v, f) == 2
    assert len(_check_properties(v, f, EXT)) == 0
    vol, rvol = R.enclosed_volume(v, f), R.enclosed_volume(rv, rf)
    assert abs(vol - rvol) <= 1e-12 * abs(rvol) and abs(vol - 4.0 / 3.0 * np.pi * 8.0) < 0.02 * 4.0 / 3.0 * np.pi * 8.0


@pytest.mark.parametrize("name", sorted(FR.hand_made()))
def test_clip_mesh_on_the_hand_made_meshes(name):
    import ferreus_rbf_rs_amd as F
    v, f, shape, count = FR.hand_made()[name]
    ov, of, stats = F.clip_mesh(v, f, FR.HAND_EXT, return_stats=True)
    wv, wf, wstats = FR.finish(v, f, FR.HAND_EXT)
    assert ov.shape == (shape[0], 3) and of.shape == (shape[1], 3)
    assert np.array_equal(of, wf) and np.array_equal(ov, wv) and stats == wstats
    if count in ("collapsed", "tiny", "duplicate", "lone"):
        assert stats[count] == 1
    plain = F.clip_mesh(v, f, FR.HAND_EXT)
    assert np.array_equal(plain[0], ov) and np.array_equal(plain[1], of)


def test_clip_mesh_cuts_a_caller_mesh_and_closes_nothing():
    """A square sheet through the whole box, larger than it: what is left is the cross-section, ending on four faces."""
    import ferreus_rbf_rs_amd as F
    ext = [0.0, 0.0, 0.0, 1.0, 1.0, 1.0]
    n = 9
    g = np.linspace(-0.5, 1.5, n)
    x, y = np.meshgrid(g, g, indexing="ij")
    v = np.stack([x.ravel(), y.ravel(), 0.3 + 0.2 * x.ravel()], 1)
    i, j = np.meshgrid(np.arange(n - 1), np.arange(n - 1), indexing="ij")
    a = (i * n + j).ravel()
    f = np.concatenate([np.stack([a, a + n, a + 1], 1), np.stack([a + 1, a + n, a + n + 1], 1)])
    ov, of, stats = F.clip_mesh(v, f, ext, return_stats=True)
    wv, wf, wstats = FR.finish(v, f, ext)
    _same_mesh((ov, of), (wv, wf), ext)
    assert stats == wstats and stats["straddling"] > 0 and stats["outside"] > 0
    _check_properties(ov, of, ext)
    area = 0.5 * np.linalg.norm(np.cross(ov[of[:, 1]] - ov[of[:, 0]], ov[of[:, 2]] - ov[of[:, 0]]), axis=1).sum()
    assert abs(area - np.sqrt(1.04)) < 1e-12


@pytest.mark.parametrize("cluster", ["none", "average"])
def test_fmm_field_equals_the_restatement_of_the_device_raw_mesh(fit, cluster):
    """The clipped mesh against the restatement applied to the device's own raw mesh of the same call arguments: the
    new stage alone, whatever the last bits of the field."""
    pts, coef = fit
    r = 0.12
    ext = [0.5, 0.7, 0.6, 3.9, 5.5, 4.3]                  # cuts the fitted sphere (centre 3, radius 1.8) with two faces
    t = _tree(pts, coef, r, deterministic=True)
    rv, rf = t.build_isosurface(ext, r, 0.0, cluster=cluster)
    v, f, stats = t.build_isosurface(ext, r, 0.0, cluster=cluster, finish="clipped", return_stats=True)
    eps = FR.bbox_eps(ext)
    cv, cf, _ = FR.clip_mesh(rv, rf, ext)
    ok, gap, spread = FR.unambiguous(cv, eps)
    print(cluster, "raw", len(rv), len(rf), "clipped", len(v), len(f), stats["finish"], "gap / eps", gap, "spread / eps", spread)
    assert ok                                              # the condition on the input, as for the lattice meshes
    wv, wf, wstats = FR.finish(rv, rf, ext)
    _same_mesh((v, f), (wv, wf), ext)
    assert stats["finish"] == wstats and stats["finish"]["straddling"] > 0
    assert len(f) > 1000 and len(_check_properties(v, f, ext)) > 0
    # the vertices made on the faces lie on the interpolant's surface as well as the lattice's edges do
    fv = t.evaluate_leaves(None, v)[:, 0]
    assert float(np.abs(fv).max()) < 0.25 * r, float(np.abs(fv).max())


def test_invariances_bitwise(fit):
    pts, coef = fit
    r = 0.15
    ext = [0.5, 0.7, 0.6, 3.9, 5.5, 4.3]
    isos = [0.0, -0.6, 0.4]
    for cluster in ("none", "average"):
        kw = dict(cluster=cluster, finish="clipped", return_stats=True)
        t = _tree(pts, coef, r, deterministic=True)
        many = t.build_isosurfaces(ext, r, isos, **kw)
        for iso, m in zip(isos, many):
            one = t.build_isosurface(ext, r, iso, **kw)
            assert np.array_equal(m[0], one[0]) and np.array_equal(m[1], one[1]) and m[2] == one[2]
        tiny = t.build_isosurfaces(ext, r, isos, batch_bytes=1, **kw)
        again = t.build_isosurfaces(ext, r, isos, **kw)
        g = _tree(pts, coef, r, deterministic=True, devices=[0, 0])
        assert g.device_count() == 2
        grp = g.build_isosurfaces(ext, r, isos, **kw)
        for ms in (tiny, again, grp):
            for a, b in zip(many, ms):
                assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]
        assert len(many[0][1]) > 300 and many[0][2]["finish"]["straddling"] > 0
        # finish="raw" is the mesh of the call without the argument, and carries no finish counts
        plain = t.build_isosurfaces(ext, r, isos, cluster=cluster, return_stats=True)
        raw = t.build_isosurfaces(ext, r, isos, cluster=cluster, return_stats=True, finish="raw")
        for a, b in zip(plain, raw):
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2] and "finish" not in b[2]


@pytest.mark.parametrize("cluster", ["none", "average"])
def test_finish_raw_is_the_mesh_without_the_argument(cluster):
    import ferreus_rbf_rs_amd as F
    lat, field = FR.lattice_field("torus_cut")
    plain = F.isosurface_from_values(field, EXT, RES, 0.0, cluster=cluster)
    raw = F.isosurface_from_values(field, EXT, RES, 0.0, cluster=cluster, finish="raw")
    assert np.array_equal(plain[0], raw[0]) and np.array_equal(plain[1], raw[1])
    _same_mesh(raw, _raw_restatement(lat, field, 0.0, cluster), EXT)
    many = F.isosurfaces_from_values(field, EXT, RES, [0.0, 0.2], cluster=cluster, finish="clipped", batch_bytes=1)
    for iso, m in zip([0.0, 0.2], many):
        one = F.isosurface_from_values(field, EXT, RES, iso, cluster=cluster, finish="clipped")
        assert np.array_equal(m[0], one[0]) and np.array_equal(m[1], one[1])


@pytest.mark.parametrize("cluster", ["none", "average"])
def test_nothing_to_keep_gives_empty_arrays(cluster):
    import ferreus_rbf_rs_amd as F
    lat, field = FR.lattice_field("sphere_cut")
    v, f, stats = F.isosurface_from_values(field, EXT, RES, 1e6, cluster=cluster, finish="clipped", return_stats=True)
    assert v.shape == (0, 3) and f.shape == (0, 3) and v.dtype == np.float64 and f.dtype == np.int64
    assert sum(stats["finish"].values()) == 0
    # a surface that only passes through the two cells of padding around the extents
    w = lat.world(lat.node_ijk())
    outside = w[..., 0] - (EXT[0] - 1.2 * lat.spacing[0])
    raw = F.isosurface_from_values(outside, EXT, RES, 0.0, cluster=cluster)
    assert len(raw[1]) > 100
    v, f, stats = F.isosurface_from_values(outside, EXT, RES, 0.0, cluster=cluster, finish="clipped", return_stats=True)
    assert v.shape == (0, 3) and f.shape == (0, 3)
    assert stats["finish"]["facets_in"] == len(raw[1]) == stats["finish"]["outside"]
    assert stats["finish"]["vertices_emitted"] == 0
    # and a caller's mesh far from the extents
    v, f = F.clip_mesh(raw[0] - [50.0, 0.0, 0.0], raw[1], EXT)
    assert v.shape == (0, 3) and f.shape == (0, 3)
    v, f = F.clip_mesh(np.zeros((0, 3)), np.zeros((0, 3), np.int64), EXT)
    assert v.shape == (0, 3) and f.shape == (0, 3)


def test_bad_meshes_are_refused_with_a_message_before_any_work():
    import ferreus_rbf_rs_amd as F
    from ferreus_rbf_rs_amd import _lib as L
    lib = L.load()
    ext = np.array(EXT)
    v, f = np.zeros((3, 3)), np.zeros((1, 3), np.int64)
    # more facets than the 32-bit ids hold: refused from the sizes alone (the arrays are never read)
    res = ctypes.c_void_p()
    rc = lib.bbfmm_isosurface_finish_mesh(None, v.ctypes.data, 3, f.ctypes.data, (1 << 26) + 1, ext.ctypes.data, ctypes.byref(res))
    assert rc == L.BAD_ARGUMENT and res
    msg = lib.bbfmm_isosurface_error(res).decode()
    lib.bbfmm_isosurface_destroy(res)
    assert "too large to clip and clean" in msg and str((1 << 26) + 1) in msg
    with pytest.raises(F.FmmError, match="names vertex 7 of 3"):
        F.clip_mesh(v, [[0, 1, 7]], EXT)
    with pytest.raises(F.FmmError, match="inverted extents"):
        F.clip_mesh(v, f, [0, 0, 0, -1, 1, 1])
    ov, of = F.clip_mesh([[1, 1, 1], [2, 1, 1], [1, 2, 1], [2, 2, 1]], [[0, 1, 2], [1, 3, 2]], EXT)   # still works
    assert ov.shape == (4, 3) and of.shape == (2, 3)
