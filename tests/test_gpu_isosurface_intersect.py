"""The self-intersection detector and the rollback of the clustered extraction (self_intersections="rollback") on the
device, against the numpy restatement of their contract (tests/isosurface_intersect_restatement.py; DESIGN.md
"Isosurfaces on the RMT lattice", self-intersection rollback).

Throughout: facets array_equal to the restatement's, vertices within 1e-12 * max|extents|, the returned counts equal to
the restatement's."""
import functools

import numpy as np
import pytest

import isosurface_restatement as R
import isosurface_cluster_restatement as C
import isosurface_finish_restatement as FR
import isosurface_intersect_restatement as X
from test_gpu_isosurface import EXT, _same_mesh, _tree, fit  # noqa: F401  (fit: a fixture)
from test_isosurface_intersect_host import A, APEX, FALSE_PAIRS, IA, RING, TRUE_PAIRS, small_noisy_sphere

pytestmark = pytest.mark.gpu

ROLLBACK = dict(cluster="average", self_intersections="rollback", return_stats=True)


def _same_as_restatement(got, want, extents):
    v, f, stats = got
    print("device", len(v), len(f), stats["self_intersections"])
    print("restatement", len(want["vertices"]), len(want["facets"]), want["self_intersections"])
    _same_mesh((v, f), (want["vertices"], want["facets"]), extents)
    assert stats["self_intersections"] == want["self_intersections"]
    assert {k: stats[k] for k in want["stats"]} == want["stats"]


def _detector_equals(v, f, extents):
    import ferreus_rbf_rs_amd as F
    ids, stats = F.mesh_self_intersections(v, f, extents, return_stats=True)
    want_ids, want, _ = X.detect(v, f, extents)
    print("device", stats, "restatement", want)
    assert ids.dtype == np.int64 and np.array_equal(ids, want_ids)
    assert [stats[n] for n in X.STAT_NAMES[:5]] == want
    return ids, stats


# ---- 1. the detector alone
def test_detector_on_the_clustered_mesh_of_the_small_noisy_sphere():
    lat, field, want = small_noisy_sphere()
    v, f = want["before"]
    ids, stats = _detector_equals(v, f, EXT)
    assert np.array_equal(ids, want["ids"]) and len(ids) > 0 and stats["inside_facets"] == len(f)
    ids_all, _ = _detector_equals(v, f, None)                      # no extents: no facet is filtered
    assert np.array_equal(ids_all, ids)


def hand_made_mesh():
    """The pairs of the host tests glued into one facet list, each pair moved to a place of its own (a stays the lower
    facet), and the fan."""
    verts, facets = [], []
    names = sorted(FALSE_PAIRS) + sorted(TRUE_PAIRS)
    for q, name in enumerate(names):
        a, ia, b, ib, _ = FALSE_PAIRS.get(name) or TRUE_PAIRS[name]
        shift = np.array([8.0 * (q % 4), 8.0 * (q // 4), 0.0])
        local = {}
        for tri, ids in ((a, ia), (b, ib)):
            for p, i in zip(tri, ids):
                if i not in local:
                    local[i] = len(verts)
                    verts.append(np.asarray(p, np.float64) + shift)
            facets.append([local[i] for i in ids])
    base = len(verts)
    shift = np.array([0.0, 40.0, 0.0])
    verts += [np.asarray(APEX) + shift] + [np.asarray(p) + shift for p in RING]
    facets += [[base, base + 1 + k, base + 1 + (k + 1) % 6] for k in range(6)]
    expect = [2 * names.index(n) + d for n in sorted(TRUE_PAIRS) for d in (0, 1)]
    return np.array(verts), np.array(facets, np.int64), np.array(sorted(expect), np.int64)


def test_detector_on_the_hand_made_mesh():
    v, f, expect = hand_made_mesh()
    ids, stats = _detector_equals(v, f, None)
    assert np.array_equal(ids, expect) and stats["true_pairs"] == len(TRUE_PAIRS)
    # extents that cut the last row of pairs and the fan away leave the others
    ext = [-5.0, -5.0, -5.0, 40.0, 23.0, 5.0]
    inside = X.inside_facets(v, f, ext)
    ids_in, stats_in = _detector_equals(v, f, ext)
    assert stats_in["inside_facets"] == len(inside) < len(f) and set(ids_in) == set(expect) & set(inside) and len(ids_in) == 2


def test_detector_on_an_empty_and_a_one_facet_mesh():
    import ferreus_rbf_rs_amd as F
    for v, f in ((np.zeros((0, 3)), np.zeros((0, 3), np.int64)), (np.array(A), np.array([IA]))):
        ids, stats = F.mesh_self_intersections(v, f, return_stats=True)
        assert ids.shape == (0,) and ids.dtype == np.int64
        assert stats == {"inside_facets": len(f), "box_pairs": 0, "moller_pairs": 0, "true_pairs": 0, "triangles": 0}
        assert F.mesh_self_intersections(v, f, EXT).shape == (0,)


# ---- 2. the extraction
def test_rollback_on_the_small_noisy_sphere():
    import ferreus_rbf_rs_amd as F
    lat, field, want = small_noisy_sphere()
    got = F.isosurface_from_values(field, EXT, 0.2, 0.0, **ROLLBACK)
    _same_as_restatement(got, want, EXT)
    assert got[2]["self_intersections"]["rolled_back"] > 0
    ids, stats = F.mesh_self_intersections(got[0], got[1], EXT, return_stats=True)
    want_ids, want_stats, _ = X.detect(want["vertices"], want["facets"], EXT)
    assert np.array_equal(ids, want_ids) and [stats[n] for n in X.STAT_NAMES[:5]] == want_stats
    assert len(ids) == 0


def test_rollback_composes_with_pass_b():
    """The noisy sphere of test_pass_b_rolls_sample_points_back (0.15 * standard_normal(seed 1) at resolution 0.1, some
    180,000 facets): pass B rolls sample points back and so does the self-intersection stage.  (The restatement of this
    lattice takes the better part of a minute on the host.)"""
    import ferreus_rbf_rs_amd as F
    lat = R.Lattice(EXT, 0.1)
    w = lat.world(lat.node_ijk())
    field = np.linalg.norm(w - [3.0, 3.0, 3.0], axis=-1) - 2.0 + 0.15 * np.random.default_rng(1).standard_normal(lat.shape)
    want = X.extract(lat, field, 0.0, EXT)
    got = F.isosurface_from_values(field, EXT, 0.1, 0.0, **ROLLBACK)
    _same_as_restatement(got, want, EXT)
    assert sum(got[2]["rolled_b"]) > 0 and got[2]["self_intersections"]["rolled_back"] > 0
    ids = F.mesh_self_intersections(got[0], got[1], EXT)
    assert np.array_equal(ids, X.detect(want["vertices"], want["facets"], EXT)[0])


# ---- 3. off by default
def test_ignore_is_the_default_and_cluster_none_does_nothing():
    import ferreus_rbf_rs_amd as F
    lat, field, want = small_noisy_sphere()
    plain = F.isosurface_from_values(field, EXT, 0.2, 0.0, cluster="average", return_stats=True)
    ignore = F.isosurface_from_values(field, EXT, 0.2, 0.0, cluster="average", return_stats=True, self_intersections="ignore")
    assert np.array_equal(plain[0], ignore[0]) and np.array_equal(plain[1], ignore[1]) and plain[2] == ignore[2]
    assert "self_intersections" not in plain[2]
    _same_mesh(plain[:2], want["before"], EXT)                      # the mesh the rollback starts from
    assert len(plain[1]) < len(want["facets"])
    none = F.isosurface_from_values(field, EXT, 0.2, 0.0, cluster="none")
    both = F.isosurface_from_values(field, EXT, 0.2, 0.0, cluster="none", self_intersections="rollback", return_stats=True)
    assert np.array_equal(none[0], both[0]) and np.array_equal(none[1], both[1])
    assert set(both[2]["self_intersections"]) == set(X.STAT_NAMES) and not any(both[2]["self_intersections"].values())
    with pytest.raises(ValueError, match="self_intersections must be one of"):
        F.isosurface_from_values(field, EXT, 0.2, 0.0, cluster="average", self_intersections="yes")


# ---- 4. the inside filter
@functools.lru_cache(maxsize=None)
def open_noisy_sphere():
    """The sphere of test_open_surface_leaves_the_shell_of_the_domain_unclustered plus 0.2 * standard_normal(seed 1)."""
    r = 0.15
    lat = R.Lattice(EXT, r)
    w = lat.world(lat.node_ijk())
    field = np.linalg.norm(w - [3.0, 3.0, 3.0], axis=-1) - 3.6 + 0.2 * np.random.default_rng(1).standard_normal(lat.shape)
    return r, lat, field, X.extract(lat, field, 0.0, EXT)


def test_only_facets_inside_the_extents_take_part():
    import ferreus_rbf_rs_amd as F
    r, lat, field, want = open_noisy_sphere()
    got = F.isosurface_from_values(field, EXT, r, 0.0, **ROLLBACK)
    _same_as_restatement(got, want, EXT)
    counts = got[2]["self_intersections"]
    assert 0 < counts["inside_facets"] < len(want["before"][1]) and counts["rolled_back"] > 0


def test_rollback_then_clip_and_clean():
    import ferreus_rbf_rs_amd as F
    r, lat, field, want = open_noisy_sphere()
    v, f, stats = F.isosurface_from_values(field, EXT, r, 0.0, finish="clipped", **ROLLBACK)
    wv, wf, wstats = FR.finish(want["vertices"], want["facets"], EXT)
    _same_mesh((v, f), (wv, wf), EXT)
    assert stats["finish"] == wstats and stats["self_intersections"] == want["self_intersections"]


# ---- 5. the FMM field
def test_fmm_field_equals_the_restatement(fit):
    pts, coef = fit
    r = 0.12
    ext = list(pts.min(0)) + list(pts.max(0))
    t = _tree(pts, coef, r)
    v, f, stats, field = t.build_isosurface(ext, r, 0.0, return_field=True, **ROLLBACK)
    lat = R.Lattice(ext, r)
    assert field.shape == lat.shape
    _same_as_restatement((v, f, stats), X.extract(lat, field, 0.0, ext), ext)
    assert stats["self_intersections"]["inside_facets"] > 1000


# ---- 6. invariances
def test_invariances_bitwise(fit):
    pts, coef = fit
    r = 0.15
    ext = list(pts.min(0)) + list(pts.max(0))
    isos = [0.0, -0.6, 0.4]
    t = _tree(pts, coef, r, deterministic=True)
    many = t.build_isosurfaces(ext, r, isos, **ROLLBACK)
    for iso, m in zip(isos, many):
        one = t.build_isosurface(ext, r, iso, **ROLLBACK)
        assert np.array_equal(m[0], one[0]) and np.array_equal(m[1], one[1]) and m[2] == one[2]
    tiny = t.build_isosurfaces(ext, r, isos, batch_bytes=1, **ROLLBACK)
    again = t.build_isosurfaces(ext, r, isos, **ROLLBACK)
    g = _tree(pts, coef, r, deterministic=True, devices=[0, 0])
    assert g.device_count() == 2
    grp = g.build_isosurfaces(ext, r, isos, **ROLLBACK)
    for ms in (tiny, again, grp):
        for a, b in zip(many, ms):
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]
    assert many[0][2]["self_intersections"]["inside_facets"] > 500
    # a caller's noisy field: the same under the batch size and among several isovalues, with sample points rolled back
    lat, field, want = small_noisy_sphere()
    isos = [0.0, 0.1]
    import ferreus_rbf_rs_amd as F
    many = F.isosurfaces_from_values(field, EXT, 0.2, isos, batch_bytes=1, **ROLLBACK)
    for iso, m in zip(isos, many):
        one = F.isosurface_from_values(field, EXT, 0.2, iso, **ROLLBACK)
        assert np.array_equal(m[0], one[0]) and np.array_equal(m[1], one[1]) and m[2] == one[2]
    assert many[0][2]["self_intersections"] == want["self_intersections"]


# ---- 7. a grid that would make the search quadratic
def test_one_huge_triangle_among_many_small_ones_is_refused():
    import ferreus_rbf_rs_amd as F
    n = 120                                                         # 2 * 119^2 = 28,322 small triangles on a unit grid
    i, j = np.meshgrid(np.arange(n, dtype=np.float64), np.arange(n, dtype=np.float64), indexing="ij")
    v = np.concatenate([np.stack([i.ravel(), j.ravel(), np.zeros(n * n)], 1),
                        [[-1e4, -1e4, 5.0], [1e4, -1e4, 5.0], [0.0, 1e4, 5.0]]])
    a = (np.arange(n - 1)[:, None] * n + np.arange(n - 1)[None, :]).ravel()
    small = np.concatenate([np.stack([a, a + n, a + 1], 1), np.stack([a + 1, a + n, a + n + 1], 1)])
    f = np.concatenate([small, [[n * n, n * n + 1, n * n + 2]]])
    with pytest.raises(F.FmmError, match="the search would be quadratic"):
        F.mesh_self_intersections(v, f)
    ids, stats = F.mesh_self_intersections(v, small, return_stats=True)      # without it the mesh goes through
    assert len(ids) == 0 and stats["inside_facets"] == len(small) and stats["box_pairs"] > len(small)
