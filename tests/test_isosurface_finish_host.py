"""Clip and clean of isosurface meshes (finish="clipped"), the parts that run without a GPU: the numpy restatement of the
contract (tests/isosurface_finish_restatement.py) against the reference's own unit test and hand-made meshes, the
library's single-triangle clip against the restatement's, and the condition on the lattice meshes of the GPU tests
under which the contract's weld is the reference's greedy one."""
import numpy as np
import pytest

import isosurface_restatement as R
import isosurface_cluster_restatement as C
import isosurface_finish_restatement as FR


def test_the_reference_unit_test():
    """clean_mesh_removes_single_triangle_components (mesh_cleanup.rs:239-255): 7 vertices, 3 facets -> 4, 2."""
    v = [[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0], [10, 0, 0], [11, 0, 0], [10, 1, 0]]
    f = [[0, 1, 2], [1, 3, 2], [4, 5, 6]]
    for weld in ("components", "greedy"):
        cv, cf, counts = FR.clean_mesh(v, f, 1.0e-9, weld)
        assert cv.shape == (4, 3) and cf.shape == (2, 3)
        assert np.array_equal(cf, [[0, 1, 2], [1, 3, 2]]) and np.array_equal(cv, np.array(v, float)[:4])
        assert counts == {"welded": 0, "weld_loose": 0, "collapsed": 0, "tiny": 0, "duplicate": 0, "lone": 1}


@pytest.mark.parametrize("name", sorted(FR.hand_made()))
def test_hand_made_meshes_hit_one_rule_each(name):
    v, f, shape, count = FR.hand_made()[name]
    for weld in ("components", "greedy"):
        ov, of, stats = FR.finish(v, f, FR.HAND_EXT, weld, literal=True)
        assert (len(ov), len(of)) == shape, (name, weld, stats)
        assert stats["facets_in"] == len(f) and stats["straddling"] == 0 and stats["outside"] == 0
        assert stats["vertices_emitted"] == 3 * len(f) and stats["weld_loose"] == 0
        for rule in ("collapsed", "tiny", "duplicate", "lone"):
            assert stats[rule] == (1 if rule == count else 0), (name, rule, stats)
        assert len(np.unique(of)) == len(ov)
    if name == "weld_across_cells":
        eps = FR.bbox_eps(FR.HAND_EXT)
        keys = FR.cell_keys(v[4:6], eps)
        assert keys[1, 0] == keys[0, 0] + 1               # the two copies lie in neighbouring cells
        assert np.array_equal(ov[4], v[4])                # and the lower index is the representative
    if name == "unused_vertex":
        assert np.array_equal(ov, v[1:]) and np.array_equal(of, f - 1)


def test_ids_follow_first_use_and_the_lowest_index_wins():
    eps = 1.0e-9
    v = np.array([[9, 9, 9], [1, 0, 0], [0, 0, 0], [0, 1, 0], [1, 1, 0], [1 + 2e-10, 0, 0]], float)
    f = np.array([[4, 3, 5], [2, 1, 3]])
    cv, cf, counts = FR.clean_mesh(v, f, eps)
    assert np.array_equal(cf, [[0, 1, 2], [3, 2, 1]])
    assert np.array_equal(cv, v[[4, 3, 1, 2]])            # vertex 5 welds into vertex 1, whose coordinates stay
    assert counts["welded"] == 1


def _random_triangles(rng, ext, eps, n):
    lo, hi = np.array(ext[:3]), np.array(ext[3:])
    size = hi - lo
    tris = lo - 0.6 * size + rng.random((n, 3, 3)) * 2.2 * size
    # small triangles near the surface of the box, and ones spanning a corner of it
    small = rng.random(n) < 0.35
    centre = lo + rng.random((n, 1, 3)) * size
    centre[..., 0] = np.where(rng.random((n, 1)) < 0.5, lo[0], hi[0])
    tris = np.where(small[:, None, None], centre + (rng.random((n, 3, 3)) - 0.5) * 0.3 * size, tris)
    corner = rng.random(n) < 0.15
    c = np.where(rng.random((n, 1, 3)) < 0.5, lo, hi)
    tris = np.where(corner[:, None, None], c + (rng.random((n, 3, 3)) - 0.5) * 0.8 * size, tris)
    # corners exactly on planes and within eps of planes (inside and outside the slack)
    for scale in (0.0, 0.4, 0.9, 1.6, 3.0):
        pick = rng.random((n, 3, 3)) < 0.06
        plane = np.where(rng.random((n, 3, 3)) < 0.5, lo, hi)
        tris = np.where(pick, plane + scale * eps * rng.choice([-1.0, 1.0], (n, 3, 3)), tris)
    return tris


@pytest.mark.parametrize("ext", [FR.EXT, [-3.0, 2.0, 100.0, -1.0, 2.5, 1000.0]])
def test_single_triangle_clip_equals_the_restatement(ext):
    from ferreus_rbf_rs_amd import isosurface as I
    eps = FR.bbox_eps(ext)
    tris = _random_triangles(np.random.default_rng(11), ext, eps, 4000)
    scale = float(np.abs(np.asarray(ext)).max())
    hist, worst = {}, 0.0
    for tri in tris:
        want, wsrc = FR.clip_triangle(tri, ext)
        got, src = I.clip_triangle(tri, ext)
        assert len(got) == len(want) and np.array_equal(src, wsrc), tri
        if len(want):
            worst = max(worst, float(np.abs(got - want).max()))
        hist[len(want)] = hist.get(len(want), 0) + 1
    print("points per polygon", sorted(hist.items()), "largest difference", worst)
    assert worst <= 1e-12 * scale
    assert hist.get(0, 0) > 100 and hist.get(3, 0) > 100 and sum(n for k, n in hist.items() if k >= 5) > 100
    assert max(hist) >= 6                                  # a box corner cut off


def test_clip_triangle_exact_cases():
    from ferreus_rbf_rs_amd import isosurface as I
    ext = [0.0, 0.0, 0.0, 1.0, 1.0, 1.0]
    inside = [[0.2, 0.2, 0.5], [0.8, 0.2, 0.5], [0.2, 0.8, 0.5]]
    p, c = I.clip_triangle(inside, ext)
    assert np.array_equal(p, inside) and c.tolist() == [0, 1, 2]
    p, c = I.clip_triangle(np.array(inside) + [2.0, 0, 0], ext)
    assert p.shape == (0, 3)
    # one corner cut off by x = 1: a quadrilateral with two points exactly on the plane
    p, c = I.clip_triangle([[0.5, 0.25, 0.5], [1.5, 0.25, 0.5], [0.5, 0.75, 0.5]], ext)
    want, wc = FR.clip_triangle([[0.5, 0.25, 0.5], [1.5, 0.25, 0.5], [0.5, 0.75, 0.5]], ext)
    assert np.array_equal(p, want) and np.array_equal(c, wc)
    assert len(p) == 4 and (c == -1).sum() == 2 and (p[c == -1, 0] == 1.0).all()
    with pytest.raises(ValueError):
        I.clip_triangle(inside, [0, 0, 0, -1, 1, 1])


def test_unknown_finish_is_a_value_error():
    import ferreus_rbf_rs_amd as F
    from ferreus_rbf_rs_amd import isosurface as I
    with pytest.raises(ValueError, match="finish must be one of"):
        F.isosurface_from_values(np.zeros((2, 2, 2)), FR.EXT, 1.0, 0.0, finish="closed")
    assert I.FINISH == {"raw": 0, "clipped": 1} and len(I.FINISH_STATS) == 10 == len(FR.FINISH_STATS)
    assert I.FINISH_STATS == FR.FINISH_STATS


def _raw_mesh(name, cluster):
    lat, field = FR.lattice_field(name)
    if cluster == "none":
        return R.extract(lat, field, 0.0)
    out = C.extract(lat, field, 0.0)
    return out["vertices"], out["facets"]


@pytest.mark.parametrize("cluster", ["none", "average"])
@pytest.mark.parametrize("name", FR.FIELDS)
def test_the_lattice_meshes_of_the_gpu_tests_are_unambiguous(name, cluster):
    """A condition on the inputs of tests/test_gpu_isosurface_finish.py: on the clipped vertices of every lattice mesh the
    reference's greedy weld and the lowest-index-of-component weld give the same partition, no vertex is further than
    eps from its representative, and distinct representatives are at least 100 eps apart."""
    v, f = _raw_mesh(name, cluster)
    eps = FR.bbox_eps(FR.EXT)
    cv, cf, counts = FR.clip_mesh(v, f, FR.EXT)
    ok, gap, spread = FR.unambiguous(cv, eps)
    a = FR.clean_mesh(cv, cf, eps, "components")
    b = FR.clean_mesh(cv, cf, eps, "greedy")
    print(name, cluster, "facets", len(f), counts, "gap / eps", gap, "spread / eps", spread, a[2])
    assert ok and gap >= 100.0 and spread <= 1.0
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]
    assert a[2]["weld_loose"] == 0
    assert counts["straddling"] > 0 and counts["outside"] > 0 and len(a[1]) > 100


def test_the_shortcuts_of_the_restatement_are_the_literal_clip():
    v, f = _raw_mesh("corner_and_inside", "none")
    a = FR.clip_mesh(v, f, FR.EXT)
    b = FR.clip_mesh(v, f, FR.EXT, literal=True)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]
