"""Following the surface on the device (follow="surface"), against the dense extraction and the numpy restatement of
its contract (tests/isosurface_follow_restatement.py; DESIGN.md "Following the surface").

The analytic cases hand the wavefront the very values the dense call sees (isosurfaces_from_values), so meshes are
compared with np.array_equal."""
import numpy as np
import pytest

import isosurface_restatement as R
import isosurface_follow_restatement as FR
from oracle import bbfmm_oracle as O

pytestmark = pytest.mark.gpu

EXT = [0.0, 0.0, 0.0, 6.0, 6.0, 6.0]
RES = 0.15


@pytest.fixture(scope="module")
def lat():
    return R.Lattice(EXT, RES)


@pytest.fixture(scope="module")
def world(lat):
    return lat.world(lat.node_ijk())


def _sphere(world, centre, radius):
    return np.linalg.norm(world - np.asarray(centre, float), axis=-1) - radius


def _equal(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def _both(field, seeds, iso=0.0, **kw):
    import ferreus_rbf_rs_amd as F
    dense = F.isosurface_from_values(field, EXT, RES, iso, **kw)
    got = F.isosurface_from_values(field, EXT, RES, iso, follow="surface", seeds=seeds, **kw)
    return dense, got


SPHERE_SEED = [[4.2, 3.0, 3.0]]


@pytest.mark.parametrize("cluster", ["none", "average"])
@pytest.mark.parametrize("finish", ["raw", "clipped"])
def test_sphere_equals_the_dense_mesh(lat, world, cluster, finish):
    field = _sphere(world, [3.0, 3.0, 3.0], 1.2)
    dense, got = _both(field, SPHERE_SEED, cluster=cluster, finish=finish, return_stats=True)
    assert len(dense[1]) > 1000
    assert _equal(got, dense)
    fol = got[2].pop("follow")
    assert got[2] == dense[2]                                         # the clustering (and finish) counts
    print({k: v for k, v in fol.items() if k != "visited"})
    assert fol["seeds"] == 1 and fol["seed_cells"] == 1 and fol["newton_steps"] == 0
    assert fol["seed_bricks"] == int(FR.seed_bricks(lat, SPHERE_SEED, 8).sum())
    assert fol["nodes"] == int(lat.inE.sum())
    assert 0 < fol["nodes_evaluated"] <= fol["nodes"] // 2
    want = FR.visited_bricks(lat, field, 0.0, SPHERE_SEED)
    assert fol["brick"] == 8 and np.array_equal(fol["visited"], want)
    assert fol["bricks_visited"] == int(want.sum()) and fol["nodes_evaluated"] == FR.nodes_evaluated(lat, want)
    assert fol["rounds"] >= 2


def test_tilted_plane_runs_into_the_shell_on_every_side(lat, world):
    """x + 0.7 y + 0.4 z = c leaves bricks through faces, edges and corners and ends in the shell of E."""
    field = world[..., 0] + 0.7 * world[..., 1] + 0.4 * world[..., 2] - 6.3
    dense, got = _both(field, [[3.0, 3.0, 3.0]], return_stats=True)
    assert len(dense[1]) > 10000
    assert _equal(got, dense)
    fol = got[2]["follow"]
    assert np.array_equal(fol["visited"], FR.visited_bricks(lat, field, 0.0, [[3.0, 3.0, 3.0]]))
    assert fol["nodes_evaluated"] < fol["nodes"]


@pytest.mark.parametrize("finish", ["raw", "clipped"])
def test_sphere_cut_by_the_box(world, finish):
    field = _sphere(world, [0.4, 3.0, 3.0], 1.2)
    dense, got = _both(field, [[1.6, 3.0, 3.0]], finish=finish)
    assert len(dense[1]) > 1000
    assert _equal(got, dense)


def test_two_spheres_one_seed_each(lat, world):
    """Centres 2.9 apart in x alone: 38 nodes of 0.075, more than 4 bricks."""
    ca, cb = [1.5, 3.0, 3.0], [4.4, 3.0, 3.0]
    assert (cb[0] - ca[0]) / lat.spacing[0] >= 32
    a, b = _sphere(world, ca, 0.9), _sphere(world, cb, 0.9)
    both = np.minimum(a, b)
    import ferreus_rbf_rs_amd as F
    seed_a, seed_b = [2.4, 3.0, 3.0], [5.3, 3.0, 3.0]
    only_a = F.isosurface_from_values(both, EXT, RES, 0.0, follow="surface", seeds=[seed_a])
    assert len(only_a[1]) > 1000
    assert _equal(only_a, F.isosurface_from_values(a, EXT, RES, 0.0))
    only_b = F.isosurface_from_values(both, EXT, RES, 0.0, follow="surface", seeds=[seed_b])
    assert _equal(only_b, F.isosurface_from_values(b, EXT, RES, 0.0))
    union = F.isosurface_from_values(both, EXT, RES, 0.0, follow="surface", seeds=[seed_b, seed_a])
    dense = F.isosurface_from_values(both, EXT, RES, 0.0)
    assert _equal(union, dense) and len(dense[1]) == len(only_a[1]) + len(only_b[1])


@pytest.mark.parametrize("brick", ["4", "16"])
def test_brick_size_does_not_change_the_mesh(lat, world, brick, monkeypatch):
    import ferreus_rbf_rs_amd as F
    field = _sphere(world, [3.0, 3.0, 3.0], 1.2)
    want = F.isosurface_from_values(field, EXT, RES, 0.0, follow="surface", seeds=SPHERE_SEED, cluster="average")
    monkeypatch.setenv("BBFMM_ISO_BRICK", brick)
    got = F.isosurface_from_values(field, EXT, RES, 0.0, follow="surface", seeds=SPHERE_SEED, cluster="average",
                                   return_stats=True)
    assert len(want[1]) > 1000 and _equal(got, want)
    fol = got[2]["follow"]
    assert fol["brick"] == int(brick)
    assert np.array_equal(fol["visited"], FR.visited_bricks(lat, field, 0.0, SPHERE_SEED, int(brick)))
    monkeypatch.setenv("BBFMM_ISO_BRICK", "5")
    with pytest.raises(F.FmmError, match="BBFMM_ISO_BRICK"):
        F.isosurface_from_values(field, EXT, RES, 0.0, follow="surface", seeds=SPHERE_SEED)


def test_several_isovalues_equal_the_single_calls(lat, world):
    """The isovalues share the evaluated nodes; each mesh is still that of its isovalue alone.  Two spheres of radius
    0.9; at 0.3 the wavefront from the seed on B covers both (they are closer than a brick and its halo), and so
    evaluates the bricks of B's sphere at -0.3, which the wavefront of -0.3 from its seed on A never visits: without
    the mark per brick per isovalue the second mesh would hold B's sphere too (5124 facets instead of 2576)."""
    import ferreus_rbf_rs_amd as F
    a, b = _sphere(world, [1.5, 3.0, 3.0], 0.9), _sphere(world, [4.4, 3.0, 3.0], 0.9)
    field = np.minimum(a, b)
    isos = [0.3, -0.3]
    seeds = [[1.5, 3.6, 3.0], [4.4, 4.2, 3.0]]                        # on A at -0.3, on B at 0.3
    many = F.isosurfaces_from_values(field, EXT, RES, isos, follow="surface", seeds=seeds, cluster="average", return_stats=True)
    visited = []
    for iso, m in zip(isos, many):
        one = F.isosurface_from_values(field, EXT, RES, iso, follow="surface", seeds=seeds, cluster="average", return_stats=True)
        assert len(one[1]) > 100 and _equal(m, one)
        assert np.array_equal(m[2]["follow"]["visited"], one[2]["follow"]["visited"])
        visited.append(FR.visited_bricks(lat, field, iso, seeds))
        assert np.array_equal(m[2]["follow"]["visited"], visited[-1])
    assert _equal(many[0], F.isosurface_from_values(field, EXT, RES, 0.3, cluster="average"))
    assert _equal(many[1], F.isosurface_from_values(a, EXT, RES, -0.3, cluster="average"))
    assert len(many[1][1]) < len(F.isosurface_from_values(field, EXT, RES, -0.3, cluster="average")[1])
    # the case is the one described: the first wavefront evaluated crossings of the second isovalue outside its bricks
    union = FR.masked_field(lat, field, visited[0] | visited[1])
    assert len(R.extract(lat, union, -0.3)[1]) > len(R.extract(lat, FR.masked_field(lat, field, visited[1]), -0.3)[1])


def test_empty_results_are_not_errors(lat, world):
    import ferreus_rbf_rs_amd as F
    field = _sphere(world, [3.0, 3.0, 3.0], 1.2)
    for seeds in ([[3.0, 3.0, 3.0]], np.zeros((0, 3))):                # the bricks at the centre are not crossed; no seeds
        n_bricks = int(FR.seed_bricks(lat, seeds, 8).sum())
        assert n_bricks == int(FR.visited_bricks(lat, field, 0.0, seeds).sum())
        for cluster, finish in (("none", "raw"), ("average", "clipped")):
            v, f, st = F.isosurface_from_values(field, EXT, RES, 0.0, follow="surface", seeds=seeds, cluster=cluster,
                                                finish=finish, return_stats=True)
            assert v.shape == (0, 3) and f.shape == (0, 3)
            assert st["follow"]["seeds"] == len(seeds) and st["follow"]["bricks_visited"] == n_bricks
            assert st["follow"]["rounds"] == (1 if len(seeds) else 0)


# ---- the FMM field
@pytest.fixture(scope="module")
def fit():
    """2,000 points on and around a sphere of radius 1.3, a LinearRbf fit with a constant trend."""
    rng = np.random.default_rng(11)
    n = 2000
    d = rng.standard_normal((n, 3))
    pts = np.array([3.0, 3.0, 3.0]) + (1.3 + rng.uniform(-0.35, 0.35, (n, 1))) * d / np.linalg.norm(d, axis=1, keepdims=True)
    vals = np.linalg.norm(pts - [3.0, 3.0, 3.0], axis=1) - 1.3
    kid = O.KERNEL_IDS["LinearRbf"]
    A = np.zeros((n + 1, n + 1))
    A[:n, :n] = O.kernel_matrix(kid, 1.0, 1.0, pts, pts)
    A[:n, n] = A[n, :n] = 1.0
    sol = np.linalg.solve(A, np.concatenate([vals, [0.0]]))
    return pts, sol[:n, None], float(sol[n]), kid


def _tree(fit, r, kid=None):
    import ferreus_rbf_rs_amd as F
    pts, coef, _, kid0 = fit
    pad = 10.0 * r
    ext = list(pts.min(0) - pad) + list(pts.max(0) + pad)
    t = F.FmmTree(pts, 7, F.KernelParams(F.KernelType(kid0 if kid is None else kid), base_range=1.0, total_sill=1.0), True,
                  False, extents=ext)
    t.set_weights(coef)
    t.set_local_coefficients(coef)
    return t


def test_tree_field_follows_from_its_source_points(fit, monkeypatch):
    import ferreus_rbf_rs_amd as F
    pts, coef, c0, _ = fit
    r = 0.15
    ext = list(pts.min(0)) + list(pts.max(0))
    iso = 0.05
    t = _tree(fit, r)
    drift = [c0, 0.0, 0.0, 0.0]
    vd, fd, field_d = t.build_isosurface(ext, r, iso, drift=drift, return_field=True)
    v, f, st, field = t.build_isosurface(ext, r, iso, drift=drift, return_field=True, return_stats=True, follow="surface")
    fol = st["follow"]
    print({k: x for k, x in fol.items() if k != "visited"})
    lat = R.Lattice(ext, r)
    scale = float(np.nanmax(np.abs(field_d)))
    # the isovalue decides every node the same way in both batchings
    assert not (np.abs(field_d[lat.inE] - iso + 1e-9) < 1e-12 * scale).any()
    known = np.isfinite(field)
    assert known.any() and not known[~lat.inE].any()
    assert np.array_equal(known, lat.inE & FR.node_mask(lat, fol["visited"], fol["brick"]))
    err = float(np.abs(field[known] - field_d[known]).max())
    print("fields", err, 1e-12 * scale)
    assert err <= 1e-12 * scale
    # return_field is the array the mesh was made from
    assert _equal((v, f), F.isosurface_from_values(field, ext, r, iso))
    assert len(fd) > 1000 and len(f) == len(fd)
    assert fol["seeds"] == len(pts) and 0 < fol["seed_cells"] <= len(pts)
    assert fol["newton_steps"] >= 1
    assert 0 < fol["nodes_evaluated"] < fol["nodes"] == int(lat.inE.sum())
    assert fol["nodes_evaluated"] == int(known.sum())
    # the reference's central differences in place of the leaf pass's gradients: the same bricks here
    monkeypatch.setenv("BBFMM_ISO_SEED_GRADIENTS", "differences")
    v2, f2, st2 = t.build_isosurface(ext, r, iso, drift=drift, return_stats=True, follow="surface")
    monkeypatch.delenv("BBFMM_ISO_SEED_GRADIENTS")
    assert st2["follow"]["newton_steps"] >= 1 and len(f2) == len(fd)
    assert np.array_equal(st2["follow"]["visited"], fol["visited"])
    # explicit seeds: one point off the surface is projected onto it and reaches the same component
    v1, f1, st1 = t.build_isosurface(ext, r, iso, drift=drift, return_stats=True, follow="surface", seeds=[[4.0, 3.1, 2.9]])
    assert st1["follow"]["seed_cells"] == 1 and st1["follow"]["newton_steps"] >= 2
    assert len(f1) == len(fd)
