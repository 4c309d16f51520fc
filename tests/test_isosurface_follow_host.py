"""Following the surface, the host side (no GPU): the numpy restatement of its contract
(tests/isosurface_follow_restatement.py; DESIGN.md "Following the surface") and refused arguments."""
import numpy as np
import pytest

import isosurface_restatement as R
import isosurface_follow_restatement as FR

EXT = [0.0, 0.0, 0.0, 6.0, 6.0, 6.0]
RES = 0.15


@pytest.fixture(scope="module")
def sphere():
    """The sphere of tests/test_gpu_isosurface_follow.py: radius 1.2 at the centre, one seed on it."""
    lat = R.Lattice(EXT, RES)
    field = np.linalg.norm(lat.world(lat.node_ijk()) - [3.0, 3.0, 3.0], axis=-1) - 1.2
    return lat, field, np.array([[4.2, 3.0, 3.0]])


def test_mesh_of_the_visited_field_equals_the_dense_mesh(sphere):
    lat, field, seeds = sphere
    visited = FR.visited_bricks(lat, field, 0.0, seeds)
    v, f = R.extract(lat, FR.masked_field(lat, field, visited), 0.0)
    vd, fd = R.extract(lat, field, 0.0)
    assert len(fd) > 1000
    assert np.array_equal(f, fd) and np.array_equal(v, vd)
    # the point of it: far fewer nodes than the dense pass (the cap of the device test)
    n, n_e = FR.nodes_evaluated(lat, visited), int(lat.inE.sum())
    print("bricks", int(visited.sum()), "of", visited.size, "nodes", n, "of", n_e)
    assert 0 < n <= n_e // 2
    assert 1 <= FR.seed_bricks(lat, seeds, 8).sum() <= 8 and not visited.all()


def test_visited_set_does_not_depend_on_the_order(sphere):
    lat, field, _ = sphere
    rng = np.random.default_rng(3)
    d = rng.standard_normal((12, 3))
    seeds = np.array([3.0, 3.0, 3.0]) + 1.2 * d / np.linalg.norm(d, axis=1, keepdims=True)
    want = FR.visited_bricks(lat, field, 0.0, seeds)
    assert want.any()
    for trial in range(3):
        got = FR.visited_bricks(lat, field, 0.0, seeds[rng.permutation(len(seeds))], order=rng)
        assert np.array_equal(got, want), trial
    # one seed reaches the same component: the same set but for the other seeds' own bricks
    assert np.array_equal(FR.visited_bricks(lat, field, 0.0, seeds[:1]) | FR.seed_bricks(lat, seeds, 8), want)


def test_seed_cells_clamp_and_deduplicate(sphere):
    lat = sphere[0]
    c = FR.seed_cells(lat, [[4.21, 3.02, 3.01], [4.21, 3.02, 3.01], [4.21 + 1e-6, 3.02, 3.01], [-50.0, 3.0, 99.0]])
    assert c.shape == (2, 3)
    assert (c.sum(1) % 2 == 0).all()                                  # cells are sample points
    assert np.abs(lat.world(c[0]) - [4.21, 3.02, 3.01]).max() <= 2 * lat.spacing.max()
    assert np.abs(lat.world(c[1]) - [0.0, 3.0, 6.0]).max() <= 2 * lat.spacing.max()   # clamped to the extents
    assert FR.seed_bricks(lat, np.zeros((0, 3)), 8).sum() == 0


def test_unknown_follow_mode_is_refused(sphere):
    import ferreus_rbf_rs_amd as F
    lat, field, seeds = sphere
    with pytest.raises(ValueError, match="follow"):
        F.isosurface_from_values(field, EXT, RES, 0.0, follow="bogus", seeds=seeds)
    with pytest.raises(ValueError, match="seeds"):
        F.isosurface_from_values(field, EXT, RES, 0.0, follow="surface")
    with pytest.raises(ValueError, match="seeds"):
        F.isosurface_from_values(field, EXT, RES, 0.0, follow="surface", seeds=np.zeros((4, 2)))
