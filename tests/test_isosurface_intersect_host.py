"""The pair predicate of the self-intersection detector on the host (F.triangle_pair, the function the device runs) and
the numpy restatement of the detector and of the rollback (tests/isosurface_intersect_restatement.py).  No GPU."""
import functools

import numpy as np
import pytest

import isosurface_restatement as R
import isosurface_cluster_restatement as C
import isosurface_intersect_restatement as X

# the triangle every hand-made pair is set against: in the plane z = 0, vertex ids 0, 1, 2
A = [[0.0, 0.0, 0.0], [2.0, 0.0, 0.0], [0.0, 2.0, 0.0]]
IA = [0, 1, 2]
RING = [[np.cos(a), np.sin(a), 0.0] for a in np.arange(6) * np.pi / 3.0]     # the fan: six triangles around an apex
APEX = [0.0, 0.0, 0.5]

# name -> (a, ids a, b, ids b, the stage that decides)
FALSE_PAIRS = {
    # b leaves the shared corner upwards and away: contact in one point, which the Moeller test does not count
    "shared vertex only": (A, IA, [[0, 0, 0], [-1, 0.5, 1], [-1, -0.5, 1.2]], [0, 3, 4], "moller"),
    "shared edge": (A, IA, [[0, 0, 0], [2, 0, 0], [1, -1, 1]], [0, 1, 3], "shared_two"),
    "coplanar quad": (A, IA, [[2, 0, 0], [2, 2, 0], [0, 2, 0]], [1, 3, 2], "shared_two"),
    # parallel planes: |n1 x n2| = 0
    "coplanar shared vertex": (A, IA, [[0, 0, 0], [-2, 0, 0], [0, -2, 0]], [0, 3, 4], "moller"),
    "nearly coplanar shared edge": (A, IA, [[0, 0, 0], [2, 0, 0], [1, 1, 1e-10]], [0, 1, 3], "shared_two"),
    # the common edge is a segment of contact of length 2, so the Moeller test passes; two coincident corners
    "coincident edge, distinct ids": (A, IA, [[0, 0, 0], [2, 0, 0], [1, -1, 1]], [10, 11, 12], "geometric_shared"),
    # b meets the plane of a along (0, 0, 0)-(1, 1, 0): Moeller passes; the edge opposite the common corner meets a on
    # its hypotenuse and a's hypotenuse meets b on that edge: no interior is pierced
    "coincident vertex, distinct ids": (A, IA, [[0, 0, 0], [1, 1, 1], [1, 1, -1]], [10, 11, 12], "geometric_shared"),
    "shared vertex, edges touch": (A, IA, [[0, 0, 0], [1, 1, 1], [1, 1, -1]], [0, 3, 4], "shared_crossing"),
    "coplanar overlap": (A, IA, [[0.5, 0.5, 0], [3, 0.5, 0], [0.5, 3, 0]], [3, 4, 5], "moller"),
    # a's box is [0, 2]^3, b lies in it, far below a's plane z = x + y
    "boxes overlap, no contact": ([[0, 0, 0], [2, 0, 2], [0, 2, 2]], IA, [[1.5, 1.5, 0.2], [2, 1.5, 0.3], [1.5, 2, 0.4]],
                                  [3, 4, 5], "moller"),
    "degenerate": (A, IA, [[0.2, 0.2, -1], [0.2, 0.2, 0], [0.2, 0.2, 1]], [3, 4, 5], "degenerate"),
}
TRUE_PAIRS = {
    # the edge opposite the shared corner runs through (0.5, 0.5, 0), inside a
    "shared vertex and a piercing": (A, IA, [[0, 0, 0], [0.5, 0.5, 1], [0.5, 0.5, -1]], [0, 3, 4], "shared_crossing"),
    "piercing": (A, IA, [[0.5, 0.2, -1], [0.5, 1.0, -1], [0.5, 0.6, 1]], [3, 4, 5], "true"),
    # one edge of b goes through the inside of a, its third corner is far away
    "edge through the interior": (A, IA, [[0.5, 0.5, -0.5], [0.6, 0.6, 0.5], [5, 5, 3]], [3, 4, 5], "true"),
}


@pytest.mark.parametrize("name", sorted(FALSE_PAIRS) + sorted(TRUE_PAIRS))
def test_hand_made_pairs(name):
    import ferreus_rbf_rs_amd as F
    a, ia, b, ib, stage = (FALSE_PAIRS.get(name) or TRUE_PAIRS[name])
    got = F.triangle_pair(a, ia, b, ib)
    want = X.triangle_pairs([a], [ia], [b], [ib])
    print(name, got, (bool(want[0][0]), X.STAGES[want[1][0]]))
    assert got == (name in TRUE_PAIRS, X.STAGES.index(stage))
    assert (bool(want[0][0]), int(want[1][0])) == got


def test_a_fan_around_a_vertex_has_no_intersection():
    import ferreus_rbf_rs_amd as F
    tris = [([APEX, RING[k], RING[(k + 1) % 6]], [0, 1 + k, 1 + (k + 1) % 6]) for k in range(6)]
    for i in range(6):
        for j in range(i + 1, 6):
            res, stage = F.triangle_pair(tris[i][0], tris[i][1], tris[j][0], tris[j][1])
            adjacent = (j - i) in (1, 5)
            assert not res and X.STAGES[stage] == ("shared_two" if adjacent else "moller"), (i, j, stage)


def random_pairs(n=20000, seed=11):
    """n pairs at three scales (edge lengths around 1, 0.1 and 0.01), a share of them forced to share 1 or 2 vertex ids,
    to have coincident corners under distinct ids, to hold a degenerate triangle, or to lie nearly in the plane of a
    triangle of edge length 1e3 (the only way past the Moeller test for a nearly coplanar pair: its parallel test
    compares unnormalised normals)."""
    rng = np.random.default_rng(seed)
    scale = np.array([1.0, 0.1, 0.01])[rng.integers(0, 3, n)]
    centre = rng.uniform(-1.0, 1.0, (n, 1, 3))
    ta = centre + scale[:, None, None] * rng.uniform(-0.6, 0.6, (n, 3, 3))
    tb = centre + scale[:, None, None] * rng.uniform(-0.6, 0.6, (n, 3, 3))
    ia = np.tile(np.arange(3), (n, 1))
    ib = np.tile(np.arange(3, 6), (n, 1))
    kind = rng.integers(0, 10, n)
    for k in range(n):
        if kind[k] in (1, 2):                    # share 1 or 2 ids (and their points), at random corners
            m = int(kind[k])
            ca, cb = rng.permutation(3)[:m], rng.permutation(3)[:m]
            tb[k, cb], ib[k, cb] = ta[k, ca], ia[k, ca]
        elif kind[k] in (3, 4):                  # coincident corners under distinct ids, up to 2e-9 apart
            m = int(kind[k]) - 2
            ca, cb = rng.permutation(3)[:m], rng.permutation(3)[:m]
            tb[k, cb] = ta[k, ca] + rng.uniform(-1e-9, 1e-9, (m, 3))
        elif kind[k] == 5:                       # a degenerate triangle
            tb[k, 2] = tb[k, 0] + 0.3 * (tb[k, 1] - tb[k, 0])
        elif kind[k] == 6:                       # a large triangle and one nearly in its plane
            ta[k] = centre[k] + 1e3 * np.array([[-1.0, -1.0, 0.0], [1.0, -1.0, 0.0], [0.0, 1.5, 0.0]])
            tb[k, :, 2] = centre[k, 0, 2] + rng.uniform(-6e-9, 6e-9, 3)
    return ta, ia, tb, ib


def test_random_pairs_equal_the_restatement():
    import ferreus_rbf_rs_amd as F
    ta, ia, tb, ib = random_pairs()
    want_res, want_stage = X.triangle_pairs(ta, ia, tb, ib)
    got = [F.triangle_pair(ta[k], ia[k], tb[k], ib[k]) for k in range(len(ta))]
    got_res, got_stage = np.array([g[0] for g in got]), np.array([g[1] for g in got])
    print("stages", dict(zip(X.STAGES, np.bincount(got_stage, minlength=7).tolist())), "true", int(got_res.sum()))
    assert np.array_equal(got_stage, want_stage)
    assert np.array_equal(got_res, want_res)
    assert (np.bincount(got_stage, minlength=7) > 0).all()          # every stage decides at least once
    assert got_res[got_stage == X.SHARED_CROSSING].any() and got_res[got_stage == X.GEOMETRIC_SHARED].any()


# ---- the restatement on the small noisy sphere: resolution 0.2, 0.2 * standard_normal(seed 3)
EXT = [0.0, 0.0, 0.0, 6.0, 6.0, 6.0]


@functools.lru_cache(maxsize=None)
def small_noisy_sphere():
    lat = R.Lattice(EXT, 0.2)
    w = lat.world(lat.node_ijk())
    field = np.linalg.norm(w - [3.0, 3.0, 3.0], axis=-1) - 2.0 + 0.2 * np.random.default_rng(3).standard_normal(lat.shape)
    return lat, field, X.extract(lat, field, 0.0, EXT)


def test_the_restatement_on_the_small_noisy_sphere():
    lat, field, got = small_noisy_sphere()
    v0, f0 = got["before"]
    counts = got["self_intersections"]
    print(len(f0), counts)
    assert counts["true_pairs"] > 0 and counts["triangles"] == len(got["ids"]) > 0
    assert counts["rolled_back"] > 0 and counts["cluster_vertices"] > 0
    assert counts["moller_pairs"] >= counts["true_pairs"] and counts["box_pairs"] > counts["moller_pairs"]
    # the raw mesh of the same field does not cross itself
    raw = C.extract(lat, field, 0.0, cluster=False)
    assert X.detect(raw["vertices"], raw["facets"], EXT)[1][3] == 0
    # after the rollback nothing is left, and no mesh edge has more than 2 faces
    ids, after, _ = X.detect(got["vertices"], got["facets"], EXT)
    assert len(ids) == 0 and after[3] == 0
    assert len(C.over_used(got["facets"])[0]) == 0
    assert len(got["facets"]) > len(f0) and len(got["vertices"]) > len(v0)
    # the detector does not depend on the order of the facets it is given
    perm = np.random.default_rng(0).permutation(len(f0))
    ids_p, counts_p, _ = X.detect(v0, f0[perm], EXT)
    assert np.array_equal(np.sort(perm[ids_p]), got["ids"])
    assert counts_p == [counts[n] for n in X.STAT_NAMES[:5]]
