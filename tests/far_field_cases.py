"""The clouds, weights and handles of the far-field tests: the smallest at which each pass can go wrong.  A plain helper
module (no tests); tests/test_far_field_reference_host.py, tests/test_gpu_far_field_passes.py,
tests/test_gpu_far_field_orders.py and tests/test_gpu_wx_passes.py share it."""
import contextlib
import os

import numpy as np

import ferreus_rbf_rs_amd as F
from conftest import clustered_points

GRID = 2.0 ** -30
ACA = 2
# the steps of four and the batches of 64 of P2M, the 64-lane batches of L2P
POPULATIONS = ([1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 47, 48, 49] + list(range(60, 69)) +
               [127, 128, 129, 191, 192, 193, 255, 256, 257])
POPULATIONS_LIMIT = 257


_CACHE = {}


def cached(key, make):
    """What several cases share (clouds, handles, references), built once; key[0] names the kind."""
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def drop_cached(keep=()):
    """Forget everything but the kinds listed: handles and references go when the cases that share them are done."""
    for key in [k for k in _CACHE if k[0] not in keep]:
        del _CACHE[key]


@contextlib.contextmanager
def environment(env):
    """The switches and table options are read when a handle is created."""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


NO_COMPRESSION = 0


def make_tree(pts, order, leaf_limit, env=None, kernel=(0, 1.0, 1.0), host_only=False, sparse=True, epsilon=1e-7,
              compression=ACA):
    with environment(env or {}):
        return F.FmmTree(pts, order, F.KernelParams(F.KernelType(kernel[0]), base_range=kernel[1], total_sill=kernel[2]), True,
                         sparse, params=F.FmmParams(leaf_limit, F.M2LCompressionType(compression), epsilon, 1024),
                         host_only=host_only)


def on_grid(x):
    return np.round(np.asarray(x) / GRID) * GRID


def populations_cloud():
    """(points, counts[4, 4, 4]): 3-D, the tree of [0, 1]^3 (centre 0.5, radius 0.501) has depth exactly 2 under the leaf
    limit 257: every level-1 octant holds more than 257 points, no level-2 cell does.  Points on the 2^-30 grid, strictly
    inside their level-2 cell."""
    rng = np.random.default_rng(20260301)
    counts = np.full((4, 4, 4), -1, dtype=np.int64)
    cells = [(i, j, k) for i in range(4) for j in range(4) for k in range(4)]
    big = [255, 256, 257, 191, 192, 193, 127, 128]                 # one per octant first: every octant splits
    rest = [c for c in POPULATIONS if c not in big]
    for o, c in enumerate(big):
        at = (2 * (o & 1) + 1, 2 * ((o >> 1) & 1), 2 * ((o >> 2) & 1) + 1)
        counts[at] = c
    free = [c for c in cells if counts[c] < 0]
    rng.shuffle(free)
    for at, c in zip(free, rest):
        counts[tuple(at)] = c
    others = [tuple(c) for c in free[len(rest):]]
    for n, at in enumerate(others):
        counts[at] = 0 if n < 2 else rng.integers(1, 65)            # two cells without points, the others at most 64
    for o in range(8):
        sub = counts[2 * (o & 1):2 * (o & 1) + 2, 2 * ((o >> 1) & 1):2 * ((o >> 1) & 1) + 2, 2 * ((o >> 2) & 1):2 * ((o >> 2) & 1) + 2]
        assert sub.sum() > POPULATIONS_LIMIT
    radius, side = 0.501, 2 * 0.501 / 4
    pts = []
    for at in cells:
        lo = 0.5 - radius + np.array(at) * side
        pts.append(on_grid(lo + side * (0.06 + 0.88 * rng.random((counts[at], 3)))))
    pts = np.concatenate(pts)
    assert pts.min() > 0 and pts.max() < 1                         # the extents: floor 0, ceil 1 on every axis
    assert len(np.unique(pts, axis=0)) == len(pts)
    return pts, counts


def assert_populations(t, counts):
    """The prescribed populations are the leaves (through leaf_sources), depth exactly 2."""
    s = t.stats()
    assert s.depth == 2
    keys, leaf = t.cells()
    ptr, _ = t.leaf_sources()
    pops = np.diff(ptr)
    level = (keys & np.uint64(0x7FFF)).astype(np.int64)
    assert (leaf[level == 2] == 1).all() and (leaf[level < 2] == 0).all()
    got = sorted(pops[level == 2].tolist())
    assert got == sorted(counts.ravel().tolist()), (got, sorted(counts.ravel().tolist()))
    assert set(POPULATIONS) <= set(got) and 0 in got


def random_cloud(d, n, seed):
    return np.unique(on_grid(0.01 + 0.98 * np.random.default_rng(seed).random((n, d))), axis=0)


def lattice(rng, m, d, per_cell):
    """lattice() of test_gpu_m2l_pairs.py."""
    g = np.stack(np.meshgrid(*[np.arange(m)] * d, indexing="ij"), -1).reshape(-1, d)[:, None, :]
    return ((g + 0.15 + 0.7 * rng.random((m ** d, per_cell, d))).reshape(-1, d)) / m


LATTICE_LIMIT = 6
# level-2 parents (coordinates 0..3) of lattice8 and how many of their eight children keep their points
# (all with x = 3 and away from the cells of lattice_sources: the cells with x <= 5 keep their full V lists)
LATTICE8_PARENTS = {(3, 1, 0): 1, (3, 1, 3): 2, (3, 1, 1): 3, (3, 1, 2): 5, (3, 2, 1): 7}


def lattice8_cloud():
    pts = lattice(np.random.default_rng(50), 8, 3, 3)
    cell = np.floor(pts * 8).astype(np.int64)
    keep = np.ones(len(pts), dtype=bool)
    for par, n_keep in LATTICE8_PARENTS.items():
        for o in range(n_keep, 8):
            child = (2 * par[0] + (o & 1), 2 * par[1] + ((o >> 1) & 1), 2 * par[2] + ((o >> 2) & 1))
            keep &= ~(cell == np.array(child)).all(axis=1)
    # A parent splits only above six points: the parent with two children gets a fourth point in one of them (4 + 3), and
    # the only child of the parent with one holds seven, so that child splits once more (the one place of depth 4).
    rng = np.random.default_rng(51)
    extra = [(np.array(c) + 0.15 + 0.7 * rng.random((k, 3))) / 8 for c, k in (((6, 2, 0), 4), ((6, 2, 6), 1))]
    return np.concatenate([pts[keep]] + extra)


def lattice16_cloud():
    return lattice(np.random.default_rng(50), 16, 3, 3)


def assert_lattice8(t, geo):
    assert t.stats().depth == 4 and (geo.level == 4).sum() <= 8          # depth 3 but for the children of one cell
    counts = sorted({len(geo.children[c]) for c in range(geo.C) if geo.level[c] == 2})
    assert counts == [1, 2, 3, 5, 7, 8], counts
    vp, _ = geo.lists["V"]
    assert (np.diff(vp)[geo.level == 3] == 189).any()


def clustered_cloud():
    return np.unique(clustered_points(np.random.default_rng(77), 6000, 3), axis=0)


CLUSTERED_LIMIT = 30


# ---- the stage-2 kernel instance of every order: debug_m2l_s2_plan() = (ga, gb, ce, co, ya, yb) under BBFMM_M2L_S2_AXES = 1
# and = 2 (tests/test_far_field_reference_host.py enumerates host-only handles against this table and explains it)
_S2_PLANS = {
    3: {2: ((1, 1, 1, 1, 0, 0), (2, 2, 1, 1, 1, 1)), 3: ((2, 2, 1, 1, 0, 0), (2, 2, 1, 1, 1, 1)),
        4: ((2, 2, 1, 1, 0, 0), (2, 2, 1, 1, 1, 1)), 5: ((5, 4, 1, 1, 0, 0), (5, 4, 1, 1, 3, 2)),
        6: ((7, 7, 1, 1, 0, 0), (8, 8, 1, 1, 4, 4)), 7: ((13, 10, 1, 1, 0, 0), (13, 10, 1, 1, 7, 6)),
        8: ((8, 8, 2, 2, 0, 0), (8, 8, 2, 2, 4, 4)), 9: ((13, 11, 2, 2, 0, 0), (14, 11, 2, 2, 8, 6)),
        10: ((8, 8, 4, 4, 0, 0), (8, 8, 4, 4, 4, 4))},
    2: {**{p: ((1, 1, 1, 1, 0, 0), (2, 2, 1, 1, 1, 1)) for p in (2, 3, 4, 5)},
        **{p: ((2, 2, 1, 1, 0, 0), (2, 2, 1, 1, 1, 1)) for p in (6, 7, 8)},
        **{p: ((4, 4, 1, 1, 0, 0), (4, 4, 1, 1, 2, 2)) for p in (9, 10)}, 11: ((5, 4, 1, 1, 0, 0), (5, 4, 1, 1, 3, 2)),
        **{p: ((7, 7, 1, 1, 0, 0), (8, 8, 1, 1, 4, 4)) for p in (12, 13, 14)},
        **{p: ((8, 8, 1, 1, 0, 0), (8, 8, 1, 1, 4, 4)) for p in (15, 16)}}}
S2_PLANS = {(d, p, axes): plans[axes - 1] for d, rows in _S2_PLANS.items() for p, plans in rows.items() for axes in (1, 2)}
# the instances (ga, gb, ya, yb) of 3-D orders 6, 8, 9 and 10, which orders 3, 4, 5 and 7 never select: what the GPU cases of
# tests/test_gpu_far_field_orders.py cover between them
GPU_INSTANCES = {(7, 7, 0, 0), (8, 8, 0, 0), (13, 11, 0, 0), (8, 8, 4, 4), (14, 11, 8, 6)}


def assert_s2_plan(t, d, order, env=None):
    """The handle runs the instance the table names for its axes (all zeros without stage-2 pairs); returns the instance."""
    plan = t.debug_m2l_s2_plan()
    if (env or {}).get("BBFMM_M2L_S2_PAIRS") == "0" or d < 2:
        assert plan == (0,) * 6 and not t.debug_m2l_pairs(stage=2)[0]
        return None
    axes = t.debug_m2l_pairs_axes(stage=2)[0]["axes"]
    if "BBFMM_M2L_S2_AXES" in (env or {}):
        assert axes == int(env["BBFMM_M2L_S2_AXES"])
    assert axes in (1, 2) and plan == S2_PLANS[d, order, axes], (plan, d, order, axes)
    return plan[0], plan[1], plan[4], plan[5]


# the columns of lattice_sources that on lattice8 reach every one of the 316 transfer vectors at level 3 between them:
# FEW_COLUMNS (below) misses (-1, -3, 3) and (-1, 3, -3), which the interior cells (2, 3, 2) and (2, 2, 3) supply
EVERY_VECTOR_COLUMNS = [0, 5, 10, 13, 14, 16, 18]


# ---- two dimensions and one
def lattice2d_cloud():
    """16 x 16 cells of three points: depth 4, 256 leaves, the four classes with interior, edge and corner cells."""
    return lattice(np.random.default_rng(60), 16, 2, 3)


def assert_lattice2d(t, geo):
    at4 = geo.level == 4
    assert t.stats().depth == 4 and at4.sum() == 256 and geo.is_leaf[at4].all()
    assert set(geo.octant[at4].tolist()) == set(range(4))
    assert (np.diff(geo.lists["V"][0])[at4] == 27).any()               # the full V list of two dimensions


def clustered2d_cloud():
    return np.unique(clustered_points(np.random.default_rng(78), 3000, 2), axis=0)


LINE_LIMIT = 5                                                         # a level-3 cell holds six points and splits
LINE_CLUSTER = 5                                                       # the level-4 cell that holds the cluster


def line_cloud():
    """One dimension: 16 cells of three points and three more in one of them, which therefore splits once more: 51 points,
    the least for a uniform level 4 (three points per cell as on the lattices) beside one deeper cell."""
    pts = lattice(np.random.default_rng(61), 16, 1, 3)
    extra = (LINE_CLUSTER + 0.15 + 0.7 * np.random.default_rng(62).random((3, 1))) / 16
    return np.concatenate([pts, extra])


def assert_line(t, geo):
    """Depth at least 4; a cell of either parity with the full V list of one dimension (three cells: the offsets -2, 2, 3
    from an even cell and -3, -2, 2 from an odd one, so no single cell sees all four vectors, the two together do); mixed
    levels next to the cluster."""
    at4 = geo.level == 4
    assert t.stats().depth >= 4 and at4.sum() == 16 and t.stats().n_w > 0
    full = at4 & (np.diff(geo.lists["V"][0]) == 3)
    assert set(geo.octant[full].tolist()) == {0, 1}
    tgt_full = full[geo.v_tgt]
    assert set(geo.v_tidx[tgt_full].tolist()) == set(geo.v_tidx.tolist()) and len(set(geo.v_tidx.tolist())) == 4


def leaf_at(geo, level, anchor):
    c = np.nonzero((geo.level == level) & (geo.anchor == np.array(anchor)).all(axis=1))[0]
    assert len(c) == 1 and geo.is_leaf[c[0]]
    return int(c[0])


def lattice2d_leaves(geo):
    """A corner, an edge and an interior leaf (all 27 vectors) of each of the four classes: twelve leaves."""
    ends = (0, 15)
    at = [kind(b0, b1) for kind in (lambda b0, b1: (ends[b0], ends[b1]), lambda b0, b1: (ends[b0], 6 + b1),
                                    lambda b0, b1: (6 + b0, 8 + b1)) for b1 in (0, 1) for b0 in (0, 1)]
    leaves = [leaf_at(geo, 4, a) for a in at]
    assert all(sorted(geo.octant[leaves[4 * k:4 * k + 4]].tolist()) == [0, 1, 2, 3] for k in range(3))
    n_v = np.diff(geo.lists["V"][0])[leaves]
    assert (n_v[8:] == 27).all() and (n_v[:8] < 27).all()
    return leaves


def line_leaves(geo):
    """Both ends and an interior leaf of the uniform level."""
    return [leaf_at(geo, 4, (0,)), leaf_at(geo, 4, (15,)), leaf_at(geo, 4, (10,))]


def one_leaf_weights(geo, n, leaves, seed):
    """One right-hand side per leaf, nonzero on that leaf's points alone."""
    return np.concatenate([leaf_weights(geo, n, leaf, 1, seed + k) for k, leaf in enumerate(leaves)], axis=1)


def live_cells(geo, w):
    """Cells with a nonzero weight below them, from the geometry alone."""
    live = np.zeros(geo.C, dtype=bool)
    for c in np.nonzero(np.diff(geo.src_ptr) > 0)[0]:
        live[c] = np.any(w[geo.src_idx[geo.src_ptr[c]:geo.src_ptr[c + 1]]] != 0)
    for c in np.argsort(-geo.level, kind="stable"):
        if live[c] and geo.parent[c] >= 0:
            live[geo.parent[c]] = True
    return live


def assert_every_vector_is_live(geo, w):
    """The condition on every M2L case: at the deepest level where all classes are present and whose V lists between them
    take every transfer vector of the tree (the uniform level of the lattices and of the line: the few cells below it
    see a handful of vectors whatever the weights), the pairs with a live source hit every one of those vectors."""
    every = set(geo.v_tidx.tolist())
    at = geo.level[geo.v_tgt]
    levels = [lv for lv in range(2, geo.depth + 1) if len(set(geo.octant[geo.level == lv].tolist())) == 1 << geo.d
              and set(geo.v_tidx[at == lv].tolist()) == every]
    assert levels, "no level takes every transfer vector"
    live = live_cells(geo, w)
    hit = set(geo.v_tidx[(at == levels[-1]) & live[geo.v_src]].tolist())
    assert hit == every, (levels[-1], len(hit), len(every))
    return levels[-1]


# ---- two-level clouds: the W lists of level-1 leaves
# The unit cube (square, interval) is split once; the octants of `refined` hold more points than the limit (the largest
# prescribed population) and split once more into level-2 leaves that all hold points, the others are level-1 leaves with
# the prescribed populations.  Every octant touches every other one, so a level-1 leaf has in its W list the children of
# each refined octant that do not touch it: 4 of a face neighbour, 6 of an edge neighbour, 7 of a vertex neighbour (2 and 3
# in two dimensions, the far child in one).  A level-1 cell has no V list; with more than one refined octant the children
# of different refined octants are in each other's V lists (M2L is live between level-2 cells, never into a level-1 leaf).
# Octant o: bit a = the upper half along axis a.  {dimension: {name: (refined octants, {octant: population})}}
TWO_LEVEL = {
    3: {"w4-7": ((7,), {0: 1, 1: 2, 2: 7, 3: 8, 4: 9, 5: 47, 6: 48}),                   # W lists of 7, 6, 6, 4, 6, 4, 4
        "w8-12": ((0, 3), {1: 49, 2: 63, 4: 64, 5: 65, 6: 66, 7: 33}),                  # 8, 8, 11, 12, 12, 11
        "w14-19": ((1, 3, 5), {0: 95, 2: 96, 4: 97, 6: 127, 7: 128}),                   # 16, 17, 17, 19, 14
        "w14-19-small": ((1, 3, 5), {0: 66, 2: 1, 4: 9, 6: 47, 7: 8}),
        "w10": ((0, 7), {1: 129, 2: 255, 3: 256, 4: 257, 5: 511, 6: 512}),              # 10 throughout
        "w8-12-big": ((0, 3), {1: 513, 2: 257, 4: 129, 5: 66, 6: 9, 7: 2})},
    2: {"w2-3": ((3,), {0: 49, 1: 257, 2: 8}),                                          # 3, 2, 2
        "w7": ((1, 2, 3), {0: 513}),
        "w4-5": ((0, 3), {1: 66, 2: 129})},                                             # 2 + 2 = 4 each
    1: {"low": ((1,), {0: 130}), "high": ((0,), {1: 513})}}
# what the 3-D layouts must show between them (tests/test_far_field_reference_host.py asserts it): the waves of a job (8),
# the rows of a chunk job (48) and of a whole-leaf job (256), 64-lane batches, the source tiles and plan_targets passes
TWO_LEVEL_POPULATIONS = {1, 2, 7, 8, 9, 47, 48, 49, 63, 64, 65, 66, 95, 96, 97, 127, 128, 129, 255, 256, 257, 511, 512, 513}
W_CELLS_BY_BITS = {3: {1: 4, 2: 6, 3: 7}, 2: {1: 2, 2: 3}, 1: {1: 1}}
SMALL_TWO_LEVEL = ("w4-7", "w8-12", "w14-19-small")                  # 3-D layouts whose level-1 leaves hold at most 66 points


def two_level_limit(d, name):
    return max(TWO_LEVEL[d][name][1].values())


def two_level_w_length(d, name, octant):
    """The W-list length of the level-1 leaf in `octant`, by the count above."""
    return sum(W_CELLS_BY_BITS[d][bin(octant ^ q).count("1")] for q in TWO_LEVEL[d][name][0])


def expected_wx_jobs(d, name, n_cu=256):
    """debug_wx_jobs() restated from the layout: add_w_jobs cuts a W list at 8 cells; a chunk job has at most 48 rows and 16
    cells, a whole-leaf job at most 256 rows, both in equal parts; the cells of a whole-leaf job halve from 16 until there are
    four jobs per compute unit, down to one cell on trees this small."""
    leaves = [(n, two_level_w_length(d, name, o)) for o, n in TWO_LEVEL[d][name][1].items()]
    ceil = lambda a, b: -(-a // b)
    part = lambda n, k: max((n * (i + 1)) // k - (n * i) // k for i in range(k))
    cells = 16
    while cells > 1 and sum(ceil(n, 256) * ceil(w, cells) for n, w in leaves) < 4 * n_cu:
        cells //= 2
    return {"n_w_jobs": sum(ceil(w, 8) for _, w in leaves),
            "n_wx_jobs": sum(ceil(n, 48) * ceil(w, 16) for n, w in leaves),
            "n_wxl_jobs": sum(ceil(n, 256) * ceil(w, cells) for n, w in leaves),
            "max_rows_wx": max(part(n, ceil(n, 48)) for n, _ in leaves),
            "max_rows_wxl": max(part(n, ceil(n, 256)) for n, _ in leaves),
            "max_cells_wx": max(part(w, ceil(w, 16)) for _, w in leaves),
            "max_cells_wxl": max(part(w, ceil(w, cells)) for _, w in leaves),
            "max_cells_w": max(min(w, 8) for _, w in leaves)}


def two_level_cloud(d, name):
    """Points on the 2^-30 grid, strictly inside their cells of the root box of centre 0.5 and radius 0.501."""
    refined, pops = TWO_LEVEL[d][name]
    assert sorted(refined + tuple(pops)) == list(range(1 << d)) and len(set(pops.values())) == len(pops)
    limit = two_level_limit(d, name)
    assert limit >= 2
    rng = np.random.default_rng([d, limit, len(name), sum(pops.values())])
    radius = 0.501
    pts = []
    for o in range(1 << d):
        lo = 0.5 - radius + radius * np.array([(o >> a) & 1 for a in range(d)])
        if o in pops:
            boxes = [(lo, radius, pops[o])]
        else:                                                         # limit + 2^d points: more than the limit, no child above it
            total, nch = limit + (1 << d), 1 << d
            boxes = [(lo + radius / 2 * np.array([(ch >> a) & 1 for a in range(d)]), radius / 2,
                      total // nch + (1 if ch < total % nch else 0)) for ch in range(nch)]
            assert all(1 <= b[2] <= limit for b in boxes)
        for blo, side, count in boxes:
            pts.append(on_grid(blo + side * (0.06 + 0.88 * rng.random((count, d)))))
    pts = np.concatenate(pts)
    pts = pts[rng.permutation(len(pts))]
    assert pts.min() > 0 and pts.max() < 1 and len(np.unique(pts, axis=0)) == len(pts)
    return np.ascontiguousarray(pts)


def assert_two_level(t, geo, d, name):
    """From the handle: depth 2, the level-1 leaves with their populations and W-list lengths, the refined octants with 2^d
    leaves that hold points, no V list at level 1, X = W^T live.  Returns {octant: cell} of the level-1 leaves."""
    refined, pops = TWO_LEVEL[d][name]
    s = t.stats()
    assert s.depth == 2 and s.n_x == s.n_w > 0, (s.depth, s.n_x, s.n_w)
    octant_of = {c: int(sum(int(geo.anchor[c][a]) << a for a in range(d))) for c in range(geo.C) if geo.level[c] == 1}
    assert sorted(octant_of.values()) == list(range(1 << d))
    n_pts, n_w, n_v = np.diff(geo.src_ptr), np.diff(geo.lists["W"][0]), np.diff(geo.lists["V"][0])
    leaves = {}
    for c, o in octant_of.items():
        assert n_v[c] == 0
        if o in pops:
            assert geo.is_leaf[c] and n_pts[c] == pops[o] and n_w[c] == two_level_w_length(d, name, o), (o, n_pts[c], n_w[c])
            leaves[o] = c
        else:
            ch = geo.children[c]
            assert not geo.is_leaf[c] and len(ch) == 1 << d and geo.is_leaf[ch].all()
            assert (n_pts[ch] > 0).all() and (n_pts[ch] <= two_level_limit(d, name)).all() and (n_w[ch] == 0).all()
    assert n_w.sum() == sum(n_w[c] for c in leaves.values())       # no other cell has a W list
    return leaves


def inside_copies(geo, leaf, pts, count, seed):
    """`count` copies of points of a leaf displaced per axis by grid multiples of 1/64 to 1/16 of the leaf's side and kept
    at least an eighth of the side inside it (count rows, cycling through the points)."""
    rng = np.random.default_rng(seed)
    rows = np.arange(count) % len(pts)
    side = geo.lengths[leaf]
    off = np.floor(rng.uniform(side / 64, side / 16, (count, geo.d)) / GRID) * GRID * rng.choice([-1.0, 1.0], (count, geo.d))
    lo, hi = geo.centres[leaf] - side / 2, geo.centres[leaf] + side / 2
    out = on_grid(np.clip(pts[rows] + off, lo + side / 8, hi - side / 8))
    assert (out > lo).all() and (out < hi).all()
    return out


def w_cell_weights(geo, n, leaf, K, seed):
    """Signed weights on the points under the cells of the W list of `leaf`, zero elsewhere."""
    wp, wi = geo.lists["W"]
    w = np.zeros((n, K))
    rng = np.random.default_rng(seed)
    stack = [int(c) for c in wi[wp[leaf]:wp[leaf + 1]]]
    while stack:
        c = stack.pop()
        stack += [int(x) for x in geo.children[c]]
        rows = geo.src_idx[geo.src_ptr[c]:geo.src_ptr[c + 1]]
        if geo.is_leaf[c]:
            w[rows] = rng.standard_normal((len(rows), K))
    return w


def dense_weights(n, K, seed):
    return np.random.default_rng(seed).standard_normal((n, K))


def lattice_sources(m):
    """Lattice cells of the sparse weights, grouped by right-hand side: one corner, one edge, one face and one interior cell
    (all 189 vectors) in each of the eight octant classes (bit a of the class = parity of coordinate a), 32 cells in 20
    right-hand sides.  The V lists of the 7^3 targets around a cell overlap unless two cells lie seven or more cells apart
    along an axis, so only cells on opposite faces x = 0, x = m - 1 share a right-hand side; the interior cells stand alone."""
    ends = (0, m - 1)
    kinds = [lambda b: (ends[b[0]], ends[b[1]], ends[b[2]]),            # corner
             lambda b: (ends[b[0]], ends[b[1]], 2 + b[2]),              # edge
             lambda b: (ends[b[0]], 4 + b[1], 4 + b[2])]                # face
    cols = []
    for kind in kinds:
        cols += [[kind((0, b1, b2)), kind((1, 1 - b1, 1 - b2))] for b2 in (0, 1) for b1 in (0, 1)]
    cols += [[(2 + (c & 1), 2 + ((c >> 1) & 1), 2 + ((c >> 2) & 1))] for c in range(8)]
    cells = [c for col in cols for c in col]
    classes = [(c[0] & 1) + 2 * (c[1] & 1) + 4 * (c[2] & 1) for c in cells]
    assert len(set(cells)) == 32 and all(sorted(classes[8 * k:8 * k + 8]) == list(range(8)) for k in range(4))
    assert all(max(abs(a - b) for a, b in zip(*col)) >= 7 for col in cols if len(col) == 2)
    return cols


# one right-hand side of each kind, together one cell in each of the eight classes: what the host walk of the tables and
# the 16^3 lattice run (a walk costs seconds per right-hand side; the 16^3 restatement grows with cells x right-hand sides)
FEW_COLUMNS = [0, 5, 10, 13, 18]


def sparse_lattice_weights(pts, m, seed, columns=None):
    """Nonzero only at the points of the cells of lattice_sources: every target cell at the leaf level receives exactly one
    (source, vector) contribution per right-hand side, so a failure names its level, class and vector."""
    cols = lattice_sources(m)
    cols = cols if columns is None else [cols[k] for k in columns]
    rng = np.random.default_rng(seed)
    at = np.floor(pts * m).astype(np.int64)
    w = np.zeros((len(pts), len(cols)))
    for k, col in enumerate(cols):
        for c in col:
            rows = np.nonzero((at == np.array(c)).all(axis=1))[0]
            assert len(rows) == 3
            w[rows, k] = rng.standard_normal(len(rows))
    return w


def leaf_weights(geo, n, leaf, K, seed):
    """Signed weights on the points of one leaf, zero elsewhere."""
    w = np.zeros((n, K))
    rows = geo.src_idx[geo.src_ptr[leaf]:geo.src_ptr[leaf + 1]]
    w[rows] = np.random.default_rng(seed).standard_normal((len(rows), K))
    return w
