"""The clouds, weights and handles of the far-field tests: the smallest at which each pass can go wrong.  A plain helper
module (no tests); tests/test_far_field_reference_host.py and tests/test_gpu_far_field_passes.py share it."""
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


def make_tree(pts, order, leaf_limit, env=None, kernel=(0, 1.0, 1.0), host_only=False, sparse=True, epsilon=1e-7):
    with environment(env or {}):
        return F.FmmTree(pts, order, F.KernelParams(F.KernelType(kernel[0]), base_range=kernel[1], total_sill=kernel[2]), True,
                         sparse, params=F.FmmParams(leaf_limit, F.M2LCompressionType(ACA), epsilon, 1024), host_only=host_only)


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
