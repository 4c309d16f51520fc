"""numpy restatement of the surface-following contract (DESIGN.md "Following the surface"), on top of
isosurface_restatement.py.

1. Bricks: the bounding box of E, shape (nk, nj, ni), is cut into bricks of B x B x B nodes from entry (0, 0, 0); the
   bricks at the high ends are partial.  A visited brick has every one of its nodes of E evaluated.
2. Seeds: world points clamped to the extents; the cell of a point is world_to_ijk (lattice.rs:98-121): with
   p = (world - lo) / spacing and U, V, W = EDGE_DELTAS[0], [2], [6], the coordinates q of p in that basis are
   ((p1 - p2 - p0) / 2, (-p2 - p0 - p1) / 2, -p2) and the cell's origin floor(q + 1e-9) mapped back to ijk.  The cell is
   the parallelepiped of U, V, W there; its 8 corners are the origin and the far ends of its 7 owned edges
   (get_edge_points::<8>), and every edge of the cell is a lattice edge between two of them.  The bricks that hold a
   corner of a seed's cell are visited.  (Seeds are not projected here: there is no field off the lattice.)
3. Mark rule: a lattice edge is known when both its ends lie in E, in visited bricks, with finite values; it is crossed
   when exactly one end has g < -1e-9.  A known crossed edge visits every brick that holds a node within
   (+-4, +-2, +-2) in (i, j, k) of either end.
4. Fixed point: the visited set is the smallest set of bricks that holds the seed bricks and is closed under rule 3.  It
   does not depend on the order of seeds, bricks or rounds (`order` below only permutes the sweep).
5. Result: the dense extraction of the field with NaN outside the visited bricks.
"""
from __future__ import annotations

import numpy as np

import isosurface_restatement as R

HALO = np.array([4, 2, 2], np.int64)
U, V, W = R.ED[0], R.ED[2], R.ED[6]


def brick_shape(lat, B):
    nk, nj, ni = lat.shape
    return (-(-nk // B), -(-nj // B), -(-ni // B))


def seed_cells(lat, seeds):
    """ijk (n, 3) of the cells of the seeds after the clamp to the extents, one row per distinct cell in order of first
    appearance."""
    s = np.asarray(seeds, np.float64).reshape(-1, 3)
    ext = lat.extents
    p = (np.minimum(np.maximum(s, ext[:3]), ext[3:]) - ext[:3]) / lat.spacing
    q = np.stack([(p[:, 1] - p[:, 2] - p[:, 0]) * 0.5, (-p[:, 2] - p[:, 0] - p[:, 1]) * 0.5, -p[:, 2]], -1)
    abc = np.floor(q + 1e-9).astype(np.int64)
    ijk = abc[:, [0]] * U + abc[:, [1]] * V + abc[:, [2]] * W
    _, first = np.unique(ijk, axis=0, return_index=True)
    return ijk[np.sort(first)]


def seed_bricks(lat, seeds, B):
    """(nbz, nby, nbx) bool: the bricks that hold a corner of a seed's cell."""
    out = np.zeros(brick_shape(lat, B), bool)
    c = ((seed_cells(lat, seeds) - lat.lo)[:, None, :] + R.CORNERS[None, :, :]).reshape(-1, 3)
    nk, nj, ni = lat.shape
    ok = ((c >= 0) & (c < np.array([ni, nj, nk]))).all(-1)
    c = c[ok] // B
    out[c[:, 2], c[:, 1], c[:, 0]] = True
    return out


def node_mask(lat, bricks, B):
    """(nk, nj, ni) bool: the nodes of the box that lie in the given bricks."""
    nk, nj, ni = lat.shape
    return np.repeat(np.repeat(np.repeat(bricks, B, 0), B, 1), B, 2)[:nk, :nj, :ni]


def _crossed_ends(lat, g, known):
    """Box coordinates (m, 3) as (i, j, k) of both ends of every known crossed edge."""
    nk, nj, ni = lat.shape
    inside = g < -R.EPS_INSIDE
    ends = []
    for l in range(7):                                    # every edge once, from its owner
        di, dj, dk = (int(x) for x in R.ED[l])
        # owner p over [a0, a1) per axis such that p + d stays in the box
        sl_p = tuple(slice(max(-d, 0), n + min(-d, 0)) for d, n in ((dk, nk), (dj, nj), (di, ni)))
        sl_q = tuple(slice(max(d, 0), n + min(d, 0)) for d, n in ((dk, nk), (dj, nj), (di, ni)))
        hit = known[sl_p] & known[sl_q] & (inside[sl_p] != inside[sl_q])
        k, j, i = np.nonzero(hit)
        p = np.stack([i + sl_p[2].start, j + sl_p[1].start, k + sl_p[0].start], -1)
        ends += [p, p + R.ED[l]]
    return np.concatenate(ends) if ends else np.zeros((0, 3), np.int64)


def visited_bricks(lat, field, isovalue, seeds, B=8, order=None, return_rounds=False):
    """(nbz, nby, nbx) bool: the fixed point of rule 4.  order: a numpy Generator; the bricks a sweep adds are then taken
    in a shuffled order and only a random half of them per sweep (the fixed point must not notice)."""
    f = np.asarray(field, np.float64).reshape(lat.shape)
    g = f - isovalue
    ijk = lat.node_ijk()
    valid = lat.inE & ((ijk.sum(-1) % 2) == 0) & np.isfinite(g)
    nk, nj, ni = lat.shape
    hi = np.array([ni, nj, nk]) - 1
    visited = seed_bricks(lat, seeds, B)
    rounds = 0
    while True:
        known = valid & node_mask(lat, visited, B)
        ends = _crossed_ends(lat, g, known)
        new = np.zeros_like(visited)
        if len(ends):
            lo_b = np.maximum(ends - HALO, 0) // B
            hi_b = np.minimum(ends + HALO, hi) // B
            # the bricks of the halo box: at most 3 x 2 x 2 (B >= 4), so lo, lo + 1, hi cover every one
            for bi in (lo_b[:, 0], np.minimum(lo_b[:, 0] + 1, hi_b[:, 0]), hi_b[:, 0]):
                for bj in (lo_b[:, 1], hi_b[:, 1]):
                    for bk in (lo_b[:, 2], hi_b[:, 2]):
                        new[bk, bj, bi] = True
        new &= ~visited
        if not new.any():
            break
        if order is not None:
            idx = np.argwhere(new)
            order.shuffle(idx)
            idx = idx[:max(1, len(idx) // 2)]
            new = np.zeros_like(visited)
            new[idx[:, 0], idx[:, 1], idx[:, 2]] = True
        visited |= new
        rounds += 1
    return (visited, rounds) if return_rounds else visited


def masked_field(lat, field, visited, B=8):
    """The field with NaN outside the visited bricks."""
    f = np.array(field, np.float64).reshape(lat.shape)
    f[~node_mask(lat, visited, B)] = np.nan
    return f


def nodes_evaluated(lat, visited, B=8):
    ijk = lat.node_ijk()
    return int((lat.inE & ((ijk.sum(-1) % 2) == 0) & node_mask(lat, visited, B)).sum())


def extract(lat, field, isovalue, seeds, B=8):
    """(vertices, facets) of rule 5."""
    return R.extract(lat, masked_field(lat, field, visited_bricks(lat, field, isovalue, seeds, B), B), isovalue)
