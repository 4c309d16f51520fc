"""numpy restatement of the clip-and-clean contract (DESIGN.md "Isosurfaces on the RMT lattice", clip and clean): what
ferreus_rmt's build_isosurface runs after extraction with BoundaryClosure::None (isosurface.rs:1009-1038),
clean_mesh(clip_mesh_to_aabb(raw)).

Tolerance (bbox_eps, aabb_clipping.rs:40-48): eps = 1e-10 * max(|hi - lo|, 1.0).

Clip (clip_mesh_to_aabb, aabb_clipping.rs:55-105), per facet in facet order: Sutherland-Hodgman against XMin, XMax, YMin,
YMax, ZMin, ZMax (clip_polygon_to_plane, aabb_clipping.rs:238-274); a point is inside a plane with slack eps
(point_inside_plane, :216-225); a crossing point is emitted only where the inside flags of prev and curr differ, at
t = 0 if |da| <= eps, 1 if |db| <= eps, else (c - a) / (b - a) (segment_plane_t, :186-213), as prev + t * (curr - prev)
(interpolate_points, :132-138), then snap_to_plane (:171-181) and snap_near_bbox (:148-168); every kept point goes through
snap_near_bbox too; a polygon of fewer than 3 points is dropped, the others are appended unwelded and fanned as
(0, k - 1, k) (:95-101).

Clean (clean_mesh, mesh_cleanup.rs:32-96): weld (push_dedup_point, :203-232, cell key round(v / max(eps, 1e-12)) with
Rust's round half away from zero, :194-197); collapsed facets (:57-59); tiny facets |ab x ac|^2 <= eps^4 (:76-81);
duplicates by sorted id triple, the first kept (:83-87); components of fewer than MIN_CONNECTED_COMPONENT_FACETS = 2
facets under vertex connectivity (:102-160), which are the facets none of whose vertices another surviving facet uses;
compaction in order of first use (compact_kept_facets, :166-191).

The weld of the contract is `weld_components`: two vertices are linked when |p - q|^2 <= eps^2 and a vertex's
representative is the lowest-index vertex of its linked component.  `weld_greedy` is the reference's literal insertion;
the two agree whenever every vertex lies within eps of its representative (`unambiguous` checks that, with margin).
"""
from __future__ import annotations

import numpy as np

import isosurface_restatement as R

FINISH_STATS = ("facets_in", "straddling", "outside", "vertices_emitted", "welded", "weld_loose", "collapsed", "tiny",
                "duplicate", "lone")


def bbox_eps(extents):
    e = np.asarray(extents, np.float64)
    d = e[3:] - e[:3]
    return 1.0e-10 * max(float(np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])), 1.0)


# ---- clip
def _snap_near(p, lo, hi, eps):
    for a in range(3):
        if abs(p[a] - lo[a]) <= eps:
            p[a] = lo[a]
        if abs(p[a] - hi[a]) <= eps:
            p[a] = hi[a]
    return p


def _inside_plane(p, plane, lo, hi, eps):
    a = plane >> 1
    return p[a] <= hi[a] + eps if plane & 1 else p[a] >= lo[a] - eps


def clip_triangle(tri, extents, eps=None):
    """(points, corners) of one triangle: the polygon the six planes leave ([] if fewer than 3 points); corners: the
    corner a point is a kept copy of, -1 for a point made on a plane."""
    e = [float(x) for x in np.asarray(extents, np.float64)]
    lo, hi = e[:3], e[3:]
    eps = bbox_eps(extents) if eps is None else eps
    poly = [([float(x) for x in p], k) for k, p in enumerate(np.asarray(tri, np.float64).reshape(3, 3))]
    for plane in range(6):
        a = plane >> 1
        c = hi[a] if plane & 1 else lo[a]
        out = []
        if poly:
            prev = poly[-1][0]
            prev_in = _inside_plane(prev, plane, lo, hi, eps)
            for curr, src in poly:
                curr_in = _inside_plane(curr, plane, lo, hi, eps)
                if curr_in != prev_in:
                    da, db = prev[a] - c, curr[a] - c
                    t = None
                    if abs(da) <= eps:
                        t = 0.0
                    elif abs(db) <= eps:
                        t = 1.0
                    elif (da < 0.0) != (db < 0.0):
                        t = (c - prev[a]) / (curr[a] - prev[a])
                    if t is not None:
                        q = [prev[x] + t * (curr[x] - prev[x]) for x in range(3)]
                        q[a] = c
                        out.append((_snap_near(q, lo, hi, eps), -1))
                if curr_in:
                    out.append((_snap_near(list(curr), lo, hi, eps), src))
                prev, prev_in = curr, curr_in
        poly = out
        if len(poly) < 3:
            break
    if len(poly) < 3:
        return np.zeros((0, 3)), np.zeros(0, np.int64)
    return np.array([p for p, _ in poly]), np.array([s for _, s in poly], np.int64)


def clip_mesh(vertices, facets, extents, literal=False):
    """clip_mesh_to_aabb: (vertices, facets, counts).  A facet whose corners are all inside every plane leaves the six
    planes as its three corners, snapped, and one whose corners are all outside one plane is dropped; unless `literal`
    those facets skip the per-facet loop (with `literal` both shortcuts are asserted instead)."""
    v = np.asarray(vertices, np.float64).reshape(-1, 3)
    f = np.asarray(facets, np.int64).reshape(-1, 3)
    e = np.asarray(extents, np.float64)
    eps = bbox_eps(e)
    lo, hi = e[:3], e[3:]
    inside = ((v >= lo - eps) & (v <= hi + eps)).all(1)
    all_in = inside[f].all(1) if len(f) else np.zeros(0, bool)
    snapped = v.copy()
    for a in range(3):
        snapped[:, a] = np.where(np.abs(snapped[:, a] - lo[a]) <= eps, lo[a], snapped[:, a])
        snapped[:, a] = np.where(np.abs(snapped[:, a] - hi[a]) <= eps, hi[a], snapped[:, a])
    # a facet with its three corners beyond one plane by more than eps can only be dropped; the others are clipped
    beyond = ((v[f] < lo - eps).all(1) | (v[f] > hi + eps).all(1)).any(1) if len(f) else np.zeros(0, bool)
    polys = [None] * len(f)
    for t in np.nonzero(np.ones(len(f), bool) if literal else ~(all_in | beyond))[0]:
        polys[t] = clip_triangle(v[f[t]], e, eps)[0]
        assert not (beyond[t] and len(polys[t]))
    out_v, out_f, n, straddling, outside = [], [], 0, 0, 0
    for t in range(len(f)):
        if polys[t] is None:
            if not all_in[t]:
                outside += 1
                continue
            p = snapped[f[t]]
        else:
            p = polys[t]
            if len(p) < 3:
                outside += 1
                continue
            if literal and all_in[t]:
                assert np.array_equal(p, snapped[f[t]])
            straddling += 0 if all_in[t] else 1
        out_v.append(p)
        k = np.arange(2, len(p))
        out_f.append(np.stack([np.full(len(k), n), n + k - 1, n + k], 1))
        n += len(p)
    cv = np.concatenate(out_v) if out_v else np.zeros((0, 3))
    cf = np.concatenate(out_f).astype(np.int64) if out_f else np.zeros((0, 3), np.int64)
    return cv, cf, {"facets_in": len(f), "straddling": straddling, "outside": outside, "vertices_emitted": len(cv)}


# ---- weld
def cell_keys(v, eps):
    """quantized_point_key: Rust's f64::round (half away from zero) and its saturating cast."""
    x = np.asarray(v, np.float64) / max(eps, 1.0e-12)
    r = np.trunc(x)
    r = r + np.where(np.abs(x - r) >= 0.5, np.sign(x), 0.0)
    r = np.where(np.isnan(r), 0.0, r)
    big = 9223372036854775807
    out = np.clip(r, -9.2e18, 9.2e18).astype(np.int64)
    out = np.where(r >= 9223372036854775808.0, big, out)
    return np.where(r <= -9223372036854775808.0, -big - 1, out)


_OFFSETS = [(dx, dy, dz) for dx in (-1, 0, 1) for dy in (-1, 0, 1) for dz in (-1, 0, 1)]


def weld_greedy(v, eps):
    """push_dedup_point over the vertices in order: rep[i], the index of the vertex whose compact entry i received."""
    keys = cell_keys(v, eps).tolist()
    pts = np.asarray(v, np.float64).tolist()
    eps2 = eps * eps
    cells, rep = {}, np.empty(len(pts), np.int64)
    for i, (p, k) in enumerate(zip(pts, keys)):
        found = -1
        for dx, dy, dz in _OFFSETS:
            ids = cells.get((k[0] + dx, k[1] + dy, k[2] + dz))
            if not ids:
                continue
            for j in ids:
                q = pts[j]
                d0, d1, d2 = p[0] - q[0], p[1] - q[1], p[2] - q[2]
                if d0 * d0 + d1 * d1 + d2 * d2 <= eps2:
                    found = j
                    break
            if found >= 0:
                break
        if found < 0:
            found = i
            cells.setdefault(tuple(k), []).append(i)
        rep[i] = found
    return rep


def weld_components(v, eps):
    """rep[i]: the lowest-index vertex of the component of i under |p - q|^2 <= eps^2.  Bit-equal vertices are linked
    (distance 0), so the search runs over the distinct points."""
    v = np.asarray(v, np.float64).reshape(-1, 3)
    if len(v) == 0:
        return np.zeros(0, np.int64)
    uniq, inv = np.unique(v + 0.0, axis=0, return_inverse=True)    # (+ 0.0: -0.0 and 0.0 are one point)
    inv = inv.reshape(-1)
    low = np.full(len(uniq), len(v), np.int64)
    np.minimum.at(low, inv, np.arange(len(v)))
    keys = cell_keys(uniq, eps).tolist()
    pts = uniq.tolist()
    eps2 = eps * eps
    parent = list(range(len(pts)))

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i

    cells = {}
    for i, (p, k) in enumerate(zip(pts, keys)):
        for dx, dy, dz in _OFFSETS:
            for j in cells.get((k[0] + dx, k[1] + dy, k[2] + dz), ()):
                q = pts[j]
                d0, d1, d2 = p[0] - q[0], p[1] - q[1], p[2] - q[2]
                if d0 * d0 + d1 * d1 + d2 * d2 <= eps2:
                    a, b = find(i), find(j)
                    if a != b:
                        parent[a] = b
        cells.setdefault(tuple(k), []).append(i)
    root = np.array([find(i) for i in range(len(pts))])
    comp_low = np.full(len(pts), len(v), np.int64)
    np.minimum.at(comp_low, root, low)
    return comp_low[root][inv]


def dist2(p, q):
    d = p - q
    return d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]


# ---- clean
def clean_mesh(vertices, facets, eps, weld="components"):
    """clean_mesh: (vertices, facets, counts)."""
    v = np.asarray(vertices, np.float64).reshape(-1, 3)
    f = np.asarray(facets, np.int64).reshape(-1, 3)
    rep = weld_components(v, eps) if weld == "components" else weld_greedy(v, eps)
    isrep = rep == np.arange(len(v))
    rid = np.cumsum(isrep) - 1                                    # welded ids in order of first appearance
    wid, wv = rid[rep], v[isrep]
    loose = int((~(dist2(v, v[rep]) <= eps * eps)).sum()) if len(v) else 0
    g = wid[f]
    collapsed = (g[:, 0] == g[:, 1]) | (g[:, 1] == g[:, 2]) | (g[:, 0] == g[:, 2])
    pa, pb, pc = wv[g[:, 0]], wv[g[:, 1]], wv[g[:, 2]]
    ab, ac = pb - pa, pc - pa
    n0 = ab[:, 1] * ac[:, 2] - ab[:, 2] * ac[:, 1]
    n1 = ab[:, 2] * ac[:, 0] - ab[:, 0] * ac[:, 2]
    n2 = ab[:, 0] * ac[:, 1] - ab[:, 1] * ac[:, 0]
    tiny = ~collapsed & (n0 * n0 + n1 * n1 + n2 * n2 <= (eps * eps) * (eps * eps))
    alive = np.nonzero(~collapsed & ~tiny)[0]
    _, firsts = np.unique(np.sort(g[alive], 1), axis=0, return_index=True) if len(alive) else (None, np.zeros(0, np.int64))
    unique_alive = np.sort(alive[firsts])
    duplicate = len(alive) - len(unique_alive)
    h = g[unique_alive]
    use = np.bincount(h.reshape(-1), minlength=len(wv))
    lone = (use[h] == 1).all(1) if len(h) else np.zeros(0, bool)
    h = h[~lone]
    flat = h.reshape(-1)
    ids, first_use = np.unique(flat, return_index=True)
    order = ids[np.argsort(first_use)]                            # in order of first use
    new = np.full(len(wv), -1, np.int64)
    new[order] = np.arange(len(order))
    counts = {"welded": int(len(v) - isrep.sum()), "weld_loose": loose, "collapsed": int(collapsed.sum()),
              "tiny": int(tiny.sum()), "duplicate": int(duplicate), "lone": int(lone.sum())}
    return wv[order], new[h].reshape(-1, 3), counts


def finish(vertices, facets, extents, weld="components", literal=False):
    """clean_mesh(clip_mesh_to_aabb(mesh)): (vertices, facets, stats), stats keyed by FINISH_STATS."""
    cv, cf, a = clip_mesh(vertices, facets, extents, literal)
    ov, of, b = clean_mesh(cv, cf, bbox_eps(extents), weld)
    a.update(b)
    return ov, of, {k: int(a[k]) for k in FINISH_STATS}


def unambiguous(clipped_vertices, eps, margin=100.0):
    """The condition under which the lowest-index-of-component weld is the reference's greedy one, with margin: both
    give the same partition, no vertex is further than eps from its representative, and distinct representatives are at
    least margin * eps apart.  Returns (ok, smallest gap between representatives / eps, largest spread in a group / eps)."""
    v = np.asarray(clipped_vertices, np.float64).reshape(-1, 3)
    a, b = weld_components(v, eps), weld_greedy(v, eps)
    spread = float(np.sqrt(dist2(v, v[a]).max(initial=0.0))) / eps
    reps = v[a == np.arange(len(v))]
    # pairs closer than margin * eps are as close along any direction: sweep along a fixed oblique one
    w = np.array([0.5377, 0.6182, 0.5735])
    u = reps @ (w / np.linalg.norm(w))
    o = np.argsort(u)
    u, p = u[o], reps[o]
    gap, k = np.inf, 1
    far = 4.0 * margin * eps
    while k < len(u):
        near = np.nonzero(u[k:] - u[:-k] < far)[0]
        if len(near) == 0:
            break
        gap = min(gap, float(np.sqrt(dist2(p[near], p[near + k]).min())))
        k += 1
    ok = bool(np.array_equal(a, b)) and spread <= 1.0 and gap >= margin * eps
    return ok, gap / eps, spread


# ---- the lattice fields of the tests: extents that are not lattice-aligned, resolution 0.25
EXT = [0.1, -0.2, 0.3, 6.3, 5.9, 6.1]
RES = 0.25


def field(name, w):
    if name == "sphere_cut":         # an off-centre sphere cut by the face x = lo
        return np.linalg.norm(w - [1.5, 3.0, 3.2], axis=-1) - 2.0
    if name == "torus_cut":          # a torus cut by the faces x = hi and y = hi
        return np.hypot(np.hypot(w[..., 0] - 4.6, w[..., 1] - 4.1) - 1.8, w[..., 2] - 3.1) - 0.7
    if name == "oblique_plane":
        return (w - [3.1, 2.9, 3.3]) @ np.array([0.31, 0.52, 0.79])
    a = np.linalg.norm(w - [6.3, 5.9, 6.1], axis=-1) - 0.9          # a small sphere around a box corner ...
    b = np.linalg.norm(w - [2.6, 2.4, 2.7], axis=-1) - 1.0          # ... and one inside
    return np.minimum(a, b)


FIELDS = ("sphere_cut", "torus_cut", "oblique_plane", "corner_and_inside")


def lattice_field(name, extents=EXT, resolution=RES):
    lat = R.Lattice(extents, resolution)
    return lat, field(name, lat.world(lat.node_ijk()))


# ---- hand-made meshes, one cleaning rule each, well away from the eps^2 and eps^4 thresholds (extents [0, 10]^3,
# eps = 1e-10 * sqrt(300)); (vertices, facets, (vertices out, facets out), the count of the rule, which is 1)
HAND_EXT = [0.0, 0.0, 0.0, 10.0, 10.0, 10.0]


def hand_made():
    eps = bbox_eps(HAND_EXT)
    strip = [[1, 1, 1], [2, 1, 1], [1, 2, 1], [2, 2, 1]]
    cases = {}
    # two copies of a vertex 0.3 eps apart across a cell boundary ((k + 0.5) * eps lies between them)
    x = (round(1.0 / eps) + 0.5) * eps
    cases["weld_across_cells"] = (strip + [[x - 0.15 * eps, 3, 1], [x + 0.15 * eps, 3, 1], [2, 3, 1]],
                                  [[0, 1, 2], [1, 3, 2], [2, 4, 6], [5, 6, 3]], (6, 4), "welded")
    cases["collapsed"] = (strip + [[2, 1, 1]], [[0, 1, 2], [1, 3, 2], [1, 4, 3]], (4, 2), "collapsed")
    cases["zero_area"] = (strip + [[3, 3, 1]], [[0, 1, 2], [1, 3, 2], [0, 3, 4]], (4, 2), "tiny")
    cases["opposite_winding"] = (strip, [[0, 1, 2], [1, 3, 2], [2, 1, 0]], (4, 2), "duplicate")
    cases["lone"] = (strip + [[7, 7, 7], [8, 7, 7], [7, 8, 7]], [[0, 1, 2], [1, 3, 2], [4, 5, 6]], (4, 2), "lone")
    cases["unused_vertex"] = ([[5, 5, 5]] + strip, [[1, 2, 3], [2, 4, 3]], (4, 2), None)
    return {k: (np.array(v, np.float64), np.array(f, np.int64), shape, count) for k, (v, f, shape, count) in cases.items()}
