"""numpy restatement of the self-intersection rollback (DESIGN.md "Isosurfaces on the RMT lattice", self-intersection
rollback): ferreus_rmt's third guard of ClusterMethod::Average (isosurface.rs:932-1007), on top of
isosurface_cluster_restatement.py.

1. The pair predicate (is_true_self_intersection, mesh_intersections.rs:125-159), vectorised over pairs, with what it
   calls: tri_tri_intersect (moller.rs:81-147), is_degenerate, max_plane_distance_to, segment_pierces_interior,
   point_in_interior (geometry/triangle.rs:108-183), unit / close_to / lerp (geometry/point.rs:103-126).  Every sum in
   the reference's order (numpy multiplies and adds separately, never fused).  `a` is the facet with the lower index.
   Constants: tolerance 1e-8; Moeller EPSILON 1e-6 with |n1 x n2|^2 <= EPSILON^2 "parallel" (unnormalised normals: the
   answer depends on the scale of the mesh, as the reference's does); unit() gives nothing at a norm <= 1e-12.
2. The detector (get_intersecting_triangles, mesh_intersections.rs:163-208): every pair a < b of facets whose bounding
   boxes overlap on closed intervals goes through the predicate; here found by a sweep along x over all facets, no
   grid.  With extents, only the facets whose three vertices are inside them with slack bbox_eps take part
   (facet_fully_inside_aabb, aabb_clipping.rs:108-129), in facet order.
3. The rollback, one round: the triangles on true pairs, their vertices that are clusters of several lattice edges, the
   sample points owning those: every cluster of such a sample point becomes singletons (pass B's update); march again.
"""
from __future__ import annotations

import numpy as np

import isosurface_cluster_restatement as C
from isosurface_finish_restatement import bbox_eps

TOL = 1.0e-8
EPSILON = 1.0e-6
UNIT_MIN = 1.0e-12
STAGES = ("degenerate", "shared_two", "moller", "shared_crossing", "geometric_shared", "near_coplanar", "true")
DEGENERATE, SHARED_TWO, MOLLER, SHARED_CROSSING, GEOMETRIC_SHARED, NEAR_COPLANAR, TRUE = range(7)
STAT_NAMES = ("inside_facets", "box_pairs", "moller_pairs", "true_pairs", "triangles", "cluster_vertices", "rolled_back")


def dot(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def norm(a):
    return np.sqrt(dot(a, a))


def unit(a):
    """(ok, unit vector) (Point::unit)."""
    n = norm(a)
    ok = ~(n <= UNIT_MIN)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        return ok, a * (1.0 / n)[..., None]


def close(a, b):
    return norm(a - b) <= TOL


def normal(t):
    return cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])


def _isect(vv0, vv1, vv2, d0, d1, d2):
    return vv0 + (vv1 - vv0) * d0 / (d0 - d1), vv0 + (vv2 - vv0) * d0 / (d0 - d2)


def _intervals(vv, d, d0d1, d0d2):
    """compute_intervals (moller.rs:39-62): (some, isect0, isect1)."""
    vv0, vv1, vv2 = vv
    d0, d1, d2 = d
    conds = [d0d1 > 0.0, d0d2 > 0.0, (d1 * d2 > 0.0) | (d0 != 0.0), d1 != 0.0, d2 != 0.0]
    outs = [_isect(vv2, vv0, vv1, d2, d0, d1), _isect(vv1, vv0, vv2, d1, d0, d2), _isect(vv0, vv1, vv2, d0, d1, d2),
            _isect(vv1, vv0, vv2, d1, d0, d2), _isect(vv2, vv0, vv1, d2, d0, d1)]
    some = conds[0] | conds[1] | conds[2] | conds[3] | conds[4]
    return some, np.select(conds, [o[0] for o in outs], np.nan), np.select(conds, [o[1] for o in outs], np.nan)


def tri_tri_intersect(t1, t2):
    """tri_tri_intersect (moller.rs:81-147) of (n, 3, 3) triangles."""
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        v0, v1, v2, u0, u1, u2 = t1[:, 0], t1[:, 1], t1[:, 2], t2[:, 0], t2[:, 1], t2[:, 2]
        n1 = cross(v1 - v0, v2 - v0)
        d1 = -dot(n1, v0)
        du = [dot(n1, u0) + d1, dot(n1, u1) + d1, dot(n1, u2) + d1]
        du0du1, du0du2 = du[0] * du[1], du[0] * du[2]
        out = ~((du0du1 > 0.0) & (du0du2 > 0.0))
        n2 = cross(u1 - u0, u2 - u0)
        d2 = -dot(n2, u0)
        dv = [dot(n2, v0) + d2, dot(n2, v1) + d2, dot(n2, v2) + d2]
        dv0dv1, dv0dv2 = dv[0] * dv[1], dv[0] * dv[2]
        out &= ~((dv0dv1 > 0.0) & (dv0dv2 > 0.0))
        d = cross(n1, n2)
        out &= ~(dot(d, d) <= EPSILON * EPSILON)
        index = np.zeros(len(t1), np.int64)                       # dominant_axis
        mx = np.abs(d[:, 0])
        c = np.abs(d[:, 1]) > mx
        index[c], mx = 1, np.where(c, np.abs(d[:, 1]), mx)
        index[np.abs(d[:, 2]) > mx] = 2
        pick = lambda p: np.take_along_axis(p, index[:, None], 1)[:, 0]
        s1, a0, a1 = _intervals([pick(v0), pick(v1), pick(v2)], dv, dv0dv1, dv0dv2)
        s2, b0, b1 = _intervals([pick(u0), pick(u1), pick(u2)], du, du0du1, du0du2)
        out &= s1 & s2
        a0, a1 = np.where(a0 > a1, a1, a0), np.where(a0 > a1, a0, a1)
        b0, b1 = np.where(b0 > b1, b1, b0), np.where(b0 > b1, b0, b1)
        return out & (np.fmin(a1, b1) - np.fmax(a0, b0) > EPSILON)


def point_in_interior(t, q):
    ok, n = unit(normal(t))
    with np.errstate(invalid="ignore"):
        ok = ok & ~(np.abs(dot(q - t[:, 0], n)) > TOL)
        c0 = dot(cross(t[:, 1] - t[:, 0], q - t[:, 0]), n)
        c1 = dot(cross(t[:, 2] - t[:, 1], q - t[:, 1]), n)
        c2 = dot(cross(t[:, 0] - t[:, 2], q - t[:, 2]), n)
        at = TOL * TOL
        return ok & (((c0 > at) & (c1 > at) & (c2 > at)) | ((c0 < -at) & (c1 < -at) & (c2 < -at)))


def segment_pierces_interior(t, p0, p1):
    ok, n = unit(normal(t))
    with np.errstate(divide="ignore", invalid="ignore"):
        d0, d1 = dot(p0 - t[:, 0], n), dot(p1 - t[:, 0], n)
        ok = ok & ~((np.abs(d0) <= TOL) | (np.abs(d1) <= TOL) | (d0 * d1 >= 0.0))
        s = d0 / (d0 - d1)
        ok = ok & ~((s <= TOL) | (s >= 1.0 - TOL))
        return ok & point_in_interior(t, p0 + (p1 - p0) * s[:, None])


def max_plane_distance_to(t, other):
    ok, n = unit(normal(t))
    m = np.zeros(len(t))
    with np.errstate(invalid="ignore"):
        for k in range(3):
            m = np.fmax(m, np.abs(dot(other[:, k] - t[:, 0], n)))
    return np.where(ok, m, np.inf)


def shared_vertex_extra_crossing(a, b):
    """Decided at the first coincident (i, j) (mesh_intersections.rs:103-118)."""
    out, decided = np.zeros(len(a), bool), np.zeros(len(a), bool)
    for i in range(3):
        for j in range(3):
            c = close(a[:, i], b[:, j]) & ~decided
            if c.any():
                ta, tb = a[c], b[c]
                out[c] = (segment_pierces_interior(tb, ta[:, (i + 1) % 3], ta[:, (i + 2) % 3])
                          | segment_pierces_interior(ta, tb[:, (j + 1) % 3], tb[:, (j + 2) % 3]))
                decided |= c
    return out


def geometric_shared_vertex_count(a, b):
    used, count = np.zeros((len(a), 3), bool), np.zeros(len(a), np.int64)
    for i in range(3):
        matched = np.zeros(len(a), bool)
        for j in range(3):
            m = ~matched & ~used[:, j] & close(a[:, i], b[:, j])
            used[:, j] |= m
            matched |= m
        count += matched
    return count


def triangle_pairs(ta, ia, tb, ib):
    """(result, stage) of n pairs: ta, tb (n, 3, 3) points, ia, ib (n, 3) vertex ids; a the lower facet."""
    ta, tb = np.asarray(ta, np.float64).reshape(-1, 3, 3), np.asarray(tb, np.float64).reshape(-1, 3, 3)
    ia, ib = np.asarray(ia, np.int64).reshape(-1, 3), np.asarray(ib, np.int64).reshape(-1, 3)
    n = len(ta)
    result, stage = np.zeros(n, bool), np.full(n, -1, np.int64)

    def decide(mask, st, value):
        m = mask & (stage < 0)
        stage[m] = st
        result[m] = value[m] if isinstance(value, np.ndarray) else value

    decide((norm(normal(ta)) <= TOL * TOL) | (norm(normal(tb)) <= TOL * TOL), DEGENERATE, False)
    shared = (ia[:, :, None] == ib[:, None, :]).any(2).sum(1)
    decide(shared >= 2, SHARED_TWO, False)
    todo = stage < 0
    hit = np.zeros(n, bool)
    hit[todo] = tri_tri_intersect(ta[todo], tb[todo])
    decide(~hit, MOLLER, False)
    todo = stage < 0
    cr = np.zeros(n, bool)
    cr[todo] = shared_vertex_extra_crossing(ta[todo], tb[todo])
    decide(shared == 1, SHARED_CROSSING, cr)
    todo = stage < 0
    geo = np.zeros(n, np.int64)
    geo[todo] = geometric_shared_vertex_count(ta[todo], tb[todo])
    decide(geo >= 2, GEOMETRIC_SHARED, False)
    decide(geo == 1, GEOMETRIC_SHARED, cr)
    todo = stage < 0
    near = np.zeros(n, bool)
    near[todo] = np.minimum(max_plane_distance_to(ta[todo], tb[todo]), max_plane_distance_to(tb[todo], ta[todo])) <= TOL
    decide(near, NEAR_COPLANAR, False)
    decide(np.ones(n, bool), TRUE, True)
    return result, stage


def inside_facets(vertices, facets, extents):
    """Ids of the facets with every corner inside the extents (facet_fully_inside_aabb)."""
    if extents is None:
        return np.arange(len(facets))
    e, eps = np.asarray(extents, np.float64), bbox_eps(extents)
    p = vertices[facets]
    return np.nonzero(((p >= e[:3] - eps) & (p <= e[3:] + eps)).all((1, 2)))[0]


def box_pairs(vertices, facets, chunk=4_000_000):
    """All (a, b), a < b, whose bounding boxes overlap on closed intervals: a sweep along x."""
    p = vertices[facets]
    lo, hi = p.min(1), p.max(1)
    order = np.argsort(lo[:, 0], kind="stable")
    slo, shi = lo[order], hi[order]
    end = np.searchsorted(slo[:, 0], shi[:, 0], side="right")       # entries after i with lo_x <= hi_x[i]
    cnt = np.maximum(end - (np.arange(len(order)) + 1), 0)
    out, i0 = [], 0
    while i0 < len(order):
        i1 = i0 + max(1, int(np.searchsorted(np.cumsum(cnt[i0:]), chunk)))
        c = cnt[i0:i1]
        a = np.repeat(np.arange(i0, i1), c)
        b = np.arange(int(c.sum())) - np.repeat(np.cumsum(c) - c, c) + a + 1
        ok = ((slo[a, 1] <= shi[b, 1]) & (slo[b, 1] <= shi[a, 1]) & (slo[a, 2] <= shi[b, 2]) & (slo[b, 2] <= shi[a, 2]))
        out.append(np.stack([order[a[ok]], order[b[ok]]], 1))
        i0 = i1
    pairs = np.concatenate(out) if out else np.zeros((0, 2), np.int64)
    return np.sort(pairs, 1)


def detect(vertices, facets, extents=None):
    """(ids of the triangles on true pairs (ascending), [inside facets, box pairs, Moeller-positive pairs, true pairs,
    triangles], the true pairs) -- get_intersecting_triangles over the inside facets, ids those of `facets`."""
    vertices, facets = np.asarray(vertices, np.float64).reshape(-1, 3), np.asarray(facets, np.int64).reshape(-1, 3)
    keep = inside_facets(vertices, facets, extents)
    f = facets[keep]
    if len(f) < 2:
        return np.zeros(0, np.int64), [len(f), 0, 0, 0, 0], np.zeros((0, 2), np.int64)
    pairs = box_pairs(vertices, f)
    res, stage = np.zeros(len(pairs), bool), np.zeros(len(pairs), np.int64)
    for s in range(0, len(pairs), 500_000):
        a, b = pairs[s:s + 500_000, 0], pairs[s:s + 500_000, 1]
        res[s:s + 500_000], stage[s:s + 500_000] = triangle_pairs(vertices[f[a]], f[a], vertices[f[b]], f[b])
    true = keep[pairs[res]]
    ids = np.unique(true)
    return ids, [len(f), len(pairs), int((stage > MOLLER).sum()), int(res.sum()), len(ids)], true


def extract(lat, field, isovalue, extents, key_perm=None):
    """The clustered mesh after the two passes of isosurface_cluster_restatement.extract and one round of the
    self-intersection rollback.  dict: vertices, facets, stats (the cluster stats), self_intersections (STAT_NAMES),
    before: (vertices, facets) the rollback started from, ids: the triangles it found there."""
    base = C.extract(lat, field, isovalue, key_perm=key_perm)
    st = C.State(lat, field, isovalue)
    labels = base["labels"].copy()
    v, f, owner = C.build_mesh(st, labels, key_perm)
    counts = dict.fromkeys(STAT_NAMES, 0)
    ids = np.zeros(0, np.int64)
    if len(f):
        ids, c, _ = detect(v, f, extents)
        counts.update(zip(STAT_NAMES[:5], c))
    before = (v, f)
    vs = np.unique(f[ids].reshape(-1)) if len(ids) else np.zeros(0, np.int64)
    vs = vs[owner[vs, 2] > 1]
    bad = np.unique(owner[vs, 0])
    counts["cluster_vertices"], counts["rolled_back"] = len(vs), len(bad)
    if len(bad):
        labels[bad] = np.where(labels[bad] >= 0, np.arange(14)[None, :], -1)
        v, f, owner = C.build_mesh(st, labels, key_perm)
    return {"vertices": v, "facets": f, "stats": base["stats"], "self_intersections": counts, "labels": labels,
            "before": before, "ids": ids}
