"""numpy restatement of the clustered extraction (DESIGN.md "Isosurfaces on the RMT lattice", vertex clustering):
ferreus_rmt's build_isosurface with ClusterMethod::Average up to and including its non-manifold rollback, on the dense
lattice of isosurface_restatement.py (whose Lattice, E, K, g = f - isovalue and `inside` are used as they are).

1. Near masks (isosurface.rs:588-610): a crossing edge is an owned edge (p, q = p + EDGE_DELTAS[l]), l < 7, with both
   ends in E, finite and on opposite sides; its near end is p if g_p / (g_p - g_q) < 0.5, else q.  N(p): the 14-bit mask
   of the edges (p, p + EDGE_DELTAS[e]) that are crossing edges with near end p (bits 7..13 through REVERSE_EDGE).
2. Partition of N(p) (test_topology, topology.rs:232-314; connected_components_masks, topology.rs:106-133;
   is_flat_hole, topology.rs:180-221): closed -> singletons; several components -> one cluster each; complement not one
   component -> singletons; flat hole -> singletons; else one cluster.  A sample point whose 14 neighbours are not all
   in E is "incomplete" and gets singletons (the reference evaluates what it misses, isosurface.rs:668-697; here E is
   fixed).
3. Candidates (isosurface.rs:738-796, average_point isosurface.rs:183-192): a single edge keeps its intersection point,
   several get the mean: sums in ascending edge order, times 1.0 / n.
4. Marching (march_tets, isosurface.rs:224-283): every tet edge resolves to the cluster that holds it at its near end;
   triangles with two equal ids are dropped (isosurface.rs:275-278).
5. Pass A (isosurface.rs:798-878): for every mesh edge with more than 2 triangles, each end cluster of several lattice
   edges becomes singletons.
6. Pass B (isosurface.rs:888-930, 326-395), at most 4 rounds: the faces on mesh edges with more than 2 faces, their
   vertices that are still clusters of several edges, the sample points owning those: every cluster of such a sample
   point becomes singletons; march again; stop when a round finds nothing.
7. Vertices: one per final cluster, by (sample point's row-major index over the box of E, lowest edge); facets in
   marching order (key, tetrahedron, table row).
"""
from __future__ import annotations

import json
import os

import numpy as np

import isosurface_restatement as R

HERE = os.path.dirname(os.path.abspath(__file__))
CT = json.load(open(os.path.join(HERE, "golden", "rmt_cluster_tables.json")))
NB = [int(x) for x in CT["NEIGHBOUR_MASKS"]]
FLAT = [(int(a), int(b)) for a, b in CT["FLAT_HOLE_MASKS"]]
ALL14 = int(CT["ALL14_MASK"])
ED, REV = R.ED, R.REV

CLOSED, MULTI_HOLE, FLAT_HOLE, MULTI_SURFACE, SIMPLE, INCOMPLETE = range(6)
CASE_NAMES = ["closed", "multi_hole", "flat_hole", "multi_surface", "simple", "incomplete"]


def bits(m):
    return [e for e in range(14) if (m >> e) & 1]


FLAT_EDGES = [(bits(a), bits(b)) for a, b in FLAT]      # two_edge_indices of every row


def components(mask):
    """connected_components_masks (topology.rs:106-133): the components as masks, by lowest edge."""
    remaining, comps = mask & ALL14, []
    while remaining:
        seed = remaining & -remaining
        remaining ^= seed
        comp, frontier = 0, seed
        while frontier:
            b = frontier & -frontier
            frontier ^= b
            comp |= b
            nbrs = NB[b.bit_length() - 1] & remaining
            remaining ^= nbrs
            frontier |= nbrs
        comps.append(comp)
    return comps


def _inside(v):
    return v < -R.EPS_INSIDE


def _near(a, b):
    """crossing_alpha(a, b).is_some_and(|t| t < 0.5) (topology.rs:162-169)."""
    if _inside(a) == _inside(b):
        return False
    return float(R.lerp_alpha(np.float64(a), np.float64(b))) < 0.5


def is_flat_hole(m, values):
    """is_flat_hole (topology.rs:180-221); values: g at the 14 neighbours."""
    for (em, om), (ab, cd) in zip(FLAT, FLAT_EDGES):
        if (m & em) != 0 or (m & om) != om:
            continue
        if len(ab) != 2 or len(cd) != 2:
            continue
        a, b, c, d = (values[ab[0]], values[ab[1]], values[cd[0]], values[cd[1]])
        if not (np.isfinite(a) and np.isfinite(b) and np.isfinite(c) and np.isfinite(d)):
            continue
        if (_near(a, d) and _near(a, c)) or (_near(b, d) and _near(b, c)):
            return True
    return False


def test_topology(mask, values=None):
    """(case, clusters as lists of edges) of a near mask (topology.rs:232-314); values None: no flat-hole test."""
    m = mask & ALL14
    if m == 0:
        return SIMPLE, []
    if m == ALL14:
        return CLOSED, [[e] for e in bits(m)]
    comps = components(m)
    if len(comps) > 1:
        return MULTI_SURFACE, [bits(c) for c in comps]
    if len(components(ALL14 & ~m)) != 1:
        return MULTI_HOLE, [[e] for e in bits(m)]
    if values is not None and is_flat_hole(m, values):
        return FLAT_HOLE, [[e] for e in bits(m)]
    return SIMPLE, [bits(m)]


test_topology.__test__ = False          # (not a pytest test)


def labels_of(mask, clusters):
    """cluster_of_edge[14]: the lowest edge of the cluster of each edge, -1 off the mask."""
    lab = np.full(14, -1, np.int64)
    for c in clusters:
        lab[c] = min(c)
    return lab


def _shift(a, d, fill):
    nk, nj, ni = a.shape
    out = np.full_like(a, fill)
    di, dj, dk = (int(x) for x in d)
    src = a[max(dk, 0):nk + min(dk, 0), max(dj, 0):nj + min(dj, 0), max(di, 0):ni + min(di, 0)]
    out[max(-dk, 0):nk + min(-dk, 0), max(-dj, 0):nj + min(-dj, 0), max(-di, 0):ni + min(-di, 0)] = src
    return out


class State:
    """Near masks, neighbour values and the partition (labels) of the sample points with near intersections."""

    def __init__(self, lat, field, isovalue):
        self.lat = lat
        self.g = np.asarray(field, np.float64).reshape(lat.shape) - isovalue
        g = self.g
        self.valid = lat.inE & np.isfinite(g)
        inside = g < -R.EPS_INSIDE
        near = np.zeros(lat.shape, np.int64)
        complete = np.ones(lat.shape, bool)
        gn = np.full(lat.shape + (14,), np.nan)
        for e in range(14):
            vq, gq, iq = _shift(self.valid, ED[e], False), _shift(g, ED[e], np.nan), _shift(inside, ED[e], False)
            complete &= _shift(lat.inE, ED[e], False)
            gn[..., e] = np.where(_shift(lat.inE, ED[e], False), gq, np.nan)
            cross = self.valid & vq & (inside != iq)
            with np.errstate(divide="ignore", invalid="ignore"):
                # t from the owner of the edge: p for e < 7, the neighbour otherwise
                near_p = (g / (g - gq) < 0.5) if e < 7 else ~(gq / (gq - g) < 0.5)
            near |= (cross & near_p).astype(np.int64) << e
        self.near = near
        k, j, i = np.nonzero(near)
        self.nodes = np.stack([k, j, i], -1)                       # row-major order
        self.act = np.full(lat.shape, -1, np.int64)
        self.act[k, j, i] = np.arange(len(k))
        self.masks = near[k, j, i]
        self.gn = gn[k, j, i]                                      # g at the 14 neighbours
        self.gp = g[k, j, i]
        self.labels = np.full((len(k), 14), -1, np.int64)
        self.cases = np.zeros(len(k), np.int64)
        comp = complete[k, j, i]
        for a in range(len(k)):
            m = int(self.masks[a])
            if not comp[a]:
                self.cases[a], cl = INCOMPLETE, [[e] for e in bits(m)]
            else:
                self.cases[a], cl = test_topology(m, self.gn[a])
            self.labels[a] = labels_of(m, cl)

    def singletons(self):
        lab = np.full_like(self.labels, -1)
        for e in range(14):
            lab[:, e] = np.where((self.masks >> e) & 1, e, -1)
        return lab


def build_mesh(st: State, labels, key_perm=None):
    """(vertices, facets, vertex -> (active sample point, lowest edge, edges in its cluster)) of a partition."""
    lat = st.lat
    leaders = labels == np.arange(14)[None, :]
    cid = np.full(labels.shape, -1, np.int64)                     # (sample point, edge) -> vertex
    flat = leaders.reshape(-1)
    lead_id = np.where(flat, np.cumsum(flat) - 1, -1).reshape(labels.shape)
    has = labels >= 0
    rows = np.nonzero(has)
    cid[rows] = lead_id[rows[0], labels[rows]]
    n_v = int(flat.sum())
    # intersection point of every near edge from its sample point (edge_intersection_point), then the means
    a_idx, e_idx = rows
    p = st.nodes[a_idx][:, ::-1] + lat.lo
    q = p + ED[e_idx]
    alpha = R.lerp_alpha(st.gp[a_idx], st.gn[a_idx, e_idx])[:, None]
    wu, wv = lat.world(p), lat.world(q)
    pts = wu + alpha * (wv - wu)
    vid = cid[a_idx, e_idx]
    sums, cnt = np.zeros((n_v, 3)), np.zeros(n_v, np.int64)
    single = np.zeros((n_v, 3))
    for e in range(14):                                            # ascending edge order within every cluster
        sel = e_idx == e
        sums[vid[sel]] = sums[vid[sel]] + pts[sel]
        single[vid[sel]] = pts[sel]
        cnt[vid[sel]] += 1
    inv = 1.0 / cnt.astype(np.float64)
    verts = np.where((cnt == 1)[:, None], single, sums * inv[:, None])
    la, le = np.nonzero(leaders)
    owner = np.stack([la, le, cnt], -1)
    # marching
    keys = lat.keys if key_perm is None else lat.keys[key_perm]
    g, valid = st.g, st.valid

    def resolve(o, l):
        """vertex of the owned edge l of the nodes o (box indices): held at o or at its other end."""
        a = st.act[o[:, 2], o[:, 1], o[:, 0]]
        id1 = np.where(a >= 0, cid[np.maximum(a, 0), l], -1)
        o2 = o + ED[l]
        a2 = st.act[o2[:, 2], o2[:, 1], o2[:, 0]]
        id2 = np.where(a2 >= 0, cid[np.maximum(a2, 0), REV[l]], -1)
        return np.where(id1 >= 0, id1, id2)

    tris = []
    for tt in range(6):
        cs = [keys] + [keys + ED[e] for e in R.TETS[tt]]
        gs, ok = [], np.ones(len(keys), bool)
        for c in cs:
            r = c - lat.lo
            gs.append(g[r[:, 2], r[:, 1], r[:, 0]])
            ok &= valid[r[:, 2], r[:, 1], r[:, 0]]
        case = sum((gs[i] < -R.EPS_INSIDE).astype(np.int64) << i for i in range(4))
        ids = np.full((len(keys), 2, 3), -1, np.int64)
        okrow = np.zeros((len(keys), 2), bool)
        for cval in range(16):
            sel = ok & (case == cval)
            for row, tri in enumerate(R.MT[cval]):
                v3 = np.stack([resolve(keys[sel] + R.TET_OWN[tt, e] - lat.lo, int(R.TET_LAB[tt, e])) for e in tri], -1)
                ids[sel, row] = v3
                okrow[sel, row] = ((v3 >= 0).all(-1) & (v3[:, 0] != v3[:, 1]) & (v3[:, 1] != v3[:, 2])
                                   & (v3[:, 0] != v3[:, 2]))
        tris.append((ids, okrow))
    ids = np.stack([t[0] for t in tris], 1)
    okm = np.stack([t[1] for t in tris], 1)
    return verts, ids[okm].astype(np.int64), owner


def over_used(facets):
    """(mesh edges with more than 2 faces (n, 2), the faces on them)."""
    if len(facets) == 0:
        return np.zeros((0, 2), np.int64), np.zeros(0, np.int64)
    e = np.sort(np.concatenate([facets[:, [0, 1]], facets[:, [1, 2]], facets[:, [2, 0]]]), 1)
    face = np.tile(np.arange(len(facets)), 3)
    u, inv, cnt = np.unique(e, axis=0, return_inverse=True, return_counts=True)
    bad = cnt > 2
    return u[bad], np.unique(face[bad[inv.reshape(-1)]])


def extract(lat, field, isovalue, cluster=True, key_perm=None):
    """dict: vertices, facets, stats, labels (the final partition) and cases of the clustered mesh; cluster False: every
    near intersection its own cluster (the raw mesh, renumbered)."""
    st = State(lat, field, isovalue)
    stats = {n: 0 for n in CASE_NAMES}
    stats.update(over_used_a=0, split_a=0, rolled_b=[0, 0, 0, 0], over_used_b=[0, 0, 0, 0])
    if not cluster:
        labels = st.singletons()
        v, f, _ = build_mesh(st, labels, key_perm)
        return {"vertices": v, "facets": f, "stats": stats, "labels": labels, "cases": st.cases}
    for c, n in enumerate(CASE_NAMES):
        stats[n] = int((st.cases == c).sum())
    labels = st.labels.copy()
    own = np.arange(14)[None, :]
    v, f, owner = build_mesh(st, labels, key_perm)
    # pass A
    edges, _ = over_used(f)
    stats["over_used_a"] = len(edges)
    split = np.unique(edges.reshape(-1))
    split = split[owner[split, 2] > 1]
    stats["split_a"] = len(split)
    if len(split):
        for a, lead in owner[split, :2]:
            labels[a] = np.where(labels[a] == lead, own[0], labels[a])
        v, f, owner = build_mesh(st, labels, key_perm)
    # pass B
    for rnd in range(4):
        edges, faces = over_used(f)
        stats["over_used_b"][rnd] = len(edges)
        vs = np.unique(f[faces].reshape(-1)) if len(faces) else np.zeros(0, np.int64)
        vs = vs[owner[vs, 2] > 1]
        bad = np.unique(owner[vs, 0])
        if len(bad) == 0:
            break
        stats["rolled_b"][rnd] = len(bad)
        labels[bad] = np.where(labels[bad] >= 0, own, -1)
        v, f, owner = build_mesh(st, labels, key_perm)
    return {"vertices": v, "facets": f, "stats": stats, "labels": labels, "cases": st.cases}


def stats_vector(stats):
    """The 16 counts in the order of bbfmm_isosurface_stats."""
    return np.array([stats[n] for n in CASE_NAMES] + [stats["over_used_a"], stats["split_a"]] + stats["rolled_b"]
                    + stats["over_used_b"], np.int64)


def min_angles(vertices, facets):
    """Smallest angle of every triangle, in radians."""
    p = vertices[facets]
    out = np.full(len(facets), np.inf)
    for i in range(3):
        a, b = p[:, (i + 1) % 3] - p[:, i], p[:, (i + 2) % 3] - p[:, i]
        c = np.einsum("ij,ij->i", a, b) / np.maximum(np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1), 1e-300)
        out = np.minimum(out, np.arccos(np.clip(c, -1.0, 1.0)))
    return out
