"""numpy restatement of the dense marching-tetrahedra contract (DESIGN.md "Isosurfaces on the RMT lattice").

Lattice (ferreus_rmt/src/lattice.rs:55-96): spacing [r/2, r*sqrt2/2, r/sqrt2], max_ijk = ceil((hi - lo) / spacing) with
max_ijk[0] += 1, world(ijk) = lo + ijk * spacing (multiply, then add).  Sample points: even i + j + k (the sublattice of
U, V, W = EDGE_DELTAS[0], [2], [6]; tests check its index).  Keys K: sample points with one of their 8 corners
(get_edge_points::<8>) inside [-2, max_ijk + 2] (extraction_ijk_inbounds); E: every corner of every key.  Vertices: one
per lattice edge (owner, label < 7) whose ends are in E, finite and on opposite sides of g < -1e-9, placed from the end
that holds it under the wavefront's t < 0.5 rule (isosurface.rs:588-610) with lerp_alpha (isosurface.rs:173-181).
Facets: march_tets (isosurface.rs:224-283) over the keys.  Order: vertices by (owner's row-major index over the bounding
box of E, label); facets by (key's row-major index, tetrahedron, table row).

Fields are arrays of shape (nk, nj, ni) over the bounding box of E (k slowest, i fastest); entries off the sample
sublattice or outside E are ignored.
"""
from __future__ import annotations

import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TABLES = json.load(open(os.path.join(HERE, "golden", "rmt_tables.json")))
ED = np.array(TABLES["EDGE_DELTAS"], dtype=np.int64)
REV = np.array(TABLES["REVERSE_EDGE"], dtype=np.int64)
TETS = np.array(TABLES["OWNED_TET_EDGES"], dtype=np.int64)
PAIRS = np.array(TABLES["TET_EDGE_PAIRS"], dtype=np.int64)
MT = TABLES["MT_TABLE"]
CORNERS = np.vstack([np.zeros((1, 3), np.int64), ED[:7]])   # get_edge_points::<8>
PAD = 2                                                    # OPEN_CLIP_IJK_PADDING
EPS_INSIDE = 1e-9


def spacing(resolution):
    s2 = np.sqrt(2.0)
    return np.array([resolution / 2.0, (resolution * s2) / 2.0, resolution / s2])


def max_ijk(extents, resolution):
    ext = np.asarray(extents, np.float64)
    m = np.ceil((ext[3:] - ext[:3]) / spacing(resolution)).astype(np.int64)
    m[0] += 1
    return m


def edge_of_delta(d):
    hit = np.nonzero((ED == np.asarray(d)).all(1))[0]
    return int(hit[0]) if len(hit) else None


class Lattice:
    """The key set K, the node set E and the bounding box of E for (extents, resolution)."""

    def __init__(self, extents, resolution):
        self.extents = np.asarray(extents, np.float64)
        self.resolution = float(resolution)
        self.spacing = spacing(resolution)
        self.max_ijk = max_ijk(extents, resolution)
        blo, bhi = np.full(3, -PAD), self.max_ijk + PAD
        # candidate keys: c + d in [blo, bhi] for some corner d
        klo, khi = blo - CORNERS.max(0), bhi - CORNERS.min(0)
        self.key_lo = klo
        self.key_shape = (khi - klo + 1)[::-1]
        c = self._grid(klo, khi)
        even = (c.sum(-1) % 2) == 0
        inb = np.zeros(even.shape, bool)
        for d in CORNERS:
            q = c + d
            inb |= ((q >= blo) & (q <= bhi)).all(-1)
        self.key_mask = even & inb                                        # (nk, nj, ni) over the key box
        # E: corners of keys; bounding box of E
        self.lo = klo + CORNERS.min(0)
        self.hi = khi + CORNERS.max(0)
        self.shape = tuple((self.hi - self.lo + 1)[::-1])                # (nk, nj, ni)
        inE = np.zeros(self.shape, bool)
        kk, kj, ki = np.nonzero(self.key_mask)
        kijk = np.stack([ki, kj, kk], -1) + klo
        for d in CORNERS:
            q = kijk + d - self.lo
            inE[q[:, 2], q[:, 1], q[:, 0]] = True
        self.inE = inE
        self.keys = kijk                                                  # row-major order over the key box
        assert (self.lo == self.key_lo + CORNERS.min(0)).all()

    @staticmethod
    def _grid(lo, hi):
        k, j, i = np.meshgrid(np.arange(lo[2], hi[2] + 1), np.arange(lo[1], hi[1] + 1), np.arange(lo[0], hi[0] + 1),
                              indexing="ij")
        return np.stack([i, j, k], -1)

    @property
    def n_keys(self):
        return int(self.key_mask.sum())

    def world(self, ijk):
        ijk = np.asarray(ijk)
        return self.extents[:3] + ijk.astype(np.float64) * self.spacing

    def node_ijk(self):
        """(nk, nj, ni, 3) absolute ijk of every entry of a field array."""
        return self._grid(self.lo, self.hi)

    def e_nodes(self):
        """ijk of the nodes of E in row-major order."""
        k, j, i = np.nonzero(self.inE)
        return np.stack([i, j, k], -1) + self.lo


def lerp_alpha(gu, gv):
    den = gu - gv
    with np.errstate(divide="ignore", invalid="ignore"):
        a = np.clip(gu / den, 0.0, 1.0)
    return np.where(np.abs(den) < 1e-30, 0.5, a)


def _tet_edge_owners():
    """Per tetrahedron and tet edge: (offset of the owner from the key, label), from get_edge_owner."""
    own = np.zeros((6, 6, 3), np.int64)
    lab = np.zeros((6, 6), np.int64)
    for t in range(6):
        corners = [np.zeros(3, np.int64)] + [ED[e] for e in TETS[t]]
        for e in range(6):
            a, b = PAIRS[e]
            eid = edge_of_delta(corners[b] - corners[a])
            assert eid is not None                     # every tet edge is a lattice edge
            if eid < 7:
                own[t, e], lab[t, e] = corners[a], eid
            else:
                own[t, e], lab[t, e] = corners[b], REV[eid]
    return own, lab


TET_OWN, TET_LAB = _tet_edge_owners()


def extract(lat: Lattice, field, isovalue):
    """(vertices (n, 3) f64, facets (m, 3) int64) for one isovalue of a field laid out over the bounding box of E."""
    f = np.asarray(field, np.float64).reshape(lat.shape)
    g = f - isovalue
    valid = lat.inE & np.isfinite(g)
    nk, nj, ni = lat.shape
    ijk = lat.node_ijk()
    even = (ijk.sum(-1) % 2) == 0
    inside = g < -EPS_INSIDE

    def shifted(a, d, fill):
        """a[p + d] for every p (fill outside the box)."""
        out = np.full_like(a, fill)
        di, dj, dk = (int(x) for x in d)
        src = a[max(dk, 0):nk + min(dk, 0), max(dj, 0):nj + min(dj, 0), max(di, 0):ni + min(di, 0)]
        out[max(-dk, 0):nk + min(-dk, 0), max(-dj, 0):nj + min(-dj, 0), max(-di, 0):ni + min(-di, 0)] = src
        return out

    cross = np.zeros(lat.shape + (7,), bool)
    gq_all = np.zeros(lat.shape + (7,))
    for l in range(7):
        vq = shifted(valid, ED[l], False)
        gq = shifted(g, ED[l], np.nan)
        iq = shifted(inside, ED[l], False)
        cross[..., l] = even & valid & vq & (inside != iq)
        gq_all[..., l] = gq
    flat = cross.reshape(-1)
    vid = np.cumsum(flat) - 1
    vid = np.where(flat, vid, -1).reshape(cross.shape)
    n_v = int(flat.sum())
    # vertex positions
    pk, pj, pi, pl = np.nonzero(cross)
    p = np.stack([pi, pj, pk], -1) + lat.lo
    q = p + ED[pl]
    gp = g[pk, pj, pi]
    gq = gq_all[pk, pj, pi, pl]
    with np.errstate(divide="ignore", invalid="ignore"):
        t = gp / (gp - gq)
    own = t < 0.5
    gu, gv = np.where(own, gp, gq), np.where(own, gq, gp)
    wu = lat.world(np.where(own[:, None], p, q))
    wv = lat.world(np.where(own[:, None], q, p))
    alpha = lerp_alpha(gu, gv)[:, None]
    verts = wu + alpha * (wv - wu)
    assert len(verts) == n_v
    # facets
    keys = lat.keys
    tris = []
    for tt in range(6):
        cs = [keys] + [keys + ED[e] for e in TETS[tt]]
        gs, ok = [], np.ones(len(keys), bool)
        for c in cs:
            r = c - lat.lo
            gs.append(g[r[:, 2], r[:, 1], r[:, 0]])
            ok &= valid[r[:, 2], r[:, 1], r[:, 0]]
        case = sum((gs[i] < -EPS_INSIDE).astype(np.int64) << i for i in range(4))
        ids = np.full((len(keys), 2, 3), -1, np.int64)
        okrow = np.zeros((len(keys), 2), bool)
        for cval in range(16):
            sel = ok & (case == cval)
            for row, tri in enumerate(MT[cval]):
                v3 = []
                for e in tri:
                    o = keys[sel] + TET_OWN[tt, e] - lat.lo
                    v3.append(vid[o[:, 2], o[:, 1], o[:, 0], TET_LAB[tt, e]])
                v3 = np.stack(v3, -1)
                ids[sel, row] = v3
                okrow[sel, row] = (v3 >= 0).all(-1)
        tris.append((ids, okrow))
    ids = np.stack([t[0] for t in tris], 1)          # (nkeys, 6, 2, 3)
    okm = np.stack([t[1] for t in tris], 1)          # (nkeys, 6, 2)
    facets = ids[okm]
    return verts, facets.astype(np.int64)


# ---- mesh checks used by the tests
def directed_edges_once(facets):
    """Closed, consistently oriented 2-manifold: every directed edge once, and its reverse once."""
    e = np.concatenate([facets[:, [0, 1]], facets[:, [1, 2]], facets[:, [2, 0]]])
    u = np.unique(e, axis=0)
    if len(u) != len(e):
        return False
    rev = {tuple(x) for x in e[:, ::-1].tolist()}
    return rev == {tuple(x) for x in e.tolist()}


def euler_characteristic(vertices, facets):
    used = np.unique(facets)
    e = np.sort(np.concatenate([facets[:, [0, 1]], facets[:, [1, 2]], facets[:, [2, 0]]]), 1)
    n_e = len(np.unique(e, axis=0))
    return len(used) - n_e + len(facets)


def enclosed_volume(vertices, facets):
    a, b, c = (vertices[facets[:, i]] for i in range(3))
    return float(np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.0)
