"""numpy restatement of the boundary-closure contract (DESIGN.md "Boundary closure"): open edges and their face masks,
the grid axes, cut and whole cells, the regions of whole cells, the selection given the band triangles, the outward
winding, and the checks a closed result has to pass.  The band triangulation itself is not restated: any correct
constrained triangulation is acceptable, and tests/test_isosurface_closure_host.py checks the one that runs by its
properties.

Faces in the reference's order XMin, XMax, YMin, YMax, ZMin, ZMax (face = 2 * axis + side); the (u, v) of a face are its
two other axes in ascending order (uv_axes, boundary_closure.rs:902-908); cell (i, j) of face f has the id
offset[f] + j * n[u] + i.
"""
from __future__ import annotations

import numpy as np

import isosurface_finish_restatement as FR

CCW_IS_OUTWARD = (False, True, True, False, False, True)   # boundary_closure.rs:947-956


def face_axes(f):
    return ((1, 2), (0, 2), (0, 1))[f >> 1]


def axis_grid(lo, hi, resolution, eps):
    """axis_grid_coordinates (boundary_closure.rs:816-828)."""
    length = np.float64(hi) - np.float64(lo)
    n = int(max(np.ceil(length / max(resolution, eps)), 1.0))
    return np.array([np.float64(hi) if i == n else np.float64(lo) + length * (np.float64(i) / np.float64(n)) for i in range(n + 1)])


def grids(extents, resolution):
    eps = FR.bbox_eps(extents)
    return [axis_grid(extents[a], extents[a + 3], resolution, eps) for a in range(3)]


def vertex_masks(v, extents, eps):
    """(n, 6) bool: the faces a vertex lies on (point_on, boundary_closure.rs:881-890)."""
    e = np.asarray(extents, np.float64)
    m = np.zeros((len(v), 6), bool)
    for a in range(3):
        m[:, 2 * a] = np.abs(v[:, a] - e[a]) <= eps
        m[:, 2 * a + 1] = np.abs(v[:, a] - e[a + 3]) <= eps
    return m


def open_edges(f):
    """The directed edges (a, b) whose undirected edge has one facet, in (facet, corner) order."""
    f = np.asarray(f, np.int64).reshape(-1, 3)
    d = np.stack([f, np.roll(f, -1, 1)], -1).reshape(-1, 2)
    if not len(d):
        return d
    s = np.sort(d, 1)
    _, inv, cnt = np.unique(s, axis=0, return_inverse=True, return_counts=True)
    return d[cnt[inv.reshape(-1)] == 1]


def cut_cells(v, f, extents, resolution):
    """(cut, edges, edge_masks): cut[f] a bool array (n[v], n[u]) per face; the open edges and their (m, 6) face masks."""
    eps = FR.bbox_eps(extents)
    tol = np.float64(1e-9) * np.float64(resolution)
    g = grids(extents, resolution)
    vm = vertex_masks(v, extents, eps)
    edges = open_edges(f)
    em = vm[edges[:, 0]] & vm[edges[:, 1]] if len(edges) else np.zeros((0, 6), bool)
    cut = []
    for face in range(6):
        ua, va = face_axes(face)
        gu, gv = g[ua], g[va]
        c = np.zeros((len(gv) - 1, len(gu) - 1), bool)
        for (a, b) in edges[em[:, face]] if len(edges) else []:
            ulo, uhi = min(v[a, ua], v[b, ua]) - tol, max(v[a, ua], v[b, ua]) + tol
            vlo, vhi = min(v[a, va], v[b, va]) - tol, max(v[a, va], v[b, va]) + tol
            iu = (gu[:-1] <= uhi) & (gu[1:] >= ulo)
            iv = (gv[:-1] <= vhi) & (gv[1:] >= vlo)
            c |= iv[:, None] & iu[None, :]
        for p in np.nonzero(vm[:, face] & (vm.sum(1) >= 2))[0]:
            iu = (gu[:-1] - tol <= v[p, ua]) & (gu[1:] + tol >= v[p, ua])
            iv = (gv[:-1] - tol <= v[p, va]) & (gv[1:] + tol >= v[p, va])
            c |= iv[:, None] & iu[None, :]
        cut.append(c)
    return cut, edges, em


def offsets(cut):
    return np.concatenate([[0], np.cumsum([c.size for c in cut])])


def cell_across(n, off, f, i, j, s):
    """The id of the cell across side s (0: v - 1, 1: u + 1, 2: v + 1, 3: u - 1) of cell (i, j) of face f."""
    ua, va = face_axes(f)
    di, dj = ((0, -1), (1, 0), (0, 1), (-1, 0))[s]
    ni, nj = i + di, j + dj
    if 0 <= ni < n[ua] and 0 <= nj < n[va]:
        return off[f] + nj * n[ua] + ni
    ax = ua if di else va
    gface = 2 * ax + (1 if di > 0 or dj > 0 else 0)
    idx = [0, 0, 0]
    idx[ua], idx[va] = i, j
    idx[f >> 1] = n[f >> 1] - 1 if f & 1 else 0
    gu, gv = face_axes(gface)
    return off[gface] + idx[gv] * n[gu] + idx[gu]


def regions(cut):
    """(labels, n, offsets, count): per cell the lowest cell id of its component of whole cells (-1 for a cut cell), cells
    linked over grid edges on a face or across a box edge; the intervals per axis; the first cell id of every face; the
    number of components."""
    n = [0, 0, 0]
    for f in (0, 2, 4):
        ua, va = face_axes(f)
        n[va], n[ua] = cut[f].shape
    off = offsets(cut)
    flat = np.concatenate([c.reshape(-1) for c in cut])
    lab = np.where(flat, -1, np.arange(len(flat)))
    where = []
    for f in range(6):
        ua, va = face_axes(f)
        where += [(f, i, j) for j in range(n[va]) for i in range(n[ua])]
    parent = list(range(len(flat)))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for q, (f, i, j) in enumerate(where):
        if flat[q]:
            continue
        for s in range(4):
            d = cell_across(n, off, f, i, j, s)
            if not flat[d]:
                a, b = find(q), find(d)
                if a != b:
                    parent[max(a, b)] = min(a, b)
    for q in range(len(flat)):
        if not flat[q]:
            lab[q] = find(q)
    return lab, n, off, int(sum(1 for q in range(len(flat)) if lab[q] == q))


def face_of(v3, extents):
    """The faces (bool 6) on which all the given points lie exactly."""
    e = np.asarray(extents, np.float64)
    return np.array([(v3[:, f >> 1] == e[(f >> 1) + 3 * (f & 1)]).all() for f in range(6)])


def select(v, band, edges, em, cut, lab, n, off, extents, resolution):
    """select_closed_plus over regions (boundary_closure.rs:259-324): band: (m, 4) rows (face, a, b, c) of all band
    triangles in the numbering of v.  Returns (seeded flag per band triangle, the set of seeded region labels)."""
    g = grids(extents, resolution)
    parent = {}

    def find(x):
        parent.setdefault(x, x)
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    def unite(a, b):
        a, b = find(a), find(b)
        if a != b:
            parent[a] = b

    opens = {(min(a, b), max(a, b)) for a, b in edges.tolist()}
    edge_tri, side = {}, {}
    for t, (f, *tri) in enumerate(band.tolist()):
        p = v[tri][:, list(face_axes(f))]
        if (p[1, 0] - p[0, 0]) * (p[2, 1] - p[0, 1]) - (p[1, 1] - p[0, 1]) * (p[2, 0] - p[0, 0]) < 0:
            tri = [tri[0], tri[2], tri[1]]             # counter-clockwise in (u, v)
        for k in range(3):
            a, b = tri[k], tri[(k + 1) % 3]
            key = (min(a, b), max(a, b))
            if key in opens:
                side[(f, a, b)] = t
            elif key in edge_tri:
                unite(("t", edge_tri[key]), ("t", t))
            else:
                edge_tri[key] = t
    at = {tuple(p): i for i, p in enumerate(v.tolist())}
    e = np.asarray(extents, np.float64)
    for f in range(6):
        ua, va = face_axes(f)
        for j, i in zip(*np.nonzero(cut[f])):
            ends = (((i, j), (i + 1, j)), ((i + 1, j), (i + 1, j + 1)), ((i, j + 1), (i + 1, j + 1)), ((i, j), (i, j + 1)))
            for s in range(4):
                label = lab[cell_across(n, off, f, int(i), int(j), s)]
                if label < 0:
                    continue
                ids = []
                for (gi, gj) in ends[s]:
                    p = [0.0, 0.0, 0.0]
                    p[ua], p[va], p[f >> 1] = g[ua][gi], g[va][gj], e[(f >> 1) + 3 * (f & 1)]
                    ids.append(at[tuple(p)])
                unite(("t", edge_tri[(min(ids), max(ids))]), ("r", int(label)))
    seeded = set()
    for (a, b), m in zip(edges.tolist(), em):
        for f in np.nonzero(m)[0]:
            key = (int(f), b, a) if CCW_IS_OUTWARD[f] else (int(f), a, b)
            if key in side:
                seeded.add(find(("t", side[key])))
    tri_seeded = np.array([find(("t", t)) in seeded for t in range(len(band))], bool)
    return tri_seeded, {int(x) for x in np.unique(lab[lab >= 0]) if find(("r", int(x))) in seeded}


def whole_cell_triangles(v, facets, cut, extents, resolution):
    """Per cap facet: (face, cell id on the face) where it is half of a whole cell, else (face, -1)."""
    g = grids(extents, resolution)
    out = []
    for tri in facets:
        p = v[tri]
        faces = np.nonzero(face_of(p, extents))[0]
        assert len(faces) >= 1, "a cap facet off the faces"
        hit = (int(faces[0]), -1)
        for f in faces:
            ua, va = face_axes(f)
            iu, iv = np.searchsorted(g[ua], p[:, ua]), np.searchsorted(g[va], p[:, va])
            if not ((g[ua][np.minimum(iu, len(g[ua]) - 1)] == p[:, ua]).all() and (g[va][np.minimum(iv, len(g[va]) - 1)] == p[:, va]).all()):
                continue
            if iu.max() - iu.min() == 1 and iv.max() - iv.min() == 1 and not cut[f][iv.min(), iu.min()]:
                hit = (int(f), int(iv.min()) * cut[f].shape[1] + int(iu.min()))
        out.append(hit)
    return np.array(out, np.int64).reshape(-1, 2)


def check_closed(v, f, n_mesh=None, extents=None):
    """A closed, consistently wound mesh without unused or repeated vertices; with n_mesh and extents also: every cap
    facet f[n_mesh:] has its vertices on one face and its normal along that face's outward axis."""
    import isosurface_restatement as R
    f = np.asarray(f, np.int64)
    und = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), 1)
    _, cnt = np.unique(und, axis=0, return_counts=True)
    assert (cnt == 2).all(), f"{int((cnt != 2).sum())} edges without exactly two facets"
    assert R.directed_edges_once(f)
    assert len(np.unique(f)) == len(v) and f.min() == 0 and f.max() == len(v) - 1
    assert len(np.unique(v, axis=0)) == len(v), "repeated vertices"
    if n_mesh is None:
        return
    e = np.asarray(extents, np.float64)
    for tri in f[n_mesh:]:
        p = v[tri]
        nrm = np.cross(p[1] - p[0], p[2] - p[0])
        faces = np.nonzero(face_of(p, extents))[0]
        assert len(faces) >= 1
        ok = False
        for face in faces:
            a = face >> 1
            sign = 1.0 if face & 1 else -1.0
            ok = ok or (nrm[a] * sign > 0 and nrm[(a + 1) % 3] == 0 and nrm[(a + 2) % 3] == 0)
        assert ok, "a cap facet that is not wound outward"
