"""The host part of the boundary closure (DESIGN.md "Boundary closure"), without a GPU: the exact orientation predicate
against rational arithmetic, and the band triangulator through its debug entry, checked by the properties any correct
constrained triangulation of the band has."""
from fractions import Fraction

import numpy as np
import pytest

from ferreus_rbf_rs_amd import isosurface as I
from ferreus_rbf_rs_amd.fmm_tree import FmmError

RES, EPS = 0.25, 1e-10


def _exact(a, b, c):
    a, b, c = ([Fraction(float(x)) for x in p] for p in (a, b, c))
    d = (b[0] - a[0]) * (c[1] - a[1]) - (b[1] - a[1]) * (c[0] - a[0])
    return (d > 0) - (d < 0)


def test_orient2d_is_the_exact_sign():
    rng = np.random.default_rng(11)
    g = 0.1 + 0.7 * np.arange(40) / 40.0                       # grid-collinear: lo + length * (i / n)
    i = rng.integers(0, 40, (1500, 3))
    a, b, c = (np.stack([g[i[:, k]], 3.0 + 2.0 * g[i[:, k]]], 1) for k in range(3))
    cases = [(a, b, c)]
    p, q = rng.uniform(-5, 5, (1500, 2)), rng.uniform(-5, 5, (1500, 2))
    t = rng.uniform(0, 1, (1500, 1))
    on = p + t * (q - p)                                       # on the line up to rounding, then one ulp off it
    cases += [(p, q, on), (p, q, np.nextafter(on, np.inf)), (p, q, np.stack([on[:, 0], np.nextafter(on[:, 1], -np.inf)], 1))]
    big = rng.uniform(-1, 1, (1500, 2)) * 10.0 ** rng.integers(-8, 9, (1500, 2))
    cases.append((big, big[::-1] * 3.0, big * (1.0 + 2.0 ** -40)))   # very different magnitudes, nearly through the origin
    n_zero = 0
    for a, b, c in cases:
        got = I.orient2d(a, b, c)
        want = np.array([_exact(*abc) for abc in zip(a, b, c)])
        assert np.array_equal(got, want)
        n_zero += int((want == 0).sum())
    assert n_zero > 100                                        # exact zeros are among the cases


# ---- the triangulator
def _cut_of(gu, gv, pts, edges, tol):
    """The cut cells of the contract for open edges alone (every point here lies on one face only)."""
    c = np.zeros((len(gv) - 1, len(gu) - 1), bool)
    for a, b in edges:
        ulo, uhi = min(pts[a][0], pts[b][0]) - tol, max(pts[a][0], pts[b][0]) + tol
        vlo, vhi = min(pts[a][1], pts[b][1]) - tol, max(pts[a][1], pts[b][1]) + tol
        c |= ((gv[:-1] <= vhi) & (gv[1:] >= vlo))[:, None] & ((gu[:-1] <= uhi) & (gu[1:] >= ulo))[None, :]
    return c


def _area2(p, t):
    a, b, c = p[t[:, 0]], p[t[:, 1]], p[t[:, 2]]
    return (b[:, 0] - a[:, 0]) * (c[:, 1] - a[:, 1]) - (b[:, 1] - a[:, 1]) * (c[:, 0] - a[:, 0])


def _check(gu, gv, pts, edges, cut):
    gu, gv, pts = np.asarray(gu, float), np.asarray(gv, float), np.asarray(pts, float).reshape(-1, 2)
    edges = np.asarray(edges, np.int64).reshape(-1, 2)
    ids = np.nonzero(cut.reshape(-1))[0]
    p, pid, t, counts = I.triangulate_band(gu, gv, pts, edges, ids, RES, EPS)
    p2, pid2, t2, counts2 = I.triangulate_band(gu, gv, pts, edges, ids, RES, EPS)
    assert p.tobytes() == p2.tobytes() and pid.tobytes() == pid2.tobytes() and t.tobytes() == t2.tobytes() and counts == counts2
    assert counts["dropped"] == 0
    if not len(ids):
        assert len(p) == 0 and len(t) == 0
        return p, pid, t
    nu = len(gu) - 1
    # the band points: the mesh points first, then grid points at their coordinates
    assert np.array_equal(pid[:len(pts)], np.arange(len(pts))) and np.array_equal(p[:len(pts)], pts)
    gp = -1 - pid[len(pts):]
    assert (gp >= 0).all() and np.array_equal(p[len(pts):], np.stack([gu[gp % (nu + 1)], gv[gp // (nu + 1)]], 1))
    # strictly positive, by the exact predicate
    assert all(_exact(*p[tri]) > 0 for tri in t)
    d = np.stack([t, np.roll(t, -1, 1)], -1).reshape(-1, 2)
    directed = {tuple(e) for e in d.tolist()}
    assert len(directed) == len(d)                             # every directed edge once: inner edges have opposite twins
    und = {(min(a, b), max(a, b)) for a, b in d.tolist()}
    # every constraint is an edge: the open edges ...
    for a, b in edges.tolist():
        assert (min(a, b), max(a, b)) in und
    # ... and the rim
    index = {int(g): k + len(pts) for k, g in enumerate(gp.tolist())}
    key = {(round(x / max(EPS, 1e-12)), round(y / max(EPS, 1e-12))): k for k, (x, y) in enumerate(pts.tolist())}

    def band_point(gi, gj):
        k = key.get((round(gu[gi] / max(EPS, 1e-12)), round(gv[gj] / max(EPS, 1e-12))))
        return k if k is not None else index[gj * (nu + 1) + gi]

    outline = set()
    nv = len(gv) - 1
    for j, i in zip(*np.nonzero(cut)):
        sides = ((i, j - 1, (i, j), (i + 1, j)), (i + 1, j, (i + 1, j), (i + 1, j + 1)), (i, j + 1, (i + 1, j + 1), (i, j + 1)),
                 (i - 1, j, (i, j + 1), (i, j)))
        for ci, cj, e0, e1 in sides:
            inside = 0 <= ci < nu and 0 <= cj < nv
            if inside and cut[cj, ci]:
                continue
            if inside:                                         # the rim: one edge, wound with the cut cell on its left
                outline.add((band_point(*e0), band_point(*e1)))
            else:                                              # the perimeter: the chain through every point on that cell side
                a, b = np.array([gu[e0[0]], gv[e0[1]]]), np.array([gu[e1[0]], gv[e1[1]]])
                ax = 0 if a[1] == b[1] else 1
                lo, hi = min(a[ax], b[ax]), max(a[ax], b[ax])
                on = [k for k in range(len(p)) if p[k][1 - ax] == a[1 - ax] and lo <= p[k][ax] <= hi]
                on.sort(key=lambda k: p[k][ax], reverse=bool(a[ax] > b[ax]))
                assert len(on) >= 2
                outline.update(zip(on[:-1], on[1:]))
    boundary = {e for e in directed if (e[1], e[0]) not in directed}
    assert boundary == outline                                 # the outline is exactly the rim plus the perimeter pieces
    want = sum((gu[i + 1] - gu[i]) * (gv[j + 1] - gv[j]) for j, i in zip(*np.nonzero(cut)))
    assert abs(0.5 * _area2(p, t).sum() - want) <= 1e-12 * want
    return p, pid, t


def _grid(n, m, lo=0.0, h=RES):
    return lo + h * np.arange(n + 1), lo + h * np.arange(m + 1)


def test_empty_bands():
    for n, m in ((1, 1), (3, 2)):
        gu, gv = _grid(n, m)
        _check(gu, gv, [], [], np.zeros((m, n), bool))
        p, pid, t = _check(gu, gv, [], [], np.ones((m, n), bool))         # all cells cut, no points: the grid alone
        assert len(p) == (n + 1) * (m + 1) and len(t) == 2 * n * m


def test_one_segment_across_one_cell():
    gu, gv = _grid(3, 3)
    pts, edges = [[0.30, 0.27], [0.45, 0.48]], [[0, 1]]
    cut = _cut_of(gu, gv, pts, edges, 1e-9 * RES)
    assert cut.sum() == 1
    p, pid, t = _check(gu, gv, pts, edges, cut)
    assert len(p) == 6


def test_a_closed_triangle_inside_one_cell():
    gu, gv = _grid(2, 2)
    pts, edges = [[0.05, 0.05], [0.2, 0.07], [0.1, 0.2]], [[0, 1], [1, 2], [2, 0]]
    cut = _cut_of(gu, gv, pts, edges, 1e-9 * RES)
    p, pid, t = _check(gu, gv, pts, edges, cut)
    assert cut.sum() == 1 and len(p) == 7 and len(t) == 8     # the triangle itself and 7 around it


def test_a_contour_through_a_grid_corner_omits_the_corner():
    gu, gv = _grid(4, 4)
    pts, edges = [[0.1, 0.1], [0.4, 0.4]], [[0, 1]]           # through the grid point (0.25, 0.25)
    cut = _cut_of(gu, gv, pts, edges, 1e-9 * RES)
    assert cut.sum() == 4
    p, pid, t = _check(gu, gv, pts, edges, cut)
    assert -1 - (1 * 5 + 1) not in pid.tolist() and len(p) == 2 + 8


def test_a_segment_along_a_grid_line():
    gu, gv = _grid(4, 3)
    pts, edges = [[0.1, 0.25], [0.9, 0.25]], [[0, 1]]         # over three grid points of the line v = 0.25
    cut = _cut_of(gu, gv, pts, edges, 1e-9 * RES)
    assert cut.sum() == 8
    p, pid, t = _check(gu, gv, pts, edges, cut)
    for gi in (1, 2, 3):
        assert -1 - (1 * 5 + gi) not in pid.tolist()


def test_a_mesh_vertex_on_the_perimeter_between_two_grid_points():
    gu, gv = _grid(3, 3)
    pts, edges = [[0.0, 0.37], [0.6, 0.37]], [[0, 1]]         # starts on the side u = 0, off the grid
    cut = _cut_of(gu, gv, pts, edges, 1e-9 * RES)
    p, pid, t = _check(gu, gv, pts, edges, cut)
    d = {tuple(e) for e in np.stack([t, np.roll(t, -1, 1)], -1).reshape(-1, 2).tolist()}
    gp = {int(-1 - g): k for k, g in enumerate(pid.tolist()) if g < 0}
    # the perimeter chain passes through the vertex: (0, 0.5) -> vertex -> (0, 0.25), wound with the face on the left
    assert (gp[2 * 4 + 0], 0) in d and (0, gp[1 * 4 + 0]) in d


def test_an_annulus():
    gu, gv = _grid(8, 8)
    k = 48
    ang = 2 * np.pi * (np.arange(k) + 0.3) / k
    outer = np.stack([1.0 + 0.83 * np.cos(ang), 1.0 + 0.83 * np.sin(ang)], 1)
    inner = np.stack([1.0 + 0.31 * np.cos(ang), 1.0 + 0.31 * np.sin(ang)], 1)
    pts = np.concatenate([outer, inner])
    edges = [[i, (i + 1) % k] for i in range(k)] + [[k + (i + 1) % k, k + i] for i in range(k)]
    cut = _cut_of(gu, gv, pts, edges, 1e-9 * RES)
    assert 0 < cut.sum() < cut.size and not cut[4, 6] and not cut[0, 0]   # whole cells between the loops and outside
    _check(gu, gv, pts, edges, cut)


def test_random_polylines_that_do_not_cross():
    rng = np.random.default_rng(3)
    for case in range(300):
        n, m = int(rng.integers(2, 9)), int(rng.integers(2, 9))
        gu, gv = _grid(n, m, lo=float(rng.uniform(-1, 1)), h=float(rng.uniform(0.2, 0.4)))
        # monotone polylines in separate horizontal bands cannot cross; ends on the sides u = min and u = max
        lines = int(rng.integers(1, 4))
        bands = np.linspace(gv[0], gv[-1], lines + 1)
        pts, edges = [], []
        for b in range(lines):
            k = int(rng.integers(2, 7))
            xs = np.sort(rng.uniform(gu[0], gu[-1], k))
            xs[0], xs[-1] = gu[0], gu[-1]
            if len(np.unique(xs)) < k:
                continue
            pad = 0.1 * (bands[b + 1] - bands[b])
            ys = rng.uniform(bands[b] + pad, bands[b + 1] - pad, k)
            first = len(pts)
            pts += np.stack([xs, ys], 1).tolist()
            edges += [[first + i, first + i + 1] for i in range(k - 1)]
        if not edges:
            continue
        cut = _cut_of(gu, gv, pts, edges, 1e-9 * RES)
        _check(gu, gv, pts, edges, cut)


def test_two_crossing_segments_are_refused():
    gu, gv = _grid(4, 4)
    pts, edges = [[0.1, 0.1], [0.9, 0.9], [0.1, 0.9], [0.9, 0.15]], [[0, 1], [2, 3]]
    cut = _cut_of(gu, gv, pts, edges, 1e-9 * RES)
    with pytest.raises(FmmError, match="cross"):
        I.triangulate_band(gu, gv, pts, edges, np.nonzero(cut.reshape(-1))[0], RES, EPS)
