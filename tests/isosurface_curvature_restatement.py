"""numpy restatement of the curvature-weighted cluster points (DESIGN.md "Curvature-weighted clusters"): ferreus_rmt's
ClusterMethod::CurvatureWeighted on the dense lattice and the fixed E of isosurface_cluster_restatement.py, whose State,
partition, marching and two passes are used as they are -- the weights change positions only.

1. Weight of a crossed edge (curvature_weight_for_edge, curvature_weighting.rs:48-234), owner o, owned label e < 7,
   other end a = o + EDGE_DELTAS[e]: for every calculation plane of row e of NEIGHBOUR_EDGE_PLANE_PAIRS / _PHIS and both
   of its neighbour edges b, Equation (1) gives theta from d = f - isovalue at o, a, b and the world vectors oa, ob
   (differences of world(ijk) of both ends); Equation (2) alpha = |theta_b| + |theta_c|; the normal estimate is the unit
   of oa_hat + scale * sum of the planes' projections (scale 2/3 with three planes); Equation (3) turns alpha into beta;
   Equation (4): the weight is 1 / min |tan(beta / 2)|, at most 1e12.  Every `return None` of the reference (a missing or
   non-finite neighbour, a vector of norm <= 1e-12, |denominator| <= EPS, a negative curvature term, no plane left) is
   the fallback weight 1 (unwrap_or(1.0), line 259).  A neighbour outside the box of E, off E or non-finite is missing.
2. Cluster point (curvature_weighted_cluster_point, :242-276, called from isosurface.rs:738-782 for clusters of one edge
   too): sum of w * p and of w in ascending edge order, then the sum times 1 / sum of w; sum of w <= EPS: the single
   point or the mean of isosurface_cluster_restatement.build_mesh.

Every function takes the number type: np.float64 is what the library computes, np.longdouble the yardstick of its
rounding.  Both start from the same float64 values of d, of the lattice origin and spacing and of the table angles.
"""
from __future__ import annotations

import json
import os

import numpy as np

import isosurface_restatement as R
import isosurface_cluster_restatement as C
import isosurface_intersect_restatement as X

HERE = os.path.dirname(os.path.abspath(__file__))
KT = json.load(open(os.path.join(HERE, "golden", "rmt_curvature_tables.json")))
PAIRS, PHIS = KT["NEIGHBOUR_EDGE_PLANE_PAIRS"], KT["NEIGHBOUR_EDGE_PLANE_PHIS"]
EPS, MAX_COT, MAX_W = KT["EPS"], KT["MAX_COT_THETA"], KT["MAX_CURVATURE_WEIGHT"]
ED, REV = R.ED, R.REV
HALF_PI = float(np.pi / 2)              # std::f64::consts::FRAC_PI_2
STAT_NAMES = ("edges", "edge_fallbacks", "clusters", "cluster_fallbacks")


def _dot(a, b):
    return a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1] + a[:, 2] * b[:, 2]


def _unit(v, T):
    """Point::unit: (v * (1 / |v|), |v| > 1e-12)."""
    n = np.sqrt(_dot(v, v))
    ok = n > T(EPS)
    return v * (T(1.0) / n)[:, None], ok


def _world(lat, ijk, T):
    return lat.extents[:3].astype(T) + ijk.astype(T) * lat.spacing.astype(T)


def weights_of_label(lat, D, owner, label, T, trace=None):
    """(weight, is the fallback) of the owned edges `label` of the sample points `owner` ((n, 3) ijk); D(ijk): d there as T,
    NaN where missing.  trace: a dict that receives, per edge, how often each clamp or special branch was taken."""
    n = len(owner)
    tr = {k: np.zeros(n, np.int64) for k in ("divisor_small", "divisor_negative", "cot_clamped", "flat", "skipped", "capped")}
    eps = T(EPS)
    none = np.zeros(n, bool)
    with np.errstate(all="ignore"):
        d_o, d_a = D(owner), D(owner + ED[label])
        none |= ~np.isfinite(d_o) | ~np.isfinite(d_a)
        ow = _world(lat, owner, T)
        oa = _world(lat, owner + ED[label], T) - ow
        oa_len = np.sqrt(_dot(oa, oa))
        none |= ~(oa_len > eps)
        oa_hat, ok = _unit(oa, T)
        none |= ~ok
        proj = np.zeros((n, 3), T)
        alphas, axes = [], []
        for pair, phis in zip(PAIRS[label], PHIS[label]):
            perp, theta, cot = [], [], []
            for nb, phi in zip(pair, phis):
                sin_phi, cos_phi = np.sin(T(phi)), np.cos(T(phi))
                d_b = D(owner + ED[nb])
                none |= ~np.isfinite(d_b)
                ob = _world(lat, owner + ED[nb], T) - ow
                ob_len = np.sqrt(_dot(ob, ob))
                none |= ~(ob_len > eps)
                across = ob - oa_hat * _dot(ob, oa_hat)[:, None]
                pd, ok = _unit(across, T)
                none |= ~ok
                den = (d_o - d_a) * ob_len                      # Equation (1)
                none |= ~(np.abs(den) > eps)
                divisor = ((d_o - d_b) * oa_len) / den - cos_phi
                th = np.where(np.abs(divisor) <= eps, np.where(np.signbit(divisor), -T(HALF_PI), T(HALF_PI)),
                              np.arctan(sin_phi / divisor))
                tan_th = np.tan(th)
                tr["divisor_small"] += np.abs(divisor) <= eps
                tr["divisor_negative"] += (np.abs(divisor) <= eps) & np.signbit(divisor)
                tr["cot_clamped"] += np.abs(tan_th) <= eps
                cot.append(np.where(np.abs(tan_th) <= eps, np.copysign(T(MAX_COT), th), T(1.0) / tan_th))
                perp.append(pd)
                theta.append(th)
            alphas.append(np.abs(theta[0]) + np.abs(theta[1]))  # Equation (2)
            ax, ok = _unit(perp[0] - perp[1], T)
            axes.append(np.where(ok[:, None], ax, perp[0]))
            proj = proj + (perp[0] * cot[0][:, None] + perp[1] * cot[1][:, None])
        scale = T(2.0) / T(3.0) if len(alphas) == 3 else T(1.0)
        n_est, ok = _unit(oa_hat + proj * scale, T)
        none |= ~ok
        min_tan = np.full(n, np.inf, T)
        for alpha, ax in zip(alphas, axes):
            axis, ok = _unit(ax, T)
            none |= ~ok
            sin_gamma = np.clip(np.abs(_dot(n_est, axis)), T(0.0), T(1.0))
            cos_gamma = np.cos(np.arcsin(sin_gamma))
            one_minus = T(1.0) - cos_gamma * cos_gamma
            sin_half = np.abs(np.sin(T(0.5) * alpha))
            flat = sin_half <= eps
            term = T(1.0) / (sin_half * sin_half) - T(1.0)      # Equation (3)
            none |= ~flat & (term < 0)
            inv = one_minus * term
            skip = ~flat & (inv <= eps)                         # the plane is left out
            beta = np.where(flat, T(0.0), T(2.0) * np.arctan(T(1.0) / np.sqrt(inv)))
            t = np.where(skip, T(np.inf), np.abs(np.tan(T(0.5) * beta)))
            min_tan = np.where(t < min_tan, t, min_tan)
            tr["flat"] += flat
            tr["skipped"] += skip
        none |= ~np.isfinite(min_tan)
        w = np.where(min_tan <= eps, T(MAX_W), np.minimum(T(1.0) / min_tan, T(MAX_W)))   # Equation (4)
        tr["capped"] += ~none & (min_tan <= eps)
    if trace is not None:
        trace.update(tr)
    return np.where(none, T(1.0), w).astype(T), none


class _Frame:
    """The two attributes of a Lattice that the world coordinates need."""

    def __init__(self, lo_world, spacing):
        self.extents, self.spacing = np.asarray(lo_world, np.float64), np.asarray(spacing, np.float64)


def weight_of_stencil(values, owner, label, lo_world, spacing, T=np.float64, trace=None):
    """(weight, fallback) of one edge from d at the owner and its 14 neighbours (NaN: missing), as
    bbfmm_isosurface_curvature_weight takes them."""
    values, owner = np.asarray(values, np.float64), np.asarray(owner, np.int64).reshape(1, 3)

    def D(ijk):
        d = (ijk - owner)[0]
        if not d.any():
            return values[:1].astype(T)
        return values[1 + R.edge_of_delta(d):][:1].astype(T)

    w, none = weights_of_label(_Frame(lo_world, spacing), D, owner, label, T, trace)
    return w[0], bool(none[0])


class Weights:
    """The weight of every crossed edge of a State, in the order (sample point that holds it, edge): the near ends."""

    def __init__(self, st: C.State, T=np.float64):
        lat, self.T = st.lat, T
        nk, nj, ni = lat.shape
        pad = np.full((nk + 4, nj + 4, ni + 8), np.nan, T)
        pad[2:-2, 2:-2, 4:-4] = np.where(lat.inE, st.g, np.nan).astype(T)

        def D(ijk):
            b = ijk - lat.lo
            return pad[b[:, 2] + 2, b[:, 1] + 2, b[:, 0] + 4]

        self.a_idx, self.e_idx = np.nonzero(st.labels >= 0)
        p = st.nodes[self.a_idx][:, ::-1] + lat.lo
        far = self.e_idx >= 7
        self.owner = np.where(far[:, None], p + ED[self.e_idx], p)
        self.label = np.where(far, REV[self.e_idx], self.e_idx)
        self.w = np.ones(len(p), T)
        self.none = np.zeros(len(p), bool)
        for l in range(7):
            sel = self.label == l
            if sel.any():
                self.w[sel], self.none[sel] = weights_of_label(lat, D, self.owner[sel], l, T)
        # the near intersection of every edge (edge_intersection_point from the sample point that holds it)
        gp, gq = st.gp[self.a_idx].astype(T), st.gn[self.a_idx, self.e_idx].astype(T)
        den = gp - gq
        with np.errstate(divide="ignore", invalid="ignore"):
            alpha = np.where(np.abs(den) < T(1e-30), T(0.5), np.clip(gp / den, T(0.0), T(1.0)))
        wu, wv = _world(lat, p, T), _world(lat, p + ED[self.e_idx], T)
        self.pts = wu + alpha[:, None] * (wv - wu)


def cluster_points(wts: Weights, labels):
    """(vertices as T, clusters whose weights summed to EPS or less) of a partition, in build_mesh's vertex order."""
    T = wts.T
    leaders = labels == np.arange(14)[None, :]
    flat = leaders.reshape(-1)
    lead_id = np.where(flat, np.cumsum(flat) - 1, -1).reshape(labels.shape)
    n_v = int(flat.sum())
    vid = lead_id[wts.a_idx, labels[wts.a_idx, wts.e_idx]]
    wsum, tw = np.zeros((n_v, 3), T), np.zeros(n_v, T)
    sums, single, cnt = np.zeros((n_v, 3), T), np.zeros((n_v, 3), T), np.zeros(n_v, np.int64)
    for e in range(14):                                            # ascending edge order within every cluster
        sel = wts.e_idx == e
        v = vid[sel]
        wsum[v] = wsum[v] + wts.pts[sel] * wts.w[sel][:, None]
        tw[v] = tw[v] + wts.w[sel]
        sums[v] = sums[v] + wts.pts[sel]
        single[v] = wts.pts[sel]
        cnt[v] += 1
    plain = np.where((cnt == 1)[:, None], single, sums * (T(1.0) / cnt.astype(T))[:, None])
    back = tw <= T(EPS)
    with np.errstate(divide="ignore", invalid="ignore"):
        verts = np.where(back[:, None], plain, wsum * (T(1.0) / tw)[:, None])
    return verts, back


def _result(st, wts, labels, facets, stats, extra=None):
    verts, back = cluster_points(wts, labels)
    out = {"vertices": verts.astype(np.float64), "vertices_T": verts, "facets": facets, "stats": stats, "labels": labels,
           "weights": wts.w, "fallback": wts.none,
           "curvature": dict(zip(STAT_NAMES, [len(wts.w), int(wts.none.sum()), len(verts), int(back.sum())]))}
    out.update(extra or {})
    return out


def extract(lat, field, isovalue, T=np.float64, base=None, st=None):
    """The curvature-weighted mesh after the two passes: the facets, stats and final partition of
    isosurface_cluster_restatement.extract (base, st: that result and its State where the caller has them), the vertices
    of cluster_points; "curvature": the four counts of STAT_NAMES, "weights" / "fallback" per crossed edge."""
    base = base or C.extract(lat, field, isovalue)
    st = st or C.State(lat, field, isovalue)
    return _result(st, Weights(st, T), base["labels"], base["facets"], base["stats"])


def extract_rollback(lat, field, isovalue, extents, T=np.float64):
    """extract() and one round of the self-intersection rollback (isosurface_intersect_restatement.extract with the
    curvature-weighted vertices): also "self_intersections" (X.STAT_NAMES), "before" and "ids"."""
    base = C.extract(lat, field, isovalue)
    st = C.State(lat, field, isovalue)
    wts = Weights(st, T)
    labels = base["labels"].copy()
    _, f, owner = C.build_mesh(st, labels)
    v = cluster_points(wts, labels)[0].astype(np.float64)
    counts = dict.fromkeys(X.STAT_NAMES, 0)
    ids = np.zeros(0, np.int64)
    if len(f):
        ids, c, _ = X.detect(v, f, extents)
        counts.update(zip(X.STAT_NAMES[:5], c))
    before = (v, f)
    vs = np.unique(f[ids].reshape(-1)) if len(ids) else np.zeros(0, np.int64)
    vs = vs[owner[vs, 2] > 1]
    bad = np.unique(owner[vs, 0])
    counts["cluster_vertices"], counts["rolled_back"] = len(vs), len(bad)
    if len(bad):
        labels[bad] = np.where(labels[bad] >= 0, np.arange(14)[None, :], -1)
        _, f, owner = C.build_mesh(st, labels)
    return _result(st, wts, labels, f, base["stats"], {"self_intersections": counts, "before": before, "ids": ids})


def gaps(lat, field, isovalue):
    """(G_v, G_w, the float64 result, the long double result): the largest |v64 - v80| / r over the vertex coordinates
    and the largest relative |w64 - w80| over the crossed edges."""
    base, st = C.extract(lat, field, isovalue), C.State(lat, field, isovalue)
    a, b = extract(lat, field, isovalue, np.float64, base, st), extract(lat, field, isovalue, np.longdouble, base, st)
    gv = float(np.abs(a["vertices_T"].astype(np.longdouble) - b["vertices_T"]).max(initial=0.0) / lat.resolution)
    gw = float((np.abs(a["weights"].astype(np.longdouble) - b["weights"]) / np.abs(b["weights"])).max(initial=0.0))
    return gv, gw, a, b


# ---- the fields of the tests: extents [0, 2]^3 at r = 0.25; the sheet and the plane leave the box through its faces,
# the plane through all six
EXT2 = [0.0, 0.0, 0.0, 2.0, 2.0, 2.0]
R2 = 0.25
FIELDS = ("sphere", "cube", "sheet", "plane")


def analytic(name, w):
    x, y, z = w[..., 0], w[..., 1], w[..., 2]
    if name == "sphere":
        return np.sqrt((x - 1.0) ** 2 + (y - 1.0) ** 2 + (z - 1.0) ** 2) - 0.8
    if name == "cube":
        return np.maximum(np.maximum(np.abs(x - 1.0), np.abs(y - 1.0)), np.abs(z - 1.0)) - 0.6
    if name == "sheet":
        return z - 1.0 - 0.2 * np.sin(3.0 * x) * np.cos(2.5 * y)
    if name == "plane":
        return 0.5 * (x - 1.0) + 0.6 * (y - 1.0) + 0.8 * (z - 1.0) + 0.05
    raise KeyError(name)


def bars(gv, gw, resolution):
    """The bars of the device tests: 200 * max(G, 1e-15), per vertex coordinate times r, per weight relative."""
    return 200.0 * max(gv, 1e-15) * resolution, 200.0 * max(gw, 1e-15)
