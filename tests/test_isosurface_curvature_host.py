"""The curvature weight of a crossed lattice edge as the library computes it on the host (the function the device kernel
runs, through bbfmm_isosurface_curvature_weight), against the numpy restatement of its contract
(tests/isosurface_curvature_restatement.py; DESIGN.md "Curvature-weighted clusters").  No GPU.

Tolerances come from the restatement alone: with G_v the largest |v64 - v80| / r over the vertex coordinates of a case and
G_w the largest relative |w64 - w80| over its crossed edges, between the restatement in float64 and in long double, the
bars are 200 * max(G_v, 1e-15) * r per coordinate and 200 * max(G_w, 1e-15) relative per weight."""
import functools
import hashlib
import json
import os

import numpy as np
import pytest

import isosurface_restatement as R
import isosurface_cluster_restatement as C
import isosurface_curvature_restatement as K

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rmt_curvature_tables.json")


@functools.lru_cache(maxsize=None)
def case(name):
    """(lattice, field, G_v, G_w, the float64 restatement, the long double one) of one of the four analytic fields."""
    lat = R.Lattice(K.EXT2, K.R2)
    field = K.analytic(name, lat.world(lat.node_ijk()))
    gv, gw, a, b = K.gaps(lat, field, 0.0)
    return lat, field, gv, gw, a, b


def test_the_library_tables_equal_the_golden_file():
    import ferreus_rbf_rs_amd.isosurface as I
    digest = open(GOLDEN + ".sha256").read().split()[0]
    assert hashlib.sha256(open(GOLDEN, "rb").read()).hexdigest() == digest
    want = {k: v for k, v in json.load(open(GOLDEN)).items() if not k.startswith("_")}
    assert I.curvature_tables() == want
    assert I.CLUSTER_METHODS["curvature"] == 2


@pytest.mark.parametrize("name", K.FIELDS)
def test_the_restatement_in_float64_against_long_double(name):
    lat, field, gv, gw, a, b = case(name)
    print(name, "shape", lat.shape, "G_v", gv, "G_w", gw, a["curvature"], "weights", float(a["weights"].min()),
          float(a["weights"].max()))
    assert gv <= 1e-13
    assert np.array_equal(a["fallback"], b["fallback"])
    assert np.array_equal(a["facets"], b["facets"]) and a["curvature"] == b["curvature"]
    assert a["curvature"]["edges"] > 500 and a["curvature"]["clusters"] < a["curvature"]["edges"]
    # positions only: the facets, the vertex count and the stats are those of the plain clustered mesh
    plain = C.extract(lat, field, 0.0)
    assert np.array_equal(a["facets"], plain["facets"]) and len(a["vertices"]) == len(plain["vertices"])
    assert a["stats"] == plain["stats"]
    moved = np.abs(a["vertices"] - plain["vertices"]).max()
    print("largest move against the mean", moved / lat.resolution, "r")
    if name != "plane":
        assert moved > 1e-6 * lat.resolution          # the weights do something
    assert moved < lat.resolution


def _library_weights(lat, st, wts):
    import ferreus_rbf_rs_amd.isosurface as I
    g = np.where(lat.inE, st.g, np.nan)
    nk, nj, ni = lat.shape
    w, back = np.zeros(len(wts.w)), np.zeros(len(wts.w), bool)
    for t, (o, l) in enumerate(zip(wts.owner, wts.label)):
        vals = np.full(15, np.nan)
        for e in range(-1, 14):
            q = o - lat.lo + (R.ED[e] if e >= 0 else 0)
            if 0 <= q[0] < ni and 0 <= q[1] < nj and 0 <= q[2] < nk:
                vals[e + 1] = g[q[2], q[1], q[0]]
        w[t], back[t] = I.curvature_weight(vals, o, int(l), lat.extents[:3], lat.spacing)
    return w, back


@pytest.mark.parametrize("name", K.FIELDS)
def test_library_weights_on_every_crossed_edge(name):
    lat, field, gv, gw, a, b = case(name)
    st = C.State(lat, field, 0.0)
    wts = K.Weights(st, np.float64)
    w, back = _library_weights(lat, st, wts)
    bar = K.bars(gv, gw, lat.resolution)[1]
    worst = float((np.abs(w - wts.w) / np.abs(wts.w)).max())
    print(name, len(w), "edges,", int(back.sum()), "fallbacks; worst relative gap", worst, "=", worst / bar, "bars; G_w", gw)
    assert np.array_equal(back, wts.none)
    assert worst <= bar
    assert (w[back] == 1.0).all()


# ---- planted stencils: the owner at ijk (2, 4, 6) of a lattice of resolution 0.25, label 0 (three planes) or 1 (two)
LO, SP = np.array([0.1, -0.2, 0.3]), R.spacing(0.25)
OWNER = np.array([2, 4, 6])


def _both(values, label):
    import ferreus_rbf_rs_amd.isosurface as I
    trace = {}
    want = K.weight_of_stencil(values, OWNER, label, LO, SP, np.float64, trace)
    got = I.curvature_weight(values, OWNER, label, LO, SP)
    far = K.weight_of_stencil(values, OWNER, label, LO, SP, np.longdouble)
    gw = float(abs(np.longdouble(want[0]) - far[0]) / abs(far[0]))
    print("library", got, "restatement", want, "G_w", gw, {k: int(v[0]) for k, v in trace.items()})
    assert got[1] == want[1] == far[1]
    assert abs(got[0] - want[0]) <= 200.0 * max(gw, 1e-15) * abs(want[0])       # the bar of this stencil
    return got, {k: int(v[0]) for k, v in trace.items()}


def _smooth(label):
    """d of a gently curved field at the owner and its 14 neighbours: a complete, well-conditioned stencil."""
    x = LO + (OWNER + np.vstack([np.zeros((1, 3), np.int64), R.ED])) * SP
    c = LO + OWNER * SP + [0.3, 0.2, 0.9]
    return np.linalg.norm(x - c, axis=1) - 0.93


@pytest.mark.parametrize("label", range(7))
def test_a_complete_stencil_has_a_weight_of_its_own(label):
    (w, back), trace = _both(_smooth(label), label)
    assert not back and w != 1.0 and 0.0 < w < 1e12
    assert not any(trace.values())


@pytest.mark.parametrize("label", [0, 1])
def test_a_missing_or_non_finite_neighbour_is_the_fallback(label):
    used = sorted({label} | {e for pair in K.PAIRS[label] for e in pair})
    for e in [-1] + used:
        for bad in (np.nan, np.inf, -np.inf):
            v = _smooth(label)
            v[e + 1] = bad
            (w, back), _ = _both(v, label)
            assert back and w == 1.0
    for e in sorted(set(range(14)) - set(used)):          # a neighbour the row does not read may be missing
        v = _smooth(label)
        v[e + 1] = np.nan
        (w, back), _ = _both(v, label)
        assert not back


def test_a_vanishing_denominator_is_the_fallback():
    v = _smooth(0)
    v[1] = v[0] - 1e-12                                    # (d_o - d_a) * |ob| <= EPS
    (w, back), _ = _both(v, 0)
    assert back and w == 1.0
    v[1] = v[0] - 1e-10
    (w, back), _ = _both(v, 0)
    assert not back


@pytest.mark.parametrize("sign", [-1.0, 1.0])
def test_a_divisor_within_eps_of_either_sign_gives_a_right_angle(sign):
    """ratio = cos(phi) + sign * 3e-13 on the first side of the first plane of label 1: theta = sign * pi / 2."""
    label, nb, phi = 1, K.PAIRS[1][0][0], K.PHIS[1][0][0]
    v = _smooth(label)
    x = (OWNER + np.vstack([R.ED[label], R.ED[nb]])) * SP - OWNER * SP
    oa_len, ob_len = np.linalg.norm(x, axis=1)
    ratio = np.cos(phi) + sign * 3e-13
    v[nb + 1] = v[0] - ratio * (v[0] - v[label + 1]) * ob_len / oa_len
    (w, back), trace = _both(v, label)
    assert trace["divisor_small"] == 1 and trace["divisor_negative"] == (1 if sign < 0 else 0)
    assert not back and 0.0 < w < 1e12


def test_a_flat_plane_and_the_cap():
    """Both neighbours of the first plane of label 1 so far from the isovalue that ratio overflows: theta = 0 on both
    sides, 1 / tan(theta) is clamped to 1e12, alpha = 0 gives sin(alpha / 2) <= EPS and beta = 0, and the weight is the
    cap."""
    label = 1
    v = _smooth(label)
    v[label + 1] = v[0] - 1e-11 / np.linalg.norm(SP * R.ED[K.PAIRS[1][0][0]])      # a denominator just over EPS
    for nb in K.PAIRS[1][0]:
        v[nb + 1] = -1e308
    (w, back), trace = _both(v, label)
    assert trace["cot_clamped"] == 2 and trace["flat"] == 1 and trace["capped"] == 1
    assert not back and w == 1e12


def test_an_exactly_linear_field():
    """d = n . x + c sampled on the lattice: the stencil is the same at every sample point up to rounding, so the edges
    of one label share one weight; the library gives what the restatement gives."""
    lat, field, gv, gw, a, b = case("plane")
    st = C.State(lat, field, 0.0)
    wts = K.Weights(st, np.float64)
    w, back = _library_weights(lat, st, wts)
    assert np.array_equal(back, wts.none) and (~back).sum() > 500
    bar = K.bars(gv, gw, lat.resolution)[1]
    for l in range(7):
        sel = (wts.label == l) & ~back
        assert sel.sum() > 10
        ref = float(np.median(wts.w[sel]))
        spread = float(np.abs(w[sel] - ref).max() / ref)
        print("label", l, int(sel.sum()), "edges, weight", ref, "spread", spread)
        assert spread <= 2 * bar
