"""Isosurface extraction on the RMT lattice, the host side (no GPU): the tables fixture, the product's tables against it,
the lattice query against tests/isosurface_restatement.py (SampleLattice::new, lattice.rs:55-96) and refused arguments."""
import hashlib
import json
import os

import numpy as np
import pytest

from conftest import ROOT
import isosurface_restatement as R

GOLDEN = os.path.join(ROOT, "tests", "golden", "rmt_tables.json")


def test_fixture_hash_matches():
    digest = open(GOLDEN + ".sha256").read().split()[0]
    assert hashlib.sha256(open(GOLDEN, "rb").read()).hexdigest() == digest


def test_product_tables_equal_the_fixture():
    from ferreus_rbf_rs_amd import isosurface as I
    ref = json.load(open(GOLDEN))
    got = I.tables()
    for name in ("EDGE_DELTAS", "REVERSE_EDGE", "OWNED_TET_EDGES", "TET_EDGE_PAIRS", "MT_TABLE"):
        assert got[name] == ref[name], name


def test_sample_sublattice_is_the_even_one():
    """U, V, W = EDGE_DELTAS[0], [2], [6] span a sublattice of index 2, and every one has an even coordinate sum:
    the sample points are exactly the ijk with even i + j + k."""
    U, V, W = R.ED[0], R.ED[2], R.ED[6]
    assert abs(round(np.linalg.det(np.stack([U, V, W], 1).astype(float)))) == 2
    assert all(int(v.sum()) % 2 == 0 for v in (U, V, W))
    assert all(int(d.sum()) % 2 == 0 for d in R.ED)          # every edge joins two sample points
    # every tetrahedron edge is a lattice edge (get_edge_owner finds it)
    assert R.TET_LAB.min() >= 0 and R.TET_LAB.max() < 7


@pytest.mark.parametrize("extents,resolution", [
    ([0, 0, 0, 10, 8, 6], 1.0),
    ([-3.2, 1.1, 5.0, 7.7, 2.2, 9.9], 0.37),
    ([0, 0, 0, 0, 0, 0], 1.0),
    ([1.0, 2.0, 3.0, 1.5, 40.0, 3.25], 2.5),
    ([329314.1, 7744801.47, -406.0, 330102.3, 7745390.0, 620.0], 5.0),
])
def test_lattice_query_matches_the_restatement(extents, resolution):
    from ferreus_rbf_rs_amd import isosurface as I
    info = I.lattice_info(extents, resolution)
    lat = R.Lattice(extents, resolution)
    assert info["max_ijk"].tolist() == lat.max_ijk.tolist()
    assert info["n_keys"] == lat.n_keys
    assert info["n_nodes"] == int(lat.inE.sum())
    assert info["lo"].tolist() == lat.lo.tolist()
    assert info["shape"] == lat.shape


def _host_tree(d=3):
    import ferreus_rbf_rs_amd as F
    pts = np.random.default_rng(0).random((300, d))
    return F.FmmTree(pts, 5, F.KernelParams(F.FmmKernelType.LinearRbf), True, True, host_only=True)


@pytest.mark.parametrize("extents,resolution,isovalue,why", [
    ([0, 0, 0, 1, 1, 1], 0.0, 0.0, "resolution"),
    ([0, 0, 0, 1, 1, 1], -1.0, 0.0, "resolution"),
    ([0, 0, 0, 1, 1, 1], float("nan"), 0.0, "resolution"),
    ([0, 0, 0, 1, 1, 1], float("inf"), 0.0, "resolution"),
    ([0, 0, float("nan"), 1, 1, 1], 0.1, 0.0, "finite"),
    ([0, 0, 0, 1, float("inf"), 1], 0.1, 0.0, "finite"),
    ([0, 0, 0, 1, -1, 1], 0.1, 0.0, "inverted"),
    ([0, 0, 0, 1, 1, 1], 0.1, float("nan"), "isovalues"),
])
def test_bad_arguments_are_refused_on_a_host_only_handle(extents, resolution, isovalue, why):
    from ferreus_rbf_rs_amd import _lib as L
    from ferreus_rbf_rs_amd import isosurface as I
    t = _host_tree()
    with pytest.raises(ValueError, match=why):
        t.build_isosurface(extents, resolution, isovalue)
    lib = L.load()
    ext = np.asarray(extents, dtype=np.float64)
    info = np.zeros(11, np.int64)
    iso = np.array([isovalue])
    if why != "isovalues":
        assert lib.bbfmm_isosurface_lattice(t._h, ext.ctypes.data, resolution, info.ctypes.data) == L.BAD_ARGUMENT
        assert why in lib.bbfmm_last_error(t._h).decode()
    vals = np.zeros(16)
    res = __import__("ctypes").c_void_p()
    rc = lib.bbfmm_isosurfaces_from_values(t._h, vals.ctypes.data, ext.ctypes.data, resolution, iso.ctypes.data, 1, 0,
                                           __import__("ctypes").byref(res))
    assert rc == L.BAD_ARGUMENT and why in lib.bbfmm_isosurface_error(res).decode()
    lib.bbfmm_isosurface_destroy(res)
    if why != "isovalues":
        with pytest.raises(ValueError):
            I.lattice_info(extents, resolution)


def test_bad_drift_and_dimension_are_refused():
    t = _host_tree()
    with pytest.raises(ValueError, match="drift"):
        t.build_isosurface([0, 0, 0, 1, 1, 1], 0.1, 0.0, drift=[0.0, float("nan"), 0.0, 0.0])
    t2 = _host_tree(d=2)
    with pytest.raises(ValueError, match="3D"):
        t2.build_isosurface([0, 0, 0, 1, 1, 1], 0.1, 0.0)


def test_host_only_handle_refuses_the_extraction_itself():
    t = _host_tree()
    with pytest.raises(RuntimeError, match="HOST_ONLY"):
        t.build_isosurface([0, 0, 0, 1, 1, 1], 0.1, 0.0)
    from ferreus_rbf_rs_amd import isosurface as I
    shape = I.lattice_info([0, 0, 0, 1, 1, 1], 0.1)["shape"]
    with pytest.raises(RuntimeError, match="HOST_ONLY"):
        I.isosurface_from_values(np.zeros(shape), [0, 0, 0, 1, 1, 1], 0.1, 0.0, tree=t)


def test_affine_drift_folds_translation_and_scale():
    from ferreus_rbf_rs_amd import isosurface as I
    c, t, s = np.array([1.5, 2.0, -3.0, 0.5]), np.array([10.0, 20.0, 30.0]), np.array([2.0, 4.0, 8.0])
    a, b = I.affine_drift(c, t, s)
    x = np.array([3.0, -1.0, 7.0])
    assert a + b @ x == pytest.approx(c[0] + c[1:] @ ((x - t) / s), rel=1e-14)
    assert I.affine_drift([4.0]) [0] == 4.0
