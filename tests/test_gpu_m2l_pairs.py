"""Stage 1 of M2L in the parity basis of the x reflection on the device: handles with the pairing on
(BBFMM_M2L_S1_PAIRS unset) and off (= 0: every vector a single, the unpaired kernel instance) against each other and
against the oracle run on the product's operators.  The shapes are the smallest at which each piece can go wrong."""
import numpy as np
import pytest

import ferreus_rbf_rs_amd as F
from conftest import clustered_points, inject_product_operators, relerr
from oracle import bbfmm_oracle as O

pytestmark = pytest.mark.gpu


def lattice(rng, m, d, per_cell):
    g = np.stack(np.meshgrid(*[np.arange(m)] * d, indexing="ij"), -1).reshape(-1, d)[:, None, :]
    return ((g + 0.15 + 0.7 * rng.random((m ** d, per_cell, d))).reshape(-1, d)) / m


def handle(pts, order, params, pairs, monkeypatch, kernel=(0, 1.0, 1.0), **env):
    """The switch and the table options are read when a handle is created."""
    monkeypatch.setenv("BBFMM_M2L_S1_PAIRS", "1" if pairs else "0")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    t = F.FmmTree(pts, order, F.KernelParams(F.KernelType(kernel[0]), base_range=kernel[1], total_sill=kernel[2]), True, True,
                  params=F.FmmParams(*params))
    for k in env:
        monkeypatch.delenv(k)
    monkeypatch.delenv("BBFMM_M2L_S1_PAIRS")
    assert t.debug_m2l_pairs()[0] == pairs
    return t


def matvec(t, w):
    import torch
    n, k = w.shape
    dw = torch.from_numpy(np.ascontiguousarray(w.T)).cuda()
    out = torch.zeros((k, n), dtype=torch.float64, device="cuda")
    t.matvec_device(dw.data_ptr(), n, k, out.data_ptr(), n, True)
    return out.cpu().numpy().T


_ORACLE = {}  # the oracle's tree of a cloud (seconds of Python): built once, shared by the tests on that cloud and order


def oracle_tree(key, pts, order, params, kernel):
    if key not in _ORACLE:
        _ORACLE[key] = O.FmmTree(pts, order, kernel[0], True, True, None, O.FmmParams(*params), base_range=kernel[1], total_sill=kernel[2])
    return _ORACLE[key]


def check(key, pts, order, params, nrhs, monkeypatch, seed, parts=False, want_groups=False, kernel=(0, 1.0, 1.0), **env):
    """y_on against y_off at 1e-12 (summation order and one rounding per combined entry: a few n eps), the error of
    y_on against the oracle no worse than that of y_off."""
    n = pts.shape[0]
    w = np.random.default_rng(seed).standard_normal((n, nrhs))
    t_on = handle(pts, order, params, True, monkeypatch, kernel, **env)
    t_off = handle(pts, order, params, False, monkeypatch, kernel, **env)
    if want_groups:  # a level cut into groups of target classes: its sources have one stage-1 operator per group
        assert any(op["kind"] == 1 and op["pairs"] for op in t_on.debug_m2l_pairs()[1])
    r = oracle_tree((key, order, kernel), pts, order, params, kernel)
    inject_product_operators(t_on, r)  # (both handles compute the same operators: the switch only changes the tables)
    r.set_weights(w)
    y_ref = r.evaluate(w, pts)
    y_on, y_off = matvec(t_on, w), matvec(t_off, w)
    e_pair, e_on, e_off = relerr(y_on, y_off), relerr(y_on, y_ref), relerr(y_off, y_ref)
    print(f"on vs off {e_pair:.2e}, on vs oracle {e_on:.2e}, off vs oracle {e_off:.2e}")
    assert np.isfinite(y_on).all()
    assert e_pair < 1e-12
    assert e_on <= 1.05 * e_off + 1e-13
    if parts:  # the shares of a 3-way partition on the one device (whole-operator tiles and own-block tiles)
        import torch
        dw = torch.from_numpy(np.ascontiguousarray(w.T)).cuda()
        acc = torch.full((nrhs, n), float("nan"), dtype=torch.float64, device="cuda")
        for rank in range(3):
            t_on.set_partition(rank, 3)
            rows = torch.from_numpy(t_on.partition_rows()).cuda()
            tmp = torch.zeros((nrhs, n), dtype=torch.float64, device="cuda")
            t_on.matvec_device(dw.data_ptr(), n, nrhs, tmp.data_ptr(), n, True)
            acc[:, rows] = tmp[:, rows]
        t_on.set_partition(0, 1)
        e_parts = relerr(acc.cpu().numpy().T, y_on)
        print(f"parts vs full {e_parts:.2e}")
        assert e_parts < 1e-13  # as test_gpu_exchange.py demands of partial against full plans
    return t_on


LATTICE_PARAMS = (6, 2, 1e-7, 1024)  # leaf limit 6 over 3 points per lattice cell: depth 4, 512 cells per class at level 4


@pytest.mark.parametrize("order", [4, 5, 7])
def test_lattice_full_and_short_tiles_interior_and_boundary_cells(order, monkeypatch):
    """Orders 4 (even: no centre plane), 5 (centre plane) and 7 (the headline's contraction and block shapes)."""
    pts = lattice(np.random.default_rng(50), 16, 3, 3)
    t = check("lattice3", pts, order, LATTICE_PARAMS, 1, monkeypatch, 51)
    assert t.stats().depth == 4


def test_two_dimensions(monkeypatch):
    pts = lattice(np.random.default_rng(52), 64, 2, 3)
    check("lattice2", pts, 6, LATTICE_PARAMS, 1, monkeypatch, 53)


def test_three_right_hand_sides(monkeypatch):
    pts = lattice(np.random.default_rng(50), 16, 3, 3)
    check("lattice3", pts, 5, LATTICE_PARAMS, 3, monkeypatch, 55)


def test_clustered_cloud_mixed_levels_and_short_tiles(monkeypatch):
    pts = np.unique(clustered_points(np.random.default_rng(56), 6000, 3), axis=0)
    check("clustered3", pts, 5, (30, 2, 1e-7, 1024), 1, monkeypatch, 57)


def test_level_cut_into_groups(monkeypatch):
    pts = lattice(np.random.default_rng(50), 16, 3, 3)
    check("lattice3", pts, 4, LATTICE_PARAMS, 1, monkeypatch, 59, want_groups=True, BBFMM_M2L_CBUF_MB="8")


def test_parts_of_a_three_way_partition(monkeypatch):
    pts = lattice(np.random.default_rng(50), 16, 3, 3)
    check("lattice3", pts, 5, LATTICE_PARAMS, 1, monkeypatch, 61, parts=True)


def test_ranks_so_low_that_a_column_block_spans_more_vectors_than_the_slot_table(monkeypatch):
    """A Gaussian with a short range: rank 2 on the fine levels, where 160 columns of pairs would span 160 list positions --
    more than the kernel's slot table (kM2lSlotWindow = 128) holds.  The tables then start a new block early."""
    pts = np.unique(clustered_points(np.random.default_rng(62), 6000, 3), axis=0)
    t = check("clustered3", pts, 5, (40, 2, 1e-5, 1024), 1, monkeypatch, 63, kernel=(100, 0.5, 0.4))
    ranks = t.m2l_ranks()
    assert ranks[t.stats().depth].max() <= 2

