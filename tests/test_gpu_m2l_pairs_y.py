"""Stage 1 of M2L in the parity basis of two axes on the device: a handle with
BBFMM_M2L_S1_AXES=2 against one with the x pairs alone (= 1) and one with the pairing off, and all three against the
oracle run on the product's operators.  Harness, shapes and tolerances are those of test_gpu_m2l_pairs.py."""
import numpy as np
import pytest

import ferreus_rbf_rs_amd as F
from conftest import clustered_points, inject_product_operators, relerr
from test_gpu_m2l_pairs import LATTICE_PARAMS, lattice, matvec, oracle_tree

pytestmark = pytest.mark.gpu


def handle(pts, order, params, axes, monkeypatch, kernel=(0, 1.0, 1.0), **env):
    """axes: 2, 1, or 0 for the pairing off.  The switches and the table options are read when a handle is created."""
    monkeypatch.setenv("BBFMM_M2L_S1_PAIRS", "1" if axes else "0")
    monkeypatch.setenv("BBFMM_M2L_S1_AXES", str(max(axes, 1)))
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    t = F.FmmTree(pts, order, F.KernelParams(F.KernelType(kernel[0]), base_range=kernel[1], total_sill=kernel[2]), True, True,
                  params=F.FmmParams(*params))
    for k in env:
        monkeypatch.delenv(k)
    monkeypatch.delenv("BBFMM_M2L_S1_PAIRS")
    monkeypatch.delenv("BBFMM_M2L_S1_AXES")
    assert t.debug_m2l_pairs_axes()[0]["axes"] == axes
    return t


def check(key, pts, order, params, nrhs, monkeypatch, seed, parts=False, want_groups=False, kernel=(0, 1.0, 1.0), **env):
    """y of the two-axis handle against the one-axis handle and against the unpaired one at 1e-12 (summation order and one
    rounding per level of a combined entry: a few n eps); its error against the oracle no worse than either of theirs."""
    n = pts.shape[0]
    w = np.random.default_rng(seed).standard_normal((n, nrhs))
    t_xy, t_x, t_off = (handle(pts, order, params, axes, monkeypatch, kernel, **env) for axes in (2, 1, 0))
    ops = t_xy.debug_m2l_pairs_axes()[1]
    assert any(op["y_pairs"] for op in ops)
    if want_groups:  # a level cut into groups of target classes: its sources have one stage-1 operator per group
        assert any(op["kind"] == 1 and op["y_pairs"] for op in ops)
    r = oracle_tree((key, order, kernel), pts, order, params, kernel)
    inject_product_operators(t_xy, r)  # (the handles compute the same operators: the switches only change the tables)
    r.set_weights(w)
    y_ref = r.evaluate(w, pts)
    y_xy, y_x, y_off = matvec(t_xy, w), matvec(t_x, w), matvec(t_off, w)
    e_x, e_off = relerr(y_xy, y_x), relerr(y_xy, y_off)
    o_xy, o_x, o_off = relerr(y_xy, y_ref), relerr(y_x, y_ref), relerr(y_off, y_ref)
    print(f"xy vs x {e_x:.2e}, xy vs off {e_off:.2e}; vs oracle: xy {o_xy:.2e}, x {o_x:.2e}, off {o_off:.2e}")
    assert np.isfinite(y_xy).all()
    assert e_x < 1e-12
    assert e_off < 1e-12
    assert o_xy <= 1.05 * o_x + 1e-13
    assert o_xy <= 1.05 * o_off + 1e-13
    if parts:  # the shares of a 3-way partition on the one device (whole-operator tiles and own-block tiles)
        import torch
        dw = torch.from_numpy(np.ascontiguousarray(w.T)).cuda()
        acc = torch.full((nrhs, n), float("nan"), dtype=torch.float64, device="cuda")
        for rank in range(3):
            t_xy.set_partition(rank, 3)
            rows = torch.from_numpy(t_xy.partition_rows()).cuda()
            tmp = torch.zeros((nrhs, n), dtype=torch.float64, device="cuda")
            t_xy.matvec_device(dw.data_ptr(), n, nrhs, tmp.data_ptr(), n, True)
            acc[:, rows] = tmp[:, rows]
        t_xy.set_partition(0, 1)
        e_parts = relerr(acc.cpu().numpy().T, y_xy)
        print(f"parts vs full {e_parts:.2e}")
        assert e_parts < 1e-13  # as test_gpu_exchange.py demands of partial against full plans
    return t_xy


@pytest.mark.parametrize("order", [4, 5, 7])
def test_lattice_full_and_short_tiles_interior_and_boundary_cells(order, monkeypatch):
    """Orders 4 (even: no centre plane), 5 (centre planes on both axes) and 7 (the headline's contraction and block
    shapes).  The 16^3 level has interior, face and edge cells of both axes, hence boundary variants with y pairs of
    vectors whose x partner is gone."""
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
    """A Gaussian with a short range: rank 2 on the fine levels, where the tables start a new block early (the slot
    window), also among the y pairs."""
    pts = np.unique(clustered_points(np.random.default_rng(62), 6000, 3), axis=0)
    t = check("clustered3", pts, 5, (40, 2, 1e-5, 1024), 1, monkeypatch, 63, kernel=(100, 0.5, 0.4))
    ranks = t.m2l_ranks()
    assert ranks[t.stats().depth].max() <= 2


@pytest.mark.parametrize("s2_pairs", ["0", "1"])
def test_both_settings_of_the_stage_2_pairs(s2_pairs, monkeypatch):
    pts = lattice(np.random.default_rng(50), 16, 3, 3)
    t = check("lattice3", pts, 5, LATTICE_PARAMS, 1, monkeypatch, 65, BBFMM_M2L_S2_PAIRS=s2_pairs)
    assert t.debug_m2l_pairs(stage=2)[0] == (s2_pairs == "1")
