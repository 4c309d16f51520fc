"""Stage 2 of M2L in the parity basis of two axes on the device: a handle with BBFMM_M2L_S2_AXES=2 against one with =1
(the x pairs alone) and one with BBFMM_M2L_S2_PAIRS=0 (the plain slot layout and the node-basis kernel), and all three
against the oracle run on the product's operators.  Harness, shapes and tolerances are those of
test_gpu_m2l_pairs_stage2.py, for the same reason: the layouts differ by exact factors, the summation order and one rounding
per combined entry.  Added to those shapes: orders 6, 8 and 9 on a small lattice and order 10 in 2-D, the smallest cases that
reach the other kernel instances and several chunks per half.  Every case asserts through debug_m2l_pairs_axes(stage=2) that y pairs are present, so none can pass
by falling back to the one-axis layout."""
import numpy as np
import pytest

import ferreus_rbf_rs_amd as F
from conftest import clustered_points, inject_product_operators, relerr
from test_gpu_m2l_pairs import LATTICE_PARAMS, lattice, matvec, oracle_tree

pytestmark = pytest.mark.gpu


def handle(pts, order, params, s2_axes, monkeypatch, kernel=(0, 1.0, 1.0), deterministic=False, **env):
    """s2_axes: 2, 1 or 0 (stage-2 pairs off).  The switches and the table options are read when a handle is created."""
    env = dict(env, BBFMM_M2L_S2_PAIRS="0" if s2_axes == 0 else "1")
    if s2_axes:
        env["BBFMM_M2L_S2_AXES"] = str(s2_axes)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    t = F.FmmTree(pts, order, F.KernelParams(F.KernelType(kernel[0]), base_range=kernel[1], total_sill=kernel[2]), True, True,
                  params=F.FmmParams(*params), deterministic=deterministic)
    for k in env:
        monkeypatch.delenv(k)
    info, ops = t.debug_m2l_pairs_axes(stage=2)
    assert info["axes"] == s2_axes
    assert all(bool(op["y_pairs"]) == (s2_axes == 2) for op in ops) and ops
    return t


def check(key, pts, order, params, nrhs, monkeypatch, seed, parts=False, kernel=(0, 1.0, 1.0), deterministic=False, **env):
    """Two axes against one axis and against pairs off at 1e-12; the error of two axes against the oracle no worse than
    that of the plain layout."""
    n = pts.shape[0]
    w = np.random.default_rng(seed).standard_normal((n, nrhs))
    t_xy = handle(pts, order, params, 2, monkeypatch, kernel, deterministic, **env)
    t_x = handle(pts, order, params, 1, monkeypatch, kernel, deterministic, **env)
    t_off = handle(pts, order, params, 0, monkeypatch, kernel, deterministic, **env)
    r = oracle_tree((key, order, kernel), pts, order, params, kernel)
    inject_product_operators(t_xy, r)  # (the handles compute the same operators: the switches only change the tables)
    r.set_weights(w)
    y_ref = r.evaluate(w, pts)
    y_off, y_x, y_xy = matvec(t_off, w), matvec(t_x, w), matvec(t_xy, w)  # (two axes last: debug_m2l_s2_last_ksplit)
    e = {"xy vs x": relerr(y_xy, y_x), "xy vs off": relerr(y_xy, y_off), "xy vs oracle": relerr(y_xy, y_ref),
         "x vs oracle": relerr(y_x, y_ref), "off vs oracle": relerr(y_off, y_ref)}
    print(", ".join(f"{k} {v:.2e}" for k, v in e.items()))
    assert np.isfinite(y_xy).all()
    assert e["xy vs x"] < 1e-12 and e["xy vs off"] < 1e-12
    assert e["xy vs oracle"] <= 1.05 * e["off vs oracle"] + 1e-13
    assert e["x vs oracle"] <= 1.05 * e["off vs oracle"] + 1e-13
    if parts:  # the shares of a 3-way partition on the one device
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


@pytest.mark.parametrize("order", [3, 5, 7])
def test_lattice_full_and_short_tiles_interior_and_face_cells(order, monkeypatch):
    """Orders 3 (one group per part: the chunks of 1 + 1), 5 (centre planes on both axes; 3 + 2 and 2 + 2) and 7 (the
    headline's chunks of 7 + 6 and 6 + 4 groups).  Cells of the x and y faces have pairs with one member absent."""
    pts = lattice(np.random.default_rng(50), 16, 3, 3)
    t = check("lattice3", pts, order, LATTICE_PARAMS, 1, monkeypatch, 51)
    assert t.stats().depth == 4


def test_even_order(monkeypatch):
    """Order 4: no centre plane, 2 + 2 and 2 + 2 groups."""
    pts = lattice(np.random.default_rng(50), 16, 3, 3)
    check("lattice3", pts, 4, LATTICE_PARAMS, 1, monkeypatch, 52)


@pytest.mark.parametrize("order", [6, 8, 9])
def test_orders_of_the_other_instances_and_several_chunks_per_half(order, monkeypatch):
    """Order 6: one chunk of 4 + 4 groups per half.  Order 8: two chunks of 4 + 4 per half, so a part is spread over the
    chunks.  Order 9: two chunks of 8 + 6 and two of 6 + 5, parts of unequal length, the last chunks partly padding.  A
    lattice of 8^3 cells (levels 2 and 3: interior, face, edge and corner cells) keeps the operators of these orders small."""
    pts = lattice(np.random.default_rng(54), 8, 3, 3)
    check("lattice3_8", pts, order, LATTICE_PARAMS, 1, monkeypatch, 54)


def test_two_dimensions(monkeypatch):
    pts = lattice(np.random.default_rng(52), 64, 2, 3)
    check("lattice2", pts, 6, LATTICE_PARAMS, 1, monkeypatch, 53)


def test_two_dimensions_two_groups_per_part(monkeypatch):
    """Order 10 in 2-D: 25 representatives per part, chunks of 2 + 2 groups."""
    pts = lattice(np.random.default_rng(52), 32, 2, 3)
    check("lattice2_32", pts, 10, LATTICE_PARAMS, 1, monkeypatch, 56)


def test_three_right_hand_sides(monkeypatch):
    pts = lattice(np.random.default_rng(50), 16, 3, 3)
    check("lattice3", pts, 5, LATTICE_PARAMS, 3, monkeypatch, 55)


def test_clustered_cloud_mixed_levels_and_skipped_steps(monkeypatch):
    pts = np.unique(clustered_points(np.random.default_rng(56), 6000, 3), axis=0)
    check("clustered3", pts, 5, (30, 2, 1e-7, 1024), 1, monkeypatch, 57)


def test_several_batches_and_a_level_cut_into_groups(monkeypatch):
    """Zero segments of absent members on the new offsets; the buffer holds another batch's values otherwise."""
    pts = lattice(np.random.default_rng(50), 16, 3, 3)
    t = check("lattice3", pts, 4, LATTICE_PARAMS, 1, monkeypatch, 59, BBFMM_M2L_CBUF_MB="8")
    assert any(op["kind"] == 1 for op in t.debug_m2l_pairs()[1])  # group operators


def test_parts_of_a_three_way_partition(monkeypatch):
    pts = lattice(np.random.default_rng(50), 16, 3, 3)
    check("lattice3", pts, 5, LATTICE_PARAMS, 1, monkeypatch, 61, parts=True)


def small_cloud():
    return np.random.default_rng(64).random((3000, 3))


def test_small_tree_takes_the_contraction_split(monkeypatch):
    """About 3000 points: so few tiles that stage 2 splits the contraction and the parts add with atomics."""
    pts = small_cloud()
    t = check("small3", pts, 5, (30, 2, 1e-7, 1024), 1, monkeypatch, 65)
    ksplit = t.debug_m2l_s2_last_ksplit()
    print(f"ksplit {ksplit}")
    assert ksplit > 1


def test_small_tree_on_a_deterministic_handle(monkeypatch):
    """BBFMM_FLAG_DETERMINISTIC: no split of the contraction, plain stores; two matvecs agree bit for bit."""
    pts = small_cloud()
    t = check("small3", pts, 5, (30, 2, 1e-7, 1024), 1, monkeypatch, 67, deterministic=True)
    assert t.debug_m2l_s2_last_ksplit() == 1
    w = np.random.default_rng(68).standard_normal((pts.shape[0], 1))
    assert (matvec(t, w) == matvec(t, w)).all()


def test_ranks_so_low_that_a_step_holds_many_vectors(monkeypatch):
    """A Gaussian with a short range: rank <= 2 on the fine levels, eight transfer vectors per 16-step."""
    pts = np.unique(clustered_points(np.random.default_rng(62), 6000, 3), axis=0)
    t = check("clustered3", pts, 5, (40, 2, 1e-5, 1024), 1, monkeypatch, 63, kernel=(100, 0.5, 0.4))
    assert t.m2l_ranks()[t.stats().depth].max() <= 2


@pytest.mark.parametrize("s1_pairs,s1_axes", [("0", "1"), ("1", "1"), ("1", "2")])
def test_switch_combinations(s1_pairs, s1_axes, monkeypatch):
    """Stage 2 on two axes, on one axis and off (inside check), with stage 1 off, on one axis and on two axes: the
    combinations of S1_PAIRS x S1_AXES x S2_PAIRS x S2_AXES (an AXES switch says nothing while its PAIRS switch is off)."""
    pts = lattice(np.random.default_rng(50), 16, 3, 3)
    t = check("lattice3", pts, 5, LATTICE_PARAMS, 1, monkeypatch, 69, BBFMM_M2L_S1_PAIRS=s1_pairs, BBFMM_M2L_S1_AXES=s1_axes)
    assert t.debug_m2l_pairs_axes()[0]["axes"] == (int(s1_axes) if s1_pairs == "1" else 0)
