"""Stage 2 of M2L in the parity basis of the x reflection on the device: handles with the pairing on (BBFMM_M2L_S2_PAIRS
unset) and off (= 0: the plain slot layout and the node-basis kernel instance) against each other and against the oracle
run on the product's operators.  The harness and the tolerances are those of test_gpu_m2l_pairs.py, for the same reason:
summation order and one rounding per combined entry.  The shapes are the smallest at which each piece can go wrong."""
import numpy as np
import pytest

import ferreus_rbf_rs_amd as F
from conftest import clustered_points, inject_product_operators, relerr
from test_gpu_m2l_pairs import LATTICE_PARAMS, lattice, matvec, oracle_tree

pytestmark = pytest.mark.gpu


def handle(pts, order, params, s2, monkeypatch, kernel=(0, 1.0, 1.0), s1=None, deterministic=False, **env):
    """Both switches and the table options are read when a handle is created."""
    env = dict(env, BBFMM_M2L_S2_PAIRS="1" if s2 else "0")
    if s1 is not None:
        env["BBFMM_M2L_S1_PAIRS"] = "1" if s1 else "0"
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    t = F.FmmTree(pts, order, F.KernelParams(F.KernelType(kernel[0]), base_range=kernel[1], total_sill=kernel[2]), True, True,
                  params=F.FmmParams(*params), deterministic=deterministic)
    for k in env:
        monkeypatch.delenv(k)
    assert t.debug_m2l_pairs(stage=2)[0] == s2
    if s1 is not None:
        assert t.debug_m2l_pairs()[0] == s1
    return t


def check(key, pts, order, params, nrhs, monkeypatch, seed, parts=False, kernel=(0, 1.0, 1.0), s1=None, deterministic=False, **env):
    """y_on against y_off at 1e-12, the error of y_on against the oracle no worse than that of y_off."""
    n = pts.shape[0]
    w = np.random.default_rng(seed).standard_normal((n, nrhs))
    t_on = handle(pts, order, params, True, monkeypatch, kernel, s1, deterministic, **env)
    t_off = handle(pts, order, params, False, monkeypatch, kernel, s1, deterministic, **env)
    r = oracle_tree((key, order, kernel), pts, order, params, kernel)
    inject_product_operators(t_on, r)  # (both handles compute the same operators: the switch only changes the tables)
    r.set_weights(w)
    y_ref = r.evaluate(w, pts)
    y_off, y_on = matvec(t_off, w), matvec(t_on, w)  # (on last: debug_m2l_s2_last_ksplit then speaks of t_on's launches)
    e_pair, e_on, e_off = relerr(y_on, y_off), relerr(y_on, y_ref), relerr(y_off, y_ref)
    print(f"on vs off {e_pair:.2e}, on vs oracle {e_on:.2e}, off vs oracle {e_off:.2e}")
    assert np.isfinite(y_on).all()
    assert e_pair < 1e-12
    assert e_on <= 1.05 * e_off + 1e-13
    if parts:  # the shares of a 3-way partition on the one device
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


@pytest.mark.parametrize("order", [4, 5, 7])
def test_lattice_full_and_short_tiles_interior_and_face_cells(order, monkeypatch):
    """Orders 4 (even: no centre plane; 2 + 2 column groups), 5 (centre plane; 5 + 4) and 7 (the headline's chunks of 13
    and 10 groups).  Cells of both x faces have pairs with one member absent."""
    pts = lattice(np.random.default_rng(50), 16, 3, 3)
    t = check("lattice3", pts, order, LATTICE_PARAMS, 1, monkeypatch, 51)
    assert t.stats().depth == 4


def test_two_dimensions(monkeypatch):
    pts = lattice(np.random.default_rng(52), 64, 2, 3)
    check("lattice2", pts, 6, LATTICE_PARAMS, 1, monkeypatch, 53)


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


@pytest.mark.parametrize("s1", [False, True])
def test_switch_combinations(s1, monkeypatch):
    """Stage 2 on against off, with stage 1 off and on: all four combinations of the two switches."""
    pts = lattice(np.random.default_rng(50), 16, 3, 3)
    check("lattice3", pts, 5, LATTICE_PARAMS, 1, monkeypatch, 69, s1=s1)
