"""The code a device group (csrc/device_group.cpp) runs when its parts sit on DIFFERENT devices, run on one device.

With `devices=[0] * parts` every part shares device 0's one copy of the weights (owner 0), so the other owners' copies, the
weight mirrors fed by the pool threads of FmmTree::stage_weights_to_device, the peer copies of weights, slots and blocks and the
threaded creation of the parts never run.  BBFMM_GROUP_OWN_COPIES=1 (read when the group is created) gives every part a logical
device of its own: owner = g, a mirror per part, peer copies between parts -- the physical device stays 0 in every HIP call.
Real peer access, hipSetDevice between distinct devices and events across devices are still not executed.

Bars: the switch changes where data is read from, never the arithmetic -- on deterministic handles the group under the switch
equals the group without it BIT FOR BIT; both equal the one-part handle to 1e-12 and the oracle on the product's operators to
1e-11 (the bars of test_gpu_device_group.py; gradients 1e-10 there and here).  bbfmm_debug_group_state shows that the paths
ran, and that the primary holds no weight mirror outside DeviceGroup::stage(): the list named the other parts' buffers as they
were during one staging, and a list left behind sent the weights of a call the primary served alone to the other parts --
after set_weights(k=1), matvec_device(k=2), evaluate(other weights, k=2) towards memory the parts had freed."""
import gc
import os
import subprocess
import sys

import numpy as np
import pytest

import ferreus_rbf_rs_amd as F
from conftest import clustered_points, inject_product_operators, relerr
from oracle import bbfmm_oracle as O

pytestmark = pytest.mark.gpu
TOL = 1e-11          # against the oracle
SAME = 1e-12         # against the one-part handle
GRAD = 1e-10         # gradients against the one-part handle
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORDER = 4
SWITCH = "BBFMM_GROUP_OWN_COPIES"


def group(monkeypatch, pts, kp, parts, own, order=ORDER, adaptive=True):
    """A deterministic group of logical parts on device 0, with or without the switch (read when the group is created)."""
    if own:
        monkeypatch.setenv(SWITCH, "1")
    else:
        monkeypatch.delenv(SWITCH, raising=False)
    g = F.FmmTree(pts, order, kp, adaptive, True, devices=[0] * parts, deterministic=True)
    monkeypatch.delenv(SWITCH, raising=False)
    st = g.debug_group_state()
    assert st["parts"] == parts and st["own_copies"] == bool(own) and st["live_mirrors"] == 0
    assert st["owners"] == (list(range(parts)) if own else [0] * parts)
    return g


def no_mirror_left(g):
    st = g.debug_group_state()
    assert st["live_mirrors"] == 0, st
    return st


def between_parts(st):
    """Copies queued between two parts under the switch: peer copies, or -- where the runtime takes no peer copy within one
    device -- the plain copies that serve in their place (then no peer copy was ever queued)."""
    assert st["own_copies"]
    assert st["peer_copies" if st["self_peer_refused"] else "plain_copies"] == 0, st
    return st["peer_copies"] + st["plain_copies"]


@pytest.fixture(scope="module")
def cloud():
    rng = np.random.default_rng(707)
    pts = np.vstack([rng.random((12000, 3)), clustered_points(rng, 3000, 3)])      # mixed levels: W / X lists live
    n = len(pts)
    kp = F.KernelParams(F.FmmKernelType.LinearRbf)
    one = F.FmmTree(pts, ORDER, kp, True, True, deterministic=True)
    assert one.stats().n_w > 0 and one.device_count() == 1
    st = one.debug_group_state()
    assert st["parts"] == 1 and st["owners"] == [0] and not st["own_copies"] and not any(
        st[k] for k in ("live_mirrors", "mirror_pieces", "peer_copies", "plain_copies", "weight_waits", "weights_in"))
    ref = O.FmmTree(pts, ORDER, 0, True, True)
    inject_product_operators(one, ref)
    w = {"a": np.asfortranarray(rng.standard_normal((n + 4, 1))),                  # N + basis_size rows (rbf.rs:1344)
         "b": np.asfortranarray(rng.standard_normal((n + 4, 1))),
         "k2": np.asfortranarray(rng.standard_normal((n, 2))),
         "k3": np.asfortranarray(rng.standard_normal((n, 3)))}
    oracle, plain = {}, {}
    for name, v in w.items():                                                      # the references: computed once
        ref.set_weights(v[:n])
        oracle[name] = ref.evaluate(v[:n], pts)
        one.set_weights(v)
        plain[name] = one.evaluate(v, pts)
        assert relerr(plain[name], oracle[name]) < TOL
    poly = np.asfortranarray(np.hstack([np.ones((n, 1)), pts]))
    return {"rng": rng, "pts": pts, "n": n, "kp": kp, "one": one, "ref": ref, "w": w, "oracle": oracle, "plain": plain, "poly": poly}


def check(y_switch, y_default, y_plain, y_oracle=None, same=SAME):
    assert np.array_equal(y_switch, y_default)                                     # where the data is read from, not the arithmetic
    assert relerr(y_switch, y_plain) < same
    if y_oracle is not None:
        assert relerr(y_switch, y_oracle) < TOL


@pytest.mark.parametrize("parts", [2, 3, 5])
def test_the_unchanged_callers_products_with_a_copy_of_the_weights_per_part(cloud, parts, monkeypatch):
    c = cloud
    pts, n, w, poly = c["pts"], c["n"], c["w"], c["poly"]
    gs, gd = group(monkeypatch, pts, c["kp"], parts, True), group(monkeypatch, pts, c["kp"], parts, False)
    out = {}
    for tag, g in (("s", gs), ("d", gd)):
        r = {}
        for name in ("a", "k2", "b"):                                              # K = 1, K = 2, a second product with other weights
            g.set_weights(w[name])
            no_mirror_left(g)
            r[name] = g.evaluate(w[name], pts.copy())                              # a fresh copy of the sources
            assert g.last_evaluate_at_sources() == 1
            no_mirror_left(g)
        r["fmv"] = g.fast_matrix_vector_product(w["a"][:, 0].copy(), basis_size=4, polynomial_matrix=poly, nugget=0.25)
        no_mirror_left(g)
        out[tag] = r
    for name in ("a", "k2", "b"):
        check(out["s"][name], out["d"][name], c["plain"][name], c["oracle"][name])
    tail = 0.25 * w["a"][:n, 0] + poly @ w["a"][n:, 0]
    check(out["s"]["fmv"][:n], out["d"]["fmv"][:n], c["plain"]["a"][:, 0] + tail, c["oracle"]["a"][:, 0] + tail)
    assert np.all(out["s"]["fmv"][n:] == 0.0)
    # the paths ran: four stagings of 1 + 2 + 1 + 1 columns, one 2 MB piece per column at this size, to every other part;
    # no part waited for another part's copy, and every part sent its partial sums to every other part in four exchanges
    st = no_mirror_left(gs)
    assert st["owners"] == list(range(parts))
    assert st["mirror_pieces"] == 5 * (parts - 1) > 0
    assert st["weight_waits"] == 0 and st["weights_in"] == 0
    assert between_parts(st) == 4 * parts * (parts - 1)
    # and without the switch none of it does: one copy on the device, which the other parts wait for
    sd = no_mirror_left(gd)
    assert sd["mirror_pieces"] == 0 and sd["peer_copies"] == 0 and sd["weights_in"] == 0
    assert sd["weight_waits"] == 4 * (parts - 1) and sd["plain_copies"] == 4 * parts * (parts - 1)


@pytest.mark.parametrize("parts", [2, 3, 5])
def test_device_resident_vectors_reach_every_part_by_a_copy_of_its_own(cloud, parts, monkeypatch):
    import torch
    c = cloud
    pts, n, w, one = c["pts"], c["n"], c["w"], c["one"]
    gs, gd = group(monkeypatch, pts, c["kp"], parts, True), group(monkeypatch, pts, c["kp"], parts, False)
    ld = n + 5
    for name, k in (("a", 1), ("k3", 3)):
        dw = torch.full((k, ld), 3.0, dtype=torch.float64, device="cuda")          # the rows past N are no weights
        dw[:, :n] = torch.from_numpy(np.ascontiguousarray(w[name][:n].T))
        res = []
        for t in (gs, gd, one):
            out = torch.full((k, ld), 7.0, dtype=torch.float64, device="cuda")
            torch.cuda.synchronize()
            before = t.debug_group_state()
            t.matvec_device(dw.data_ptr(), ld, k, out.data_ptr(), ld, sync=True)
            st = no_mirror_left(t)
            if t is gs:     # the weights to the other owners column by column, the blocks back, the slots in between
                assert st["weights_in"] - before["weights_in"] == (parts - 1) * k
                assert between_parts(st) - between_parts(before) == (parts - 1) * k + (parts - 1) + parts * (parts - 1)
            else:
                assert st["weights_in"] == 0 and st["peer_copies"] == 0
            o = out.cpu().numpy()
            assert np.all(o[:, n:] == 7.0)                                         # rows past N are left alone
            res.append(np.ascontiguousarray(o[:, :n].T))
        check(res[0], res[1], res[2], c["oracle"][name])
    # a call the first part serves alone right behind it, and a host-buffer product after that
    x = c["rng"].random((300, 3))
    wh = np.asfortranarray(w["k3"])
    check(gs.evaluate(wh, x), gd.evaluate(wh, x), one.evaluate(wh, x))
    assert gs.last_evaluate_path() == 0
    no_mirror_left(gs)
    for g in (gs, gd):
        g.set_weights(w["b"])
    check(gs.evaluate(w["b"], pts), gd.evaluate(w["b"], pts), c["plain"]["b"], c["oracle"]["b"])
    no_mirror_left(gs)


def test_row_sets_first_and_second_sighting_and_the_empty_set(cloud, monkeypatch):
    c = cloud
    pts, n, w, one, poly, rng = c["pts"], c["n"], c["w"], c["one"], c["poly"], c["rng"]
    gs, gd = group(monkeypatch, pts, c["kp"], 3, True), group(monkeypatch, pts, c["kp"], 3, False)
    idx = np.sort(rng.choice(n, n // 7, replace=False))
    idx3 = np.sort(rng.choice(n, n // 5, replace=False))                           # never shown to the patched entry
    wa = w["a"][:, 0].copy()
    w1 = np.asfortranarray(w["a"][:n])
    tail = 0.5 * wa[idx] + poly[idx] @ wa[n:]
    r = {}
    for tag, g in (("s", gs), ("d", gd), ("1", one)):
        q = {}
        q["first"] = g.fast_matrix_vector_product(wa, basis_size=4, target_indices=idx, polynomial_matrix=poly, nugget=0.5)
        q["second"] = g.fast_matrix_vector_product(wa, basis_size=4, target_indices=idx, polynomial_matrix=poly, nugget=0.5)
        if g is not one:
            q["empty"] = g.fast_matrix_vector_product(wa, basis_size=4, target_indices=np.zeros(0, dtype=np.int64))
        g.set_weights(w1)
        q["rows"] = g.evaluate(w1, pts[idx])                                       # a set the patched call has shown
        q["path_rows"] = g.last_evaluate_path()
        g.set_weights(w1)
        q["rows3_first"] = g.evaluate(w1, pts[idx3])                               # first sighting: the first part alone
        q["path3_first"] = g.last_evaluate_path()
        g.set_weights(w1)
        q["rows3_second"] = g.evaluate(w1, pts[idx3])                              # second sighting: dealt to the parts
        q["path3_second"] = g.last_evaluate_path()
        if g is not one:
            no_mirror_left(g)
        r[tag] = q
    for tag in ("s", "d"):
        assert (r[tag]["path_rows"], r[tag]["path3_first"], r[tag]["path3_second"]) == (2, 0, 2)
        assert not r[tag]["empty"].any() and np.count_nonzero(r[tag]["first"]) <= len(idx)
    ya = c["oracle"]["a"]
    for name in ("first", "second"):
        check(r["s"][name], r["d"][name], r["1"][name])
        assert relerr(r["s"][name][idx], ya[idx, 0] + tail) < TOL
    check(r["s"]["rows"], r["d"]["rows"], r["1"]["rows"], ya[idx])
    check(r["s"]["rows3_first"], r["d"]["rows3_first"], r["1"]["rows3_first"], ya[idx3])
    check(r["s"]["rows3_second"], r["d"]["rows3_second"], r["1"]["rows3_second"], ya[idx3])
    assert gs.debug_group_state()["mirror_pieces"] > 0


def test_arbitrary_targets_sharded_over_parts_that_each_read_their_own_copy(cloud, monkeypatch):
    c = cloud
    pts, n, w, one, ref, rng = c["pts"], c["n"], c["w"], c["one"], c["ref"], c["rng"]
    monkeypatch.setenv("BBFMM_GROUP_SHARD_MIN", "1000")                            # (read when the group is created)
    gs, gd = group(monkeypatch, pts, c["kp"], 3, True), group(monkeypatch, pts, c["kp"], 3, False)
    x = rng.random((3301, 3))
    wk = w["k2"]
    r = {}
    for tag, g in (("s", gs), ("d", gd), ("1", one)):
        q = {}
        g.set_weights(wk)
        q["v"] = g.evaluate(wk, x)
        q["path"] = g.last_evaluate_path()
        q["vg"], q["g"] = g.evaluate_with_gradients(wk, x)
        g.set_local_coefficients(wk)
        q["leaves"] = g.evaluate_leaves(wk, x)
        q["path_leaves"] = g.last_evaluate_path()
        if g is not one:
            no_mirror_left(g)
            assert (q["path"], q["path_leaves"]) == (3, 3)
        r[tag] = q
    ref.set_weights(wk)
    v_o = ref.evaluate(wk, x)
    check(r["s"]["v"], r["d"]["v"], r["1"]["v"], v_o)
    check(r["s"]["vg"], r["d"]["vg"], r["1"]["vg"], v_o)
    check(r["s"]["g"], r["d"]["g"], r["1"]["g"], same=GRAD)
    check(r["s"]["leaves"], r["d"]["leaves"], r["1"]["leaves"], v_o)
    st = gs.debug_group_state()
    assert st["weight_waits"] == 0 and st["mirror_pieces"] == 2 * 2                # one staging of two columns to two parts
    assert gd.debug_group_state()["weight_waits"] > 0                              # complete_all: the parts wait for the owner's copy


def test_calls_the_first_part_serves_alone_leave_the_other_parts_copies_alone(cloud, monkeypatch):
    """The sequence that sent weights towards freed memory, and its neighbours: after EVERY call the primary holds no mirror
    and the value is the plain handle's."""
    import torch
    c = cloud
    pts, n, w, one, rng = c["pts"], c["n"], c["w"], c["one"], c["rng"]
    gs = group(monkeypatch, pts, c["kp"], 3, True)
    x50 = rng.random((50, 3))
    w1, w1o = np.asfortranarray(w["a"][:n]), np.asfortranarray(w["b"][:n])
    w2, w2o = w["k2"], np.asfortranarray(rng.standard_normal((n, 2)))
    dw = torch.from_numpy(np.ascontiguousarray(w2.T)).cuda()

    def device_product(t):
        out = torch.zeros((2, n), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        t.matvec_device(dw.data_ptr(), n, 2, out.data_ptr(), n, sync=True)
        return out.cpu().numpy().T

    def step(call, path=None, refused=None):
        ys, errs = [], []
        for t in (gs, one):
            try:
                ys.append(call(t))
                errs.append(None)
            except ValueError as e:
                ys.append(None)
                errs.append(str(e))
        st = no_mirror_left(gs)
        if refused is not None:                                                    # a refusal is the same refusal on both
            assert errs[0] is not None and errs[1] is not None and refused in errs[0] and refused in errs[1], errs
        else:
            assert errs == [None, None], errs
            if ys[0] is not None:
                assert relerr(ys[0], ys[1]) < SAME
        if path is not None:
            assert gs.last_evaluate_path() == path
        return st

    # set_weights(k=1), matvec_device(k=2) -- every part's copy grows --, evaluate(other weights, k=2, 50 targets)
    step(lambda t: t.set_weights(w1))
    step(device_product, 1)
    pieces = step(lambda t: t.evaluate(w2o, x50), 0)["mirror_pieces"]
    assert pieces == 2                                                             # the one staging of set_weights: nothing since
    step(lambda t: t.evaluate(w2, pts), None)
    # set_weights(k=2), evaluate(other weights, k=1): refused by both handles, and nothing was sent anywhere;
    # other weights of the same width are the first part's alone
    step(lambda t: t.set_weights(w2))
    assert step(lambda t: t.evaluate(w1o, x50), refused="column count given to set_weights")["mirror_pieces"] == pieces + 4
    assert step(lambda t: t.evaluate(w2o, x50), 0)["mirror_pieces"] == pieces + 4
    # set_weights, a row set never seen (the first part alone), set_weights, the sources (the group again)
    idx = np.sort(rng.choice(n, n // 6, replace=False))
    step(lambda t: t.set_weights(w1))
    step(lambda t: t.evaluate(w1, pts[idx]), 0)
    step(lambda t: t.set_weights(w1))
    y = gs.evaluate(w1, pts)
    assert gs.last_evaluate_path() == 1 and no_mirror_left(gs)["mirror_pieces"] == pieces + 4 + 2 + 2
    assert relerr(y, c["plain"]["a"]) < SAME and relerr(y, c["oracle"]["a"]) < TOL


@pytest.mark.parametrize("n", [2, 300])
def test_tiny_clouds_parts_that_own_no_row_still_hold_a_copy(n, monkeypatch):
    rng = np.random.default_rng(n)
    pts = rng.random((n, 3))
    kp = F.KernelParams(F.FmmKernelType.LinearRbf)
    one = F.FmmTree(pts, ORDER, kp, True, True, deterministic=True)
    gs, gd = group(monkeypatch, pts, kp, 4, True), group(monkeypatch, pts, kp, 4, False)
    if n == 2:
        assert np.count_nonzero(np.diff(gs.group_bounds()) == 0) >= 2              # parts without a row
    w = np.asfortranarray(rng.standard_normal((n, 1)))
    # a tree of depth 0 or 1 has no far field (every leaf touches every other): the sum itself is the reference
    dense = O.dense_sum(0, 1.0, 1.0, pts, pts, w)
    r = []
    for g in (gs, gd, one):
        g.set_weights(w)
        y = g.evaluate(w, pts)
        ym = g.fast_matrix_vector_product(w[:, 0].copy())
        yi = g.fast_matrix_vector_product(w[:, 0].copy(), target_indices=np.arange(0, n, 2))
        r.append((y, ym, yi))
    for a, b, c1 in zip(*r):
        check(a, b, c1)
    assert relerr(r[0][0], dense) < TOL and relerr(r[0][1], dense[:, 0]) < TOL
    st = no_mirror_left(gs)
    assert st["owners"] == [0, 1, 2, 3] and st["mirror_pieces"] == 3 * 3           # three stagings, one column, three other parts


@pytest.mark.parametrize("d,adaptive,kind", [(2, True, "ThinPlateSplineRbf"), (3, False, "CubicRbf")])
def test_two_dimensions_and_a_regular_tree(d, adaptive, kind, monkeypatch):
    rng = np.random.default_rng(50 + d)
    n, order = 9000, 5
    pts = rng.random((n, d))
    kp = F.KernelParams(getattr(F.FmmKernelType, kind))
    one = F.FmmTree(pts, order, kp, adaptive, True, deterministic=True)
    ref = O.FmmTree(pts, order, O.KERNEL_IDS[kind], adaptive, True)
    inject_product_operators(one, ref)
    gs = group(monkeypatch, pts, kp, 4, True, order, adaptive)
    gd = group(monkeypatch, pts, kp, 4, False, order, adaptive)
    w = np.asfortranarray(rng.standard_normal((n, 2)))
    ref.set_weights(w)
    y_o = ref.evaluate(w, pts)
    r = []
    for g in (gs, gd, one):
        g.set_weights(w)
        r.append((g.evaluate(w, pts), g.fast_matrix_vector_product(w[:, 0].copy())))
    check(r[0][0], r[1][0], r[2][0], y_o)
    check(r[0][1], r[1][1], r[2][1], y_o[:, 0])
    st = no_mirror_left(gs)
    assert st["mirror_pieces"] == 3 * 3 and between_parts(st) > 0


def test_one_queueing_thread_and_one_per_part_give_the_same_bits(cloud, monkeypatch):
    import torch
    c = cloud
    pts, n, w = c["pts"], c["n"], c["w"]
    dw = torch.from_numpy(np.ascontiguousarray(w["k3"].T)).cuda()
    res = []
    for threads in (None, "0"):
        if threads is None:
            monkeypatch.delenv("BBFMM_GROUP_THREADS", raising=False)
        else:
            monkeypatch.setenv("BBFMM_GROUP_THREADS", threads)                     # (read when the group is created)
        g = group(monkeypatch, pts, c["kp"], 3, True)
        g.set_weights(w["k2"])
        y = g.evaluate(w["k2"], pts)
        out = torch.zeros((3, n), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        g.matvec_device(dw.data_ptr(), n, 3, out.data_ptr(), n, sync=True)
        st = no_mirror_left(g)
        assert st["mirror_pieces"] == 4 and st["weights_in"] == 6
        res.append((y, out.cpu().numpy().T))
        del g
    assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1])
    assert relerr(res[0][0], c["plain"]["k2"]) < SAME and relerr(res[0][1], c["plain"]["k3"]) < SAME
    assert relerr(res[0][0], c["oracle"]["k2"]) < TOL and relerr(res[0][1], c["oracle"]["k3"]) < TOL


def test_forty_groups_with_a_copy_per_part_give_their_device_memory_back(cloud, monkeypatch):
    """The measure of test_handles_give_their_device_memory_back (scripts/group_lifecycle_check.py): no drift of the device's
    free memory over the second half of the rounds, no steady growth of the resident set."""
    import psutil
    import torch
    c = cloud
    pts, n, w = c["pts"], c["n"], c["w"]
    x = c["rng"].random((3300, 3))
    monkeypatch.setenv("BBFMM_GROUP_SHARD_MIN", "1000")
    dw = torch.from_numpy(np.ascontiguousarray(w["k2"].T)).cuda()
    proc = psutil.Process()
    rounds, free, rss = 40, [], []
    for _ in range(rounds):
        g = group(monkeypatch, pts, c["kp"], 3, True)
        g.set_weights(w["k2"])
        g.evaluate(w["k2"], pts)
        g.evaluate(w["k2"], x)                                                     # sharded: every part completes from its copy
        out = torch.zeros_like(dw)
        g.matvec_device(dw.data_ptr(), n, 2, out.data_ptr(), n, True)
        g.fast_matrix_vector_product(w["a"][:n, 0].copy(), target_indices=np.arange(0, n, 3))
        assert g.debug_group_state()["live_mirrors"] == 0
        del g, out
        gc.collect()
        torch.cuda.empty_cache()
        free.append(torch.cuda.mem_get_info(0)[0])
        rss.append(proc.memory_info().rss)
    half = rounds // 2
    inc = sorted(rss[i + 1] - rss[i] for i in range(half, rounds - 1))
    assert abs(free[half] - free[-1]) / 1e6 < 64 and inc[len(inc) // 2] / 1e6 < 1.0


@pytest.mark.timeout(900)
def test_random_call_sequences_with_a_copy_per_part_equal_the_plain_handle():
    """tests/checks/group_sequence_fuzz.py as test_gpu_device_group.py runs it (sequences, seed, calls per sequence), with the
    switch in the environment: what a group keeps between calls must not show when every part keeps a copy of its own."""
    env = {k: v for k, v in os.environ.items() if not k.startswith("BBFMM_")}
    env[SWITCH] = "1"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "checks", "group_sequence_fuzz.py"), "10", "5", "14"], env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=800)
    lines = p.stdout.decode().strip().splitlines()
    assert p.returncode == 0, "\n".join(l for l in lines if '"ok": false' in l)[:3000] + p.stderr.decode()[-1500:]
    assert '"failures": 0' in lines[-1]
