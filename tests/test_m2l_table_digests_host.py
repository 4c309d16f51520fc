"""The integer M2L tables pinned family by family: FmmTree.debug_m2l_table_digests() against
tests/golden/m2l_table_digests.json.  The other host tests hold the tables to their definition and the host walk to the
oracle; the walk does not read the active-step lists or the split of the stage-2 tiles, and a definition does not show that
an ordering stayed as it was.  A change that means to move the tables records the file anew,

    python tests/test_m2l_table_digests_host.py --record tests/golden/m2l_table_digests.json

and the file's diff shows which families of which configurations moved.  Beside the digests the file keeps the operator
ranks, the depth and the cell count of every configuration: where those differ the ACA ran differently on this machine and
the recorded digests say nothing about the tables.  Every configuration uses the default kernel of the neighbouring tests
(sums, products and square roots only).  No GPU."""
import contextlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

if __name__ == "__main__":  # recording / printing: what conftest.py does for pytest
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import ferreus_rbf_rs_amd as F
from test_m2l_pairs_host import lattice_cloud
from test_m2l_pairs_stage2_y_host import WALK_CASES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "m2l_table_digests.json")
SWITCHES = ("BBFMM_M2L_CBUF_MB", "BBFMM_M2L_S1_PAIRS", "BBFMM_M2L_S2_PAIRS", "BBFMM_M2L_S1_AXES", "BBFMM_M2L_S2_AXES",
            "BBFMM_M2L_VARIANTS")
ACA, NONE = 2, 0


def _uniform(d):  # the cloud of test_m2l_pairs_stage2_y_host.py test_pair_structure_and_slot_layout_of_the_target_lists
    return lambda: np.random.default_rng(70 + d).random((2000, d))


def _walk_cloud(name):
    return lambda: WALK_CASES[name](np.random.default_rng(45))[0]


def _configs():
    """name -> (cloud, order, FmmParams, switches)"""
    out = {}
    uni = (30, ACA, 1e-4, 1024)
    for d in (2, 3):
        for order in (3, 4, 5, 7):
            out[f"uniform{d}d_order{order}"] = (_uniform(d), order, uni, {})
    for order in (7, 4):
        for key, val in [("S1_PAIRS", "0"), ("S2_PAIRS", "0"), ("S1_AXES", "1"), ("S1_AXES", "2"), ("S2_AXES", "1"), ("S2_AXES", "2"),
                         ("VARIANTS", "0")]:
            out[f"uniform3d_order{order}_{key}={val}"] = (_uniform(3), order, uni, {"BBFMM_M2L_" + key: val})
    for name in ("clustered3d", "planar2d", "low_ranks", "lattice_order7", "lattice_order4"):
        _, order, params = WALK_CASES[name](np.random.default_rng(45))
        out[name] = (_walk_cloud(name), order, params, {})
    # several batches and a level cut into groups of target classes (test_m2l_pairs_stage2_host.py)
    out["multibatch"] = (lambda: np.random.default_rng(46).random((6000, 3)), 4, (30, ACA, 1e-5, 1024), {"BBFMM_M2L_CBUF_MB": "0.25"})
    # boundary variants: the 32^3 lattice of test_m2l_pairs_host.py with the run length that test sets
    lattice32 = lambda: lattice_cloud(np.random.default_rng(43), 32, 3, 2)
    out["lattice32"] = (lattice32, 3, (6, ACA, 1e-3, 1024), {"BBFMM_M2L_VARIANTS": "1"})
    out["lattice32_S1_AXES=2"] = (lattice32, 3, (6, ACA, 1e-3, 1024), {"BBFMM_M2L_VARIANTS": "1", "BBFMM_M2L_S1_AXES": "2"})
    # no pairs at all: uncompressed operators.  (A shared-basis handle, the other path without pairs, needs a device.)
    out["uncompressed"] = (_uniform(3), 3, (30, NONE, 1e-4, 1024), {})
    return out


CONFIGS = _configs()
ONE_THREAD = ("uniform3d_order7", "multibatch", "lattice32_S1_AXES=2")  # rebuilt in a process whose pool has one thread


@contextlib.contextmanager
def _switches(env):
    """The switches are read when a handle is created: those of `env` set, every other one unset."""
    saved = {k: os.environ.pop(k, None) for k in SWITCHES}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def build(name, pts=None):
    cloud, order, params, env = CONFIGS[name]
    with _switches(env):
        return F.FmmTree(cloud() if pts is None else pts, order, F.KernelParams(F.KernelType(0)), True, True,
                         params=F.FmmParams(params[0], F.M2LCompressionType(params[1]), *params[2:]), host_only=True)


def record_of(t):
    digests, flops_level = t.debug_m2l_table_digests()
    s = t.stats()
    return {"depth": int(s.depth), "n_cells": int(s.n_cells), "ranks": np.asarray(t.m2l_ranks()).astype(int).tolist(),
            "digests": digests, "flops_k1": float(s.m2l_flops_k1), "flops_level": flops_level}


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_fixture_holds_exactly_these_configurations(golden):
    assert sorted(golden) == sorted(CONFIGS)


@pytest.mark.parametrize("name", list(CONFIGS))
def test_tables_are_the_recorded_ones(name, golden):
    want = golden[name]
    pts = CONFIGS[name][0]()
    t = build(name, pts)
    got = record_of(t)
    for key in ("ranks", "depth", "n_cells"):
        assert got[key] == want[key], f"{key} differ from the recorded ones: the fixture does not apply (the operators, not the tables, moved)"
    for family in F.FmmTree.M2L_DIGEST_FAMILIES:
        assert got["digests"][family] == want["digests"][family], f"the tables of family {family!r} moved"
    assert got["flops_k1"] == want["flops_k1"] and got["flops_level"] == want["flops_level"]  # sums in a fixed order
    assert record_of(build(name, pts)) == got, "a second build of the same handle gives other tables"
    if name == "multibatch":  # otherwise the group operators are not covered: more batches than levels with M2L work means
        # that a level is cut into groups of target classes, and its sources then have one operator per group (kind 1)
        assert t.stats().m2l_batches > max(1, t.stats().depth - 1) and any(op["kind"] == 1 for op in t.debug_m2l_pairs()[1])
    if name.startswith("lattice32"):
        assert t.debug_m2l_variants()[0] >= 1
    if name == "uncompressed":
        assert not t.debug_m2l_pairs()[0] and not t.debug_m2l_pairs(stage=2)[0]


def test_tables_do_not_depend_on_the_number_of_host_threads(golden):
    """The pool is sized once per process (BBFMM_HOST_THREADS), so the one-thread builds run in a child process."""
    env = dict(os.environ, BBFMM_HOST_THREADS="1", PYTHONPATH=ROOT)
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--print", *ONE_THREAD], env=env, stdout=subprocess.PIPE,
                         stderr=subprocess.PIPE, timeout=600)
    assert out.returncode == 0, out.stderr.decode()[-2000:]
    got = json.loads(out.stdout.decode().strip().splitlines()[-1])
    for name in ONE_THREAD:
        assert got[name] == golden[name], name


if __name__ == "__main__":
    from ferreus_rbf_rs_amd import build as _b
    _b.build()
    if sys.argv[1] == "--record":
        def lines(rec):  # one line per entry and per family, so that a diff names what moved
            flat = [(k, v) for k, v in rec.items() if k != "digests"] + [("digests", None)]
            return ",\n".join(f'  {json.dumps(k)}: ' + (json.dumps(v) if v is not None else "{\n" + ",\n".join(
                f'   {json.dumps(fam)}: {json.dumps(h)}' for fam, h in rec["digests"].items()) + "\n  }") for k, v in flat)
        with open(sys.argv[2], "w") as f:
            f.write("{\n" + ",\n".join(f' {json.dumps(name)}: {{\n{lines(record_of(build(name)))}\n }}' for name in CONFIGS) + "\n}\n")
    elif sys.argv[1] == "--print":
        print(json.dumps({name: record_of(build(name)) for name in sys.argv[2:]}))
