"""The grid coordinates and the cut of target runs into jobs, host side (where = 0), against the numpy restatement
bit for bit (no GPU)."""
import numpy as np
import pytest

from evaluate_grid_restatement import grid_coords, rotation_z, split_runs
from ferreus_rbf_rs_amd import fmm_tree as T

GRIDS = [
    # origin, steps, shape, (r0, n) slabs
    ([0.1], [[0.37]], [29], [(0, 29), (5, 11)]),
    ([0.1, -2.0], 0.013 * rotation_z(30.0, 2), [17, 13], [(0, 221), (20, 57)]),
    ([0.1, 0.2, 0.3], np.diag([0.01, 0.02, 0.03]), [7, 5, 3], [(0, 105)]),
    ([1000.1, -2000.2, 30.3], 5.0 * rotation_z(30.0), [17, 13, 11], [(0, 2431), (13 * 11 + 7, 400)]),   # rotated, mid-plane slab
    ([0.1, 0.2, 0.3], 0.7 * rotation_z(-12.5), [9, 1, 6], [(0, 54), (4, 31)]),                           # a shape with a 1
    ([0.1, 0.2, 0.3], 0.7 * rotation_z(77.0), [1, 1, 1], [(0, 1)]),
]


@pytest.mark.parametrize("case", range(len(GRIDS)))
def test_grid_coords_host_equal_the_restatement(case):
    origin, steps, shape, slabs = GRIDS[case]
    for r0, n in slabs:
        got = T.debug_grid_coords(0, origin, steps, shape, r0, n)
        want = grid_coords(origin, steps, shape, r0, n)
        assert got.shape == want.shape
        assert np.array_equal(got.view(np.uint64), np.asfortranarray(want).view(np.uint64))


def test_grid_coords_rejects_rows_outside_the_grid():
    with pytest.raises(ValueError):
        T.debug_grid_coords(0, [0.0, 0.0], np.eye(2), [3, 4], 10, 3)


def runs_for(cap):
    lengths = [0, 1, cap, cap + 1, 3 * cap - 1, 1000, 0, 1]
    begin = np.cumsum([0] + lengths[:-1]) + 7          # the runs need not start at 0
    return begin, begin + np.array(lengths), np.arange(len(lengths)) * 3 + 1, lengths


@pytest.mark.parametrize("cap", [1, 16, 512])
def test_split_runs_host_equal_the_rule(cap):
    tb, te, jc, lengths = runs_for(cap)
    ob, oe, oc = T.debug_split_runs(0, tb, te, jc, cap)
    wb, we, wc = split_runs(tb, te, jc, cap)
    assert np.array_equal(ob, wb) and np.array_equal(oe, we) and np.array_equal(oc, wc)
    # the jobs tile each run, none is empty, none exceeds cap, and their sizes differ by at most one
    pos = 0
    for b, e, c, n in zip(tb, te, jc, lengths):
        q = -(-n // cap)
        jb, je, jcell = ob[pos:pos + q], oe[pos:pos + q], oc[pos:pos + q]
        pos += q
        if n == 0:
            continue
        assert jb[0] == b and je[-1] == e and np.array_equal(jb[1:], je[:-1]) and np.all(jcell == c)
        sizes = je - jb
        assert sizes.min() >= 1 and sizes.max() <= cap and sizes.max() - sizes.min() <= 1
    assert pos == len(ob)


def test_split_runs_bad_arguments():
    with pytest.raises(ValueError):
        T.debug_split_runs(0, [0], [5], [1], 0)            # cap >= 1
    with pytest.raises(ValueError):
        T.debug_split_runs(0, [5], [0], [1], 4)            # a negative length
    ob, oe, oc = T.debug_split_runs(0, [], [], [], 4)
    assert len(ob) == len(oe) == len(oc) == 0
