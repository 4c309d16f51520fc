"""The composite field's program kernel: the same columns on the device equal the host bit for bit, values and gradients,
at sizes around the block edges and past one grid-stride wrap (256 threads, at most 4096 blocks)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import field_program_restatement as FR
from ferreus_rbf_rs_amd import _lib as L
from test_field_program_host import PROGRAMS, bits, debug_program

WRAP = 256 * 4096                                     # one pass of the grid


@pytest.mark.parametrize("m", [1, 255, 256, 257, 1000])
@pytest.mark.parametrize("case", range(len(PROGRAMS)))
def test_device_program_equals_the_host_bit_for_bit(case, m):
    scale, offset, codes = PROGRAMS[case]
    V, G = FR.columns(200 + case, m, len(scale), True)
    for grads in (None, G):
        rc_h, vh, gh = debug_program(0, scale, offset, codes, V, grads)
        rc_d, vd, gd = debug_program(1, scale, offset, codes, V, grads)
        assert rc_h == L.OK and rc_d == L.OK
        assert np.array_equal(bits(vd), bits(vh))
        if grads is not None:
            assert np.array_equal(bits(gd), bits(gh))


def test_device_program_past_a_grid_stride_wrap():
    scale, offset, codes = PROGRAMS[4]
    m = WRAP + 257
    V, G = FR.columns(300, m, len(scale), True)
    _, vh, gh = debug_program(0, scale, offset, codes, V, G)
    rc, vd, gd = debug_program(1, scale, offset, codes, V, G)
    assert rc == L.OK and np.array_equal(bits(vd), bits(vh)) and np.array_equal(bits(gd), bits(gh))
    rv, rg = FR.program(scale, offset, codes, V, G)
    assert np.array_equal(bits(vd), bits(rv)) and np.array_equal(bits(gd), bits(rg))
