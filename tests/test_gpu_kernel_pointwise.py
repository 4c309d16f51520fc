"""The device branch of csrc/kernels.hpp -- v_rsq_f64 / v_rcp_f64 seeds with FMA refinement, the hand-written logarithm,
the Spheroidal far values as a power of the reciprocal square root, the device library's exp and pow: what every P2P /
M2P / P2L pair is evaluated with -- against extended precision, element by element (bbfmm_debug_math /
bbfmm_debug_kernel_values with where = 1).  The tables, the error measure and the derived budget are those of
tests/kernel_reference.py and tests/kernel_pointwise.py; tests/test_kernel_reference_host.py holds the host branch to
the same measure."""
import numpy as np
import pytest

import ferreus_rbf_rs_amd as F
import kernel_pointwise as KP
import kernel_reference as KR
from test_kernel_reference_host import CASES, SILL

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("which", list(F.fmm_tree.DEBUG_MATH))
def test_device_primitives(which):
    """bb_sqrt and bb_sqrt_rsqrt within 2 ulp, bb_rcp within 1 ulp, bb_log within 3.1 ulp of the correctly rounded result
    over 2^-200 .. 2^200 and the edge sets; sqrt(0) = 0 exactly and an absolute error below 1e-150 under the 1e-300 clamp."""
    KP.check_primitive(1, which, F.debug_math(1, which, KP.primitive_inputs(which)))


@pytest.mark.parametrize("kid,br", CASES)
def test_device_kernel_functions_pointwise(kid, br):
    """kernel_value_r2 and the value and factor of kernel_value_grad_r2 on the device within the budget of
    kernel_pointwise.budget(1, kid), on the same side of every zero rule and of the Spheroidal switch as the reference."""
    KP.check_kernel(1, kid, br, SILL, F.debug_kernel_values(1, kid, br, SILL, KR.table_for(kid, br)))


def test_device_and_host_branch_decide_alike():
    """The two branches of kernels.hpp on the sets the rules sit on: exact zeros in the same places."""
    r2 = np.concatenate([[0.0], KR.neighbours(KR.EPS, 8), KR.neighbours(KR.EPS ** 2, 8)])
    for kid in KR.KERNEL_IDS:
        h, d = F.debug_kernel_values(0, kid, 1.0, SILL, r2), F.debug_kernel_values(1, kid, 1.0, SILL, r2)
        for a, b in zip(h, d):
            assert np.array_equal(a == 0, b == 0), kid
