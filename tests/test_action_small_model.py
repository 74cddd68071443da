"""
CPU tests of the matrix-free route's mathematics at the sizes of its small form (n <= 16,
qoc_amd/csrc/qocx_action16.hip): tests/action_model.py at n = 2, 4, 5, 8, 13 and 16 against the oracle, at
the project's gates - 1e-10 for cost and final state, 1e-8 of the largest entry for the gradient. The
model has no size in it, so this passes with or without the kernels: it pins the mathematics at the
sizes tests/test_gpu_action_small.py holds the device to.
"""

import numpy as np
import pytest

from oracle import qoc_numpy as onp
from tests import action_model as am
from tests.helpers import rel_err
from tests.test_action_model import problem

SIZES = (2, 4, 5, 8, 13, 16)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("degree", [None, 18])
def test_model_equals_oracle(n, degree):
    p = problem(n, 100 + n)
    cost, grads, final, used = am.evaluate_with_grad(p["h0"], p["g"], p["psi0"], p["target"], p["N"],
                                                     p["T"], p["controls"], degree=degree)
    assert len(used) == 12 and 1 <= min(used) <= max(used) <= am.MAX_DEGREE, used
    ref_cost, ref_grads, ref_final = onp.evaluate_with_grad(p["oracle"], p["controls"])
    print("n={} degrees {}: cost {:.1e} final {:.1e} grad {:.1e}".format(
        n, sorted(set(used)), abs(cost - ref_cost), np.abs(final - ref_final[0, :, 0]).max(),
        rel_err(grads, ref_grads)))
    assert abs(cost - ref_cost) < 1e-10
    assert np.abs(final - ref_final[0, :, 0]).max() < 1e-10
    assert rel_err(grads, ref_grads) < 1e-8
