"""
The problems of tests/action_bits_cases.py do what tests/test_gpu_action_bits.py needs of them, checked
without a GPU by the NumPy twin of the degree rule (tests/action_degree_model.py): the ramp takes every pulse
through at least three Taylor degrees - whether the spectral bound of a step is the exact radius or the
engine's (at most 1 % above it) -, and the host's 1-norm bound over the knots stays below 0.9 theta_18, so
that the route never yields to the Pade route.
"""

import pytest

from tests import action_bits_cases as cases
from tests import action_degree_model as dm
from tests import action_model as am


@pytest.mark.parametrize("K", cases.CONTROL_COUNTS)
@pytest.mark.parametrize("n", cases.SIZES)
def test_every_pulse_climbs_through_three_degrees_below_theta_18(n, K):
    p = cases.case(n, K)
    assert p["controls"].shape == (cases.B, cases.N, K)
    for b in range(cases.B):
        bounds = dm.step_bounds(p["h0"], p["g"], cases.N, p["T"], p["controls"][b])
        assert len(bounds) == 24
        # the host's bound is taken over the knots: dt (||H0||_1 + sum_k max |u_k| ||G_k||_1)
        host = cases.DT * (1.0 + abs(p["controls"][b]).max(axis=0).sum())
        assert max(b1 for b1, _ in bounds) <= host < 0.9 * am.THETA[am.MAX_DEGREE], (n, K, b, host)
        for inflate in (1.0, 1.01):  # the exact spectral radii, and the engine's bound at its loosest
            degrees = {dm.degree_rule(b1, inflate * b2) for b1, b2 in bounds}
            assert len(degrees) >= 3 and max(degrees) <= am.MAX_DEGREE, (n, K, b, sorted(degrees))
