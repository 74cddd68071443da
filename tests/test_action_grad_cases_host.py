"""
The problems of tests/action_grad_cases.py reach the edges of the gradient kernel that
tests/test_gpu_action_grad_bits.py is there for, checked without a GPU by the NumPy twin of the degree rule
(tests/action_degree_model.py) - whether the spectral bound of a step is the exact radius or the engine's (at
most 1 % above it):

  ramp  m = 1 and 2 (one term of rho, an even partial sum alone), an odd and an even degree in the middle,
        and no two neighbouring steps of the first seed at the same degree;
  flat  one degree in every step of every seed;
  top   m = 18, the most the route executes, under the 1-norm rule (knob "action_degree" = 0) - with the
        host's knot bound at or below theta_18, so that the route never yields to the Pade route.
"""

import pytest

from tests import action_degree_model as dm
from tests import action_grad_cases as cases
from tests import action_model as am


def degree_tables(p, inflate):
    """[seed][step] by the rule the case runs under."""
    tables = []
    for b in range(cases.B):
        bounds = dm.step_bounds(p["h0"], p["g"], cases.N, p["T"], p["controls"][b])
        assert len(bounds) == cases.N - 1
        tables.append([dm.degree_rule(b1, inflate * b2, p["rule"]) for b1, b2 in bounds])
    return tables


@pytest.mark.parametrize("inflate", [1.0, 1.01])
@pytest.mark.parametrize("n,K,shape", cases.CASES)
def test_the_step_tables_hold_the_degrees_the_cases_are_there_for(n, K, shape, inflate):
    p = cases.case(n, K, shape)
    assert p["controls"].shape == (cases.B, cases.N, K)
    # the host's bound is taken over the knots: dt (||H0||_1 + sum_k max |u_k| ||G_k||_1)
    host = cases.DT * (cases.H0_NORM + abs(p["controls"]).max(axis=1).sum(axis=1).max())
    assert host <= am.THETA[am.MAX_DEGREE], (n, K, shape, host)
    tables = degree_tables(p, inflate)
    seen = {m for table in tables for m in table}
    assert max(seen) <= am.MAX_DEGREE
    if shape == "ramp":
        assert {1, 2} <= seen and {m for m in seen if 2 < m < max(seen) and m % 2} \
            and {m for m in seen if 2 < m < max(seen) and not m % 2}, sorted(seen)
        assert all(a != b for a, b in zip(tables[0], tables[0][1:])), tables[0]
    elif shape == "flat":
        assert seen == {8}, sorted(seen)
    else:
        assert am.MAX_DEGREE in seen and min(seen) <= 3, sorted(seen)


def test_the_cases_cover_the_sizes_and_control_counts():
    assert {n for n, _, _ in cases.CASES} == {17, 25, 32}
    assert {K for _, K, _ in cases.CASES} == {1, 2, 3, 4}
    assert {shape for _, _, shape in cases.CASES} == set(cases.SHAPES)
