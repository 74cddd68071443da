"""
GPU tests (-m gpu) of the matrix-free route at n <= 16 (qoc_amd/csrc/qocx_action16.hip, knob
"action_small" = 1) against the exact step propagators of tests/schroedinger_exact.py - a reference that does
not share its scheme. Cases: tests/action_small_exact_cases.py, ladder and GUE operators at n = 3, 8, 16 with
the largest spectral step bound at 0.97 of a threshold theta'_m.

Gates. Per quantity the larger of
  - ten times the NumPy model's own distance from exact on THESE cases, measured on the CPU by
    tools/measure_action_small_exact.py (profiles/action_small_exact.jsonl, the line "worst": cost 4.45e-16,
    states 2.05e-15, gradient 1.16e-14), and
  - the gate tests/schroedinger_exact.py holds every device route of the matrix-free family to (ten times the
    family's worst in profiles/schroedinger_exact.jsonl, or ten times the reference's disagreement with
    mpmath at 40 digits where that is larger): cost 7.3e-15, states 4.4e-14, gradient 6.1e-13.
The second is the larger for all three. Neither comes from what the engine gives.
"""

import numpy as np
import pytest

from tests import action_small_exact_cases as sc
from tests import schroedinger_exact as ex
from tests import schroedinger_exact_cases as xc
from tests.test_gpu_schroedinger_exact import Evidence, assert_route, device_results, run_with_knobs

pytestmark = pytest.mark.gpu

# profiles/action_small_exact.jsonl, "worst"
MODEL_VS_EXACT = dict(cost=4.45e-16, states=2.05e-15, gradient=1.16e-14)
GATES = {q: max(10 * MODEL_VS_EXACT[q], ex.GATES["matrix_free"][q]) for q in MODEL_VS_EXACT}


@pytest.fixture(scope="module")
def engine():
    from qoc_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


@pytest.mark.parametrize("name", sc.NAMES)
def test_the_small_route_against_the_exact_reference(engine, name):
    case = sc.build(name)
    want = xc.exact_results(name)
    evidence = Evidence(engine)
    engine.set_knob("action_small", 1)
    try:
        got = run_with_knobs(engine, case, lambda: device_results(engine, case, evidence))
    finally:
        engine.set_knob("action_small", 0)
    errors = xc.compare(got, want)
    ratios = {key: errors[key] / GATES[key] for key in errors}
    worst = max(ratios, key=ratios.get)
    print(name, "worst error over its gate: %s %.3g / %.3g = %.3g" % (
        worst, errors[worst], GATES[worst], ratios[worst]), errors)
    assert_route(case, evidence)  # every step on the route, the case's degree the highest, no rerun
    for key in sorted(errors):
        assert errors[key] <= GATES[key], (key, errors[key], GATES[key])


def test_the_cases_sit_where_they_claim():
    """Sizes 3, 8, 16 on both operator kinds, every bound at 0.97 of its threshold and below theta_18 in the
    host's 1-norm (so that the route does not yield)."""
    assert sorted((xc._BUILT.get(n) or sc.build(n)).n for n in sc.NAMES) == [3, 3, 8, 8, 16, 16]
    for name in sc.NAMES:
        case = sc.build(name)
        dec = xc.decisions(case)
        assert abs(np.max(dec["bound"][:, :, 1]) / xc.THN[case.degree] - xc.NEAR) < 1e-12
        assert np.max(dec["bound"][:, :, 0]) < 1.09
        assert int(np.max(dec["degree"])) == case.degree
