"""
CPU tests of the matrix-free route under step costs and several costs (qoc_amd/csrc/qocx_action_costs.hip):
tests/action_costs_model.py - the Taylor series per step with the general adjoint and the descriptor
costs of tests/state_costs.py - against the oracle (onp.evaluate_with_grad) on the problems of
tests/action_costs_cases.py, at the gates tests/test_action_model.py holds the one-target model to:
1e-10 for cost and final state, 1e-8 of the largest entry for the gradient. And the keyword that opts an
evaluator in, on a stand-in backend.
"""

import numpy as np
import pytest

from tests import action_costs_cases as acc
from tests import action_costs_model as acm
from tests import action_model as am
from tests.helpers import rel_err
from tests.test_action_states_model import StandIn, StandInWithKnobs
from tests.test_gpu_action import DT, hermitian


def run(p, name, b, **kw):
    return acm.evaluate_with_grad(p["h0"], p["g"], p["init"][0], acc.costs_of(name, p), acc.CES, p["N"],
                                  p["T"], p["controls"][b], **kw)


@pytest.mark.parametrize("N", acc.STEP_COUNTS)
@pytest.mark.parametrize("n", acc.SIZES)
@pytest.mark.parametrize("name", acc.SETS)
def test_model_equals_oracle(name, n, N):
    p = acc.build(n, N)
    worst = dict(cost=0.0, final=0.0, grad=0.0)
    executed = set()
    for b, (ref_cost, ref_grads, ref_final) in enumerate(acc.references(name, p)):
        cost, grads, final, used = run(p, name, b)
        executed |= set(used)
        worst["cost"] = max(worst["cost"], abs(cost - ref_cost))
        worst["final"] = max(worst["final"], np.abs(final - ref_final[0, :, 0]).max())
        worst["grad"] = max(worst["grad"], rel_err(grads, ref_grads))
        forward = run(p, name, b, want_grad=False)
        assert forward[0] == cost and forward[1] is None and np.array_equal(forward[2], final)
    print("{} n={} N={} degrees {}: {}".format(name, n, N, sorted(executed),
                                               " ".join("%s=%.1e" % kv for kv in worst.items())))
    assert len(executed) >= 3 and max(executed) <= am.MAX_DEGREE
    assert worst["cost"] < 1e-10 and worst["final"] < 1e-10 and worst["grad"] < 1e-8, worst


@pytest.mark.parametrize("degree", ["+2", 18])
@pytest.mark.parametrize("N", acc.STEP_COUNTS)
def test_model_equals_oracle_at_other_degrees(N, degree):
    """The degree of every step two above the largest the bound asks for, and the largest there is."""
    p = acc.build(17, N)
    name = "target_after_ragged_forbid"  # a step forbid, a step target and a final target
    for b, (ref_cost, ref_grads, ref_final) in enumerate(acc.references(name, p)):
        m = max(run(p, name, b)[3]) + 2 if degree == "+2" else degree
        cost, grads, final, used = run(p, name, b, degree=m)
        assert set(used) == {m}
        assert abs(cost - ref_cost) < 1e-10 and np.abs(final - ref_final[0, :, 0]).max() < 1e-10
        assert rel_err(grads, ref_grads) < 1e-8


def test_one_final_target_is_the_one_target_model():
    """Under one final coherent target the true cotangent is the scalar times the back-propagated target:
    the general adjoint and the unit adjoint of tests/action_model.py agree to rounding."""
    p = acc.build(20, 14)
    cost_desc = acc.costs_of("final_coherent", p)[0]
    for b in range(3):
        mine = run(p, "final_coherent", b)
        unit = am.evaluate_with_grad(p["h0"], p["g"], p["init"][0], cost_desc.vectors[0], p["N"], p["T"],
                                     p["controls"][b], scale=cost_desc.scale)
        assert mine[3] == unit[3] and np.array_equal(mine[2], unit[2])
        assert abs(mine[0] - unit[0]) < 1e-14 and rel_err(mine[1], unit[1]) < 1e-13


# ---- the keyword ---------------------------------------------------------------------------------------

def build_evaluator(backend, n=20, states=1, costs="step", **kw):
    from qoc_amd.core import device
    from qoc_amd.standard import ForbidStates, TargetStateInfidelity
    rng = np.random.default_rng(5)
    h0, g = hermitian(rng, n), hermitian(rng, n)
    psi0 = np.eye(n, dtype=np.complex128)[:states, :, None]
    target = np.eye(n, dtype=np.complex128)[states:2 * states, :, None]
    cost_list = [TargetStateInfidelity(target)]
    if costs == "step":
        forbidden = np.eye(n, dtype=np.complex128)[2 * states:4 * states].reshape(states, 2, n, 1)
        cost_list.append(ForbidStates(forbidden, 11))
    return device.SchroedingerEvaluator(DT * 10, lambda u, t: h0 + u[0] * g, psi0, 11, control_count=1,
                                        control_eval_count=11, costs=cost_list, backend=backend, **kw)


def test_keyword_sets_the_knob_where_there_are_knobs():
    from qoc_amd.core import device
    assert device.MATRIX_FREE_VALUES == ("default", "wide", "states", "all", "costs")
    backend = StandInWithKnobs()
    assert build_evaluator(backend, matrix_free="costs").matrix_free == "costs"
    assert backend.knobs["action_costs"] == 1 and backend.problems == 1
    assert "action" not in backend.knobs and "action_states" not in backend.knobs
    for value in ("default", "wide", "states", "all"):  # ... set exactly the knobs they set before
        backend = StandInWithKnobs()
        build_evaluator(backend, matrix_free=value)
        assert "action_costs" not in backend.knobs, value
    bare = StandIn()  # no knobs: ignored
    build_evaluator(bare, matrix_free="costs")
    assert bare.problems == 1


def test_keyword_and_latency_mode():
    """The route yields to latency mode, so a problem asked onto it is not put there: one state, 17 <= n
    <= 32, and not the single final target (which has kernels of its own, and latency mode with them)."""
    for value, n, states, costs, latency in (
            ("costs", 20, 1, "step", 0), ("costs", 17, 1, "step", 0), ("costs", 32, 1, "step", 0),
            ("costs", 20, 1, "final", 1), ("costs", 20, 2, "step", 1), ("costs", 16, 1, "step", 1),
            ("costs", 33, 1, "step", 1), ("default", 20, 1, "step", 1), ("all", 20, 1, "step", 1)):
        backend = StandInWithKnobs()
        build_evaluator(backend, n=n, states=states, costs=costs, matrix_free=value, latency_mode=True)
        tag = (value, n, states, costs)
        assert backend.knobs["latency"] == latency, tag
        assert backend.knobs["sweep_impl"] == (3 if latency and 16 < n <= 32 else 1), tag
        backend = StandInWithKnobs()
        build_evaluator(backend, n=n, states=states, costs=costs, matrix_free=value)
        assert backend.knobs["latency"] == 0 and backend.knobs["sweep_impl"] == 1, tag


@pytest.mark.parametrize("bad", ["cost", "Costs", "COSTS", "step_costs"])
def test_keyword_refuses_anything_else(bad):
    backend = StandInWithKnobs()
    with pytest.raises(ValueError, match="matrix_free") as info:
        build_evaluator(backend, matrix_free=bad)
    for value in ("default", "wide", "states", "all", "costs"):
        assert '"%s"' % value in str(info.value)
    assert backend.problems == 0 and not backend.knobs
