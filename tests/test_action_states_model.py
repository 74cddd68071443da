"""
CPU tests of the matrix-free route with two to four states per seed (qoc_amd/csrc/qocx_action_states.hip):
tests/action_states_model.py against the oracle on the fixture of tests/test_gpu_action.py extended to
S states (13 steps, K = 2, ||H0||_1 = ||G_k||_1 = 1, seeds of amplitude 1e-3 / 1 / 5, psi0 = eye(n)[:S],
random normalised targets, one coherent final TargetStateInfidelity), its identity with the one-state
model at S = 1, and the keyword that opts an evaluator in, on a stand-in backend.

The gates: the model works in the oracle's precision and differs from it by the truncation of the
series (below 2^-53 relative by the choice of the degree) and by rounding: 1e-13 for the cost and the
final states, 1e-12 of the largest entry for the gradient.
"""

import numpy as np
import pytest

from tests import action_model as am
from tests import action_states_model as asm
from tests.helpers import rel_err
from tests.test_gpu_action import DT, N, hermitian, problem

SIZES = (17, 20, 32)
STATES = (2, 3, 4)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("S", STATES)
def test_model_equals_oracle(n, S):
    p = problem(n, states=S)
    target = p["descs"][0]["vectors"]
    worst = dict(cost=0.0, final=0.0, grad=0.0)
    executed = set()
    for b, (ref_cost, ref_grads, ref_final) in enumerate(p["refs"]):
        cost, grads, final, used = asm.evaluate_with_grad(p["h0"], p["g"], p["psi0"], target, N, p["T"],
                                                          p["controls"][b])
        executed |= set(used)
        worst["cost"] = max(worst["cost"], abs(cost - ref_cost))
        worst["final"] = max(worst["final"], np.abs(final - ref_final[:, :, 0]).max())
        worst["grad"] = max(worst["grad"], rel_err(grads, ref_grads))
    print("n={} S={} degrees {}: {}".format(n, S, sorted(executed),
                                            " ".join("%s=%.1e" % kv for kv in worst.items())))
    assert len(executed) >= 3 and max(executed) <= am.MAX_DEGREE, executed
    assert worst["cost"] < 1e-13 and worst["final"] < 1e-13 and worst["grad"] < 1e-12, worst


@pytest.mark.parametrize("n", SIZES)
def test_one_state_is_the_one_state_model_bit_for_bit(n):
    p = problem(n, states=1)
    target = p["descs"][0]["vectors"]
    for b in range(len(p["controls"])):
        one = am.evaluate_with_grad(p["h0"], p["g"], p["psi0"][0], target[0], N, p["T"], p["controls"][b])
        many = asm.evaluate_with_grad(p["h0"], p["g"], p["psi0"], target, N, p["T"], p["controls"][b])
        assert one[0] == many[0] and one[3] == many[3]
        assert np.array_equal(one[1], many[1]) and np.array_equal(one[2], many[2][0])


# ---- the keyword ---------------------------------------------------------------------------------------

class StandIn:
    """What SchroedingerEvaluator needs of a backend to be built, with or without knobs."""

    def __init__(self):
        self.knobs = {}
        self.problems = 0

    def set_schroedinger_problem(self, *args, **kw):
        self.problems += 1


class StandInWithKnobs(StandIn):
    def set_knob(self, name, value):
        self.knobs[name] = value


def build_evaluator(backend, states=2, **kw):
    from qoc_amd.core import device
    from qoc_amd.standard import TargetStateInfidelity
    n = 20
    rng = np.random.default_rng(5)
    h0, g = hermitian(rng, n), hermitian(rng, n)
    psi0 = np.eye(n, dtype=np.complex128)[:states, :, None]
    target = np.eye(n, dtype=np.complex128)[states:2 * states, :, None]
    return device.SchroedingerEvaluator(DT * 10, lambda u, t: h0 + u[0] * g, psi0, 11, control_count=1,
                                        control_eval_count=11, costs=[TargetStateInfidelity(target)],
                                        backend=backend, **kw)


def test_keyword_sets_the_knobs_where_there_are_knobs():
    from qoc_amd.core import device
    assert 2 <= device.ACTION_STATES_DEFAULT <= 4
    for value in (None, "default"):
        plain = StandInWithKnobs()
        ev = build_evaluator(plain) if value is None else build_evaluator(plain, matrix_free=value)
        assert ev.matrix_free == "default" and plain.problems == 1
        assert "action" not in plain.knobs and "action_states" not in plain.knobs  # the default touches neither
    wide = StandInWithKnobs()
    build_evaluator(wide, matrix_free="wide")
    assert wide.knobs["action"] == 2 and "action_states" not in wide.knobs
    states = StandInWithKnobs()
    assert build_evaluator(states, matrix_free="states").matrix_free == "states"
    assert states.knobs["action_states"] == device.ACTION_STATES_DEFAULT and "action" not in states.knobs
    assert states.problems == 1
    both = StandInWithKnobs()
    assert build_evaluator(both, matrix_free="all").matrix_free == "all"
    assert both.knobs["action_states"] == device.ACTION_STATES_DEFAULT and both.knobs["action"] == 2
    bare = StandIn()  # no knobs: ignored
    build_evaluator(bare, matrix_free="states")
    build_evaluator(bare, matrix_free="all")
    assert bare.problems == 2


def test_keyword_and_latency_mode():
    """The route yields to latency mode, so a problem whose states were asked onto it is not put there;
    every other combination keeps the latency knobs it had."""
    from qoc_amd.core import device
    for value, states, latency in (("default", 2, 1), ("wide", 2, 1), ("states", 2, 0), ("all", 2, 0),
                                   ("states", 1, 1), ("states", device.ACTION_STATES_DEFAULT + 1, 1)):
        backend = StandInWithKnobs()
        build_evaluator(backend, states=states, matrix_free=value, latency_mode=True)
        assert backend.knobs["latency"] == latency and backend.knobs["sweep_impl"] == (3 if latency else 1), value
        backend = StandInWithKnobs()
        build_evaluator(backend, states=states, matrix_free=value)
        assert backend.knobs["latency"] == 0 and backend.knobs["sweep_impl"] == 1


@pytest.mark.parametrize("bad", ["States", "state", "ALL", "", None, 4, True])
def test_keyword_refuses_anything_else(bad):
    backend = StandInWithKnobs()
    with pytest.raises(ValueError, match="matrix_free") as info:
        build_evaluator(backend, matrix_free=bad)
    for value in ("default", "wide", "states", "all"):
        assert '"%s"' % value in str(info.value)
    assert backend.problems == 0 and not backend.knobs
