"""
CPU tests of the keyword that opts an evaluator into the matrix-free route at n <= 16
(matrix_free="small", knob "action_small" = 1, qoc_amd/csrc/qocx_action16.hip), on the stand-in backends
of tests/test_action_wide_model.py: "small" sets the knob to 1 and nothing else of the route's, "all" and
"default" do not touch it, a backend without knobs ignores it, anything else is a ValueError.
"""

import numpy as np
import pytest

from tests.test_action_model import hermitian
from tests.test_action_wide_model import StandIn, StandInWithKnobs

ROUTE_KNOBS = ("action", "action_states", "action_costs", "action_small")


def build_evaluator(backend, n=8, **kw):
    from qoc_amd.core import device
    from qoc_amd.standard import TargetStateInfidelity
    rng = np.random.default_rng(5)
    h0, g = hermitian(rng, n), hermitian(rng, n)
    psi0 = np.eye(n, dtype=np.complex128)[:1, :, None]
    target = np.eye(n, dtype=np.complex128)[1:2, :, None]
    return device.SchroedingerEvaluator(0.5, lambda u, t: h0 + u[0] * g, psi0, 11, control_count=1,
                                        control_eval_count=11, costs=[TargetStateInfidelity(target)],
                                        backend=backend, **kw)


def test_small_sets_the_knob_and_nothing_else_of_the_route():
    backend = StandInWithKnobs()
    assert build_evaluator(backend, matrix_free="small").matrix_free == "small"
    assert backend.knobs["action_small"] == 1 and backend.problems == 1
    assert [k for k in ROUTE_KNOBS if k in backend.knobs] == ["action_small"]
    assert backend.knobs["latency"] == 0  # (not a latency-mode evaluator: the route would yield to it)


def test_small_leaves_latency_mode_to_the_caller():
    """The single-seed entry points keep their route: the keyword does not switch latency mode off."""
    backend = StandInWithKnobs()
    build_evaluator(backend, matrix_free="small", latency_mode=True)
    assert backend.knobs["action_small"] == 1 and backend.knobs["latency"] == 1


@pytest.mark.parametrize("value", ["default", "all", "wide", "states", "costs"])
def test_other_values_do_not_touch_the_knob(value):
    backend = StandInWithKnobs()
    build_evaluator(backend, matrix_free=value)
    assert "action_small" not in backend.knobs and backend.problems == 1
    plain = StandInWithKnobs()
    build_evaluator(plain)
    assert "action_small" not in plain.knobs


def test_a_backend_without_knobs_ignores_it():
    bare = StandIn()
    build_evaluator(bare, matrix_free="small")
    assert bare.problems == 1


@pytest.mark.parametrize("bad", ["Small", "tiny", "", None, 1, True])
def test_keyword_refuses_anything_else(bad):
    backend = StandInWithKnobs()
    with pytest.raises(ValueError, match="matrix_free"):
        build_evaluator(backend, matrix_free=bad)
    assert backend.problems == 0 and not backend.knobs


@pytest.mark.parametrize("entry", ["evolve_schroedinger_discrete", "grape_schroedinger_discrete",
                                   "grape_schroedinger_discrete_batch"])
def test_entry_points_say_what_the_keyword_takes(entry):
    from qoc_amd.core import schroedingerdiscrete
    assert "small" in getattr(schroedingerdiscrete, entry).__doc__
