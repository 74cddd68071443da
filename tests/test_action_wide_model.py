"""
CPU tests of the matrix-free route's mathematics at the sizes of its wide form (33 <= n <= 64,
qoc_amd/csrc/qocx_action4.hip): tests/action_model.py at n = 40 and 64 against the oracle and against
the dense reverse rule, at the tolerances of tests/test_action_model.py - 1e-10 for cost and final
state, 1e-8 of the largest entry for the gradient, 1e-13 of the largest entry for the cotangent. And
the keyword that opts an evaluator into the wide route, on a stand-in backend.
"""

import numpy as np
import pytest

from oracle import qoc_numpy as onp
from tests import action_model as am
from tests.helpers import rel_err
from tests.test_action_model import hermitian, problem

SIZES = (40, 64)


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


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("m", [1, 7, 13, 18])
def test_generator_cotangent_is_the_reverse_rule_of_the_polynomial(n, m):
    rng = np.random.default_rng(7 * n + m)
    a = -1j * 0.2 * hermitian(rng, n)
    psi = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    lam = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    psi /= np.linalg.norm(psi)
    lam /= np.linalg.norm(lam)
    _, v = am.forward_step(a, psi, m)
    _, w = am.adjoint_step(a, lam, m)
    abar = am.generator_cotangent(v, w, m)
    dense = am.dense_reverse_rule(a, psi, lam, m)
    assert np.abs(abar - dense).max() < 1e-13 * max(1.0, np.abs(dense).max())


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


def build_evaluator(backend, **kw):
    from qoc_amd.core import device
    from qoc_amd.standard import TargetStateInfidelity
    n = 40
    rng = np.random.default_rng(5)
    h0, g = hermitian(rng, n), hermitian(rng, n)
    psi0 = np.eye(n, dtype=np.complex128)[:1, :, None]
    target = np.eye(n, dtype=np.complex128)[1:2, :, None]
    return device.SchroedingerEvaluator(0.5, lambda u, t: h0 + u[0] * g, psi0, 11, control_count=1,
                                        control_eval_count=11, costs=[TargetStateInfidelity(target)],
                                        backend=backend, **kw)


def test_keyword_sets_the_knob_where_there_is_one():
    plain = StandInWithKnobs()
    assert build_evaluator(plain).matrix_free == "default"
    assert "action" not in plain.knobs and plain.problems == 1  # the default touches nothing
    explicit = StandInWithKnobs()
    build_evaluator(explicit, matrix_free="default")
    assert "action" not in explicit.knobs
    wide = StandInWithKnobs()
    assert build_evaluator(wide, matrix_free="wide").matrix_free == "wide"
    assert wide.knobs["action"] == 2 and wide.problems == 1
    bare = StandIn()  # no knobs: ignored
    build_evaluator(bare, matrix_free="wide")
    assert bare.problems == 1


@pytest.mark.parametrize("bad", ["Wide", "narrow", "", None, 2, True])
def test_keyword_refuses_anything_else(bad):
    backend = StandInWithKnobs()
    with pytest.raises(ValueError, match="matrix_free"):
        build_evaluator(backend, matrix_free=bad)
    assert backend.problems == 0 and not backend.knobs
