"""
GPU tests (-m gpu): the gradient kernel of the matrix-free route (qoc_amd/csrc/qocx_action.hip:
action_grad_kernel<2>) computes, bit for bit, what it computed before it read E_k = -i dt G_k from an image
built by the problem setter, formed every rho_i of a step in place of the terms in LDS, took the rank-1
updates' rho by broadcast inside the multiply-adds, and reduced the 2 K sums of a step together - none of
which may change the operands, the order or the association of a floating-point operation.
tests/golden/action_grad/ holds cost, gradient and final states of the problems of
tests/action_grad_cases.py as the library BEFORE that change computed them
(tools/record_action_grad_bits.py); the comparison is np.array_equal.

n = 17, 25, 32; K = 1 .. 4; three seeds, 13 steps, as one launch and cut into eight; pulses that run a step
at m = 1, 2, at odd and even degrees, at one degree throughout, and at m = 18, the degree that sizes the
kernel's LDS (tests/test_action_grad_cases_host.py).

The image is built where dt and the G_k are set: a second problem on the same engine - another evolution
time, other G_k - must give what a fresh engine gives. And one duration sweep of tests/action_features.py,
where the durations reach the device as controls on a fixed reference time, against the oracle at that
file's gates.
"""

import numpy as np
import pytest

from tests import action_features as af
from tests import action_grad_cases as cases
from tests.test_gpu_action import assert_gates, executed

pytestmark = pytest.mark.gpu

STEPS = cases.N - 1


@pytest.fixture(scope="module")
def engine():
    from qoc_amd.engine import Engine
    e = Engine(0)
    yield e
    e.set_knob("action_degree", 1)
    e.set_pipeline(0)
    e.close()


_golden = {}


def golden(n, K, shape):
    if (n, K, shape) not in _golden:
        with np.load(cases.golden_path(n, K, shape)) as f:
            _golden[(n, K, shape)] = tuple(f[name] for name in cases.NAMES)
    return _golden[(n, K, shape)]


def assert_bits(tag, out, ref):
    for name, x, y in zip(cases.NAMES, out, ref):
        assert x.shape == y.shape and x.dtype == y.dtype, (tag, name)
        differing = int(np.count_nonzero(x != y))
        print("{} {}: {} of {} entries differ, max |difference| {:.3e}".format(
            tag, name, differing, x.size, float(np.abs(x - y).max())))
        assert np.array_equal(x, y), (tag, name)


def evaluate_on_the_route(engine, p, segments=0):
    cases.set_problem(engine, p)
    engine.set_pipeline(segments)
    try:
        out = engine.evaluate(p["controls"], True)
        degrees = executed(engine)
    finally:
        engine.set_pipeline(0)
        engine.set_knob("action_degree", 1)
    assert sum(degrees.values()) == cases.B * STEPS and engine.action_reruns() == 0, degrees
    return out, degrees


@pytest.mark.parametrize("segments", [1, 8])
@pytest.mark.parametrize("n,K,shape", cases.CASES)
def test_the_bits_of_the_parent(engine, n, K, shape, segments):
    out, degrees = evaluate_on_the_route(engine, cases.case(n, K, shape), segments)
    print("n={} K={} {} segments={} degrees {}".format(n, K, shape, segments, degrees))
    if shape == "ramp":
        assert {1, 2} <= set(degrees), degrees
    elif shape == "flat":
        assert set(degrees) == {8}, degrees
    else:
        assert 18 in degrees, degrees
    assert_bits("n=%d K=%d %s segments=%d" % (n, K, shape, segments), out, golden(n, K, shape))


def fresh(p):
    from qoc_amd.engine import Engine
    e = Engine(0)
    try:
        return evaluate_on_the_route(e, p)[0]
    finally:
        e.close()


@pytest.mark.parametrize("change", ["evolution_time", "controls_operators"])
def test_a_second_problem_on_the_engine_reads_no_image_of_the_first(engine, change):
    first = cases.case(25, 2, "ramp")
    second = dict(first)
    if change == "evolution_time":
        second["T"] = 0.8 * first["T"]
    else:
        other = cases.case(25, 2, "flat")
        second["g"] = other["g"]
    evaluate_on_the_route(engine, first)
    out = evaluate_on_the_route(engine, second)[0]
    ref = fresh(second)
    assert_bits("after " + change, out, ref)
    # (and the change is one the gradient sees)
    assert not np.array_equal(out[1], golden(25, 2, "ramp")[1])


def test_a_duration_sweep_against_the_oracle(engine):
    from qoc_amd.core import device
    from qoc_amd.standard import HamiltonianSweep, TargetStateInfidelity
    p = af.durations()
    w = HamiltonianSweep.durations(af.hamiltonian(p), p["times"], p["T"])
    ev = device.SchroedingerEvaluator(
        p["T"], w, p["psi0"][:, :, None], af.N, control_count=2, control_eval_count=p["Nc"],
        costs=[TargetStateInfidelity(p["target"][:, :, None])], backend=engine)
    errors, grads, finals, _ = ev.evaluate_batch(p["u"])
    degrees = executed(engine)
    assert sum(degrees.values()) == p["B"] * (af.N - 1) and engine.action_reruns() == 0, degrees
    out = (np.asarray(errors), np.asarray(grads).reshape(p["u"].shape),
           np.asarray(finals).reshape(p["B"], 1, p["n"]))
    seeds = []
    for b in range(p["B"]):
        cost, g, final = af.onp.evaluate_with_grad(af.oracle_problem(p, p["Nc"], p["times"][b]), p["u"][b])
        seeds.append((cost, np.real(g), final))
    assert_gates("durations", out, seeds)
