"""
GPU tests (-m gpu): the matrix-free route (qoc_amd/csrc/qocx_action.hip) computes, bit for bit, what it
computed before its sweeps began to read their step words and controls through the scalar unit a step
ahead, before two controls had a sweep build of their own, and before the gradient kernel fetched its G_k
fragments and its coefficients in batches - none of which may change the operands, the order or the
association of a floating-point operation. tests/golden/action_bits/ holds cost, gradient and final states
of the problems of tests/action_bits_cases.py as the library BEFORE that change computed them
(tools/record_action_bits.py); the comparison is np.array_equal.

n = 17 and 32; K = 1 (the second register image zero-filled), 2 (the exact build), 3 (one control read per
step); three seeds, 24 steps, amplitudes that ramp through at least three Taylor degrees per pulse
(tests/test_action_bits_cases_host.py). The same bits with the evaluation cut into one and into eight time
segments - every launch boundary, the carried vectors, and the look-ahead of a launch's last step, which
must stay inside the launch -, and without the gradient, where nothing is stored for the gradient kernel.
"""

import numpy as np
import pytest

from tests import action_bits_cases as cases

pytestmark = pytest.mark.gpu

CASES = [(n, K) for n in cases.SIZES for K in cases.CONTROL_COUNTS]


@pytest.fixture(scope="module")
def engine():
    from qoc_amd.engine import Engine
    e = Engine(0)
    yield e
    e.set_pipeline(0)
    e.close()


_golden = {}


def golden(n, K):
    if (n, K) not in _golden:
        _golden[(n, K)] = tuple(np.load(cases.golden_path(n, K, name)) for name in cases.NAMES)
    return _golden[(n, K)]


def executed(engine):
    return {m: c for m, c in engine.action_degrees().items() if c}


def assert_bits(tag, out, ref, names=cases.NAMES):
    for name in names:
        x, y = out[cases.NAMES.index(name)], ref[cases.NAMES.index(name)]
        assert x.shape == y.shape and x.dtype == y.dtype, (tag, name)
        differing = int(np.count_nonzero(x != y))
        print("{} {}: {} of {} entries differ, max |difference| {:.3e}".format(
            tag, name, differing, x.size, float(np.abs(x - y).max())))
        assert np.array_equal(x, y), (tag, name)


@pytest.mark.parametrize("n,K", CASES)
def test_the_bits_of_the_parent(engine, n, K):
    p = cases.case(n, K)
    cases.set_problem(engine, p)
    engine.set_pipeline(0)
    out = engine.evaluate(p["controls"], True)
    degrees = executed(engine)
    print("n={} K={} degrees {}".format(n, K, degrees))
    assert sum(degrees.values()) == cases.B * (cases.N - 1) and len(degrees) >= 3, degrees
    assert engine.action_reruns() == 0
    assert_bits("n=%d K=%d" % (n, K), out, golden(n, K))


@pytest.mark.parametrize("segments", [1, 8])
@pytest.mark.parametrize("n,K", CASES)
def test_the_same_bits_however_the_steps_are_cut(engine, n, K, segments):
    p = cases.case(n, K)
    cases.set_problem(engine, p)
    engine.set_pipeline(segments)
    try:
        out = engine.evaluate(p["controls"], True)
        assert sum(executed(engine).values()) == cases.B * (cases.N - 1)
    finally:
        engine.set_pipeline(0)
    assert_bits("n=%d K=%d segments=%d" % (n, K, segments), out, golden(n, K))


@pytest.mark.parametrize("n,K", CASES)
def test_the_same_cost_and_states_without_the_gradient(engine, n, K):
    p = cases.case(n, K)
    cases.set_problem(engine, p)
    engine.set_pipeline(0)
    out = engine.evaluate(p["controls"], False)
    assert sum(executed(engine).values()) == cases.B * (cases.N - 1)
    assert out[1] is None
    assert_bits("n=%d K=%d forward only" % (n, K), out, golden(n, K), names=("cost", "final"))
