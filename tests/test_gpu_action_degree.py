"""
GPU tests (-m gpu) of the degree rule of the matrix-free route (knob "action_degree"; qoc_amd/csrc/
qocx_action.h, the step table of qocx_kernels.hip, the buffer sizing of qocx_host_resident.hip): the
degrees the device executes are those of the NumPy twin (tests/action_degree_model.py) step for step, under
the default rule and under the parent's (knob 0), on the default route and on the wide one; the oracle's
gates hold (1e-10 cost and final states, 1e-8 of the largest entry for the gradient); nothing is run again
on the Pade route; and the Pade orders of the same problem do not move with the knob.
tests/test_action_degree_model.py and tests/test_action_degree_host.py check the rule and the host's
spectral bound on the CPU.
"""

import ctypes

import numpy as np
import pytest

from oracle import qoc_numpy as onp
from tests import action_degree_model as dm
from tests import action_model as am
from tests.helpers import rel_err

pytestmark = pytest.mark.gpu

N, K, DT = 14, 2, 0.05  # 13 steps


@pytest.fixture(scope="module")
def engine():
    from qoc_amd.engine import Engine
    e = Engine(0)
    yield e
    e.set_knob("action", 1)
    e.set_knob("action_degree", 1)
    e.close()


def hermitian(rng, n):
    m = rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))
    m = (m + m.conj().T) / 2
    return m / onp.one_norm(m)


def diagonal(rng, n):
    d = rng.uniform(-1, 1, n)
    return np.diag(d / np.abs(d).max()).astype(np.complex128)


def engine_norm2(m):
    """What the engine takes for ||m||_2: its spectral bound, never above the 1-norm."""
    from qoc_amd import engine as em
    m = np.ascontiguousarray(m, dtype=np.complex128)
    out = ctypes.c_double(0.0)
    assert em.load_library().qocx_debug_spectral_bound(
        m.view(np.float64).ctypes.data_as(ctypes.POINTER(ctypes.c_double)), m.shape[0], ctypes.byref(out)) == 0
    rho = float(np.abs(np.linalg.eigvalsh(m)).max())
    assert rho <= out.value <= 1.01 * rho
    return min(out.value, onp.one_norm(m))


_cache = {}


def problem(n, make=hermitian):
    """As the fixture of tests/test_gpu_action.py: ||H0||_1 = ||G_k||_1 = 1 and three seeds - quiet, of order
    one, loud - so that the 1-norm rule alone spreads the degrees over 8 .. 15; the spectral norms of the
    dense operators are near 0.3, of the diagonal ones 1. The seed of the generator is the first from
    1000 + n on at which no step's bound lies within 1e-6 (relative) of a threshold of either table."""
    key = (n, make.__name__)
    if key in _cache:
        return _cache[key]
    from qoc_amd.engine import COST_TARGET_COHERENT
    T = DT * (N - 1)
    for seed in range(1000 + n, 1100 + n):
        rng = np.random.default_rng(seed)
        h0, g = make(rng, n), [make(rng, n) for _ in range(K)]
        target = rng.standard_normal((1, n)) + 1j * rng.standard_normal((1, n))
        target /= np.linalg.norm(target)
        controls = rng.uniform(-1, 1, (3, N, K)) * np.array([1e-3, 1.0, 5.0])[:, None, None]
        norms2 = [engine_norm2(h0)] + [engine_norm2(m) for m in g]
        bounds = [dm.step_bounds(h0, g, N, T, controls[b], norms2) for b in range(3)]
        if min(dm.margin_to_thresholds(b) for b in bounds) > 1e-6:
            break
    psi0 = np.eye(n, dtype=np.complex128)[:1]
    if make is diagonal:  # (a basis state would only pick up a phase: no gradient to compare)
        psi0 = rng.standard_normal((1, n)) + 1j * rng.standard_normal((1, n))
        psi0 /= np.linalg.norm(psi0)
    oracle = onp.SchroedingerProblem(
        T, lambda u, t: h0 + sum(u[k] * g[k] for k in range(K)), psi0[:, :, None], N,
        control_eval_count=N, costs=[onp.TargetStateInfidelity(target[:, :, None])], control_count=K)
    p = dict(n=n, h0=h0, g=g, psi0=psi0, T=T, controls=controls, bounds=bounds,
             descs=[dict(kind=COST_TARGET_COHERENT, step_cost=0, scale=1.0, vectors=target)])
    p["refs"] = [onp.evaluate_with_grad(oracle, controls[b]) for b in range(3)]
    _cache[key] = p
    return p


def histogram(p, rule):
    out = {}
    for seed in p["bounds"]:
        for b1, b2 in seed:
            m = dm.degree_rule(b1, b2, rule)
            out[m] = out.get(m, 0) + 1
    return out


def set_problem(engine, p):
    engine.set_schroedinger_problem(p["n"], 1, K, N, N, p["T"], p["h0"][None], np.stack(p["g"])[None],
                                    p["psi0"], costs=p["descs"])


def assert_gates(tag, out, refs):
    worst = dict(cost=0.0, final=0.0, grad=0.0)
    for b, (rc, rg, rf) in enumerate(refs):
        worst["cost"] = max(worst["cost"], abs(out[0][b] - rc))
        worst["final"] = max(worst["final"], np.abs(out[2][b] - rf[:, :, 0]).max())
        worst["grad"] = max(worst["grad"], rel_err(out[1][b], rg))
    print("{}: {}".format(tag, " ".join("%s=%.2e" % kv for kv in worst.items())))
    assert worst["cost"] < 1e-10 and worst["final"] < 1e-10 and worst["grad"] < 1e-8, (tag, worst)


def executed(engine):
    return {m: c for m, c in engine.action_degrees().items() if c}


def check_both_rules(engine, p):
    """The default rule, the parent's, and the default again: histograms of the twin, gates, no rerun, and
    the third evaluation equal to the first bit for bit."""
    assert min(dm.margin_to_thresholds(b) for b in p["bounds"]) > 1e-6
    new_h, parent_h = histogram(p, 1), histogram(p, 0)
    assert max(parent_h) <= am.MAX_DEGREE and parent_h == histogram_one_norm(p)
    set_problem(engine, p)
    before = engine.action_reruns()
    first = engine.evaluate(p["controls"], True)
    print("n={} rule 1: {}  rule 0: {}".format(p["n"], new_h, parent_h))
    assert executed(engine) == new_h
    assert_gates("n=%d action_degree 1" % p["n"], first, p["refs"])
    engine.set_knob("action_degree", 0)
    try:
        parent = engine.evaluate(p["controls"], True)
        assert executed(engine) == parent_h
        assert_gates("n=%d action_degree 0" % p["n"], parent, p["refs"])
    finally:
        engine.set_knob("action_degree", 1)
    again = engine.evaluate(p["controls"], True)
    assert executed(engine) == new_h
    for x, y in zip(first, again):
        assert np.array_equal(x, y)
    assert engine.action_reruns() == before
    return new_h, parent_h


def histogram_one_norm(p):
    out = {}
    for seed in p["bounds"]:
        for b1, _ in seed:
            m = am.degree_for(b1)
            out[m] = out.get(m, 0) + 1
    return out


@pytest.mark.parametrize("n", [17, 32])
def test_degrees_on_the_default_route(engine, n):
    new_h, parent_h = check_both_rules(engine, problem(n))
    # dense operators: the spectral norms are a third of the 1-norms, and the rule takes terms away
    assert sum(m * c for m, c in new_h.items()) < sum(m * c for m, c in parent_h.items())
    assert max(new_h) < max(parent_h)


def test_degrees_on_the_wide_route(engine):
    engine.set_knob("action", 2)
    try:
        new_h, parent_h = check_both_rules(engine, problem(40))
    finally:
        engine.set_knob("action", 1)
    assert max(new_h) < max(parent_h)


def test_diagonal_operators(engine):
    """||.||_1 = ||.||_2: the two bounds of a step are equal and its degree is the lesser of the two tables'
    (theta'_m is above theta_m for m <= 14 and below it from m = 15 on: the rule is a true minimum)."""
    p = problem(20, diagonal)
    for seed in p["bounds"]:
        for b1, b2 in seed:
            assert abs(b1 - b2) <= 1e-9 * b1
    new_h, parent_h = check_both_rules(engine, p)
    assert max(new_h) <= max(parent_h)


def test_bit_identity_across_chunks_segments_and_schedules(engine):
    p = problem(20)
    set_problem(engine, p)
    ref = engine.evaluate(p["controls"], True)
    assert executed(engine) == histogram(p, 1)

    def same(tag):
        out = engine.evaluate(p["controls"], True)
        assert executed(engine) == histogram(p, 1), tag
        for x, y in zip(ref, out):
            assert np.array_equal(x, y), tag

    try:
        engine.set_chunk(1)
        same("chunk 1")
        engine.set_chunk(0)
        for segments in (1, 3, 8):
            engine.set_pipeline(segments)
            same("segments %d" % segments)
            engine.set_knob("bidir", 0)
            same("segments %d, one-sided" % segments)
            engine.set_knob("bidir", 1)
    finally:
        engine.set_chunk(0)
        engine.set_pipeline(0)
        engine.set_knob("bidir", 1)


def test_pade_orders_do_not_move_with_the_knob(engine):
    p = problem(20)
    set_problem(engine, p)
    engine.set_knob("action", 0)
    try:
        one = engine.evaluate(p["controls"], True)
        orders_one = engine.pade_orders()
        assert not executed(engine)
        engine.set_knob("action_degree", 0)
        zero = engine.evaluate(p["controls"], True)
        orders_zero = engine.pade_orders()
        assert not executed(engine)
    finally:
        engine.set_knob("action_degree", 1)
        engine.set_knob("action", 1)
    assert orders_one == orders_zero and sum(orders_one.values()) == 3 * (N - 1)
    for x, y in zip(one, zero):
        assert np.array_equal(x, y)


def test_the_knob_takes_zero_and_one_only(engine):
    for bad in (-1, 2):
        with pytest.raises(Exception):
            engine.set_knob("action_degree", bad)
    engine.set_knob("action_degree", 1)
