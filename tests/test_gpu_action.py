"""
GPU tests (-m gpu) of the matrix-free route (qoc_amd/csrc/qocx_action.hip): one state, Hermitian
H, 17 <= n <= 32, one final TargetStateInfidelity - the sweeps apply exp(a) by the truncated Taylor
series and nothing is factored. Against the oracle and against the Pade route at the project's
gates (1e-10 cost and final states, 1e-8 of the largest entry for the gradient), bit-identity across
chunks, time segments and schedules, exact zeros in the padding, and every condition under which
the route must yield to the Pade route. tests/test_action_model.py checks the mathematics on the CPU.
"""

import json
import os

import numpy as np
import pytest

from oracle import qoc_numpy as onp
from tests.helpers import rel_err

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, K, DT = 14, 2, 0.05  # 13 steps
SIZES = (17, 20, 32)


@pytest.fixture(scope="module")
def engine():
    from qoc_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


def hermitian(rng, n):
    m = rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))
    m = (m + m.conj().T) / 2
    return m / onp.one_norm(m)


_cache = {}


def problem(n, states=1, skew=0.0, step_cost=False):
    """||H0||_1 = ||G_k||_1 = 1, so a step's bound is DT (1 + sum |u_k|): seed 0 quiet (degree 8),
    seed 1 of order one, seed 2 loud (up to 0.05 * 11 = 0.55: degree 15)."""
    key = (n, states, skew, step_cost)
    if key in _cache:
        return _cache[key]
    rng = np.random.default_rng(1000 + n)
    h0, g = hermitian(rng, n), [hermitian(rng, n) for _ in range(K)]
    if skew:
        h0 = h0 + 1j * skew * hermitian(rng, n)  # not Hermitian
    psi0 = np.eye(n, dtype=np.complex128)[:states]
    target = rng.standard_normal((states, n)) + 1j * rng.standard_normal((states, n))
    target /= np.linalg.norm(target, axis=1, keepdims=True)
    controls = rng.uniform(-1, 1, (3, N, K)) * np.array([1e-3, 1.0, 5.0])[:, None, None]
    T = DT * (N - 1)
    from qoc_amd.engine import COST_TARGET_COHERENT, COST_TARGET_INCOHERENT
    descs = [dict(kind=COST_TARGET_COHERENT, step_cost=0, scale=1.0, vectors=target)]
    ocosts = [onp.TargetStateInfidelity(target[:, :, None])]
    if step_cost:
        descs.append(dict(kind=COST_TARGET_INCOHERENT, step_cost=1, scale=1.3 / (N - 1), vectors=target))
        ocosts.append(onp.TargetStateInfidelityTime(N, target[:, :, None], neglect_relative_pahse=True,
                                                    cost_multiplier=1.3))
    oracle = onp.SchroedingerProblem(
        T, lambda u, t: h0 + sum(u[k] * g[k] for k in range(K)), psi0[:, :, None], N,
        control_eval_count=N, costs=ocosts, control_count=K)
    p = dict(n=n, S=states, h0=h0, g=g, psi0=psi0, T=T, descs=descs, oracle=oracle, controls=controls)
    p["refs"] = [onp.evaluate_with_grad(oracle, controls[b]) for b in range(len(controls))]
    _cache[key] = p
    return p


def set_problem(engine, p):
    engine.set_schroedinger_problem(p["n"], p["S"], K, N, N, p["T"], p["h0"][None], np.stack(p["g"])[None],
                                    p["psi0"], costs=p["descs"])


def assert_gates(tag, out, refs):
    """out = (cost[B], grads[B], final[B, S, n]) against [(cost, grads, final[S, n, 1])] per seed."""
    worst = dict(cost=0.0, final=0.0, grad=0.0)
    for b, (rc, rg, rf) in enumerate(refs):
        worst["cost"] = max(worst["cost"], abs(out[0][b] - rc))
        worst["final"] = max(worst["final"], np.abs(out[2][b] - rf[:, :, 0]).max())
        worst["grad"] = max(worst["grad"], rel_err(out[1][b], rg))
    print("{}: {}".format(tag, " ".join("%s=%.2e" % kv for kv in worst.items())))
    assert worst["cost"] < 1e-10 and worst["final"] < 1e-10 and worst["grad"] < 1e-8, (tag, worst)
    return worst


def executed(engine):
    return {m: c for m, c in engine.action_degrees().items() if c}


# ---- 1. parity with the oracle ---------------------------------------------------------------------

@pytest.mark.parametrize("n", SIZES)
def test_parity_with_the_oracle(engine, n):
    p = problem(n)
    set_problem(engine, p)
    engine.set_pipeline(3)  # the vectors are carried from launch to launch
    try:
        out = engine.evaluate(p["controls"], True)
        degrees = executed(engine)
    finally:
        engine.set_pipeline(0)
    print("n={} degrees {}".format(n, degrees))
    assert sum(degrees.values()) == 3 * (N - 1) and len(degrees) >= 3, degrees
    assert engine.action_reruns() == 0
    assert_gates("action n=%d" % n, out, p["refs"])


# ---- 2. agreement with the Pade route ----------------------------------------------------------------

_differences = {}


@pytest.mark.parametrize("n", SIZES)
def test_agreement_with_the_pade_route(engine, n):
    p = problem(n)
    set_problem(engine, p)
    action = engine.evaluate(p["controls"], True)
    assert executed(engine)
    engine.set_knob("action", 0)
    try:
        pade = engine.evaluate(p["controls"], True)
        assert not executed(engine)
    finally:
        engine.set_knob("action", 1)
    refs = [(pade[0][b], pade[1][b], pade[2][b][:, :, None]) for b in range(3)]
    worst = assert_gates("action against Pade n=%d" % n, action, refs)
    _differences[n] = dict(n=n, steps=N - 1, seeds=3, max_abs_cost=worst["cost"],
                           max_abs_final=worst["final"], max_rel_grad=worst["grad"])
    with open(os.path.join(ROOT, "profiles", "action_vs_pade.jsonl"), "w") as f:
        for size in sorted(_differences):
            f.write(json.dumps(_differences[size]) + "\n")


# ---- 3. bit-identity -----------------------------------------------------------------------------------

def test_bit_identity_across_chunks_segments_and_schedules(engine):
    p = problem(20)
    set_problem(engine, p)
    ref = engine.evaluate(p["controls"], True)
    assert executed(engine)

    def same(tag):
        out = engine.evaluate(p["controls"], True)
        assert executed(engine), tag
        for x, y in zip(ref, out):
            assert np.array_equal(x, y), tag

    try:
        engine.set_chunk(1)
        same("chunk 1")
        engine.set_chunk(0)
        for segments in (1, 2, 3, 8):
            engine.set_pipeline(segments)
            same("segments %d" % segments)
            engine.set_knob("bidir", 0)
            same("segments %d, one-sided" % segments)
            engine.set_knob("bidir", 1)
        engine.set_pipeline(0)
        forward = engine.evaluate(p["controls"], False)
        assert executed(engine)
        assert np.array_equal(forward[0], ref[0]) and np.array_equal(forward[2], ref[2])
    finally:
        engine.set_chunk(0)
        engine.set_pipeline(0)
        engine.set_knob("bidir", 1)


# ---- 4. padding ------------------------------------------------------------------------------------------

def test_padding_stays_exactly_zero(engine):
    """n = 17 on 32 padded rows: the pad rows and columns of a are zero, so the pad entries of every
    Taylor term are exactly zero. The public download returns the n true entries; that they were not
    polluted from the padding shows in the bit-identity with the state embedded in n = 20 (three
    decoupled levels appended: the same arithmetic on the first 17 entries plus exact zeros)."""
    p = problem(17)
    set_problem(engine, p)
    small = engine.evaluate(p["controls"], True)
    assert executed(engine)
    n2 = 20
    h0 = np.zeros((n2, n2), dtype=np.complex128)
    h0[:17, :17] = p["h0"]
    g = np.zeros((K, n2, n2), dtype=np.complex128)
    g[:, :17, :17] = np.stack(p["g"])
    psi0 = np.zeros((1, n2), dtype=np.complex128)
    psi0[:, :17] = p["psi0"]
    target = np.zeros((1, n2), dtype=np.complex128)
    target[:, :17] = p["descs"][0]["vectors"]
    engine.set_schroedinger_problem(n2, 1, K, N, N, p["T"], h0[None], g[None], psi0,
                                    costs=[dict(p["descs"][0], vectors=target)])
    big = engine.evaluate(p["controls"], True)
    assert executed(engine)
    assert np.all(big[2][:, :, 17:] == 0)
    assert np.array_equal(big[2][:, :, :17], small[2])
    assert np.array_equal(big[0], small[0]) and np.array_equal(big[1], small[1])


# ---- 5. the route yields ---------------------------------------------------------------------------------

def check_yield(engine, p, controls=None, refs=None):
    out = engine.evaluate(p["controls"] if controls is None else controls, True)
    assert not executed(engine)
    assert_gates("yield", out, p["refs"] if refs is None else refs)


def test_yields_to_pade_order_13(engine):
    p = problem(20)
    set_problem(engine, p)
    engine.set_knob("pade_order", 13)
    try:
        check_yield(engine, p)
        assert engine.pade_orders()[13] == 3 * (N - 1)
    finally:
        engine.set_knob("pade_order", 0)
    engine.evaluate(p["controls"], True)
    assert executed(engine)


def test_yields_to_two_states(engine):
    p = problem(20, states=2)
    set_problem(engine, p)
    check_yield(engine, p)


def test_yields_to_a_step_cost(engine):
    p = problem(20, step_cost=True)
    engine.set_schroedinger_problem(p["n"], 1, K, N, N, p["T"], p["h0"][None], np.stack(p["g"])[None],
                                    p["psi0"], costs=p["descs"], cost_eval_step=1)
    check_yield(engine, p)


def test_yields_to_a_non_hermitian_drift(engine):
    p = problem(20, skew=0.05)
    set_problem(engine, p)
    check_yield(engine, p)


def test_yields_to_a_host_bound_above_theta_18(engine):
    p = problem(20)
    set_problem(engine, p)
    loud = p["controls"].copy()
    loud[2] = 12.0 + p["controls"][2] / 5  # 11 < u < 13 at every knot and every midpoint
    assert DT * (1 + 2 * 11.0) > 1.09
    refs = p["refs"][:2] + [onp.evaluate_with_grad(p["oracle"], loud[2])]
    check_yield(engine, p, loud, refs)
    engine.evaluate(p["controls"], True)
    assert executed(engine)


def test_stale_host_bound_runs_again_on_the_pade_route(engine):
    """The resident optimizer step moves the controls on the device without telling the host's bound:
    an SGD step with a huge rate from quiet controls makes every step louder than the buffers were
    sized for. The degree is decided on the device, the status bit sends the evaluation to the Pade
    route, and the counter says so."""
    p = problem(20)
    set_problem(engine, p)
    quiet = p["controls"][:1]
    engine.upload_controls(quiet)
    engine.opt_begin()
    engine.eval_resident(True)
    first = engine.download_results(True)
    degrees = executed(engine)
    assert degrees and max(degrees) <= 9, degrees
    before = engine.action_reruns()
    rate = 4.0 / np.abs(first[1]).max()  # the largest control moves by 4: a bound near 0.05 * 5
    flags = np.ones(1, dtype=np.uint8)
    engine.opt_step(0, flags, flags, rate)
    moved = quiet - rate * first[1]
    engine.eval_resident(True)
    out = engine.download_results(True)
    ref = onp.evaluate_with_grad(p["oracle"], moved[0])
    assert_gates("after the step", out, [ref])
    assert engine.action_reruns() == before + 1 and not executed(engine)
