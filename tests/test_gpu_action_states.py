"""
GPU tests (-m gpu) of the matrix-free route with two to four states per seed
(qoc_amd/csrc/qocx_action_states.hip, knob "action_states"): Hermitian H, 17 <= n <= 32, one coherent
final TargetStateInfidelity - a wave per state applies exp(a) by the truncated Taylor series, the
gradient kernel adds the states' generator cotangents. On the fixture of tests/test_gpu_action.py
extended to S states: against the oracle and against the Pade route at the project's gates (1e-10 cost
and final states, 1e-8 of the largest entry for the gradient), bit-identity across chunks, time
segments and schedules and with the one-state kernel, exact zeros in the padding, and every condition
under which the route must yield. tests/test_action_states_model.py checks the mathematics on the CPU.
"""

import json
import os

import numpy as np
import pytest

from oracle import qoc_numpy as onp
from tests.test_gpu_action import DT, K, N, ROOT, SIZES, assert_gates, executed, problem, set_problem

pytestmark = pytest.mark.gpu

STATES = (2, 3, 4)


@pytest.fixture(scope="module")
def engine():
    from qoc_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture
def states4(engine):
    """knob "action_states" = 4 for the test, 0 after it"""
    engine.set_knob("action_states", 4)
    try:
        yield engine
    finally:
        engine.set_knob("action_states", 0)


# ---- 1. parity with the oracle ---------------------------------------------------------------------

@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("S", STATES)
def test_parity_with_the_oracle(states4, n, S):
    engine = states4
    p = problem(n, states=S)
    set_problem(engine, p)
    engine.set_pipeline(3)  # the vectors are carried from launch to launch
    try:
        out = engine.evaluate(p["controls"], True)
        degrees = executed(engine)
    finally:
        engine.set_pipeline(0)
    print("n={} S={} degrees {}".format(n, S, degrees))
    assert sum(degrees.values()) == 3 * (N - 1) and len(degrees) >= 3, degrees
    assert engine.action_reruns() == 0
    assert_gates("action n=%d S=%d" % (n, S), out, p["refs"])


# ---- 2. agreement with the Pade route ----------------------------------------------------------------

_differences = {}


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("S", STATES)
def test_agreement_with_the_pade_route(engine, n, S):
    p = problem(n, states=S)
    set_problem(engine, p)
    engine.set_knob("action_states", 4)
    try:
        action = engine.evaluate(p["controls"], True)
        assert executed(engine)
    finally:
        engine.set_knob("action_states", 0)
    pade = engine.evaluate(p["controls"], True)
    assert not executed(engine)
    refs = [(pade[0][b], pade[1][b], pade[2][b][:, :, None]) for b in range(3)]
    worst = assert_gates("action against Pade n=%d S=%d" % (n, S), action, refs)
    _differences[(n, S)] = dict(n=n, states=S, steps=N - 1, seeds=3, max_abs_cost=worst["cost"],
                                max_abs_final=worst["final"], max_rel_grad=worst["grad"])
    with open(os.path.join(ROOT, "profiles", "action_states_vs_pade.jsonl"), "w") as f:
        for key in sorted(_differences):
            f.write(json.dumps(_differences[key]) + "\n")


# ---- 3. bit-identity -----------------------------------------------------------------------------------

@pytest.mark.parametrize("S", STATES)
def test_bit_identity_across_chunks_segments_and_schedules(states4, S):
    engine = states4
    p = problem(20, states=S)
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


# ---- 4. a state is the one-state problem ---------------------------------------------------------------

def test_a_state_is_the_one_state_problem_bit_for_bit(states4):
    """The chain of state s reads nothing of the other states: its final state is, bit for bit, that of
    the one-state problem with psi0 = e_s on the one-state kernel (whose cost the forward chain does not
    read)."""
    engine = states4
    S = 3
    p = problem(20, states=S)
    set_problem(engine, p)
    many = engine.evaluate(p["controls"], False)
    assert executed(engine)
    for s in range(S):
        engine.set_schroedinger_problem(p["n"], 1, K, N, N, p["T"], p["h0"][None], np.stack(p["g"])[None],
                                        p["psi0"][s:s + 1],
                                        costs=[dict(p["descs"][0], vectors=p["descs"][0]["vectors"][s:s + 1])])
        one = engine.evaluate(p["controls"], False)
        assert executed(engine)
        assert np.array_equal(one[2][:, 0], many[2][:, s]), s


# ---- 5. padding ------------------------------------------------------------------------------------------

def test_padding_stays_exactly_zero(states4):
    """n = 17, S = 2 embedded in n = 20 with three decoupled levels (tests/test_gpu_action.py)."""
    engine = states4
    S = 2
    p = problem(17, states=S)
    set_problem(engine, p)
    small = engine.evaluate(p["controls"], True)
    assert executed(engine)
    n2 = 20
    h0 = np.zeros((n2, n2), dtype=np.complex128)
    h0[:17, :17] = p["h0"]
    g = np.zeros((K, n2, n2), dtype=np.complex128)
    g[:, :17, :17] = np.stack(p["g"])
    psi0 = np.zeros((S, n2), dtype=np.complex128)
    psi0[:, :17] = p["psi0"]
    target = np.zeros((S, n2), dtype=np.complex128)
    target[:, :17] = p["descs"][0]["vectors"]
    engine.set_schroedinger_problem(n2, S, K, N, N, p["T"], h0[None], g[None], psi0,
                                    costs=[dict(p["descs"][0], vectors=target)])
    big = engine.evaluate(p["controls"], True)
    assert executed(engine)
    assert np.all(big[2][:, :, 17:] == 0)
    assert np.array_equal(big[2][:, :, :17], small[2])
    assert np.array_equal(big[0], small[0]) and np.array_equal(big[1], small[1])


# ---- 6. the route yields ---------------------------------------------------------------------------------

def check_yield(engine, p, controls=None, refs=None):
    out = engine.evaluate(p["controls"] if controls is None else controls, True)
    assert not executed(engine)
    assert_gates("yield", out, p["refs"] if refs is None else refs)


def check_taken(engine, p):
    set_problem(engine, p)
    engine.evaluate(p["controls"], True)
    assert executed(engine)


def test_yields_to_five_states(states4):
    p = problem(20, states=5)
    set_problem(states4, p)
    check_yield(states4, p)


def test_yields_to_more_states_than_the_knob_says(engine):
    p = problem(20, states=3)
    set_problem(engine, p)
    engine.set_knob("action_states", 2)
    try:
        check_yield(engine, p)
        check_taken(engine, problem(20, states=2))
    finally:
        engine.set_knob("action_states", 0)


def test_knob_refuses_other_values(engine):
    for bad in (1, 5, -1, 64):
        with pytest.raises(Exception):
            engine.set_knob("action_states", bad)
    p = problem(20, states=2)  # ... and is still 0
    set_problem(engine, p)
    check_yield(engine, p)


def test_yields_to_an_incoherent_target(states4):
    from qoc_amd.engine import COST_TARGET_INCOHERENT
    p = problem(20, states=2)
    target = p["descs"][0]["vectors"]
    oracle = onp.SchroedingerProblem(
        p["T"], lambda u, t: p["h0"] + sum(u[k] * p["g"][k] for k in range(K)), p["psi0"][:, :, None], N,
        control_eval_count=N, costs=[onp.TargetStateInfidelity(target[:, :, None], neglect_relative_pahse=True)],
        control_count=K)
    refs = [onp.evaluate_with_grad(oracle, p["controls"][b]) for b in range(3)]
    states4.set_schroedinger_problem(p["n"], 2, K, N, N, p["T"], p["h0"][None], np.stack(p["g"])[None], p["psi0"],
                                     costs=[dict(kind=COST_TARGET_INCOHERENT, step_cost=0, scale=1.0, vectors=target)])
    check_yield(states4, p, refs=refs)


def test_yields_to_a_step_cost(states4):
    p = problem(20, states=2, step_cost=True)
    states4.set_schroedinger_problem(p["n"], 2, K, N, N, p["T"], p["h0"][None], np.stack(p["g"])[None],
                                     p["psi0"], costs=p["descs"], cost_eval_step=1)
    check_yield(states4, p)


def test_yields_to_a_non_hermitian_drift(states4):
    p = problem(20, states=2, skew=0.05)
    set_problem(states4, p)
    check_yield(states4, p)


def test_yields_to_pade_order_13(states4):
    engine = states4
    p = problem(20, states=2)
    set_problem(engine, p)
    engine.set_knob("pade_order", 13)
    try:
        check_yield(engine, p)
        assert engine.pade_orders()[13] == 3 * (N - 1)
    finally:
        engine.set_knob("pade_order", 0)
    engine.evaluate(p["controls"], True)
    assert executed(engine)


def test_yields_at_n_16(states4):
    p = problem(16, states=2)
    set_problem(states4, p)
    check_yield(states4, p)


def test_yields_at_n_40_on_the_wide_route(states4):
    engine = states4
    p = problem(40, states=2)
    set_problem(engine, p)
    engine.set_knob("action", 2)
    try:
        check_yield(engine, p)
    finally:
        engine.set_knob("action", 1)


def test_yields_to_a_host_bound_above_theta_18(states4):
    engine = states4
    p = problem(20, states=2)
    set_problem(engine, p)
    loud = p["controls"].copy()
    loud[2] = 12.0 + p["controls"][2] / 5  # 11 < u < 13 at every knot and every midpoint
    assert DT * (1 + 2 * 11.0) > 1.09
    refs = p["refs"][:2] + [onp.evaluate_with_grad(p["oracle"], loud[2])]
    check_yield(engine, p, loud, refs)
    engine.evaluate(p["controls"], True)
    assert executed(engine)


# ---- 7. a stale host bound -------------------------------------------------------------------------------

def test_stale_host_bound_runs_again_on_the_pade_route(states4):
    """tests/test_gpu_action.py, with two states: the resident SGD step makes every step louder than the
    buffers were sized for, every wave of a workgroup reads the same degree and leaves before the
    workgroup's barrier, the status bit sends the evaluation to the Pade route."""
    engine = states4
    p = problem(20, states=2)
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


# ---- 8. the public interface ---------------------------------------------------------------------------

def test_keyword_of_the_public_interface(monkeypatch):
    from qoc_amd.core import device
    from qoc_amd.core.schroedingerdiscrete import grape_schroedinger_discrete_batch
    from qoc_amd.standard import TargetStateInfidelity
    p = problem(20, states=2)
    h0, g = p["h0"], p["g"]
    made, degrees = [], []
    real = device.make_backend

    def recording(*args, **kw):
        """the backend of an evaluator, noting the degrees of each of its resident evaluations"""
        backend = real(*args, **kw)
        evaluate = backend.eval_resident

        def eval_resident(want_grad):
            evaluate(want_grad)
            degrees[-1].append(executed(backend))

        backend.eval_resident = eval_resident
        made.append(backend)
        degrees.append([])
        return backend

    monkeypatch.setattr(device, "make_backend", recording)
    initial = p["controls"][:2] * np.array([100.0, 0.5])[:, None, None]  # amplitudes 0.1 and 0.5

    def run(value):
        return grape_schroedinger_discrete_batch(
            K, N, [TargetStateInfidelity(p["descs"][0]["vectors"][:, :, None])], p["T"],
            lambda u, t: h0 + sum(u[j] * g[j] for j in range(K)), p["psi0"][:, :, None], N, initial,
            iteration_count=3, log_iteration_step=0, matrix_free=value)

    try:
        states = run("states")
        assert len(made) == 1 and len(degrees[0]) >= 3 and all(degrees[0]), degrees
        default = run("default")
        assert len(made) == 2 and len(degrees[1]) >= 3 and not any(degrees[1]), degrees
        assert np.abs(np.asarray(states.best_error) - np.asarray(default.best_error)).max() < 1e-10
    finally:
        for e in made:
            e.close()
