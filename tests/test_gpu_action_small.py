"""
GPU tests (-m gpu) of the matrix-free route at n <= 16 (qoc_amd/csrc/qocx_action16.hip, knob
"action_small" = 1): one state, Hermitian H, one final TargetStateInfidelity - one wave per seed applies
exp(a) by the truncated Taylor series, its four rows of 16 lanes the four real products of a complex one,
and nothing is factored. Problems as in tests/test_gpu_action_wide.py (13 steps, operators of unit 1-norm,
a quiet, an ordinary and a loud seed in one upload), at n = 2 (smallest), 4 (four columns), 5, 8 (where the
Pade route switches to pack8), 9 (just past it), 13 (ragged) and 16 (full). Against the oracle and the Pade
route at the project's gates (1e-10 cost and final states, 1e-8 of the largest entry for the gradient); the
default knob leaves every launch as it was, and no other knob of the route reaches n <= 16; no effect
above 16; bit-identity across chunks, time segments and schedules; exact zeros in the padding; the control
counts on either side of the kernel's boundaries; every condition under which the route must yield (Pade
order 13, two states, a step cost, a non-Hermitian drift, latency mode, a bound above theta_18, tables with
nt > 1, quadratic terms, kept step states, knob "unit_adjoint" = 0, Magnus M4, a final ForbidStates); one
composed problem (a duration sweep) and the keyword.
tests/test_action_small_model.py checks the mathematics on the CPU; tests/test_gpu_action_features.py holds the
route to the oracle away from Nc = N, a plain batch and a coherent target of scale 1.
"""

import json
import os

import numpy as np
import pytest

from oracle import qoc_numpy as onp
from tests.helpers import rel_err
from tests.test_gpu_action_wide import DT, K, N, assert_gates, executed, problem, same_bits, set_problem

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (2, 4, 5, 8, 9, 13, 16)
STEPS = N - 1


@pytest.fixture(scope="module")
def engine():
    from qoc_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture()
def small(engine):
    """The engine with the route switched on; the defaults come back afterwards."""
    engine.set_knob("action_small", 1)
    yield engine
    engine.set_knob("action_small", 0)
    engine.set_knob("action", 1)
    engine.set_knob("action_states", 0)
    engine.set_knob("latency", 0)
    engine.set_knob("pade_order", 0)
    engine.set_knob("bidir", 1)
    engine.set_chunk(0)
    engine.set_pipeline(0)


def on_the_route(engine, seeds=3):
    degrees = executed(engine)
    assert sum(degrees.values()) == seeds * STEPS, degrees
    return degrees


# ---- 1. parity with the oracle ---------------------------------------------------------------------

@pytest.mark.parametrize("n", SIZES)
def test_parity_with_the_oracle(small, n):
    p = problem(n)
    set_problem(small, p)
    small.set_pipeline(3)  # the vectors are carried from launch to launch
    reruns = small.action_reruns()
    out = small.evaluate(p["controls"], True)
    degrees = on_the_route(small)
    print("n={} degrees {}".format(n, degrees))
    assert len(degrees) >= 3, degrees
    assert small.action_reruns() == reruns
    assert_gates("small action n=%d" % n, out, p["refs"])


# ---- 2. agreement with the Pade route ----------------------------------------------------------------

_differences = {}


@pytest.mark.parametrize("n", SIZES)
def test_agreement_with_the_pade_route(small, n):
    p = problem(n)
    set_problem(small, p)
    action = small.evaluate(p["controls"], True)
    on_the_route(small)
    small.set_knob("action_small", 0)
    pade = small.evaluate(p["controls"], True)
    assert not executed(small)
    assert_gates("Pade n=%d" % n, pade, p["refs"])
    refs = [(pade[0][b], pade[1][b], pade[2][b][:, :, None]) for b in range(3)]
    worst = assert_gates("small action against Pade n=%d" % n, action, refs)
    _differences[n] = dict(n=n, steps=STEPS, seeds=3, max_abs_cost=worst["cost"],
                           max_abs_final=worst["final"], max_rel_grad=worst["grad"])
    with open(os.path.join(ROOT, "profiles", "action_small_vs_pade.jsonl"), "w") as f:
        for size in sorted(_differences):
            f.write(json.dumps(_differences[size]) + "\n")


# ---- 3. the default is unchanged, and no other knob reaches n <= 16 -------------------------------------

@pytest.mark.parametrize("n", (8, 16))
def test_default_knob_keeps_the_pade_route(engine, n):
    from qoc_amd.engine import Engine
    p = problem(n)
    fresh = Engine(0)  # no knob of it was ever set
    try:
        set_problem(fresh, p)
        untouched = fresh.evaluate(p["controls"], True)
        assert not executed(fresh)
    finally:
        fresh.close()
    set_problem(engine, p)
    engine.set_knob("action_small", 0)
    off = engine.evaluate(p["controls"], True)
    assert not executed(engine)
    same_bits(untouched, off)


def test_other_knobs_of_the_route_do_not_reach_16(engine):
    p = problem(16)
    set_problem(engine, p)
    ref = engine.evaluate(p["controls"], True)
    assert not executed(engine)
    engine.set_knob("action", 2)
    engine.set_knob("action_states", 4)
    try:
        out = engine.evaluate(p["controls"], True)
        assert not executed(engine)
    finally:
        engine.set_knob("action", 1)
        engine.set_knob("action_states", 0)
    same_bits(ref, out)


@pytest.mark.parametrize("n", (17, 32))
def test_no_effect_above_16(engine, n):
    p = problem(n)
    set_problem(engine, p)
    one = engine.evaluate(p["controls"], True)
    degrees = executed(engine)
    assert degrees
    engine.set_knob("action_small", 1)
    try:
        two = engine.evaluate(p["controls"], True)
        assert executed(engine) == degrees
    finally:
        engine.set_knob("action_small", 0)
    same_bits(one, two)


def test_the_knob_takes_0_and_1_only(engine):
    for bad in (-1, 2, 16):
        with pytest.raises(Exception, match="action_small"):
            engine.set_knob("action_small", bad)
    engine.set_knob("action_small", 0)


# ---- 4. bit-identity across launch cuts, exact zeros in the padding ------------------------------------

@pytest.mark.parametrize("n", (5, 16))
def test_bit_identity_across_chunks_segments_and_schedules(small, n):
    p = problem(n)
    set_problem(small, p)
    ref = small.evaluate(p["controls"], True)
    on_the_route(small)

    def same(tag):
        out = small.evaluate(p["controls"], True)
        on_the_route(small)
        same_bits(ref, out, tag)

    small.set_chunk(1)
    same("chunk 1")
    small.set_chunk(2)
    same("chunk 2")
    small.set_chunk(0)
    for segments in (1, 2, 3, 8):
        small.set_pipeline(segments)
        same("segments %d" % segments)
        small.set_knob("bidir", 0)
        same("segments %d, one-sided" % segments)
        small.set_knob("bidir", 1)
    small.set_pipeline(0)
    forward = small.evaluate(p["controls"], False)
    on_the_route(small)
    assert np.array_equal(forward[0], ref[0]) and np.array_equal(forward[2], ref[2])


@pytest.mark.parametrize("n, n2", [(5, 7), (13, 16)])
def test_padding_stays_exactly_zero(small, n, n2):
    """The pad rows and columns of a are zero, so the pad entries of every Taylor term are exactly zero, and
    the order of the sums does not depend on n: the state embedded in n2 > n (decoupled levels appended) is
    the same arithmetic on the first n entries plus exact zeros."""
    p = problem(n)
    set_problem(small, p)
    inner = small.evaluate(p["controls"], True)
    on_the_route(small)
    h0 = np.zeros((n2, n2), dtype=np.complex128)
    h0[:n, :n] = p["h0"]
    g = np.zeros((K, n2, n2), dtype=np.complex128)
    g[:, :n, :n] = np.stack(p["g"])
    psi0 = np.zeros((1, n2), dtype=np.complex128)
    psi0[:, :n] = p["psi0"]
    target = np.zeros((1, n2), dtype=np.complex128)
    target[:, :n] = p["target"]
    small.set_schroedinger_problem(n2, 1, K, N, N, p["T"], h0[None], g[None], psi0,
                                   costs=[dict(p["descs"][0], vectors=target)])
    big = small.evaluate(p["controls"], True)
    on_the_route(small)
    assert np.all(big[2][:, :, n:] == 0)
    assert np.array_equal(big[2][:, :, :n], inner[2])
    assert np.array_equal(big[0], inner[0]) and np.array_equal(big[1], inner[1])


# ---- 5. control counts -------------------------------------------------------------------------------------

@pytest.mark.parametrize("n, k", [(4, 1), (4, 3), (4, 5), (16, 1), (16, 3), (16, 5)])
def test_control_counts(small, n, k):
    """The sweep holds ONE control's image in registers, the next THREE as the lanes' own doubles in LDS,
    and reads any further one from its image in every step: K = 1 is registers alone, K = 3 registers and
    LDS, K = 5 all three (the fifth control is the one read per step)."""
    p = problem(n, k=k)
    set_problem(small, p)
    out = small.evaluate(p["controls"], True)
    on_the_route(small)
    assert_gates("small action n=%d K=%d" % (n, k), out, p["refs"])


# ---- 6. the route yields ---------------------------------------------------------------------------------

def check_yield(small, p, controls=None, refs=None):
    """No degrees under "action_small" = 1, the oracle's numbers, and the Pade route's bit for bit."""
    controls = p["controls"] if controls is None else controls
    out = small.evaluate(controls, True)
    assert not executed(small)
    assert_gates("yield", out, p["refs"] if refs is None else refs)
    small.set_knob("action_small", 0)
    try:
        pade = small.evaluate(controls, True)
    finally:
        small.set_knob("action_small", 1)
    same_bits(out, pade)


def test_yields_to_pade_order_13(small):
    p = problem(8)
    set_problem(small, p)
    small.set_knob("pade_order", 13)
    check_yield(small, p)
    assert small.pade_orders()[13] == 3 * STEPS
    small.set_knob("pade_order", 0)
    small.evaluate(p["controls"], True)
    on_the_route(small)


def test_yields_to_two_states(small):
    p = problem(8, states=2)
    set_problem(small, p)
    check_yield(small, p)


def test_yields_to_a_step_cost(small):
    p = problem(8, step_cost=True)
    set_problem(small, p, cost_eval_step=1)
    check_yield(small, p)


def test_yields_to_a_non_hermitian_drift(small):
    p = problem(8, skew=0.05)
    set_problem(small, p)
    check_yield(small, p)


def test_yields_to_latency_mode(small):
    p = problem(8)
    set_problem(small, p)
    small.set_knob("latency", 1)
    check_yield(small, p)
    small.set_knob("latency", 0)
    small.evaluate(p["controls"], True)
    on_the_route(small)


def test_yields_to_a_host_bound_above_theta_18(small):
    p = problem(8)
    set_problem(small, p)
    loud = p["controls"].copy()
    loud[2] = 12.0 + p["controls"][2] / 5  # 11 < u < 13 at every knot and every midpoint
    assert DT * (1 + 2 * 11.0) > 1.09
    refs = p["refs"][:2] + [onp.evaluate_with_grad(p["oracle"], loud[2])]
    check_yield(small, p, loud, refs)
    small.evaluate(p["controls"], True)
    on_the_route(small)


def run_again_on_the_route(small, p):
    """The plain condition is back: the route runs."""
    small.evaluate(p["controls"], True)
    on_the_route(small)


def oracle_of(p, costs=None, hamiltonian=None, cls=onp.SchroedingerProblem, **kw):
    """The oracle's problem of problem(n) under other costs, another Hamiltonian or another Magnus policy."""
    h0, g = p["h0"], p["g"]

    def linear(u, t):
        return h0 + sum(u[j] * g[j] for j in range(K))

    return cls(p["T"], linear if hamiltonian is None else hamiltonian, p["psi0"][:, :, None], N,
               control_eval_count=N, costs=costs or [onp.TargetStateInfidelity(p["target"][:, :, None])],
               control_count=K, **kw)


def test_yields_to_time_dependent_tables(small):
    """nt = N - 1: H0(t) and G_k(t) of tests/time_dependent_drive.py, every sample different from its
    neighbour. The kernel reads ONE h0 and ONE set of G_k images: were the predicate to let such a problem
    through, the tables would be frozen at their first sample and the oracle's gates missed by orders of
    magnitude. The loudest seed stays below theta_18, so the host's bound is not what makes the route yield."""
    from tests import time_dependent_drive as tdd
    q = tdd.drive_problem(n=8, N=N, Nc=5, K=K, S=1, policy="M2", costs="final")
    assert q["h0"].shape[0] == q["g"].shape[0] == STEPS and q["nodes"] == 1
    controls = tdd.controls(q, 3, quiet=0.12, loud=0.9)
    assert q["dt"] * (1.3 * onp.one_norm(q["drive"].h0) + np.max(np.abs(controls) @ tdd.g_norms(q))) < 1.09
    tdd.set_engine_problem(small, q)
    refs = [onp.evaluate_with_grad(q["oracle"], u) for u in controls]
    check_yield(small, q, controls, refs)
    p = problem(8)
    set_problem(small, p)
    run_again_on_the_route(small, p)


def test_yields_to_quadratic_terms(small):
    """qocx_set_quadratic_terms, one term u_0^2 Q: the quadratic effective controls know no step table."""
    from tests.state_costs import _SlopesAtControls  # (d H / d u_k at the controls under evaluation)
    from tests.test_gpu_action_wide import hermitian
    p = problem(8)
    h0, g = p["h0"], p["g"]
    quad = 0.1 * hermitian(np.random.default_rng(808), 8)
    set_problem(small, p)
    small.set_quadratic_terms(np.array([[0, 0]], dtype=np.int32), quad[None])
    refs = []
    for u in p["controls"]:
        prob = oracle_of(p, hamiltonian=lambda c, t: h0 + c[0] * g[0] + c[1] * g[1] + c[0] * c[0] * quad,
                         cls=_SlopesAtControls)
        prob.slopes = lambda c: [g[0] + 2 * c[0] * quad, g[1]]
        prob.at_controls = u
        refs.append(onp.evaluate_with_grad(prob, u))
    assert abs(refs[1][0] - p["refs"][1][0]) > 1e-6  # (the term is felt)
    check_yield(small, p, refs=refs)
    small.set_quadratic_terms(np.zeros((0, 2), dtype=np.int32), None)
    run_again_on_the_route(small, p)


def test_yields_to_kept_step_states(small):
    """qocx_set_keep_step_states: the route keeps Taylor terms, not states. The states of every system step
    come from the Pade route, at the gate of the final states."""
    p = problem(8)
    set_problem(small, p)
    small.set_keep_step_states(True)
    try:
        check_yield(small, p)
        small.evaluate(p["controls"], True)
        assert not executed(small)
        steps = small.download_step_states()
    finally:
        small.set_keep_step_states(False)
    assert steps.shape == (3, N, 1, 8)
    worst = 0.0
    for b in range(3):
        states = []
        onp.evaluate(p["oracle"], p["controls"][b], intermediate=states)
        assert len(states) == N
        worst = max(worst, max(np.abs(steps[b, j] - states[j][:, :, 0]).max() for j in range(N)))
    print("step states against the oracle {:.2e}".format(worst))
    assert worst < 1e-10
    run_again_on_the_route(small, p)


def test_yields_to_the_knob_unit_adjoint_0(small):
    p = problem(8)
    set_problem(small, p)
    small.set_knob("unit_adjoint", 0)
    try:
        check_yield(small, p)
    finally:
        small.set_knob("unit_adjoint", 1)
    run_again_on_the_route(small, p)


def test_yields_to_magnus_m4(small):
    """M4 on a constant system (nt = 1): two quadrature nodes per step as the M4-linear effective controls."""
    p = problem(8)
    set_problem(small, p, magnus_policy="M4")
    oracle = oracle_of(p, magnus_policy="M4")
    refs = [onp.evaluate_with_grad(oracle, u) for u in p["controls"]]
    assert max(rel_err(r[1], s[1]) for r, s in zip(refs, p["refs"])) > 1e-6  # (the policy is felt)
    check_yield(small, p, refs=refs)
    set_problem(small, p)
    run_again_on_the_route(small, p)


def test_yields_to_a_final_forbid_states(small):
    """One final ForbidStates descriptor at S = 1 is not the unit adjoint's one separable target."""
    from tests import state_costs as sc
    p = problem(8)
    rng = np.random.default_rng(88)
    forbidden = rng.standard_normal((2, 8)) + 1j * rng.standard_normal((2, 8))
    forbidden /= np.linalg.norm(forbidden, axis=1, keepdims=True)
    cost = sc.DescriptorCost(sc.FORBID, 0, 0.9, forbidden, [2])
    q = dict(p, descs=[cost.descriptor()])
    set_problem(small, q)
    oracle = oracle_of(p, costs=[cost])
    refs = [onp.evaluate_with_grad(oracle, u) for u in p["controls"]]
    check_yield(small, q, refs=refs)
    set_problem(small, p)
    run_again_on_the_route(small, p)


@pytest.mark.parametrize("n", (8, 16))
def test_stale_host_bound_runs_again_on_the_pade_route(small, n):
    """The resident optimizer step moves the controls on the device without telling the host's bound
    (tests/test_gpu_action.py): every step then asks for a degree beyond the buffers. The status bit
    sends the evaluation to the Pade route, and the counter says so."""
    p = problem(n)
    set_problem(small, p)
    quiet = p["controls"][:1]
    small.upload_controls(quiet)
    small.opt_begin()
    small.eval_resident(True)
    first = small.download_results(True)
    degrees = executed(small)
    assert degrees and max(degrees) <= 9, degrees
    before = small.action_reruns()
    rate = 4.0 / np.abs(first[1]).max()  # the largest control moves by 4: a bound near 0.05 * 5
    flags = np.ones(1, dtype=np.uint8)
    small.opt_step(0, flags, flags, rate)
    moved = quiet - rate * first[1]
    small.eval_resident(True)
    out = small.download_results(True)
    ref = onp.evaluate_with_grad(p["oracle"], moved[0])
    assert_gates("after the step", out, [ref])
    assert small.action_reruns() == before + 1 and not executed(small)
    small.set_knob("action_small", 0)  # the same controls, where the step left them on the device
    small.eval_resident(True)
    same_bits(out, small.download_results(True))


# ---- 7. one composed problem ---------------------------------------------------------------------------------

def test_a_duration_sweep_stays_on_the_route(small):
    """Four seeds at n = 8, each at a duration of its own: on the device the (K + 1)-channel plain problem,
    so it takes the route with the plain predicate. Every seed against the oracle on its member(b)."""
    from qoc_amd.core import device
    from qoc_amd.standard import HamiltonianSweep, TargetStateInfidelity
    p = problem(8)
    h0, g = p["h0"], p["g"]
    rng = np.random.default_rng(88)
    taus = np.array([0.5, 0.8, 1.0, 1.3])
    u = rng.uniform(-1, 1, (4, N, K)) * np.array([1e-3, 1.0, 5.0, 2.5])[:, None, None]
    sweep = HamiltonianSweep.durations(lambda c, t: h0 + sum(c[j] * g[j] for j in range(K)), taus * p["T"], p["T"])
    ev = device.SchroedingerEvaluator(
        p["T"], sweep, p["psi0"][:, :, None], N, control_count=K, control_eval_count=N,
        costs=[TargetStateInfidelity(p["target"][:, :, None])], backend=small, matrix_free="small")
    reruns = small.action_reruns()
    errors, grads, finals, _ = ev.evaluate_batch(u)
    on_the_route(small, seeds=4)
    assert small.action_reruns() == reruns
    out = (np.asarray(errors), np.asarray(grads).reshape(u.shape), np.asarray(finals).reshape(4, 1, 8))
    refs = []
    for b in range(4):
        member = onp.SchroedingerProblem(p["T"], sweep.member(b), p["psi0"][:, :, None], N, control_eval_count=N,
                                         costs=[onp.TargetStateInfidelity(p["target"][:, :, None])],
                                         control_count=K)
        cost, grad, final = onp.evaluate_with_grad(member, u[b])
        refs.append((cost, np.real(grad), final))
    assert_gates("durations n=8", out, refs)


# ---- 8. the keyword ----------------------------------------------------------------------------------------

def test_keyword_of_the_evaluator(engine):
    from qoc_amd.core import device
    from qoc_amd.standard import TargetStateInfidelity
    p = problem(8)
    h0, g = p["h0"], p["g"]

    def build(**kw):
        return device.SchroedingerEvaluator(
            p["T"], lambda u, t: h0 + sum(u[j] * g[j] for j in range(K)), p["psi0"][:, :, None], N,
            control_count=K, control_eval_count=N, costs=[TargetStateInfidelity(p["target"][:, :, None])],
            backend=engine, **kw)

    try:
        ev = build(matrix_free="default")
        errors, grads, finals, _ = ev.evaluate_batch(p["controls"])
        assert not executed(engine)
        ev = build(matrix_free="small")
        small_out = ev.evaluate_batch(p["controls"])
        on_the_route(engine)
        for b, (rc, rg, rf) in enumerate(p["refs"]):
            assert abs(small_out[0][b] - rc) < 1e-10 and abs(errors[b] - rc) < 1e-10
            assert rel_err(np.asarray(small_out[1][b]).reshape(rg.shape), rg) < 1e-8
        with pytest.raises(ValueError, match="matrix_free"):
            build(matrix_free="tiny")
    finally:
        engine.set_knob("action_small", 0)
