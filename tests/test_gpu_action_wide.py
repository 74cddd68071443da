"""
GPU tests (-m gpu) of the wide matrix-free route (qoc_amd/csrc/qocx_action4.hip, knob "action" = 2):
one state, Hermitian H, 33 <= n <= 64, one final TargetStateInfidelity - workgroups of three (n <= 48)
or four waves apply exp(a) by the truncated Taylor series and nothing is factored. Problems as in
tests/test_gpu_action.py (13 steps, operators of unit 1-norm, a quiet, an ordinary and a loud seed in
one upload), at n = 33 (one row past two tiles), 40 (ragged three tiles), 48 (full three tiles), 49
(one row into the fourth tile) and 64 (full four tiles). Against the oracle and the Pade route at the
project's gates (1e-10 cost and final states, 1e-8 of the largest entry for the gradient); the default
knob leaves every launch as it was; bit-identity across chunks, time segments and schedules; exact
zeros in the padding; and every condition under which the route must yield.
tests/test_action_wide_model.py checks the mathematics on the CPU.
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
SIZES = (33, 40, 48, 49, 64)


@pytest.fixture(scope="module")
def engine():
    from qoc_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture()
def wide(engine):
    """The engine with the wide route switched on; the default comes back afterwards."""
    engine.set_knob("action", 2)
    yield engine
    engine.set_knob("action", 1)
    engine.set_knob("latency", 0)
    engine.set_knob("pade_order", 0)
    engine.set_knob("bidir", 1)
    engine.set_chunk(0)
    engine.set_pipeline(0)


def hermitian(rng, n):
    m = rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))
    m = (m + m.conj().T) / 2
    return m / onp.one_norm(m)


_cache = {}


def problem(n, states=1, skew=0.0, step_cost=False, k=K):
    """||H0||_1 = ||G_k||_1 = 1, so a step's bound is DT (1 + sum |u_k|): seed 0 quiet, seed 1 of order
    one, seed 2 loud (k = 2: up to 0.05 * 11 = 0.55, degree 15). The oracle's answers are computed once."""
    key = (n, states, skew, step_cost, k)
    if key in _cache:
        return _cache[key]
    rng = np.random.default_rng(1000 + n)
    h0, g = hermitian(rng, n), [hermitian(rng, n) for _ in range(k)]
    if skew:
        h0 = h0 + 1j * skew * hermitian(rng, n)  # not Hermitian
    psi0 = np.eye(n, dtype=np.complex128)[:states]
    target = rng.standard_normal((states, n)) + 1j * rng.standard_normal((states, n))
    target /= np.linalg.norm(target, axis=1, keepdims=True)
    controls = rng.uniform(-1, 1, (3, N, k)) * np.array([1e-3, 1.0, 5.0])[:, None, None]
    T = DT * (N - 1)
    from qoc_amd.engine import COST_TARGET_COHERENT, COST_TARGET_INCOHERENT
    descs = [dict(kind=COST_TARGET_COHERENT, step_cost=0, scale=1.0, vectors=target)]
    ocosts = [onp.TargetStateInfidelity(target[:, :, None])]
    if step_cost:
        descs.append(dict(kind=COST_TARGET_INCOHERENT, step_cost=1, scale=1.3 / (N - 1), vectors=target))
        ocosts.append(onp.TargetStateInfidelityTime(N, target[:, :, None], neglect_relative_pahse=True,
                                                    cost_multiplier=1.3))
    oracle = onp.SchroedingerProblem(
        T, lambda u, t: h0 + sum(u[j] * g[j] for j in range(k)), psi0[:, :, None], N,
        control_eval_count=N, costs=ocosts, control_count=k)
    p = dict(n=n, S=states, K=k, h0=h0, g=g, psi0=psi0, T=T, descs=descs, oracle=oracle, controls=controls,
             target=target)
    p["refs"] = [onp.evaluate_with_grad(oracle, controls[b]) for b in range(len(controls))]
    _cache[key] = p
    return p


def set_problem(engine, p, **kw):
    engine.set_schroedinger_problem(p["n"], p["S"], p["K"], N, N, p["T"], p["h0"][None],
                                    np.stack(p["g"])[None], p["psi0"], costs=p["descs"], **kw)


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


def same_bits(a, b, tag=""):
    for x, y in zip(a, b):
        assert np.array_equal(x, y), tag


# ---- 1. parity with the oracle ---------------------------------------------------------------------

@pytest.mark.parametrize("n", SIZES)
def test_parity_with_the_oracle(wide, n):
    p = problem(n)
    set_problem(wide, p)
    wide.set_pipeline(3)  # the vectors are carried from launch to launch
    out = wide.evaluate(p["controls"], True)
    degrees = executed(wide)
    print("n={} degrees {}".format(n, degrees))
    assert sum(degrees.values()) == 3 * (N - 1) and len(degrees) >= 3, degrees
    assert wide.action_reruns() == 0
    assert_gates("wide action n=%d" % n, out, p["refs"])


# ---- 2. agreement with the Pade route ----------------------------------------------------------------

_differences = {}


@pytest.mark.parametrize("n", SIZES)
def test_agreement_with_the_pade_route(wide, n):
    p = problem(n)
    set_problem(wide, p)
    action = wide.evaluate(p["controls"], True)
    assert executed(wide)
    wide.set_knob("action", 0)
    pade = wide.evaluate(p["controls"], True)
    assert not executed(wide)
    assert_gates("Pade n=%d" % n, pade, p["refs"])
    refs = [(pade[0][b], pade[1][b], pade[2][b][:, :, None]) for b in range(3)]
    worst = assert_gates("wide action against Pade n=%d" % n, action, refs)
    _differences[n] = dict(n=n, steps=N - 1, seeds=3, max_abs_cost=worst["cost"],
                           max_abs_final=worst["final"], max_rel_grad=worst["grad"])
    with open(os.path.join(ROOT, "profiles", "action_wide_vs_pade.jsonl"), "w") as f:
        for size in sorted(_differences):
            f.write(json.dumps(_differences[size]) + "\n")


# ---- 3. the default is unchanged -----------------------------------------------------------------------

def test_default_knob_keeps_the_pade_route_above_32(engine):
    from qoc_amd.engine import Engine
    p = problem(40)
    fresh = Engine(0)  # no knob of it was ever set
    try:
        set_problem(fresh, p)
        untouched = fresh.evaluate(p["controls"], True)
        assert not executed(fresh)
    finally:
        fresh.close()
    set_problem(engine, p)
    engine.set_knob("action", 0)
    try:
        off = engine.evaluate(p["controls"], True)
        assert not executed(engine)
    finally:
        engine.set_knob("action", 1)
    same_bits(untouched, off)
    again = engine.evaluate(p["controls"], True)  # (and at the default's own value, set explicitly)
    assert not executed(engine)
    same_bits(untouched, again)


def test_wide_knob_changes_nothing_at_32(engine):
    p = problem(32)
    set_problem(engine, p)
    one = engine.evaluate(p["controls"], True)
    degrees = executed(engine)
    assert degrees
    engine.set_knob("action", 2)
    try:
        two = engine.evaluate(p["controls"], True)
        assert executed(engine) == degrees
    finally:
        engine.set_knob("action", 1)
    same_bits(one, two)


# ---- 4. bit-identity across launch cuts, exact zeros in the padding ------------------------------------

@pytest.mark.parametrize("n", (40, 49))
def test_bit_identity_across_chunks_segments_and_schedules(wide, n):
    p = problem(n)
    set_problem(wide, p)
    ref = wide.evaluate(p["controls"], True)
    assert executed(wide)

    def same(tag):
        out = wide.evaluate(p["controls"], True)
        assert executed(wide), tag
        same_bits(ref, out, tag)

    wide.set_chunk(1)
    same("chunk 1")
    wide.set_chunk(2)
    same("chunk 2")
    wide.set_chunk(0)
    for segments in (1, 2, 3, 8):
        wide.set_pipeline(segments)
        same("segments %d" % segments)
        wide.set_knob("bidir", 0)
        same("segments %d, one-sided" % segments)
        wide.set_knob("bidir", 1)
    wide.set_pipeline(0)
    forward = wide.evaluate(p["controls"], False)
    assert executed(wide)
    assert np.array_equal(forward[0], ref[0]) and np.array_equal(forward[2], ref[2])


@pytest.mark.parametrize("n, n2", [(33, 40), (49, 52)])
def test_padding_stays_exactly_zero(wide, n, n2):
    """The pad rows and columns of a are zero, so the pad entries of every Taylor term are exactly zero.
    The public download returns the n true entries; that they were not polluted from the padding shows
    in the bit-identity with the state embedded in n2 > n of the same tile count (decoupled levels
    appended: the same arithmetic on the first n entries plus exact zeros)."""
    p = problem(n)
    set_problem(wide, p)
    small = wide.evaluate(p["controls"], True)
    assert executed(wide)
    h0 = np.zeros((n2, n2), dtype=np.complex128)
    h0[:n, :n] = p["h0"]
    g = np.zeros((K, n2, n2), dtype=np.complex128)
    g[:, :n, :n] = np.stack(p["g"])
    psi0 = np.zeros((1, n2), dtype=np.complex128)
    psi0[:, :n] = p["psi0"]
    target = np.zeros((1, n2), dtype=np.complex128)
    target[:, :n] = p["target"]
    wide.set_schroedinger_problem(n2, 1, K, N, N, p["T"], h0[None], g[None], psi0,
                                  costs=[dict(p["descs"][0], vectors=target)])
    big = wide.evaluate(p["controls"], True)
    assert executed(wide)
    assert np.all(big[2][:, :, n:] == 0)
    assert np.array_equal(big[2][:, :, :n], small[2])
    assert np.array_equal(big[0], small[0]) and np.array_equal(big[1], small[1])


# ---- 5. the route yields ---------------------------------------------------------------------------------

def check_yield(wide, p, controls=None, refs=None):
    """No degrees under "action" = 2, the oracle's numbers, and the Pade route's bit for bit."""
    controls = p["controls"] if controls is None else controls
    out = wide.evaluate(controls, True)
    assert not executed(wide)
    assert_gates("yield", out, p["refs"] if refs is None else refs)
    wide.set_knob("action", 0)
    try:
        pade = wide.evaluate(controls, True)
    finally:
        wide.set_knob("action", 2)
    same_bits(out, pade)


def test_yields_to_pade_order_13(wide):
    p = problem(40)
    set_problem(wide, p)
    wide.set_knob("pade_order", 13)
    check_yield(wide, p)
    assert wide.pade_orders()[13] == 3 * (N - 1)
    wide.set_knob("pade_order", 0)
    wide.evaluate(p["controls"], True)
    assert executed(wide)


def test_yields_to_two_states(wide):
    p = problem(40, states=2)
    set_problem(wide, p)
    check_yield(wide, p)


def test_yields_to_a_step_cost(wide):
    p = problem(40, step_cost=True)
    set_problem(wide, p, cost_eval_step=1)
    check_yield(wide, p)


def test_yields_to_a_non_hermitian_drift(wide):
    p = problem(40, skew=0.05)
    set_problem(wide, p)
    check_yield(wide, p)


def test_yields_to_latency_mode(wide):
    p = problem(40)
    set_problem(wide, p)
    wide.set_knob("latency", 1)
    check_yield(wide, p)
    wide.set_knob("latency", 0)
    wide.evaluate(p["controls"], True)
    assert executed(wide)


def test_yields_to_a_host_bound_above_theta_18(wide):
    p = problem(40)
    set_problem(wide, p)
    loud = p["controls"].copy()
    loud[2] = 12.0 + p["controls"][2] / 5  # 11 < u < 13 at every knot and every midpoint
    assert DT * (1 + 2 * 11.0) > 1.09
    refs = p["refs"][:2] + [onp.evaluate_with_grad(p["oracle"], loud[2])]
    check_yield(wide, p, loud, refs)
    wide.evaluate(p["controls"], True)
    assert executed(wide)


@pytest.mark.parametrize("n", (40, 64))
def test_stale_host_bound_runs_again_on_the_pade_route(wide, n):
    """The resident optimizer step moves the controls on the device without telling the host's bound
    (tests/test_gpu_action.py): every step then asks for a degree beyond the buffers. The status bit
    sends the evaluation to the Pade route, and the counter says so."""
    p = problem(n)
    set_problem(wide, p)
    quiet = p["controls"][:1]
    wide.upload_controls(quiet)
    wide.opt_begin()
    wide.eval_resident(True)
    first = wide.download_results(True)
    degrees = executed(wide)
    assert degrees and max(degrees) <= 9, degrees
    before = wide.action_reruns()
    rate = 4.0 / np.abs(first[1]).max()  # the largest control moves by 4: a bound near 0.05 * 5
    flags = np.ones(1, dtype=np.uint8)
    wide.opt_step(0, flags, flags, rate)
    moved = quiet - rate * first[1]
    wide.eval_resident(True)
    out = wide.download_results(True)
    ref = onp.evaluate_with_grad(p["oracle"], moved[0])
    assert_gates("after the step", out, [ref])
    assert wide.action_reruns() == before + 1 and not executed(wide)
    wide.set_knob("action", 0)  # the same controls, where the step left them on the device
    wide.eval_resident(True)
    same_bits(out, wide.download_results(True))


# ---- 6. control counts -------------------------------------------------------------------------------------

@pytest.mark.parametrize("n, k", [(40, 1), (40, 3), (64, 1), (64, 3)])
def test_control_counts(wide, n, k):
    """One control (its image in registers, nothing read per step) and three (all but the first are
    read per step)."""
    p = problem(n, k=k)
    set_problem(wide, p)
    out = wide.evaluate(p["controls"], True)
    degrees = executed(wide)
    assert sum(degrees.values()) == 3 * (N - 1), degrees
    assert_gates("wide action n=%d K=%d" % (n, k), out, p["refs"])


# ---- 7. the keyword ----------------------------------------------------------------------------------------

def test_keyword_of_the_evaluator(engine):
    from qoc_amd.core import device
    from qoc_amd.standard import TargetStateInfidelity
    p = problem(40)
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
        ev = build(matrix_free="wide")
        wide_out = ev.evaluate_batch(p["controls"])
        degrees = executed(engine)
        assert sum(degrees.values()) == 3 * (N - 1), degrees
        for b, (rc, rg, rf) in enumerate(p["refs"]):
            assert abs(wide_out[0][b] - rc) < 1e-10 and abs(errors[b] - rc) < 1e-10
            assert rel_err(np.asarray(wide_out[1][b]).reshape(rg.shape), rg) < 1e-8
        with pytest.raises(ValueError, match="matrix_free"):
            build(matrix_free="narrow")
    finally:
        engine.set_knob("action", 1)
