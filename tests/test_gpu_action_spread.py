"""
GPU tests (-m gpu): the sweeps of the matrix-free route (qoc_amd/csrc/qocx_action.hip) with their vector in
spread form, and each sweep as ONE launch up to the crossing of the two. None of it may move a bit: only which
lane holds a value and how the steps are cut into launches changed.

1. The problems of tests/action_bits_cases.py against tests/golden/action_bits/ with the evaluation cut into
   2, 3 and 5 time segments: an odd segment count, a crossing that is not the middle, a fused first half.
2. The large-launch plan - three pieces in the outer segments, the fused way to the crossing - at the
   smallest batch that reaches it, 64 seeds x 256 steps (and x 257, where the pieces of a segment have
   unequal lengths), n = 17 and 32, K = 2: the default pipeline, and the knob "action_plan" = 0 (a launch
   per piece), against ONE launch of the same build (set_pipeline(1)), which tests/test_gpu_action_bits.py
   ties to the recorded bits. With and without the gradient.
3. Four seeds of the n = 32 problem of 2. against the oracle at the gates of tests/test_gpu_action.py.

Every evaluation here must have run on the matrix-free route: its executed degrees sum to B (N - 1) and it
was never handed back to the Pade route.
"""

import math

import numpy as np
import pytest

from oracle import qoc_numpy as onp
from tests import action_bits_cases as cases
from tests import action_degree_model as dm
from tests import action_model as am
from tests.helpers import rel_err

pytestmark = pytest.mark.gpu

CASES = [(n, K) for n in cases.SIZES for K in cases.CONTROL_COUNTS]
NAMES = cases.NAMES  # out[0] cost, out[1] grad, out[2] final


@pytest.fixture(scope="module")
def engine():
    from qoc_amd.engine import Engine
    e = Engine(0)
    yield e
    e.set_pipeline(0)
    e.close()


def evaluate_on_the_route(engine, controls, want_grad, steps):
    out = engine.evaluate(controls, want_grad)
    degrees = {m: c for m, c in engine.action_degrees().items() if c}
    assert sum(degrees.values()) == len(controls) * steps, degrees
    assert engine.action_reruns() == 0
    return out


def assert_bits(tag, out, ref, names=NAMES):
    for name in names:
        x, y = out[NAMES.index(name)], ref[NAMES.index(name)]
        assert x.shape == y.shape and x.dtype == y.dtype, (tag, name)
        print("{} {}: {} of {} entries differ, max |difference| {:.3e}".format(
            tag, name, int(np.count_nonzero(x != y)), x.size, float(np.abs(x - y).max())))
        assert np.array_equal(x, y), (tag, name)


# ---- 1. the recorded bits under other cuts ------------------------------------------------------------

_golden = {}


def golden(n, K):
    if (n, K) not in _golden:
        _golden[(n, K)] = tuple(np.load(cases.golden_path(n, K, name)) for name in NAMES)
    return _golden[(n, K)]


@pytest.mark.parametrize("segments", [2, 3, 5])
@pytest.mark.parametrize("n,K", CASES)
def test_the_recorded_bits_under_two_three_and_five_segments(engine, n, K, segments):
    p = cases.case(n, K)
    cases.set_problem(engine, p)
    engine.set_pipeline(segments)
    try:
        out = evaluate_on_the_route(engine, p["controls"], True, cases.N - 1)
    finally:
        engine.set_pipeline(0)
    assert_bits("n=%d K=%d segments=%d" % (n, K, segments), out, golden(n, K))


# ---- 2. the large-launch plan against one launch ------------------------------------------------------

BIG_B, BIG_K, PERIOD = 64, 2, 8
BIG = [(17, 256), (32, 256), (17, 257), (32, 257)]

_big = {}


def big_case(n, steps):
    """64 seeds, K = 2, ||H0||_1 = ||G_k||_1 = 1; the amplitudes ramp as in action_bits_cases, but again
    and again with a period of 8 knots, so that every launch piece (12 steps and more) sees the whole ramp."""
    if (n, steps) in _big:
        return _big[(n, steps)]
    N = steps + 1
    rng = np.random.default_rng(9000 + 10 * n + steps)
    h0, g = cases.hermitian(rng, n), [cases.hermitian(rng, n) for _ in range(BIG_K)]
    psi0 = np.eye(n, dtype=np.complex128)[:1]
    target = rng.standard_normal((1, n)) + 1j * rng.standard_normal((1, n))
    target /= np.linalg.norm(target)
    ramp = np.resize(np.linspace(0.03, 1.0, PERIOD), N)
    shape = rng.uniform(0.7, 1.0, (BIG_B, N, BIG_K)) * rng.choice([-1.0, 1.0], (BIG_B, N, BIG_K))
    peaks = np.resize(np.array(cases.PEAKS), BIG_B)
    controls = shape * ramp[None, :, None] * (peaks / BIG_K)[:, None, None]
    p = dict(n=n, K=BIG_K, N=N, h0=h0, g=g, psi0=psi0, target=target, T=cases.DT * steps, controls=controls)
    _big[(n, steps)] = p
    return p


def set_big_problem(engine, p):
    from qoc_amd.engine import COST_TARGET_COHERENT
    engine.set_schroedinger_problem(
        p["n"], 1, p["K"], p["N"], p["N"], p["T"], p["h0"][None], np.stack(p["g"])[None], p["psi0"],
        costs=[dict(kind=COST_TARGET_COHERENT, step_cost=0, scale=1.0, vectors=p["target"])])


def launch_pieces(steps, segments=8, parts_out=3):
    """The host's cut of a large two-sided evaluation (qocx_host_resident.hip: segment_bounds, run_two_sided):
    eight segments, the two in the middle of half weight, the first and the last in three pieces."""
    weights = [1.0] * segments
    weights[segments // 2 - 1] = weights[segments // 2] = 0.5
    lo, run = [0], 0.0
    for w in weights:
        run += w
        lo.append(max(lo[-1] + 1, int(math.floor(steps * run / sum(weights) + 0.5))))
    lo[segments] = steps
    pieces = []
    for i in range(segments):
        parts = parts_out if i in (0, segments - 1) else 1
        pieces += [(lo[i] + (lo[i + 1] - lo[i]) * q // parts, lo[i] + (lo[i + 1] - lo[i]) * (q + 1) // parts)
                   for q in range(parts)]
    return pieces


def assert_every_piece_runs_two_degrees(p, steps):
    """By the NumPy twin of the degree rule, for seed 0 (a piece that executes two degrees for one seed
    executes two degrees): with the exact spectral radii and with the engine's bound at its loosest."""
    pieces = launch_pieces(steps)
    assert len(pieces) == 12 and pieces[0][0] == 0 and pieces[-1][1] == steps
    assert BIG_B * steps >= 16384  # the batch at which the host takes this plan
    bounds = dm.step_bounds(p["h0"], p["g"], p["N"], p["T"], p["controls"][0])
    assert len(bounds) == steps
    for inflate in (1.0, 1.01):
        degrees = [dm.degree_rule(b1, inflate * b2) for b1, b2 in bounds]
        for a, b in pieces:
            assert b - a >= PERIOD and len(set(degrees[a:b])) >= 2, (a, b, degrees[a:b])
    host = cases.DT * (1.0 + abs(p["controls"]).max(axis=1).sum(axis=1).max())
    assert host < 0.9 * am.THETA[am.MAX_DEGREE], host


_one_launch = {}


def one_launch(engine, n, steps, want_grad):
    """The evaluation as one launch of the same build; the problem stays set."""
    p = big_case(n, steps)
    set_big_problem(engine, p)
    key = (n, steps, want_grad)
    if key not in _one_launch:
        engine.set_pipeline(1)
        try:
            _one_launch[key] = evaluate_on_the_route(engine, p["controls"], want_grad, steps)
        finally:
            engine.set_pipeline(0)
    return p, _one_launch[key]


@pytest.mark.parametrize("n,steps", BIG)
def test_the_large_plan_gives_the_bits_of_one_launch(engine, n, steps):
    p, ref = one_launch(engine, n, steps, True)
    assert_every_piece_runs_two_degrees(p, steps)
    out = evaluate_on_the_route(engine, p["controls"], True, steps)
    assert_bits("n=%d steps=%d default plan" % (n, steps), out, ref)


@pytest.mark.parametrize("n,steps", BIG[2:])
def test_a_launch_per_piece_gives_the_same_bits(engine, n, steps):
    p, ref = one_launch(engine, n, steps, True)
    engine.set_knob("action_plan", 0)
    try:
        out = evaluate_on_the_route(engine, p["controls"], True, steps)
    finally:
        engine.set_knob("action_plan", 1)
    assert_bits("n=%d steps=%d a launch per piece" % (n, steps), out, ref)


@pytest.mark.parametrize("n,steps", BIG)
def test_the_large_plan_without_the_gradient(engine, n, steps):
    p, ref = one_launch(engine, n, steps, False)
    out = evaluate_on_the_route(engine, p["controls"], False, steps)
    assert out[1] is None and ref[1] is None
    assert_bits("n=%d steps=%d forward only" % (n, steps), out, ref, names=("cost", "final"))
    # ... and the forward sweep alone leaves what it leaves beside the adjoint sweep
    assert_bits("n=%d steps=%d forward only against both" % (n, steps), out, one_launch(engine, n, steps, True)[1],
                names=("cost", "final"))


def test_the_knob_takes_zero_and_one_only(engine):
    from qoc_amd.engine import QocxError
    for bad in (-1, 2):
        with pytest.raises(QocxError):
            engine.set_knob("action_plan", bad)
    engine.set_knob("action_plan", 1)


# ---- 3. parity with the oracle ------------------------------------------------------------------------

def test_four_seeds_of_the_large_plan_against_the_oracle(engine):
    n, steps, seeds = 32, 256, 4
    p = big_case(n, steps)
    set_big_problem(engine, p)
    out = evaluate_on_the_route(engine, p["controls"], True, steps)
    h0, g, target = p["h0"], p["g"], p["target"]
    oracle = onp.SchroedingerProblem(
        p["T"], lambda u, t: h0 + u[0] * g[0] + u[1] * g[1], p["psi0"][:, :, None], p["N"],
        control_eval_count=p["N"], costs=[onp.TargetStateInfidelity(target[:, :, None])], control_count=BIG_K)
    worst = dict(cost=0.0, final=0.0, grad=0.0)
    for b in range(seeds):
        rc, rg, rf = onp.evaluate_with_grad(oracle, p["controls"][b])
        worst["cost"] = max(worst["cost"], abs(out[0][b] - rc))
        worst["final"] = max(worst["final"], np.abs(out[2][b] - rf[:, :, 0]).max())
        worst["grad"] = max(worst["grad"], rel_err(out[1][b], rg))
    print("large plan against the oracle: " + " ".join("%s=%.2e" % kv for kv in worst.items()))
    assert worst["cost"] < 1e-10 and worst["final"] < 1e-10 and worst["grad"] < 1e-8, worst
