"""
GPU tests (-m gpu) of the matrix-free route under step costs and several costs
(qoc_amd/csrc/qocx_action_costs.hip, knob "action_costs"): one state, Hermitian H, 17 <= n <= 32, any set
of device cost descriptors - the sweeps apply exp(a) by the truncated Taylor series, the adjoint sweep
carries the true cotangent, nothing is factored. On the problems of tests/action_costs_cases.py (three
seeds, 12 or 13 steps, cost_eval_step 3, the descriptor sets of tests/state_costs.py): against the oracle
and against the Pade route at the project's gates (1e-10 cost and final states, 1e-8 of the largest entry
for the gradient), bit-identity across chunks, time segments and schedules, exact zeros in the padding,
and every condition under which the route must yield. tests/test_action_costs_model.py checks the
mathematics on the CPU, tests/test_action_costs_cases_host.py that a misread cost table could not pass.
"""

import json
import os

import numpy as np
import pytest

from tests import action_costs_cases as acc
from tests import state_costs as sc
from tests.test_gpu_action import ROOT, assert_gates, executed

pytestmark = pytest.mark.gpu

K, CES = acc.K, acc.CES
MIXED = "target_after_ragged_forbid"  # a step forbid, a step target and a final target


@pytest.fixture(scope="module")
def engine():
    from qoc_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture
def costs1(engine):
    """knob "action_costs" = 1 for the test, 0 after it"""
    engine.set_knob("action_costs", 1)
    try:
        yield engine
    finally:
        engine.set_knob("action_costs", 0)


def variant(p, costs, **changes):
    """The problem p with some inputs changed and the oracle's references for `costs` on it (scales as
    balanced on p)."""
    q = {k: v for k, v in p.items() if isinstance(k, str)}
    q.update(changes)
    q["refs"] = [sc.evaluate(q, costs, b) for b in range(len(q["controls"]))]
    return q


def seeds_one_by_one(engine, controls):
    outs = [engine.evaluate(controls[b:b + 1], True) for b in range(len(controls))]
    return tuple(np.concatenate([o[i] for o in outs]) for i in range(3))


# ---- 1. parity with the oracle ---------------------------------------------------------------------

@pytest.mark.parametrize("N", acc.STEP_COUNTS)
@pytest.mark.parametrize("n", acc.SIZES)
@pytest.mark.parametrize("name", acc.NEW_SETS)
def test_parity_with_the_oracle(costs1, name, n, N):
    engine = costs1
    p = acc.build(n, N)
    acc.set_problem(engine, p, acc.descriptors(name, p))
    engine.set_pipeline(3)  # vector, cotangent and partial cost are carried from launch to launch
    try:
        out = engine.evaluate(p["controls"], True)
        degrees = executed(engine)
    finally:
        engine.set_pipeline(0)
    print("{} n={} N={} degrees {}".format(name, n, N, degrees))
    assert sum(degrees.values()) == 3 * (N - 1) and len(degrees) >= 3, degrees
    assert engine.action_reruns() == 0
    assert_gates("action costs %s n=%d N=%d" % (name, n, N), out, acc.references(name, p))


# ---- 2. agreement with the Pade route ----------------------------------------------------------------

_differences = {}


@pytest.mark.parametrize("N", acc.STEP_COUNTS)
@pytest.mark.parametrize("n", acc.SIZES)
@pytest.mark.parametrize("name", acc.NEW_SETS)
def test_agreement_with_the_pade_route(engine, name, n, N):
    p = acc.build(n, N)
    acc.set_problem(engine, p, acc.descriptors(name, p))
    engine.set_knob("action_costs", 1)
    try:
        action = engine.evaluate(p["controls"], True)
        assert executed(engine)
    finally:
        engine.set_knob("action_costs", 0)
    pade = engine.evaluate(p["controls"], True)
    assert not executed(engine)
    refs = [(pade[0][b], pade[1][b], pade[2][b][:, :, None]) for b in range(3)]
    worst = assert_gates("action costs against Pade %s n=%d N=%d" % (name, n, N), action, refs)
    _differences[(name, n, N)] = dict(set=name, n=n, steps=N - 1, seeds=3, cost_eval_step=CES,
                                      max_abs_cost=worst["cost"], max_abs_final=worst["final"],
                                      max_rel_grad=worst["grad"])
    with open(os.path.join(ROOT, "profiles", "action_costs_vs_pade.jsonl"), "w") as f:
        for key in sorted(_differences):
            f.write(json.dumps(_differences[key]) + "\n")


# ---- 3. bit-identity -----------------------------------------------------------------------------------

def one_sided_bounds(nsteps, nseg):
    """segment_bounds of qocx_host_resident.hip for the one-sided schedule."""
    wgt = [1.0] * nseg
    if nseg >= 4:
        wgt[nseg - 2], wgt[nseg - 1] = 0.6, 0.35
    lo, run = [0], 0.0
    for i in range(nseg):
        run += wgt[i]
        lo.append(max(lo[i] + 1, int(np.floor(nsteps * run / sum(wgt) + 0.5))))
    lo[nseg] = nsteps
    for i in range(nseg - 1, 0, -1):
        lo[i] = min(lo[i], lo[i + 1] - 1)
    return lo


def test_segment_boundaries_meet_the_cost_steps():
    """12 steps in two segments: cost step 6 opens the second one; 13 steps in two: cost step 6 is the last
    step of the first; and eight segments put boundaries on cost steps and beside them."""
    assert one_sided_bounds(12, 2) == [0, 6, 12] and one_sided_bounds(13, 2) == [0, 7, 13]
    assert one_sided_bounds(12, 3) == [0, 4, 8, 12] and one_sided_bounds(13, 3) == [0, 4, 9, 13]
    assert {3, 9} <= set(one_sided_bounds(12, 8)) and len(one_sided_bounds(12, 8)) == 9


@pytest.mark.parametrize("N", acc.STEP_COUNTS)
@pytest.mark.parametrize("name", [MIXED, "two_forbids"])
def test_bit_identity_across_chunks_segments_and_schedules(costs1, name, N):
    engine = costs1
    p = acc.build(20, N)
    acc.set_problem(engine, p, acc.descriptors(name, p))
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
            same("segments %d, bidir 0" % segments)
            engine.set_knob("bidir", 1)
            forward = engine.evaluate(p["controls"], False)
            assert executed(engine)
            assert np.array_equal(forward[0], ref[0]) and np.array_equal(forward[2], ref[2]), segments
        engine.set_pipeline(0)
        forward = engine.evaluate(p["controls"], False)
        assert executed(engine)
        assert np.array_equal(forward[0], ref[0]) and np.array_equal(forward[2], ref[2])
    finally:
        engine.set_chunk(0)
        engine.set_pipeline(0)
        engine.set_knob("bidir", 1)


# ---- 4. step costs of scale 0 --------------------------------------------------------------------------

@pytest.mark.parametrize("n", acc.SIZES)
def test_step_costs_of_scale_zero_leave_the_one_target_problem(costs1, n):
    """One final coherent target, alone (the unit adjoint's kernels) and beside step descriptors of scale 0
    (the kernels of this route): the forward chains do the same arithmetic, so the final states are equal
    bit for bit; costs and gradients - the unit adjoint against the general one - agree at the gates."""
    engine = costs1
    p = acc.build(n, 13)
    target = acc.descriptors("final_coherent", p)
    acc.set_problem(engine, p, target)
    alone = engine.evaluate(p["controls"], True)
    assert executed(engine)
    silent = [dict(d, scale=0.0) for d in acc.descriptors("two_forbids", p) + acc.descriptors("step_coherent", p)]
    acc.set_problem(engine, p, target + silent)
    beside = engine.evaluate(p["controls"], True)
    assert executed(engine)
    assert np.array_equal(alone[2], beside[2])
    refs = [(alone[0][b], alone[1][b], alone[2][b][:, :, None]) for b in range(3)]
    assert_gates("scale 0 n=%d" % n, beside, refs)


# ---- 5. padding ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n, n2", [(17, 20), (20, 24)])
def test_padding_stays_exactly_zero(costs1, n, n2):
    """The problem embedded in n2 levels, the appended ones decoupled: the same arithmetic on the first n
    entries plus exact zeros (tests/test_gpu_action.py), through the cost code and the cotangents too."""
    engine = costs1
    p = acc.build(n, 13)
    descs = acc.descriptors(MIXED, p)
    acc.set_problem(engine, p, descs)
    small = engine.evaluate(p["controls"], True)
    assert executed(engine)

    def embed(a, axes):
        out = np.zeros([n2 if ax in axes else d for ax, d in enumerate(a.shape)], dtype=np.complex128)
        out[tuple(slice(0, d) for d in a.shape)] = a
        return out

    big_descs = [dict(d, vectors=embed(np.asarray(d["vectors"]), (1,))) for d in descs]
    engine.set_schroedinger_problem(n2, 1, K, p["N"], p["N"], p["T"], embed(p["h0"], (0, 1))[None],
                                    embed(p["g"], (1, 2))[None], embed(p["init"], (1,)), costs=big_descs,
                                    cost_eval_step=CES)
    big = engine.evaluate(p["controls"], True)
    assert executed(engine)
    assert np.all(big[2][:, :, n:] == 0)
    assert np.array_equal(big[2][:, :, :n], small[2])
    assert np.array_equal(big[0], small[0]) and np.array_equal(big[1], small[1])


# ---- 6. the route yields ---------------------------------------------------------------------------------

def check_yield(engine, p, refs, one_by_one=False):
    out = seeds_one_by_one(engine, p["controls"]) if one_by_one else engine.evaluate(p["controls"], True)
    assert not executed(engine)
    assert_gates("yield", out, refs)


def check_taken(engine, p, name=MIXED):
    acc.set_problem(engine, p, acc.descriptors(name, p))
    engine.evaluate(p["controls"], True)
    assert executed(engine)


def test_yields_with_the_knob_at_0(engine):
    p = acc.build(20, 13)
    for name in (MIXED, "forbid_final", "two_finals"):
        acc.set_problem(engine, p, acc.descriptors(name, p))
        check_yield(engine, p, acc.references(name, p))


@pytest.mark.parametrize("name", acc.UNIT_SETS)
def test_one_final_target_keeps_its_kernels(engine, name):
    """unit_ok: the knob changes nothing - the same results bit for bit, at 1 and at 0."""
    p = acc.build(20, 14)
    acc.set_problem(engine, p, acc.descriptors(name, p))
    at0 = engine.evaluate(p["controls"], True)
    assert executed(engine)
    engine.set_knob("action_costs", 1)
    try:
        at1 = engine.evaluate(p["controls"], True)
        assert executed(engine)
    finally:
        engine.set_knob("action_costs", 0)
    for x, y in zip(at0, at1):
        assert np.array_equal(x, y)
    assert_gates("unit %s" % name, at1, acc.references(name, p))


def test_yields_on_the_wide_route(costs1):
    engine = costs1
    p = acc.build(40, 13)
    acc.set_problem(engine, p, acc.descriptors(MIXED, p))
    engine.set_knob("action", 2)
    try:
        check_yield(engine, p, acc.references(MIXED, p))
    finally:
        engine.set_knob("action", 1)


def test_yields_to_two_states(costs1):
    from tests.test_gpu_action import N, problem
    engine = costs1
    p = problem(20, states=2, step_cost=True)
    engine.set_knob("action_states", 4)
    try:
        engine.set_schroedinger_problem(p["n"], 2, K, N, N, p["T"], p["h0"][None], np.stack(p["g"])[None],
                                        p["psi0"], costs=p["descs"], cost_eval_step=1)
        check_yield(engine, p, p["refs"])
    finally:
        engine.set_knob("action_states", 0)


def test_yields_at_n_16(costs1):
    p = acc.build(16, 13)
    acc.set_problem(costs1, p, acc.descriptors(MIXED, p))
    check_yield(costs1, p, acc.references(MIXED, p))


def test_yields_to_host_injected_cotangents(costs1):
    """What a plugin cost without a descriptor becomes: cotangents of the states supplied by the host."""
    from tests.oracle_backend import _InjectedCotangent
    engine = costs1
    p = acc.build(20, 13)
    costs = acc.costs_of(MIXED, p)
    acc.set_problem(engine, p, acc.descriptors(MIXED, p))
    rng = np.random.default_rng(11)
    bars = 1e-2 * (rng.standard_normal((3, 1, 1, 20)) + 1j * rng.standard_normal((3, 1, 1, 20)))
    refs = [sc.evaluate(p, list(costs) + [_InjectedCotangent({6: bars[b, 0]}, True)], b) for b in range(3)]
    engine.upload_controls(p["controls"])
    engine.set_state_cotangents([6], bars)
    try:
        engine.eval_resident(True)
        out = engine.download_results(True)
        assert not executed(engine)
        assert_gates("injected", out, refs)
    finally:
        engine.set_state_cotangents(None, None)
    check_taken(engine, p)


def test_yields_to_kept_step_states(costs1):
    engine = costs1
    p = acc.build(20, 13)
    acc.set_problem(engine, p, acc.descriptors(MIXED, p))
    engine.set_keep_step_states(True)
    try:
        check_yield(engine, p, acc.references(MIXED, p))
    finally:
        engine.set_keep_step_states(False)
    check_taken(engine, p)


def test_yields_to_a_non_hermitian_drift(costs1):
    p = acc.build(20, 13)
    costs = acc.costs_of(MIXED, p)
    skew = p["h0"] + 0.05j * acc.hermitian(np.random.default_rng(3), 20)
    q = variant(p, costs, h0=skew)
    acc.set_problem(costs1, q, acc.descriptors(MIXED, p))
    check_yield(costs1, q, q["refs"])


def test_yields_to_effective_controls(costs1):
    """H quadratic in the controls (qocx_set_quadratic_terms): the quadratic effective controls."""
    engine = costs1
    p = acc.build(20, 13)
    costs = acc.costs_of(MIXED, p)
    quad = 0.5 * acc.hermitian(np.random.default_rng(4), 20)
    q = variant(p, costs, kind="quadratic", quadratic=(np.array([[0, 0]], dtype=np.int32), quad[None]))
    acc.set_problem(engine, q, acc.descriptors(MIXED, p))
    engine.set_quadratic_terms(*q["quadratic"])
    check_yield(engine, q, q["refs"])


def test_yields_to_latency_mode(costs1):
    engine = costs1
    p = acc.build(20, 13)
    acc.set_problem(engine, p, acc.descriptors(MIXED, p))
    engine.set_knob("latency", 1)
    try:
        check_yield(engine, p, acc.references(MIXED, p), one_by_one=True)
    finally:
        engine.set_knob("latency", 0)
    check_taken(engine, p)


def test_yields_to_pade_order_13(costs1):
    engine = costs1
    p = acc.build(20, 13)
    acc.set_problem(engine, p, acc.descriptors(MIXED, p))
    engine.set_knob("pade_order", 13)
    try:
        check_yield(engine, p, acc.references(MIXED, p))
        assert engine.pade_orders()[13] == 3 * (p["N"] - 1)
    finally:
        engine.set_knob("pade_order", 0)
    check_taken(engine, p)


def test_yields_to_a_host_bound_above_theta_18(costs1):
    engine = costs1
    p = acc.build(20, 13)
    costs = acc.costs_of(MIXED, p)
    loud = p["controls"].copy()
    loud[2] = 12.0 + p["controls"][2] / 5  # 11 < u < 13 at every knot and every midpoint
    assert acc.DT * (1 + 2 * 11.0) > 1.09
    q = variant(p, costs, controls=loud)
    acc.set_problem(engine, q, acc.descriptors(MIXED, p))
    check_yield(engine, q, q["refs"])
    check_taken(engine, p)


# ---- 7. a stale host bound -------------------------------------------------------------------------------

def test_stale_host_bound_runs_again_on_the_pade_route():
    """tests/test_gpu_action_states.py, under step costs: the resident SGD step makes every step louder than
    the buffers were sized for, the sweep raises the status bit and the evaluation runs again, once, on the
    Pade route. (An engine of its own: the counter of the module's engine stays 0.)"""
    from qoc_amd.engine import Engine
    engine = Engine(0)
    try:
        engine.set_knob("action_costs", 1)
        p = acc.build(20, 13)
        costs = acc.costs_of(MIXED, p)
        acc.set_problem(engine, p, acc.descriptors(MIXED, p))
        quiet = p["controls"][:1]
        engine.upload_controls(quiet)
        engine.opt_begin()
        engine.eval_resident(True)
        first = engine.download_results(True)
        degrees = executed(engine)
        assert degrees and max(degrees) <= 9, degrees
        assert engine.action_reruns() == 0
        rate = 4.0 / np.abs(first[1]).max()  # the largest control moves by 4: a bound near 0.05 * 5
        flags = np.ones(1, dtype=np.uint8)
        engine.opt_step(0, flags, flags, rate)
        moved = quiet - rate * first[1]
        engine.eval_resident(True)
        out = engine.download_results(True)
        q = variant(p, costs, controls=moved)
        assert_gates("after the step", out, q["refs"])
        assert engine.action_reruns() == 1 and not executed(engine)
    finally:
        engine.close()


# ---- 8. the knob -----------------------------------------------------------------------------------------

def test_knob_refuses_other_values(engine):
    for bad in (2, -1, 3, 64):
        with pytest.raises(Exception):
            engine.set_knob("action_costs", bad)
    p = acc.build(20, 13)  # ... and is still 0
    acc.set_problem(engine, p, acc.descriptors(MIXED, p))
    check_yield(engine, p, acc.references(MIXED, p))


# ---- 9. the public interface ---------------------------------------------------------------------------

def test_keyword_of_the_public_interface(monkeypatch):
    from qoc_amd.core import device
    from qoc_amd.core.schroedingerdiscrete import grape_schroedinger_discrete_batch
    from qoc_amd.standard import ForbidStates, TargetStateInfidelity
    p = acc.build(20, 14)
    h0, g, N = p["h0"], p["g"], p["N"]
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
    costs = [TargetStateInfidelity(p["vec"]["A"][:, :, None]),
             ForbidStates(p["vec"]["F1"][:2].reshape(1, 2, 20, 1), N, CES)]

    def run(value):
        return grape_schroedinger_discrete_batch(
            K, N, costs, p["T"], lambda u, t: h0 + sum(u[j] * g[j] for j in range(K)), p["init"][:, :, None],
            N, initial, cost_eval_step=CES, iteration_count=3, log_iteration_step=0, matrix_free=value)

    try:
        opted = run("costs")
        assert len(made) == 1 and len(degrees[0]) >= 3 and all(degrees[0]), degrees
        default = run("default")
        assert len(made) == 2 and len(degrees[1]) >= 3 and not any(degrees[1]), degrees
        assert np.abs(np.asarray(opted.best_error) - np.asarray(default.best_error)).max() < 1e-10
        with pytest.raises(ValueError, match="matrix_free"):
            run("cost")
    finally:
        for e in made:
            e.close()
