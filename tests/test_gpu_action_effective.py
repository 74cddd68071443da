"""
GPU tests (-m gpu) of the matrix-free route on EFFECTIVE controls (qoc_amd/csrc/qocx_action_eff.hip, knob
"action_eff" = 1): M4 on a time-independent system and Hamiltonians quadratic in the controls, whose step
generator is linear in Ke effective controls over an augmented operator set, on the Taylor sweeps of
qocx_action.hip (17 <= n <= 32), qocx_action16.hip (n <= 16, "action_small" = 1 as well) and qocx_action4.hip
(33 <= n <= 64, "action" = 2 as well). Cases, fixture and model: tests/action_effective.py.

Every case asserts that the route ran - the executed degrees are the model's histogram exactly, nothing ran
again on the Pade route -, parity with the oracle at the project's gates (1e-10 cost and final states, 1e-8
of the largest gradient entry) and agreement with the Pade route of the same problem (knob 0, no degree
executed) at the same gates; the worst differences go to profiles/action_effective_vs_pade.jsonl.
tests/test_action_effective_host.py shows on the CPU that the cases stay on the route, that the histogram
is safe to demand, that a correct implementation reaches the gates and that no plausibly wrong kernel could.
"""

import json
import os

import numpy as np
import pytest

from oracle import qoc_numpy as onp
from tests import action_effective as ae
from tests import action_features as af
from tests import helpers
from tests.helpers import rel_err
from tests.test_gpu_action_wide import assert_gates, executed, same_bits

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = ae.STEPS
DEFAULTS = dict(action_eff=0, action=1, action_small=0, action_states=0, action_costs=0, latency=0,
                pade_order=0, bidir=1)


@pytest.fixture(scope="module")
def engine():
    from qoc_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(autouse=True)
def defaults_afterwards(engine):
    yield
    for name, value in DEFAULTS.items():
        engine.set_knob(name, value)
    engine.set_chunk(0)
    engine.set_pipeline(0)
    helpers.set_backend_factory(None)


_differences = {}


def record(tag, worst, **what):
    _differences[tag] = dict(dict(case=tag, steps=STEPS, max_abs_cost=worst["cost"],
                                  max_abs_final=worst["final"], max_rel_grad=worst["grad"]), **what)
    with open(os.path.join(ROOT, "profiles", "action_effective_vs_pade.jsonl"), "w") as f:
        for key in sorted(_differences):
            f.write(json.dumps(_differences[key]) + "\n")


def set_problem(engine, p, magnus=None, **kw):
    """The engine's problem of a case (its quadratic terms included), with the route's knobs for its size."""
    engine.set_knob("action_eff", 1)
    for name, value in ae.knobs(p["case"]).items():
        engine.set_knob(name, value)
    K = len(p["g"])
    engine.set_schroedinger_problem(p["n"], 1, K, p["Nc"], ae.N, ae.T, p["h0"][None], p["g"][None], p["psi0"],
                                    costs=af.descriptors(p), interpolation=p["interpolation"],
                                    magnus_policy=magnus or ("M4" if p["kind"] == "m4" else "M2"), **kw)
    if p["terms"]:
        engine.set_quadratic_terms(np.array(p["terms"], dtype=np.int32), p["q"])


def on_both_routes(engine, evaluate, histogram):
    """evaluate() on the route - the executed degrees are `histogram`, nothing ran again - and on the Pade
    route (knob 0), where no degree is executed."""
    reruns = engine.action_reruns()
    action = evaluate()
    degrees = executed(engine)
    print("degrees {}".format(dict(sorted(degrees.items()))))
    assert degrees == histogram, (degrees, histogram)
    assert engine.action_reruns() == reruns
    engine.set_knob("action_eff", 0)
    try:
        pade = evaluate()
        assert not executed(engine)
    finally:
        engine.set_knob("action_eff", 1)
    return action, pade


def as_refs(out):
    return [(out[0][b], out[1][b], out[2][b][:, :, None]) for b in range(len(out[0]))]


def model_histogram(p, items=None, scales=None):
    items = p["controls"] if items is None else items
    scales = [None] * len(items) if scales is None else scales
    return ae.histogram([ae.degrees_of(p, u, c) for u, c in zip(items, scales)])


def check_case(engine, case):
    p = ae.build(case)
    tag = ae.case_id(case)
    set_problem(engine, p)
    action, pade = on_both_routes(engine, lambda: engine.evaluate(p["controls"], True), model_histogram(p))
    assert_gates(tag, action, ae.references(p))
    assert_gates(tag + " Pade", pade, ae.references(p))
    worst = assert_gates(tag + " against Pade", action, as_refs(pade))
    record(tag, worst, kind=case[0], n=case[1], K=case[2], Ke=ae.effective_count(case), interpolation=case[3],
           knots=case[4], seeds=3)


# ---- 1 - 5. the cases ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ae.M4_COUNTS, ids=ae.case_id)
def test_m4_control_counts(engine, case):
    """Ke = 2 (the exact two-image build), 5 (all five images in registers) and 9 (seven images streamed)."""
    check_case(engine, case)


@pytest.mark.parametrize("case", ae.M4_KNOTS, ids=ae.case_id)
def test_m4_knots_and_slices(engine, case):
    """The two nodes of a step read different knots or slices, and the scatter carries two cotangents per step."""
    check_case(engine, case)


@pytest.mark.parametrize("case", ae.QUADRATIC, ids=ae.case_id)
def test_quadratic_terms(engine, case):
    check_case(engine, case)


@pytest.mark.parametrize("case", ae.SMALL, ids=ae.case_id)
def test_at_most_16_levels(engine, case):
    """qocx_action16.hip: Ke = 5 is one image in registers, three in LDS and one streamed."""
    check_case(engine, case)


@pytest.mark.parametrize("case", ae.WIDE, ids=ae.case_id)
def test_33_to_64_levels(engine, case):
    check_case(engine, case)


def test_the_streamed_build_of_five_channels_gives_the_same_numbers(engine):
    """Knob "action_eff_exact" = 0: the Ke = 5 problem on action_sweep_kernel<2, 2>, three images read per step."""
    case = ae.M4_COUNTS[1]
    p = ae.build(case)
    set_problem(engine, p)
    exact = engine.evaluate(p["controls"], True)
    engine.set_knob("action_eff_exact", 0)
    try:
        streamed = engine.evaluate(p["controls"], True)
        assert executed(engine) == model_histogram(p)
    finally:
        engine.set_knob("action_eff_exact", 1)
    assert_gates("streamed Ke = 5", streamed, ae.references(p))
    assert_gates("streamed against exact", streamed, as_refs(exact))


# ---- 6. seed tables -----------------------------------------------------------------------------------------

def test_an_ensemble_over_a_quadratic_base_with_term_scales(engine):
    p = ae.ensemble()
    B, M, kr = p["B"], p["M"], p["kr"]
    set_problem(engine, p)
    engine.set_ensemble(p["scales"], p["offsets"], p["weights"])

    def evaluate():
        out = engine.evaluate(p["u"], True)
        return out[0], out[1], out[2][:, :, 0, :], engine.ensemble_member_costs()

    # without term scales a member is bit for bit the plain (K_r + J)-channel problem, on this route too
    bare = evaluate()
    assert sum(executed(engine).values()) == B * M * STEPS
    set_problem(engine, p)
    plain = engine.evaluate(p["items"], True)
    assert sum(executed(engine).values()) == B * M * STEPS
    assert np.array_equal(bare[3].reshape(-1), plain[0])
    assert np.array_equal(bare[2].reshape(B * M, -1), plain[2].reshape(B * M, -1))
    # with them: the oracle on every item, reduced with the weights
    engine.set_ensemble(p["scales"], p["offsets"], p["weights"])
    engine.set_ensemble_quadratic_scales(p["term_scale"])
    action, pade = on_both_routes(engine, evaluate, model_histogram(p, p["items"], p["item_scale"]))
    refs = [ae.reference(p, u, c) for u, c in zip(p["items"], p["item_scale"])]
    seeds, members = [], np.empty((B, M))
    for b in range(B):
        mine = refs[b * M:(b + 1) * M]
        members[b] = [r[0] for r in mine]
        seeds.append((sum(p["weights"][m] * mine[m][0] for m in range(M)),
                      sum(p["weights"][m] * p["scales"][m] * mine[m][1][:, :kr] for m in range(M)),
                      np.concatenate([r[2] for r in mine])))
    assert_gates("ensemble", action, seeds)
    assert np.abs(action[3] - members).max() < 1e-10
    assert np.abs(bare[3] - members).max() > 1e-6  # (the term scales are felt)
    worst = assert_gates("ensemble against Pade", action, as_refs(pade))
    assert np.abs(action[3] - pade[3]).max() < 1e-10
    record("ensemble-quadratic-scales", worst, kind="quad", n=p["n"], K=3, Ke=5, knots=p["Nc"], seeds=B, members=M)


def test_a_duration_sweep_under_m4(engine):
    """Through the evaluator: the channels [G_0, G_1, H0] on [tau u, tau] with a zero drift - the A_k of the
    commutator set are zero operators. Every seed against the oracle at its own duration, against the Pade
    route, and bit for bit the plain three-channel M4 problem on the expanded controls."""
    from qoc_amd.core import device
    from qoc_amd.models import MagnusPolicy
    from qoc_amd.standard import HamiltonianSweep, TargetStateInfidelity
    p = ae.durations()
    x = p["expanded"]
    B = p["B"]
    sweep = HamiltonianSweep.durations(af.hamiltonian(p), p["times"], p["T"])
    ev = device.SchroedingerEvaluator(
        p["T"], sweep, p["psi0"][:, :, None], ae.N, control_count=2, control_eval_count=p["Nc"],
        costs=[TargetStateInfidelity(p["target"][:, :, None])], magnus_policy=MagnusPolicy.M4, backend=engine,
        matrix_free="effective")

    def evaluate():
        errors, grads, finals, _ = ev.evaluate_batch(p["u"])
        return (np.asarray(errors), np.asarray(grads).reshape(p["u"].shape), np.asarray(finals).reshape(B, 1, p["n"]))

    action, pade = on_both_routes(engine, evaluate, model_histogram(x))
    seeds = []
    for b in range(B):
        cost, grads, final = onp.evaluate_with_grad(ae.oracle_problem(p, p["u"][b], evolution_time=p["times"][b]),
                                                    p["u"][b])
        seeds.append((cost, np.real(grads), final))
    assert_gates("durations", action, seeds)
    worst = assert_gates("durations against Pade", action, as_refs(pade))
    record("durations-m4", worst, kind="m4", n=p["n"], K=3, Ke=9, knots=p["Nc"], seeds=B)
    # (the evaluator probes its operators, G_k = H(e_k) - H(0): not the bits of p["g"]. The same sweep set on
    # the engine over p["g"] itself is, seed by seed, the plain problem on the expanded controls.)
    def set_expanded():
        engine.set_schroedinger_problem(x["n"], 1, 3, x["Nc"], ae.N, ae.T, x["h0"][None], x["g"][None], x["psi0"],
                                        costs=af.descriptors(x), magnus_policy="M4")

    tau = p["taus"]
    set_expanded()
    engine.set_sweep(np.repeat(tau[:, None], 2, axis=1), tau[:, None])
    swept = engine.evaluate(p["u"], True)
    assert executed(engine) == model_histogram(x)
    assert_gates("durations, engine against evaluator", swept, as_refs(action))
    set_expanded()
    plain = engine.evaluate(x["controls"], True)
    assert executed(engine) == model_histogram(x)
    assert np.array_equal(plain[0], swept[0]) and np.array_equal(plain[2], swept[2])


# ---- 7. bits ------------------------------------------------------------------------------------------------

def test_bit_identity_across_chunks_segments_and_forward_only(engine):
    p = ae.build(ae.BITS_CASE)
    set_problem(engine, p)
    histogram = model_histogram(p)
    ref = engine.evaluate(p["controls"], True)
    assert executed(engine) == histogram

    def same(tag):
        out = engine.evaluate(p["controls"], True)
        assert executed(engine) == histogram, tag
        same_bits(ref, out, tag)

    for chunk in (1, 2):
        engine.set_chunk(chunk)
        same("chunk %d" % chunk)
    engine.set_chunk(0)
    for segments in (1, 3, 4):
        engine.set_pipeline(segments)
        same("segments %d" % segments)
    engine.set_pipeline(0)
    forward = engine.evaluate(p["controls"], False)
    assert executed(engine) == histogram
    assert np.array_equal(forward[0], ref[0]) and np.array_equal(forward[2], ref[2])


# ---- 8. the resident optimiser ------------------------------------------------------------------------------

def test_the_resident_optimiser_stays_on_the_route_after_a_clip_that_binds(engine):
    p = ae.build(ae.OPTIMISER_CASE)
    set_problem(engine, p)
    max_norms = np.full(2, 1.0)
    assert np.abs(p["controls"]).max() > 1.0
    reruns = engine.action_reruns()
    engine.upload_controls(p["controls"])
    engine.opt_begin()
    ones, zeros = np.ones(3, dtype=np.uint8), np.zeros(3, dtype=np.uint8)
    a = af.ADAM
    route = []
    for it in range(2):
        engine.opt_clip(max_norms)
        engine.eval_resident(True)
        route.append((sum(executed(engine).values()), engine.action_reruns() - reruns))
        if it == 0:
            engine.opt_step(1, ones, ones, a["learning_rate"], a["beta_1"], a["beta_2"], a["epsilon"],
                            1 - a["beta_1"], 1 - a["beta_2"])
    resident = engine.download_results(True)
    engine.opt_step(1, ones, zeros, a["learning_rate"], a["beta_1"], a["beta_2"], a["epsilon"],
                    1 - a["beta_1"] ** 2, 1 - a["beta_2"] ** 2)  # (nothing moves: the best controls are these)
    controls, _ = engine.opt_download_best()
    print("(degrees, reruns) per evaluation {}".format(route))
    assert route == [(3 * STEPS, 0)] * 2, route
    assert np.abs(controls).max() <= 1.0 + 1e-12 and np.abs(controls - np.clip(p["controls"], -1, 1)).max() > 1e-3
    again = engine.evaluate(controls, True)
    assert sum(executed(engine).values()) == 3 * STEPS
    assert_gates("resident against evaluate", resident, as_refs(again))
    assert_gates("resident against the oracle", resident, [ae.reference(p, u) for u in controls])


# ---- 9. the route yields ------------------------------------------------------------------------------------

def check_yield(engine, evaluate):
    """With "action_eff" = 1: no degree, and the knob-0 results bit for bit."""
    engine.set_knob("action_eff", 1)
    out = evaluate()
    assert not executed(engine)
    engine.set_knob("action_eff", 0)
    off = evaluate()
    assert not executed(engine)
    same_bits(out, off)
    engine.set_knob("action_eff", 1)


def test_yields_to_m6(engine):
    p = ae.build(ae.OPTIMISER_CASE)
    set_problem(engine, p, magnus="M6")
    check_yield(engine, lambda: engine.evaluate(p["controls"], True))


def test_yields_to_m4_on_a_time_dependent_system(engine):
    p = ae.build(ae.OPTIMISER_CASE)
    engine.set_knob("action_eff", 1)
    wobble = 1 + 0.01 * np.arange(2 * STEPS)
    engine.set_schroedinger_problem(p["n"], 1, 2, p["Nc"], ae.N, ae.T, wobble[:, None, None] * p["h0"][None],
                                    np.broadcast_to(p["g"][None], (2 * STEPS,) + p["g"].shape).copy(), p["psi0"],
                                    costs=af.descriptors(p), magnus_policy="M4")
    check_yield(engine, lambda: engine.evaluate(p["controls"], True))


def test_yields_to_a_non_hermitian_term(engine):
    p = ae.build(ae.QUADRATIC[2])
    set_problem(engine, p)
    engine.evaluate(p["controls"], True)
    assert executed(engine)
    engine.set_quadratic_terms(np.array(p["terms"], dtype=np.int32), p["q"] + 0.05j * p["q"])
    check_yield(engine, lambda: engine.evaluate(p["controls"], True))


def test_yields_to_two_states(engine):
    p = ae.build(ae.OPTIMISER_CASE)
    engine.set_knob("action_eff", 1)
    engine.set_knob("action_states", 4)
    psi0 = np.eye(p["n"], dtype=np.complex128)[:2]
    target = np.stack([p["target"][0], np.roll(p["target"][0], 1)])
    engine.set_schroedinger_problem(p["n"], 2, 2, p["Nc"], ae.N, ae.T, p["h0"][None], p["g"][None], psi0,
                                    costs=[dict(kind=0, step_cost=0, scale=1.0, vectors=target)], magnus_policy="M4")
    check_yield(engine, lambda: engine.evaluate(p["controls"], True))


def test_yields_to_a_step_cost(engine):
    p = ae.build(ae.OPTIMISER_CASE)
    engine.set_knob("action_eff", 1)
    engine.set_knob("action_costs", 1)
    costs = af.descriptors(p) + [dict(kind=1, step_cost=1, scale=1.3 / STEPS, vectors=p["target"])]
    engine.set_schroedinger_problem(p["n"], 1, 2, p["Nc"], ae.N, ae.T, p["h0"][None], p["g"][None], p["psi0"],
                                    costs=costs, magnus_policy="M4")
    check_yield(engine, lambda: engine.evaluate(p["controls"], True))


@pytest.mark.parametrize("knob, value", [("latency", 1), ("pade_order", 13)])
def test_yields_to_a_knob(engine, knob, value):
    p = ae.build(ae.OPTIMISER_CASE)
    set_problem(engine, p)
    engine.evaluate(p["controls"], True)
    assert executed(engine)
    engine.set_knob(knob, value)
    check_yield(engine, lambda: engine.evaluate(p["controls"], True))
    engine.set_knob(knob, 0)
    engine.evaluate(p["controls"], True)
    assert sum(executed(engine).values()) == 3 * STEPS


@pytest.mark.parametrize("case", [ae.OPTIMISER_CASE, ae.QUADRATIC[0]], ids=ae.case_id)
def test_yields_to_a_host_bound_above_theta_18(engine, case):
    p = ae.build(case)
    set_problem(engine, p)
    loud = p["controls"].copy()
    loud[2] = 12.0 + p["controls"][2] / 5
    assert ae.host_bound(p, loud) > ae.THETA_18
    check_yield(engine, lambda: engine.evaluate(loud, True))
    engine.evaluate(p["controls"], True)
    assert sum(executed(engine).values()) == 3 * STEPS


@pytest.mark.parametrize("case", [ae.OPTIMISER_CASE, ae.QUADRATIC[0]], ids=ae.case_id)
def test_the_knob_at_0_executes_no_degree(case):
    """A context whose knobs were never set; then the knob, which the parent commit does not know."""
    from qoc_amd.engine import Engine
    p = ae.build(case)
    fresh = Engine(0)
    try:
        K = len(p["g"])
        fresh.set_schroedinger_problem(p["n"], 1, K, p["Nc"], ae.N, ae.T, p["h0"][None], p["g"][None], p["psi0"],
                                       costs=af.descriptors(p), interpolation=p["interpolation"],
                                       magnus_policy="M4" if p["kind"] == "m4" else "M2")
        if p["terms"]:
            fresh.set_quadratic_terms(np.array(p["terms"], dtype=np.int32), p["q"])
        untouched = fresh.evaluate(p["controls"], True)
        assert not executed(fresh)
        fresh.set_knob("action_eff", 0)
        off = fresh.evaluate(p["controls"], True)
        assert not executed(fresh)
        same_bits(untouched, off)
        assert_gates("knob 0", off, ae.references(p))
        fresh.set_knob("action_eff", 1)
        fresh.evaluate(p["controls"], True)
        assert sum(executed(fresh).values()) == 3 * STEPS
        for bad in (-1, 2):
            with pytest.raises(Exception, match="action_eff"):
                fresh.set_knob("action_eff", bad)
    finally:
        fresh.close()


# ---- 10. Python ---------------------------------------------------------------------------------------------

def python_problem(case):
    from qoc_amd.models import MagnusPolicy
    from qoc_amd.standard import QuadraticHamiltonian
    p = ae.build(case)
    linear = af.hamiltonian(p)
    if p["kind"] == "m4":
        return p, linear, MagnusPolicy.M4
    return p, QuadraticHamiltonian(linear, [(k, l, p["q"][i]) for i, (k, l) in enumerate(p["terms"])]), MagnusPolicy.M2


@pytest.mark.parametrize("case", ae.PYTHON_CASES, ids=ae.case_id)
def test_keyword_of_the_evaluator(engine, case):
    from qoc_amd.core import device
    from qoc_amd.standard import TargetStateInfidelity
    p, system, magnus = python_problem(case)

    def build(**kw):
        return device.SchroedingerEvaluator(
            ae.T, system, p["psi0"][:, :, None], ae.N, control_count=p["K"], control_eval_count=p["Nc"],
            costs=[TargetStateInfidelity(p["target"][:, :, None])], magnus_policy=magnus, backend=engine, **kw)

    default = build(matrix_free="default").evaluate_batch(p["controls"])
    assert not executed(engine)
    effective = build(matrix_free="effective").evaluate_batch(p["controls"])
    assert executed(engine) == model_histogram(p)
    for b, (rc, rg, rf) in enumerate(ae.references(p)):
        assert abs(effective[0][b] - rc) < 1e-10 and abs(effective[0][b] - default[0][b]) < 1e-10
        assert rel_err(np.asarray(effective[1][b]).reshape(rg.shape), rg) < 1e-8
        assert rel_err(np.asarray(effective[1][b]), np.asarray(default[1][b])) < 1e-8
        assert np.abs(np.asarray(effective[2][b]) - np.asarray(default[2][b])).max() < 1e-10
    with pytest.raises(ValueError, match="\"effective\""):
        build(matrix_free="augmented")


@pytest.mark.parametrize("case", ae.PYTHON_CASES, ids=ae.case_id)
def test_three_adam_iterations_of_129_seeds_end_at_the_same_errors(engine, case):
    """129 seeds: one more than latency mode, which the route yields to, takes."""
    import qoc_amd
    from qoc_amd.standard import Adam, TargetStateInfidelity
    p, system, magnus = python_problem(case)
    B, K, Nc = 129, p["K"], p["Nc"]
    rng = np.random.default_rng(129)
    loud = 1.0  # (the clip's bound; DT (1 + 2 + 2) = 0.25 with the terms)
    start = rng.uniform(-1, 1, (B, Nc, K)) * np.resize([1e-3, 0.5, loud], B)[:, None, None]
    helpers.set_backend_factory(lambda: engine)
    route, evaluate = [], engine.eval_resident

    def recording(want_grad=True):
        evaluate(want_grad)
        route.append(sum(executed(engine).values()))

    def run(keyword):
        engine.eval_resident = recording
        try:
            return qoc_amd.grape_schroedinger_discrete_batch(
                K, Nc, [TargetStateInfidelity(p["target"][:, :, None])], ae.T, system, p["psi0"][:, :, None], ae.N,
                start, iteration_count=3, log_iteration_step=0, optimizer=Adam(), magnus_policy=magnus,
                max_control_norms=np.full(K, loud), matrix_free=keyword)
        finally:
            del engine.eval_resident

    effective = run("effective")
    assert route and all(r == B * STEPS for r in route), route
    del route[:]
    engine.set_knob("action_eff", 0)
    default = run("default")
    assert route and not any(route), route
    worst = np.abs(np.asarray(effective.best_error) - np.asarray(default.best_error)).max()
    print("best errors, effective against default: {:.2e}".format(worst))
    assert worst < 1e-9
