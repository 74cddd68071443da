"""
GPU tests (-m gpu) of the matrix-free route away from K = 2, Nc = N, linear interpolation and a plain
batch (qoc_amd/csrc/qocx_action.hip, qocx_action4.hip, qocx_action16.hip, qocx_action_states.hip,
qocx_action_costs.hip, the step table and the scatter they share with the Pade route), on the problems of
tests/action_features.py:

  * K = 1 (the k < K guard of the register images) and K = 3, 5 (the images streamed per step);
  * Nc = 2, 5, 27 linear and Nc = 3, 13 piecewise constant (control_at and the scatter's CSR weights), on
    the unit adjoint at one and at three states and on the one-real layout of the costs kernels;
  * an ensemble, a sweep and a duration sweep (K_r + J channels, no spectral bound on the host, H0 as a
    channel), bit-identical across chunks that split a seed's members, segments and schedules;
  * the resident optimiser after a clip that binds: real and complex controls, a ControlBasis, a
    control cost;
  * the Python multi-start above the latency threshold, plain and as a duration search;
  * the n <= 16 kernel (knob "action_small" = 1, tag "small") on all of the above at its own sizes and its
    own control counts - K = 1, 2, 4 (register and LDS images), 6 and 9 (images streamed per step), the step
    table launched for the sweeps alone - and under one final incoherent target of scale 0.7.

Every test asserts that the route ran (the degree counts sum to items x steps, no rerun unless said),
parity with the oracle at the project's gates (1e-10 cost and final states, 1e-8 of the largest gradient
entry) and agreement with the Pade route (knob "action" = 0 - at n <= 16, where that knob does not reach,
"action_small" = 0 -, no degree executed) at the same gates.
tests/test_action_features_host.py shows on the CPU that the cases stay on the route, that a correct
Taylor implementation reaches the gates and that no plausibly wrong kernel could.
"""

import json
import os

import numpy as np
import pytest

from tests import action_features as af
from tests import helpers
from tests.helpers import rel_err
from tests.test_gpu_action import ROOT, assert_gates, executed

pytestmark = pytest.mark.gpu

STEPS = af.N - 1
KNOBS = dict(one={}, states=dict(action_states=4), costs=dict(action_costs=1), wide=dict(action=2),
             small=dict(action_small=1))
DEFAULTS = dict(action=1, action_states=0, action_costs=0, action_small=0, bidir=1)


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
    with open(os.path.join(ROOT, "profiles", "action_features_vs_pade.jsonl"), "w") as f:
        for key in sorted(_differences):
            f.write(json.dumps(_differences[key]) + "\n")


def set_problem(engine, p):
    for name, value in KNOBS[p["kernel"]].items():
        engine.set_knob(name, value)
    engine.set_schroedinger_problem(p["n"], p["S"], len(p["g"]), p["Nc"], af.N, p["T"], p["h0"][None],
                                    p["g"][None], p["psi0"], costs=af.descriptors(p), cost_eval_step=p["ces"],
                                    interpolation=p["interpolation"])


def route_knob(p):
    """(the knob that sends the problem of this kernel to the Pade route at 0, the value that brings it back):
    "action" does not reach n <= 16."""
    if p["kernel"] == "small":
        return "action_small", 1
    return "action", KNOBS[p["kernel"]].get("action", 1)


def on_both_routes(engine, p, evaluate, items):
    """evaluate() on the route - its degrees cover items x steps, nothing ran again - and on the Pade
    route, where no degree is executed."""
    reruns = engine.action_reruns()
    action = evaluate()
    degrees = executed(engine)
    print("degrees {}".format(degrees))
    assert sum(degrees.values()) == items * STEPS, degrees
    assert engine.action_reruns() == reruns
    knob, back = route_knob(p)
    engine.set_knob(knob, 0)
    try:
        pade = evaluate()
        assert not executed(engine)
    finally:
        engine.set_knob(knob, back)
    return action, pade


def as_refs(out):
    return [(out[0][b], out[1][b], out[2][b][:, :, None]) for b in range(len(out[0]))]


def check_case(engine, case):
    p = af.build(*case)
    tag = "{}-n{}-K{}-S{}-{}-Nc{}".format(*case)
    set_problem(engine, p)
    action, pade = on_both_routes(engine, p, lambda: engine.evaluate(p["controls"], True), 3)
    assert_gates(tag, action, af.references(p))
    worst = assert_gates(tag + " against Pade", action, as_refs(pade))
    record(tag, worst, kernel=case[0], n=case[1], K=case[2], states=case[3], interpolation=case[4],
           knots=case[5], seeds=3)


# ---- 1. the control count -------------------------------------------------------------------------------

@pytest.mark.parametrize("case", af.CONTROL_COUNTS, ids=lambda c: "{}-n{}-K{}-S{}".format(*c))
def test_control_counts(engine, case):
    """K = 1: one image in registers and the guard that keeps a second one out; K = 3 and 5: the images
    of the controls k >= 2 are read per step. The small kernel: K = 1 registers alone, K = 2 and 4 one and
    three images in LDS, K = 6 and 9 two and five images read per step."""
    check_case(engine, case + (af.LINEAR, af.N))


# ---- 2. the interpolation ---------------------------------------------------------------------------------

def knots_id(c):  # (K is named where it is not 3)
    return "{}-n{}-S{}-{}-Nc{}".format(*(c[:2] + c[3:])) + ("" if c[2] == 3 else "-K%d" % c[2])


@pytest.mark.parametrize("case", af.INTERPOLATIONS, ids=knots_id)
def test_knots_and_slices(engine, case):
    """control_at feeds the step's controls and its degree, the scatter's weights carry the step
    cotangents back: under the unit adjoint's scalar at one and three states, and in the one-real layout
    of the costs kernels."""
    check_case(engine, case)


# ---- 3. seed tables -----------------------------------------------------------------------------------

def ensemble_references(p):
    refs = af.item_reference(p, p["items"])
    M, kr = p["M"], p["kr"]
    seeds, members = [], np.empty((p["B"], M))
    for b in range(p["B"]):
        mine = refs[b * M:(b + 1) * M]
        members[b] = [r[0] for r in mine]
        seeds.append((sum(p["weights"][m] * mine[m][0] for m in range(M)),
                      sum(p["weights"][m] * p["scales"][m] * mine[m][1][:, :kr] for m in range(M)),
                      np.concatenate([r[2] for r in mine])))
    return seeds, members


def evaluate_ensemble(engine, p):
    out = engine.evaluate(p["u"], True)
    return out[0], out[1], out[2][:, :, 0, :], engine.ensemble_member_costs()


def table(name):
    """The seed table of a parameter: "ensemble", "sweep", "small-ensemble", "small-sweep",
    "small-ensemble-streamed"."""
    if name == "small-ensemble-streamed":
        return af.ensemble_streamed()
    kernel, what = ("small", name[len("small-"):]) if name.startswith("small-") else ("one", name)
    return getattr(af, what)(kernel)


@pytest.mark.parametrize("name", ["one", "small", "small-streamed"])
def test_an_ensemble_against_the_oracle(engine, name):
    """"small-streamed": K_r + J = 6 at n = 16 - the two perturbations are the images read per step."""
    p = af.ensemble_streamed() if name == "small-streamed" else af.ensemble(name)
    tag = "ensemble" if name == "one" else name.replace("small", "small-ensemble")
    set_problem(engine, p)
    engine.set_ensemble(p["scales"], p["offsets"], p["weights"])
    action, pade = on_both_routes(engine, p, lambda: evaluate_ensemble(engine, p), p["B"] * p["M"])
    seeds, members = ensemble_references(p)
    assert_gates(tag, action, seeds)
    assert np.abs(action[3] - members).max() < 1e-10
    worst = assert_gates(tag + " against Pade", action, as_refs(pade))
    assert np.abs(action[3] - pade[3]).max() < 1e-10
    record(tag, worst, n=p["n"], K=len(p["g"]), knots=p["Nc"], seeds=p["B"], members=p["M"])


def sweep_references(p):
    refs = af.item_reference(p, p["items"])
    kr = p["kr"]
    seeds = [(r[0], p["scales"][b] * r[1][:, :kr], r[2]) for b, r in enumerate(refs)]
    scale_sens = np.array([np.sum(p["u"][b] * r[1][:, :kr], axis=0) for b, r in enumerate(refs)])
    offset_sens = np.array([np.sum(r[1][:, kr:], axis=0) for r in refs])
    return seeds, scale_sens, offset_sens


def evaluate_sweep(engine, p):
    return engine.evaluate(p["u"], True) + engine.sweep_sensitivities()


@pytest.mark.parametrize("kernel", ["one", "small"])
def test_a_sweep_against_the_oracle(engine, kernel):
    p = af.sweep(kernel)
    tag = "sweep" if kernel == "one" else kernel + "-sweep"
    set_problem(engine, p)
    engine.set_sweep(p["scales"], p["offsets"])
    action, pade = on_both_routes(engine, p, lambda: evaluate_sweep(engine, p), p["B"])
    seeds, scale_sens, offset_sens = sweep_references(p)
    assert_gates(tag, action, seeds)
    worst = assert_gates(tag + " against Pade", action, as_refs(pade))
    sens = dict(scale=max(rel_err(action[3], scale_sens), rel_err(action[3], pade[3])),
                offset=max(rel_err(action[4], offset_sens), rel_err(action[4], pade[4])))
    print("sweep sensitivities {}".format(sens))
    assert sens["scale"] < 1e-8 and sens["offset"] < 1e-8, sens
    record(tag, worst, n=p["n"], K=4, knots=p["Nc"], seeds=p["B"], max_rel_scale_sens=sens["scale"],
           max_rel_offset_sens=sens["offset"])


@pytest.mark.parametrize("kernel", ["one", "small"])
def test_a_duration_sweep_against_the_oracle_at_every_duration(engine, kernel):
    from qoc_amd.core import device
    from qoc_amd.standard import HamiltonianSweep, TargetStateInfidelity
    p = af.durations(kernel)
    tag = "durations" if kernel == "one" else kernel + "-durations"
    keyword = dict(matrix_free="small") if kernel == "small" else {}  # (the evaluator sets the knob)
    h = af.hamiltonian(p)
    w = HamiltonianSweep.durations(h, p["times"], p["T"])
    ev = device.SchroedingerEvaluator(
        p["T"], w, p["psi0"][:, :, None], af.N, control_count=2, control_eval_count=p["Nc"],
        costs=[TargetStateInfidelity(p["target"][:, :, None])], backend=engine, **keyword)

    def evaluate():
        errors, grads, finals, _ = ev.evaluate_batch(p["u"])
        return (np.asarray(errors), np.asarray(grads).reshape(p["u"].shape),
                np.asarray(finals).reshape(p["B"], 1, p["n"]), ev.sweep_sensitivities())

    action, pade = on_both_routes(engine, p, evaluate, p["B"])
    # every seed is the plain problem at its own duration
    seeds = []
    for b in range(p["B"]):
        cost, grads, final = af.onp.evaluate_with_grad(af.oracle_problem(p, p["Nc"], p["times"][b]), p["u"][b])
        seeds.append((cost, np.real(grads), final))
    assert_gates(tag, action, seeds)
    worst = assert_gates(tag + " against Pade", action, as_refs(pade))
    # dE / dT by the expanded problem: channels [G_0, G_1, H0] on [tau u, tau] over the reference time
    refs = af.item_reference(p["expanded"], p["items"])
    worst_t = 0.0
    for b, r in enumerate(refs):
        want_s = np.sum(p["u"][b] * r[1][:, :2], axis=0)
        want_t = (np.sum(want_s) + np.sum(r[1][:, 2])) / p["T"]
        scale = max(abs(want_t), np.max(np.abs(want_s)) / p["T"])
        for out in (action, pade):
            worst_t = max(worst_t, abs(out[3]["evolution_time_gradients"][b] - want_t) / scale)
    print("durations dE/dT {:.2e}".format(worst_t))
    assert worst_t < 1e-8
    record(tag, worst, n=p["n"], K=3, knots=p["Nc"], seeds=p["B"], max_rel_time_gradient=worst_t)


@pytest.mark.parametrize("name", ["ensemble", "sweep", "small-ensemble", "small-sweep", "small-ensemble-streamed"])
def test_seed_tables_are_bit_identical_across_chunks_segments_and_schedules(engine, name):
    """A chunk of one or two items splits the three members of a seed; the carry buffers are sized per
    chunk."""
    p = table(name)
    set_problem(engine, p)
    if "ensemble" in name:
        engine.set_ensemble(p["scales"], p["offsets"], p["weights"])
        evaluate, items = (lambda: evaluate_ensemble(engine, p)), p["B"] * p["M"]
    else:
        engine.set_sweep(p["scales"], p["offsets"])
        evaluate, items = (lambda: evaluate_sweep(engine, p)), p["B"]
    reruns = engine.action_reruns()
    ref = evaluate()
    assert sum(executed(engine).values()) == items * STEPS

    def same(tag):
        out = evaluate()
        assert sum(executed(engine).values()) == items * STEPS, tag
        for x, y in zip(ref, out):
            assert np.array_equal(x, y), tag

    for chunk in (1, 2):
        engine.set_chunk(chunk)
        same("chunk %d" % chunk)
    engine.set_chunk(0)
    for segments in (1, 3):
        engine.set_pipeline(segments)
        for bidir in (0, 1):
            engine.set_knob("bidir", bidir)
            same("segments %d, bidir %d" % (segments, bidir))
    engine.set_chunk(1)
    same("chunk 1, segments 3")
    assert engine.action_reruns() == reruns


# ---- 4. the resident optimiser ----------------------------------------------------------------------

def drive(engine, p, steps=3):
    """opt_begin, then `steps` times clip - evaluate - Adam step, then clip - evaluate once more. Returns
    (the costs of every evaluation, (degree count, reruns) of every evaluation, the last evaluation's
    results, the controls it evaluated)."""
    from qoc_amd.engine import CONTROL_VARIATION, PATH_SCHROEDINGER
    variant = p["variant"]
    if variant == "control_cost":
        count = p["K"] * (p["Nc"] - 1) * 2
        engine.set_control_costs(PATH_SCHROEDINGER, False, [dict(
            kind=CONTROL_VARIATION, order=1, multiplier=af.VARIATION_MULTIPLIER / count)])
    engine.upload_controls(p["controls"])
    if variant == "complex":
        engine.opt_begin_complex()
    elif variant == "basis":
        engine.opt_begin_basis(False, p["matrix"], p["coefficients"])
    else:
        engine.opt_begin()
    B = len(p["controls"])
    costs, route, best = [], [], np.full(B, np.inf)
    ones, zeros = np.ones(B, dtype=np.uint8), np.zeros(B, dtype=np.uint8)
    a = af.ADAM
    try:
        for it in range(steps + 1):
            engine.opt_clip(p["max_norms"])
            engine.eval_resident(True)
            route.append((sum(executed(engine).values()), engine.action_reruns()))
            cost = engine.download_costs()
            costs.append(cost)
            if it == steps:  # the best controls are those of this evaluation; nothing moves
                out = engine.download_results(True)
                engine.opt_step(1, ones, zeros, a["learning_rate"], a["beta_1"], a["beta_2"], a["epsilon"],
                                1 - a["beta_1"] ** (it + 1), 1 - a["beta_2"] ** (it + 1))
            else:
                improved = cost < best
                best = np.where(improved, cost, best)
                engine.opt_step(1, improved.astype(np.uint8), ones, a["learning_rate"], a["beta_1"],
                                a["beta_2"], a["epsilon"], 1 - a["beta_1"] ** (it + 1),
                                1 - a["beta_2"] ** (it + 1))
        controls, _ = engine.opt_download_best()
    finally:
        if variant == "control_cost":
            engine.set_control_costs(PATH_SCHROEDINGER, False, [])
    return costs, route, out, controls


STARTS = [(v, "one") for v in af.OPTIMISER_STARTS] + [(v, "small") for v in af.OPTIMISER_STARTS]


@pytest.mark.parametrize("variant, kernel", STARTS, ids=[v if k == "one" else k + "-" + v for v, k in STARTS])
def test_the_resident_optimiser_stays_on_the_route_after_a_clip_that_binds(engine, variant, kernel):
    p = af.optimiser_start(variant, kernel)
    tag = variant if kernel == "one" else kernel + "-" + variant
    set_problem(engine, p)
    reruns = engine.action_reruns()
    costs, route, out, controls = drive(engine, p)
    print("{}: (degrees, reruns) per evaluation {}".format(tag, route))
    assert all(r == (3 * STEPS, reruns) for r in route), route
    engine.set_knob(route_knob(p)[0], 0)
    pade_costs, pade_route, pade_out, pade_controls = drive(engine, p)
    assert all(r == (0, reruns) for r in pade_route), pade_route
    steps = max(np.abs(c - d).max() for c, d in zip(costs, pade_costs))
    print("{}: costs against Pade after every step {:.2e}".format(tag, steps))
    assert steps < 1e-10
    # the clip bound, and the point the optimiser reached is the oracle's
    if variant == "complex":
        start = np.hypot(p["controls"][..., 0], p["controls"][..., 1]).max()
        reached = np.hypot(controls[..., 0], controls[..., 1]).max()
    else:
        start, reached = np.abs(p["controls"]).max(), np.abs(controls).max()
    assert start > p["max_norms"].max() and reached <= p["max_norms"].max() * (1 + 1e-12), (start, reached)
    assert np.abs(controls - p["controls"]).max() > 1e-3  # (it has moved)
    assert_gates("optimiser " + tag, out, [af.optimiser_reference(p, u) for u in controls])
    worst = assert_gates("optimiser %s against Pade" % tag, out, as_refs(pade_out))
    record(("small-optimiser-" if kernel == "small" else "optimiser-") + variant, worst, n=p["n"],
           K=len(p["g"]), knots=p["Nc"], seeds=3, max_abs_cost_after_a_step=steps)


# ---- 5. the Python multi-start above the latency threshold ------------------------------------------

@pytest.mark.parametrize("kernel, search", [("one", False), ("one", True), ("small", False), ("small", True)],
                         ids=["plain", "duration_search", "small-plain", "small-duration_search"])
def test_multistart_of_129_seeds_runs_on_the_route(engine, kernel, search):
    """129 seeds: one more than latency mode takes. A duration search moves tau on the device: the
    host's mirror of the tables goes stale, and an evaluation may run again on the Pade route - counted
    and printed, not a failure. The small kernel (n = 13) is asked for by the driver's keyword,
    matrix_free="small": below 129 items the driver turns latency mode on, which the route yields to."""
    import qoc_amd
    from qoc_amd.standard import Adam, HamiltonianSweep, TargetStateInfidelity
    B, Nc, K, weight = 129, 5, 2, 0.2
    p = af.build(kernel, 17 if kernel == "one" else 13, K, 1, af.LINEAR, Nc)
    keyword = dict(matrix_free="small") if kernel == "small" else {}
    rng = np.random.default_rng(129)
    start = rng.uniform(-1, 1, (B, Nc, K)) * np.resize(af.amplitudes(K), B)[:, None, None]
    h = af.hamiltonian(p)
    times = p["T"] * np.resize([0.6, 0.8, 1.0], B)
    bounds = (0.5 * p["T"], 1.05 * p["T"])
    # the loudest seed at the longest duration of the box stays on the route
    assert 1.05 * af.host_bound(p, start) <= 0.9 * 1.09
    system = HamiltonianSweep.durations(h, times, p["T"], time_bounds=bounds, time_weight=weight) if search else h
    helpers.set_backend_factory(lambda: engine)
    reruns = engine.action_reruns()
    route, evaluate = [], engine.eval_resident

    def recording(want_grad=True):  # (degree count, reruns so far) of every evaluation of the run
        evaluate(want_grad)
        route.append((sum(executed(engine).values()), engine.action_reruns() - reruns))

    engine.eval_resident = recording
    try:
        result = qoc_amd.grape_schroedinger_discrete_batch(
            K, Nc, [TargetStateInfidelity(p["target"][:, :, None])], p["T"], system, p["psi0"][:, :, None], af.N,
            start, iteration_count=3, log_iteration_step=0, optimizer=Adam(),
            max_control_norms=np.full(K, af.AMPLITUDES[-1]),  # (the clip's bound: DT (1 + 2 * 5) = 0.55)
            **keyword)
    finally:
        del engine.eval_resident
    print("multi-start{}{}: (degrees, reruns) per evaluation {}".format(
        " small" if kernel == "small" else "", " duration search" if search else "", route))
    if search:  # (three iterations and the sensitivities at the best points, after the loop)
        assert len(route) >= 4 and all(r[0] in (0, B * STEPS) for r in route), route
        assert route[-1][0] == B * STEPS or route[-1][1] > route[-2][1], route
    else:
        assert route == [(B * STEPS, 0)] * 3, route
    worst = 0.0
    for b in range(B):
        T_b = result.best_evolution_times[b] if search else p["T"]
        cost, _ = af.onp.evaluate(af.oracle_problem(p, Nc, T_b), np.asarray(result.best_controls[b]))
        if search:
            cost += weight * T_b / p["T"]
        worst = max(worst, abs(result.best_error[b] - cost))
    print("multi-start: best_error against the oracle {:.2e}".format(worst))
    assert worst < 1e-10


# ---- 6. one final incoherent target on the small route ---------------------------------------------------

@pytest.mark.parametrize("kernel, n", af.INCOHERENT_TARGETS)
def test_the_incoherent_one_state_target_on_the_small_route(engine, kernel, n):
    """unit_ok admits one final INCOHERENT target at S = 1: the incoherent branches of unit_adjoint_scales<1>
    and eval_costs<1> with this kernel's lane arguments, at a scale that is not 1. Then knob "unit_adjoint" =
    0: the route yields - no degree, the oracle's numbers, the Pade route's bit for bit - and comes back."""
    p = af.incoherent(kernel, n)
    tag = "{}-incoherent-n{}".format(kernel, n)
    set_problem(engine, p)
    action, pade = on_both_routes(engine, p, lambda: engine.evaluate(p["controls"], True), 3)
    assert_gates(tag, action, af.references(p))
    worst = assert_gates(tag + " against Pade", action, as_refs(pade))
    record(tag, worst, kernel=kernel, n=n, K=3, states=1, interpolation=af.LINEAR, knots=5, seeds=3,
           target="incoherent", scale=af.INCOHERENT_SCALE)
    knob, back = route_knob(p)
    engine.set_knob("unit_adjoint", 0)
    try:
        out = engine.evaluate(p["controls"], True)
        assert not executed(engine)
        assert_gates(tag + " unit_adjoint 0", out, af.references(p))
        engine.set_knob(knob, 0)
        try:
            off = engine.evaluate(p["controls"], True)
        finally:
            engine.set_knob(knob, back)
        for x, y in zip(out, off):
            assert np.array_equal(x, y)
    finally:
        engine.set_knob("unit_adjoint", 1)
    engine.evaluate(p["controls"], True)
    assert sum(executed(engine).values()) == 3 * STEPS
