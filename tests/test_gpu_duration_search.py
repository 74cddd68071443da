"""
GPU tests (-m gpu) of the duration search of a sweep (HamiltonianSweep.durations(time_bounds=...) ->
qocx_sweep_set_durations, qocx_duration.hip): the tables derived on the device are bit for bit the
host's tau * base tables, the gradient with respect to tau is the chain rule in its stated order,
errors and dE/dT agree with the oracle, and the resident route walks the host loop's trajectory bit
for bit with tau as one more parameter of every seed.
"""

import numpy as np
import pytest

import qoc_amd
import qoc_amd.standard.costs as product_costs
from oracle import qoc_numpy as onp
from qoc_amd import engine as engine_mod
from qoc_amd.core import device
from qoc_amd.standard import ControlBasis, ControlVariation, HamiltonianSweep
from tests import cases as cases_mod
from tests import helpers
from tests.helpers import rel_err
from tests.test_gpu_sweep import (OPTIMIZERS, engine_problem, make_engine, real_engine,  # noqa: F401
                                  route_problem, routes)

pytestmark = pytest.mark.gpu

ERR_STATE = -3  # QOCX_ERR_STATE (include/qocx.h)


def clip(tau, lo, hi):
    return np.minimum(np.maximum(tau, lo), hi)


def chain_rule(s0, d0, scale_sens, offset_sens, weight):
    """The order of duration_gradient_kernel (qocx_duration.hip), all seeds at once."""
    g = np.zeros(s0.shape[0])
    for k in range(s0.shape[1]):
        g = g + s0[:, k] * scale_sens[:, k]
    for j in range(d0.shape[1]):
        g = g + d0[:, j] * offset_sens[:, j]
    return g + weight


# ---- 1. the tables and the gradient, bit for bit -----------------------------------------------------

TABLE_CASES = {
    "one_seed": dict(n=3, B=1),
    "320_entries_cross_a_block": dict(n=3, B=40, kr=7, J=1, Nc=5, N=9),
    "three_fixed_channels": dict(n=3, kr=2, J=3),
    "complex_pairs": dict(n=16, kr=4, J=1),
    "257_seeds": dict(n=3, B=257, N=6, Nc=4),
    "outside_the_box": dict(n=3, B=5),
    "scales_of_one": dict(n=3, B=3),
}


@pytest.mark.parametrize("name", sorted(TABLE_CASES))
def test_tables_and_gradient_of_the_device_are_the_hosts_bit_for_bit(name):
    p = engine_problem(**TABLE_CASES[name])
    B, kr, J = p["B"], p["kr"], p["J"]
    s0 = p["scales"]
    if name == "complex_pairs":
        s0 = np.repeat(s0[:, :2], 2, axis=1)
    d0 = p["offsets"].copy()
    d0[:, 0] = 1.0  # the drift
    lo, hi = 0.5, 1.5
    tau = np.linspace(0.6, 1.4, B) if B > 1 else np.array([0.8])
    if name == "outside_the_box":
        tau = np.array([0.1, 0.5, 0.9, 1.5, 7.0])
    held = clip(tau, lo, hi)
    given = None if name == "scales_of_one" else s0
    if given is None:
        s0 = np.ones((B, kr))
    search, plain = make_engine(p), make_engine(p)
    try:
        search.set_sweep(None, p["offsets"])  # (any tables: the durations replace them)
        search.sweep_set_durations(tau, given, d0, lo, hi, 0.0)
        search.upload_controls(p["u"])
        search.eval_resident(True)
        cost, grads, final = search.download_results()
        scale_sens, offset_sens = search.sweep_sensitivities()
        tau_dev, tau_grad = search.sweep_download_durations()
        plain.set_sweep(held[:, None] * s0, held[:, None] * d0)
        plain.upload_controls(p["u"])
        plain.eval_resident(True)
        pcost, pgrads, pfinal = plain.download_results()
        pscale_sens, poffset_sens = plain.sweep_sensitivities()
    finally:
        search.close()
        plain.close()
    assert np.array_equal(tau_dev, held)
    assert np.array_equal(cost, pcost) and np.array_equal(final, pfinal)
    assert np.array_equal(grads, pgrads) and np.any(grads != 0.0)
    assert np.array_equal(scale_sens, pscale_sens) and np.array_equal(offset_sens, poffset_sens)
    assert tau_grad.shape == (B,)
    assert np.array_equal(tau_grad, chain_rule(s0, d0, scale_sens, offset_sens, 0.0))
    plain_sum = np.sum(scale_sens * s0, axis=1) + np.sum(offset_sens * d0, axis=1)
    scale = np.sum(np.abs(scale_sens * s0), axis=1) + np.sum(np.abs(offset_sens * d0), axis=1)
    print("chain rule against the plain sums:", np.max(np.abs(tau_grad - plain_sum) / scale))
    assert np.all(np.abs(tau_grad - plain_sum) <= 1e-12 * scale)


def test_the_price_of_time_is_two_exact_additions_on_the_device():
    p = engine_problem(3, B=4)
    d0 = p["offsets"].copy()
    d0[:, 0] = 1.0
    tau = np.array([0.6, 0.9, 1.1, 1.4])
    out = {}
    eng = make_engine(p)
    try:
        for weight in (0.0, 0.2):
            eng.set_sweep(None, p["offsets"])
            eng.sweep_set_durations(tau, p["scales"], d0, 0.5, 1.5, weight)
            eng.upload_controls(p["u"])
            eng.eval_resident(True)
            out[weight] = (eng.download_costs(), eng.sweep_download_durations()[1],
                           eng.download_results()[1])
            eng.eval_resident(False)  # the cost term alone
            assert np.array_equal(eng.download_costs(), out[weight][0])
    finally:
        eng.close()
    assert np.array_equal(out[0.2][0], out[0.0][0] + 0.2 * tau)
    assert np.array_equal(out[0.2][1], out[0.0][1] + 0.2)
    assert np.array_equal(out[0.2][2], out[0.0][2])  # the controls' gradients do not see it


@pytest.mark.parametrize("kind", ["sgd", "adam_clipped"])
def test_the_step_kernel_keeps_and_steps_tau_past_a_block_of_seeds(kind):
    """257 seeds, one thread each: best tau of the improved seeds, the update of the flagged ones -
    Adam's first step written out in NumPy, operation by operation - and the clip that follows."""
    p = engine_problem(n=3, B=257, N=6, Nc=4)
    B = p["B"]
    d0 = p["offsets"].copy()
    d0[:, 0] = 1.0
    lo, hi = 0.5, 1.5
    tau0 = np.linspace(0.5, 1.5, B)
    improved = np.arange(B) % 2 == 0
    update = np.arange(B) % 3 != 0
    rate, beta_1, beta_2, epsilon = 0.4, 0.9, 0.999, 1e-8
    eng = make_engine(p)
    try:
        eng.set_sweep(None, p["offsets"])
        eng.sweep_set_durations(tau0, p["scales"], d0, lo, hi, 0.1)
        eng.upload_controls(p["u"])
        eng.opt_begin()
        eng.opt_clip(np.full(p["kr"], 10.0))
        eng.eval_resident(True)
        tau, g = eng.sweep_download_durations()
        assert np.array_equal(tau, tau0)
        if kind == "sgd":
            eng.opt_step(0, improved, update, rate)
            step = rate * g
        else:
            bound = float(np.median(np.abs(g)))  # (clips the gradients of half the seeds)
            eng.opt_step(1, improved, update, rate, beta_1, beta_2, epsilon, 1 - beta_1, 1 - beta_2,
                         bound)
            gc = np.clip(g, -bound, bound)
            assert np.any(gc != g) and np.any(gc == g)
            m = beta_1 * np.zeros(B) + (1 - beta_1) * gc
            v = beta_2 * np.zeros(B) + (1 - beta_2) * (gc * gc)
            step = rate * ((m / (1 - beta_1)) / (np.sqrt(v / (1 - beta_2)) + epsilon))
        stepped = eng.sweep_download_durations(want_grad=False)[0]
        best = eng.opt_download_best_durations()
        with pytest.raises(engine_mod.QocxError, match="evaluation with gradients"):
            eng.sweep_download_durations()
        eng.opt_clip(np.full(p["kr"], 10.0))
        clipped = eng.sweep_download_durations(want_grad=False)[0]
    finally:
        eng.close()
    want = np.where(update, tau0 - step, tau0)
    assert np.array_equal(stepped, want)
    assert np.any(want < lo) or np.any(want > hi)
    assert np.array_equal(best, np.where(improved, tau0, 0.0))
    assert np.array_equal(clipped, clip(want, lo, hi))


# ---- 2. against the oracle -----------------------------------------------------------------------------

def test_a_duration_search_of_c2_transmon_against_the_oracle_at_four_durations():
    case = cases_mod.case_c2_transmon()
    ref, B = case.T, 4
    times = ref * np.array([0.5, 0.8, 1.0, 1.3])
    h = case.hamiltonian()
    target = case.cost_specs[0][1]["target_states"]
    rng = np.random.default_rng(77)
    u = np.stack([case.controls[0]] + [0.1 * rng.standard_normal((case.Nc, case.K))
                                       for _ in range(B - 1)])
    h0 = np.asarray(h(np.zeros(case.K), 0.0))

    def expanded(r, t):
        return (h(r[:case.K], t) - h0) + r[case.K] * h0

    out = {}
    for weight in (0.0, 0.2):
        w = HamiltonianSweep.durations(h, times, ref, time_bounds=(0.4 * ref, 1.5 * ref),
                                       time_weight=weight)
        ev = device.SchroedingerEvaluator(
            ref, w, case.initial_states, case.N, control_count=case.K,
            control_eval_count=case.Nc, costs=[product_costs.TargetStateInfidelity(target)])
        errors, grads, finals, _ = ev.evaluate_batch(u)
        out[weight] = (errors, ev.duration_gradients(), ev.evolution_time_gradients())
        assert np.array_equal(ev.evolution_times(), as_times(w, times))
        sens = ev.sweep_sensitivities()
        chain = w.time_gradients(sens["control_scales"], sens["offsets"]) * ref + weight
        assert rel_err(out[weight][1], chain) < 1e-12
    errors, _, time_grads = out[0.0]
    for b in range(B):
        problem = onp.SchroedingerProblem(
            times[b], h, case.initial_states, case.N, control_eval_count=case.Nc,
            costs=[onp.TargetStateInfidelity(target)], control_count=case.K)
        err, gr, fin = onp.evaluate_with_grad(problem, u[b])
        assert abs(errors[b] - err) < 1e-10
        tau = times[b] / ref
        wide = onp.SchroedingerProblem(
            ref, expanded, case.initial_states, case.N, control_eval_count=case.Nc,
            costs=[onp.TargetStateInfidelity(target)], control_count=case.K + 1)
        r = np.concatenate([tau * u[b], np.full((case.Nc, 1), tau)], axis=1)
        _, g_wide, _ = onp.evaluate_with_grad(wide, r)
        g_wide = np.real(g_wide)
        want_s = np.sum(u[b] * g_wide[:, :case.K], axis=0)
        want_d = np.sum(g_wide[:, case.K:], axis=0)
        want_t = (np.sum(want_s) + want_d[0]) / ref
        print("seed", b, "dE/dT", time_grads[b], "oracle", want_t)
        assert abs(time_grads[b] - want_t) < 1e-8 * max(abs(want_t),
                                                        np.max(np.abs(want_s)) / ref)
    tau = times / ref
    assert np.array_equal(out[0.2][0], out[0.0][0] + 0.2 * tau)
    assert np.array_equal(out[0.2][1], out[0.0][1] + 0.2)
    assert np.array_equal(out[0.2][2], (out[0.0][1] + 0.2) / ref)


@pytest.mark.parametrize("weight", [0.0, 0.3])
def test_two_level_known_answer_on_the_engine(weight):
    sx = np.array([[0, 1], [1, 0]], dtype=np.complex128)
    times, ref = np.array([1.2, 2.0, 2.6]), 2.0
    w = HamiltonianSweep.durations(lambda u, t: 0.5 * u[0] * sx, times, ref,
                                   time_bounds=(0.5, 4.0), time_weight=weight)
    psi0 = cases_mod.column_states(np.eye(2)[:, :1])
    target = cases_mod.column_states(np.eye(2)[:, 1:])
    ev = device.SchroedingerEvaluator(ref, w, psi0, 11, control_count=1, control_eval_count=5,
                                      costs=[product_costs.TargetStateInfidelity(target)])
    errors, _, _, _ = ev.evaluate_batch(np.ones((3, 5, 1)))
    want = np.cos(times / 2) ** 2 + weight * times / ref
    want_grad = -0.5 * np.sin(times) + weight / ref
    print("errors", errors - want, "gradients", ev.evolution_time_gradients() - want_grad)
    assert np.max(np.abs(errors - want)) < 1e-9
    assert np.max(np.abs(ev.evolution_time_gradients() - want_grad)) < 1e-9


# ---- 3. multi-start GRAPE: the routes -----------------------------------------------------------------

def searching(w, weight=0.0, bounds=None):
    """The duration sweep of route_problem() as a search (default box: 0.4 to 1.4 reference times,
    the longest start)."""
    ref = w.reference_time
    return HamiltonianSweep.durations(
        w._source, w.evolution_times, ref, control_scales=w._user_scales,
        perturbations=w._extra_perturbations, offsets=w._user_offsets[:, 1:],
        time_bounds=(0.4 * ref, 1.4 * ref) if bounds is None else bounds, time_weight=weight)


def as_times(w, times):
    """T_b as the search reports it: tau_b = T_b / reference_time, times reference_time."""
    return (np.asarray(times) / w.reference_time) * w.reference_time


def run_both(routes, optimizer, w, head, tail, start, **kw):
    resident, host = OPTIMIZERS[optimizer]
    kw = dict(dict(iteration_count=5, log_iteration_step=0), **kw)
    a = qoc_amd.grape_schroedinger_discrete_batch(*head, w, *tail, start.copy(),
                                                  optimizer=resident(), **kw)
    assert (routes["resident"], routes["host"]) == (1, 0)
    b = qoc_amd.grape_schroedinger_discrete_batch(*head, w, *tail, start.copy(), optimizer=host(),
                                                  **kw)
    assert (routes["resident"], routes["host"]) == (1, 1)
    return a, b


def assert_bit_identical(a, b):
    assert np.array_equal(a.best_error, b.best_error)
    assert np.array_equal(a.best_iteration, b.best_iteration)
    assert np.array_equal(a.iterations_run, b.iterations_run)
    for s in range(len(a.best_error)):
        assert np.array_equal(a.best_controls[s], b.best_controls[s])
        assert np.array_equal(a.best_final_states[s], b.best_final_states[s])
    assert np.array_equal(a.best_evolution_times, b.best_evolution_times)
    for key in ("control_scales", "offsets", "evolution_time_gradients"):
        assert np.array_equal(a.sweep_sensitivities[key], b.sweep_sensitivities[key])


def start_state(w, head, tail, u0, **kw):
    """(errors, d error / d tau) of every seed at its start."""
    (K, Nc, costs, T), (psi0, N) = head, tail
    ev = device.SchroedingerEvaluator(T, w, psi0, N, control_count=K, control_eval_count=Nc,
                                      costs=costs, **kw)
    errors = ev.evaluate_batch(u0)[0]
    return errors, ev.duration_gradients()


VARIANTS = ("plain", "sine_basis", "control_variation", "complex", "priced", "stopped_seed",
            "pinned_seed")


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("optimizer", ["adam", "sgd"])
def test_resident_route_equals_host_loop_with_tau_as_a_parameter(routes, optimizer, variant):
    """Bit for bit, which needs both routes on the same kernel variants: the engine picks those by
    its bound of the step norm - the resident route's from max_control_norms at T_max, the host
    loop's from the uploaded pulse at the current durations, never the larger. The box and the norms
    keep the resident bound where the factorisation takes the diagonally dominant form (eps_max of
    qocx_api.hip <= 0.40: 0.37 at theta = 0.63 here, real and complex), so the host's does too."""
    complex_controls = variant == "complex"
    plain, head, tail, rng = route_problem(complex_controls=complex_controls)
    K, Nc, costs, T = head
    start_times = plain.evolution_times.copy()
    kw = dict(max_control_norms=np.full(K, 0.45 if complex_controls else 0.9))
    weight, bounds = (0.05 if variant == "priced" else 0.0), None
    if complex_controls:
        # (pulses the modulus clip does not reach in five iterations: where it acts, the two routes
        # round the clipped complex controls differently on the plain problem already - NumPy's
        # complex division against the device's reciprocal -, which is not this feature's to settle)
        u0 = 0.05 * (rng.standard_normal((3, Nc, K)) + 1j * rng.standard_normal((3, Nc, K)))
        u0 = u0 * np.minimum(1.0, 0.08 / np.abs(u0))
        kw["complex_controls"] = True
    elif variant == "sine_basis":
        basis = ControlBasis.sine(Nc, 4)
        u0 = 0.3 * rng.standard_normal((3, 4, K))
        for s in range(3):
            u0[s] *= min(1.0, 0.8 / np.max(np.abs(basis.expand(u0[s]))))
        kw["control_basis"] = basis
    else:
        u0 = np.clip(0.6 * rng.standard_normal((3, Nc, K)), -0.9, 0.9)
    if variant == "control_variation":
        head = (K, Nc, costs + [ControlVariation(K, Nc, cost_multiplier=0.4, order=1)], T)
    stopped = pinned = None
    if variant == "stopped_seed":
        errors, _ = start_state(searching(plain), head, tail, u0)
        order = np.argsort(errors)
        stopped = int(order[0])
        kw["min_error"] = 0.5 * (errors[order[0]] + errors[order[1]])
    if variant == "pinned_seed":
        # the box ends at the start of the seed whose error falls with its duration there
        _, tau_grad = start_state(searching(plain), head, tail, u0)
        pinned = int(np.argmin(tau_grad))
        assert tau_grad[pinned] < 0
        bounds = (0.4 * T, start_times[pinned])
        start_times = np.minimum(start_times, start_times[pinned])
        plain = HamiltonianSweep.durations(
            plain._source, start_times, T, control_scales=plain._user_scales,
            perturbations=plain._extra_perturbations, offsets=plain._user_offsets[:, 1:])
    w = searching(plain, weight, bounds)
    a, b = run_both(routes, optimizer, w, head, tail, u0, **kw)
    for s in range(3):
        print("seed {}: T {} -> {} | best_error {:.3e} apart, controls {:.3e} relative".format(
            s, start_times[s], a.best_evolution_times[s], abs(a.best_error[s] - b.best_error[s]),
            rel_err(a.best_controls[s], b.best_controls[s])))
    assert_bit_identical(a, b)
    assert np.any(a.best_iteration > 0)
    assert np.any(a.best_evolution_times != as_times(w, start_times))
    lo, hi = w.time_bounds
    assert np.all((a.best_evolution_times >= lo) & (a.best_evolution_times <= hi))
    if variant == "sine_basis":
        for s in range(3):
            assert np.array_equal(a.best_coefficients[s], b.best_coefficients[s])
    if stopped is not None:  # stopped by min_error at iteration 0: its tau never moved
        assert a.iterations_run[stopped] == 1 and a.best_iteration[stopped] == 0
        assert a.best_evolution_times[stopped] == as_times(w, start_times)[stopped]
        assert np.any(a.iterations_run > 1)
    if pinned is not None:
        assert w.time_bounds[1] == start_times[pinned]
        assert a.best_evolution_times[pinned] == w.tau_bounds[1] * T


# ---- 4. refusals of the ABI; a plain sweep afterwards --------------------------------------------------

def test_engine_refusals():
    p = engine_problem(3, B=3)
    d0 = p["offsets"].copy()
    d0[:, 0] = 1.0
    tau = np.array([0.7, 1.0, 1.2])
    eng = make_engine(p)
    try:
        eng._sweep = dict(B=3, J=p["J"], Kr=p["kr"])
        with pytest.raises(engine_mod.QocxError, match="no sweep set") as info:
            eng.sweep_set_durations(tau, p["scales"], d0, 0.5, 1.5)
        assert info.value.code == ERR_STATE
        eng.set_sweep(p["scales"], p["offsets"])
        with pytest.raises(engine_mod.QocxError, match="no durations set") as info:
            eng.sweep_download_durations()
        assert info.value.code == ERR_STATE
        for bad in ((0.0, 1.5, 0.0), (1.5, 0.5, 0.0), (0.5, np.inf, 0.0), (0.5, 1.5, -1.0),
                    (0.5, 1.5, np.nan)):
            with pytest.raises(engine_mod.QocxError):
                eng.sweep_set_durations(tau, p["scales"], d0, *bad)
        with pytest.raises(engine_mod.QocxError, match="non-finite duration"):
            eng.sweep_set_durations([0.7, np.nan, 1.2], p["scales"], d0, 0.5, 1.5)
        eng.sweep_set_durations(tau, p["scales"], d0, 0.5, 1.5)
        assert np.array_equal(eng.sweep_download_durations(want_grad=False)[0], tau)
        with pytest.raises(engine_mod.QocxError, match="evaluation with gradients") as info:
            eng.sweep_download_durations()
        assert info.value.code == ERR_STATE
        eng.upload_controls(p["u"])
        eng.eval_resident(False)
        with pytest.raises(engine_mod.QocxError, match="evaluation with gradients"):
            eng.sweep_download_durations()
        eng.opt_begin()
        with pytest.raises(engine_mod.QocxError, match="duration search") as info:
            eng.opt_lbfgs_begin(5)
        assert info.value.code == ERR_STATE
        with pytest.raises(engine_mod.QocxError, match="gradients to step with"):
            eng.opt_step(0, np.ones(3, bool), np.ones(3, bool), 0.1)
        # a new sweep clears the search
        eng.set_sweep(p["scales"], p["offsets"])
        with pytest.raises(engine_mod.QocxError, match="no durations set"):
            eng.sweep_download_durations(want_grad=False)
    finally:
        eng.close()


def test_a_plain_duration_sweep_after_a_search_is_what_a_fresh_engine_gives(routes):
    plain, head, tail, rng = route_problem()
    K, Nc = head[0], head[1]
    u0 = np.clip(0.6 * rng.standard_normal((3, Nc, K)), -1, 1)
    resident, _ = OPTIMIZERS["adam"]
    kw = dict(iteration_count=4, log_iteration_step=0, max_control_norms=np.full(K, 1.0))
    shared = engine_mod.Engine(0)
    helpers.set_backend_factory(lambda: shared)
    try:
        searched = qoc_amd.grape_schroedinger_discrete_batch(
            *head, searching(plain, 0.05), *tail, u0.copy(), optimizer=resident(), **kw)
        after = qoc_amd.grape_schroedinger_discrete_batch(*head, plain, *tail, u0.copy(),
                                                          optimizer=resident(), **kw)
    finally:
        helpers.set_backend_factory(None)
        shared.close()
    fresh = qoc_amd.grape_schroedinger_discrete_batch(*head, plain, *tail, u0.copy(),
                                                      optimizer=resident(), **kw)
    assert routes["resident"] == 3 and routes["host"] == 0
    assert searched.best_evolution_times is not None and after.best_evolution_times is None
    assert np.array_equal(after.best_error, fresh.best_error)
    assert np.array_equal(after.best_iteration, fresh.best_iteration)
    for s in range(3):
        assert np.array_equal(after.best_controls[s], fresh.best_controls[s])
        assert np.array_equal(after.best_final_states[s], fresh.best_final_states[s])
    for key in ("control_scales", "offsets", "evolution_time_gradients"):
        assert np.array_equal(after.sweep_sensitivities[key], fresh.sweep_sensitivities[key])
