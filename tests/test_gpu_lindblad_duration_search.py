"""
GPU tests (-m gpu) of the duration search of a Lindblad sweep (LindbladSweep.duration_search ->
qocx_lindblad_sweep_set_durations, qocx_lindblad_duration.hip): tau_b = T_b / reference_time is one
more optimised parameter of seed b, and seed b is tau_b times the whole Lindbladian.

1. the gradient with respect to tau is the chain rule through scales, offsets and rate factors in its
   stated order, bit for bit, and the price of time one product and one sum;
2. with a launch order that differs from the seed order every seed keeps the gradient it has alone;
3. an evaluation of the search is the fixed-duration sweep at the same (clipped) tau, to rounding;
4. dE_b/dtau_b against central differences of the fixed-step model of member(b);
5. a decaying level whose best duration is known in closed form: the gradient vanishes there, a
   resident SGD search finds it from both sides, and a seed at the lower bound stays there;
6. the step kernel keeps and steps tau past a block of seeds;
7. the resident route walks the host loop's trajectory bit for bit;
8. the engine's refusals, and a fixed-duration sweep after a search.

Shapes: N = 7 system steps and Nc = 4 (N = 4, Nc = 3 above one tile), B = 3 seeds.
"""

import numpy as np
import pytest

import qoc_amd
from oracle import qoc_lindblad_numpy as ol
from qoc_amd.core import device
from qoc_amd.engine import Engine, QocxError
from qoc_amd.standard import (SGD, Adam, ControlBasis, ControlVariation, LindbladSweep,
                              TargetDensityInfidelity)
from tests import cases as cases_mod
from tests import gpu_helpers as gh
from tests import helpers
from tests import lindblad_model as lm
from tests.test_gpu_lindblad_ensemble import routes  # noqa: F401 (fixture)
from tests.test_gpu_lindblad_sweep import route_problem, sized_case
from tests.test_lindblad_host_api import product_cost_list

pytestmark = pytest.mark.gpu

B = 3
ERR_ARG, ERR_STATE = -1, -3
TAGS = {"n4_l1": (4, 1, "real", 1), "n4_l2": (4, 2, "real", 1),
        "n16_l3_s2_complex_ops": (16, 3, "random", 2), "n20_l2": (20, 2, "real", 1)}


@pytest.fixture(autouse=True)
def real_engine():
    helpers.set_backend_factory(None)
    yield
    helpers.set_backend_factory(None)


@pytest.fixture(scope="module")
def engine():
    e = Engine(0)
    yield e
    e.close()


def clip(tau, lo, hi):
    return np.minimum(np.maximum(tau, lo), hi)


def chain_rule(s0, d0, c0, scale_sens, offset_sens, rate_sens, weight):
    """The order of lindblad_duration_gradient_kernel (qocx_lindblad_duration.hip), all seeds at once."""
    g = np.zeros(s0.shape[0])
    for k in range(s0.shape[1]):
        g = g + s0[:, k] * scale_sens[:, k]
    for j in range(d0.shape[1]):
        g = g + d0[:, j] * offset_sens[:, j]
    for l in range(c0.shape[1]):
        g = g + c0[:, l] * rate_sens[:, l]
    return g + weight


def tables(case, seed, seeds=B):
    """Non-trivial control scales, one user channel beside the drift (J = 2) and rate factors."""
    rng = np.random.default_rng(seed)
    L = len(case.dissipators)
    return dict(control_scales=1 + 0.05 * rng.standard_normal((seeds, case.K)),
                perturbations=0.5 * cases_mod.gue(rng, case.n)[None],
                offsets=0.3 * rng.standard_normal((seeds, 1)),
                rate_scales=np.array([[0.5, 1.0, 2.0][(b + l) % 3] for b in range(seeds)
                                      for l in range(L)], dtype=np.float64).reshape(seeds, L))


def base_tables(tab):
    """(s0, delta0, c0) as the engine holds them: the drift column of delta0 is 1."""
    d0 = np.concatenate([np.ones((len(tab["offsets"]), 1)), tab["offsets"]], axis=1)
    return tab["control_scales"], d0, tab["rate_scales"]


def search_sweep(case, tab, taus, box=(0.4, 1.5), weight=0.0):
    return LindbladSweep.duration_search(case.hamiltonian(), case.T * np.asarray(taus), case.T,
                                         (box[0] * case.T, box[1] * case.T), weight, **tab)


def evaluator(engine, case, w, costs=None):
    return device.LindbladEvaluator(
        case.T, case.initial_densities, case.N, hamiltonian=w, lindblad_data=case.lindblad_data(),
        control_count=case.K, control_eval_count=case.Nc,
        costs=product_cost_list(case) if costs is None else costs,
        cost_eval_step=case.cost_eval_step, backend=engine)


def pulses(case, seed, seeds=B, amplitude=0.5):
    return amplitude * np.random.default_rng(seed).standard_normal((seeds, case.Nc, case.K))


def code_of(call, *args, **kw):
    with pytest.raises(QocxError) as err:
        call(*args, **kw)
    return err.value.code


# ---- 1. the chain rule, bit for bit -----------------------------------------------------------------

@pytest.mark.parametrize("tag", sorted(TAGS))
def test_the_gradient_is_the_chain_rule_in_its_stated_order_and_the_price_two_operations(engine, tag):
    case = sized_case(*TAGS[tag])
    tab = tables(case, 700 + len(tag))
    s0, d0, c0 = base_tables(tab)
    taus = np.array([0.7, 1.0, 1.2])
    u = pulses(case, 701)
    out = {}
    for weight in (0.0, 0.3):
        w = search_sweep(case, tab, taus, weight=weight)
        ev = evaluator(engine, case, w)
        errors, grads, _, _ = ev.evaluate_batch(u)
        tau, tau_grad = engine.lindblad_sweep_download_durations()
        scale_sens, offset_sens, rate_sens = engine.lindblad_sweep_sensitivities()
        assert rate_sens is not None and rate_sens.shape == c0.shape
        assert np.array_equal(tau, w.evolution_times / case.T)
        assert np.max(np.abs(tau - taus)) < 1e-15
        assert np.array_equal(tau_grad, chain_rule(s0, d0, c0, scale_sens, offset_sens, rate_sens,
                                                   weight))
        assert np.array_equal(ev.duration_gradients(), tau_grad)
        out[weight] = (errors, tau_grad, grads)
        # (every table carries a signal: far above rounding)
        for part in (scale_sens, offset_sens, rate_sens):
            assert np.min(np.max(np.abs(part), axis=1)) > 1e-6
    assert np.array_equal(out[0.3][0], out[0.0][0] + 0.3 * tau)
    assert np.array_equal(out[0.3][1], out[0.0][1] + 0.3)
    assert np.array_equal(out[0.3][2], out[0.0][2])  # the controls' gradients do not see the price


# ---- 2. launch order != seed order --------------------------------------------------------------------

def test_every_seed_keeps_its_gradient_when_the_launch_order_is_not_the_seed_order(engine):
    """Seed 0 runs three times as long as seed 1 on a pulse twenty times as strong, so it falls into
    a finer sub-division group; groups launch in ascending count, so seed 1 is launched first."""
    case = sized_case(*TAGS["n4_l2"])
    tab = tables(case, 710, seeds=2)
    taus = np.array([1.5, 0.5])
    u = np.random.default_rng(711).standard_normal((2, case.Nc, case.K))
    u *= (np.array([4.0, 0.2]) / np.max(np.abs(u), axis=(1, 2)))[:, None, None]
    ev = evaluator(engine, case, search_sweep(case, tab, taus, weight=0.1))
    errors, grads, _, _ = ev.evaluate_batch(u)
    together = engine.lindblad_last_subintervals()
    tau_grad = ev.duration_gradients()
    alone, counts = [], []
    for b in range(2):
        one = {k: (v if k == "perturbations" else v[b:b + 1]) for k, v in tab.items()}
        ev1 = evaluator(engine, case, search_sweep(case, one, taus[b:b + 1], weight=0.1))
        e1, g1, _, _ = ev1.evaluate_batch(u[b:b + 1])
        counts.append(engine.lindblad_last_subintervals())
        alone.append(ev1.duration_gradients()[0])
        assert np.array_equal(e1[0], errors[b]) and np.array_equal(g1[0], grads[b])
    print("sub-intervals per seed", counts)
    assert counts[0] > counts[1] and together == sum(counts)  # two groups, seed 1's launched first
    assert np.array_equal(tau_grad, np.array(alone))
    assert abs(alone[0] - alone[1]) > 1e-6


# ---- 3. a search evaluation is the fixed sweep at the same tau ------------------------------------------

@pytest.mark.parametrize("tag", sorted(TAGS))
def test_a_search_evaluation_is_the_fixed_duration_sweep_at_the_clipped_tau(engine, tag):
    """To rounding, not bit for bit (tau * sum (c0 gamma) L^H L against sum (tau c0 gamma) L^H L): 1e-12
    on the errors and 1e-10 of the largest entry on the gradients, the project's gates for two
    summation orders of one scheme. Both must run on the same grid, which is asserted first. The
    time gradient compared is d E_b / d T_b = (duration_gradients() - time_weight) / reference_time."""
    case = sized_case(*TAGS[tag])
    tab = tables(case, 720 + len(tag))
    weight, box = 0.2, (0.6, 1.3)
    asked = np.array([0.3, 1.0, 1.7])  # two of them outside the box
    u = pulses(case, 721)
    w = search_sweep(case, tab, [1.0, 1.0, 1.0], box, weight)
    held = clip(asked, *w.tau_bounds)
    ev = evaluator(engine, case, w)
    ev.set_durations(asked)
    assert np.array_equal(ev.durations(), held)
    errors, grads, finals, _ = ev.evaluate_batch(u)
    count = engine.lindblad_last_subintervals()
    time_grads = (ev.duration_gradients() - weight) / case.T
    fixed = LindbladSweep.durations(case.hamiltonian(), case.T * held, case.T, **tab)
    fv = evaluator(engine, case, fixed)
    fv.want_rate_sensitivities(True)
    f_errors, f_grads, f_finals, _ = fv.evaluate_batch(u)
    assert engine.lindblad_last_subintervals() == count
    f_time_grads = fv.sweep_sensitivities()["evolution_time_gradients"]
    fv.want_rate_sensitivities(False)
    print(tag, "errors", np.max(np.abs(errors - weight * held - f_errors)), "gradients",
          np.max(np.abs(grads - f_grads)) / np.max(np.abs(f_grads)), "dE/dT",
          np.max(np.abs(time_grads - f_time_grads)) / np.max(np.abs(f_time_grads)))
    assert np.max(np.abs((errors - weight * held) - f_errors)) < 1e-12
    assert np.max(np.abs(finals - f_finals)) < 1e-12
    assert np.max(np.abs(grads - f_grads)) < 1e-10 * np.max(np.abs(f_grads))
    assert np.max(np.abs(time_grads - f_time_grads)) < 1e-10 * np.max(np.abs(f_time_grads))
    assert np.min(np.abs(f_time_grads)) > 1e-6


# ---- 4. finite differences -----------------------------------------------------------------------------

def test_the_duration_gradient_agrees_with_central_differences_of_the_model():
    """dE_b/dtau_b of the engine against (E_b(tau_b + h) - E_b(tau_b - h)) / 2h of the fixed-step model
    (tests/lindblad_model.py, the forward pass of the oracle backend) of sweep.member(b) with
    sweep.member_lindblad_data(b, .) of the fixed-duration sweeps at tau_b +- h, all three on the one
    grid the model picks at tau_b + h. h = 1e-4 tau_b (tests/test_lindblad_sweep_host.py scanned it:
    the central difference is good to 3e-12 there); the gate is that of the rate sensitivities,
    helpers.lindblad_grad_close: 1e-8 of the largest entry."""
    case = sized_case(*TAGS["n4_l2"])
    tab = tables(case, 730)
    taus = np.array([0.7, 1.0, 1.2])
    u = pulses(case, 731)
    eng = Engine(0)
    try:
        ev = evaluator(eng, case, search_sweep(case, tab, taus))
        ev.evaluate_batch(u)
        got = ev.duration_gradients()
    finally:
        eng.close()
    costs = [getattr(ol, k)(**kw) for k, kw in case.cost_specs]
    data = case.lindblad_data()
    K, dt = case.K, case.T / (case.N - 1)

    def structured(w, b):
        hamiltonian, lindblad_data = w.member(b), w.member_lindblad_data(b, data)
        h0 = hamiltonian(np.zeros(K), 0.0)
        return lm.StructuredLindblad(h0, [hamiltonian(np.eye(K)[k], 0.0) - h0 for k in range(K)],
                                     *lindblad_data(0.0))

    want = np.zeros(B)
    for b in range(B):
        h = 1e-4 * taus[b]
        systems = []
        for tau in (taus[b] + h, taus[b] - h):
            moved = taus.copy()
            moved[b] = tau
            systems.append(structured(LindbladSweep.durations(case.hamiltonian(), case.T * moved,
                                                              case.T, **tab), b))
        umax = np.max(np.abs(u[b]), axis=0)
        ksub = max(1, int(np.ceil(systems[0].norm_bound(umax) * dt / 0.4)))
        up, down = (lm.evaluate_with_grad(s, u[b], case.initial_densities, case.T, case.N, costs,
                                          want_grad=False, subdivision=ksub)[0] for s in systems)
        want[b] = (up - down) / (2 * h)
    print("dE/dtau", got, "central differences", want, "difference", got - want)
    assert np.min(np.abs(want)) > 1e-4
    assert helpers.lindblad_grad_close(got, want, case)
    # ... and beside the differences the exact sensitivity (tests/lindblad_exact.py: the forward
    # sensitivity equation of the factor tau on the whole Lindbladian, two integrators), at its gate
    from tests import lindblad_exact as ex
    fixed = LindbladSweep.durations(case.hamiltonian(), case.T * taus, case.T, **tab)
    exact = np.zeros(B)
    for b in range(B):
        s = structured(fixed, b)
        r = ex.linear(s.h0, s.g, s.ops, s.gammas, u[b], case.T, case.N, case.initial_densities, costs,
                      directions=[None])
        assert 10 * r.disagreement["derivative"] <= ex.GATE_LINEAR_DERIVATIVE
        exact[b] = r.derivative[0] / taus[b]
    print("exact", exact, "difference", got - exact, "over its gate",
          np.max(np.abs(got - exact)) / np.max(np.abs(exact)) / ex.GATE_LINEAR_DERIVATIVE)
    assert np.max(np.abs(got - exact)) <= ex.GATE_LINEAR_DERIVATIVE * np.max(np.abs(exact))


# ---- 5. a known answer with an interior minimum -------------------------------------------------------

GAMMA, PRICE = 0.7, 0.1
T_STAR = np.log(GAMMA / (2 * PRICE)) / GAMMA


def decaying_level(times, box, weight, target_level=0, seeds=None):
    """|1> decays into |0> with gamma; H is diagonal, so the control on sigma_z cannot move
    populations. With the target |0><0| the error is E(T) = 1 - (1 - exp(-gamma T)) / 2."""
    sz = np.diag([0.0, 1.0]).astype(np.complex128)
    lower = np.array([[0, 1], [0, 0]], dtype=np.complex128)  # |0><1|
    rho0 = np.zeros((1, 2, 2), dtype=np.complex128)
    rho0[0, 1, 1] = 1
    target = np.zeros((1, 2, 2), dtype=np.complex128)
    target[0, target_level, target_level] = 1
    w = LindbladSweep.duration_search(lambda u, t: 0.3 * sz + u[0] * sz, times, 1.0, box, weight)
    data = lambda t: (np.array([GAMMA]), lower[None])  # noqa: E731
    return w, data, rho0, [TargetDensityInfidelity(target)]


def test_the_gradient_vanishes_at_the_known_best_duration(engine):
    """E + lambda T has its minimum at T* = ln(gamma / 2 lambda) / gamma = 1.790; there the engine's
    gradient is below 1e-8 gamma / 2, the gradient gate of DESIGN section 9 on dE/dT(0) = gamma / 2."""
    w, data, rho0, costs = decaying_level([T_STAR, 1.0], (0.5, 4.0), PRICE)
    ev = device.LindbladEvaluator(1.0, rho0, 7, hamiltonian=w, lindblad_data=data, control_count=1,
                                  control_eval_count=4, costs=costs, backend=engine)
    errors, _, _, _ = ev.evaluate_batch(np.zeros((2, 4, 1)))
    grad = ev.duration_gradients()
    closed = 1 - (1 - np.exp(-GAMMA * np.array([T_STAR, 1.0]))) / 2 + PRICE * np.array([T_STAR, 1.0])
    print("T*", T_STAR, "gradient there", grad[0], "errors - closed form", errors - closed)
    assert abs(grad[0]) < 1e-8 * GAMMA / 2
    assert abs(grad[1] - (-GAMMA / 2 * np.exp(-GAMMA) + PRICE)) < 1e-8 * GAMMA / 2
    assert np.max(np.abs(errors - closed)) < 1e-10


def test_a_resident_sgd_search_finds_the_known_best_duration_from_both_sides(routes):
    """Starts at 0.8 and 3.0 inside (0.5, 4.0), for as many iterations as the same recursion on the
    closed form needs to come within 1e-9 of T*. Gradient error over curvature bounds the offset of
    the engine's fixed point by 1e-8 (gamma / 2) / (gamma lambda) = 1e-8 / (2 lambda) = 5e-8; the
    gate of 1e-6 leaves a factor 20."""
    rate, starts = 8.0, np.array([0.8, 3.0])
    tau, iterations = starts.copy(), 0
    while np.max(np.abs(tau - T_STAR)) >= 1e-9:
        tau = clip(tau - rate * (-GAMMA / 2 * np.exp(-GAMMA * tau) + PRICE), 0.5, 4.0)
        iterations += 1
        assert iterations < 200
    w, data, rho0, costs = decaying_level(starts, (0.5, 4.0), PRICE)
    result = qoc_amd.grape_lindblad_discrete_batch(
        1, 4, costs, 1.0, rho0, 7, np.zeros((2, 4, 1)), hamiltonian=w, lindblad_data=data,
        iteration_count=iterations + 1, log_iteration_step=0, optimizer=SGD(learning_rate=rate))
    assert routes == {"resident": 1, "host": 0}
    print("iterations", iterations + 1, "found", result.best_evolution_times, "T*", T_STAR)
    assert np.max(np.abs(result.best_evolution_times - T_STAR)) < 1e-6
    best = 1 - (1 - np.exp(-GAMMA * T_STAR)) / 2 + PRICE * T_STAR
    assert np.max(np.abs(result.best_error - best)) < 1e-10


def test_a_seed_at_the_lower_bound_whose_error_grows_with_time_stays_there(routes):
    """lambda = 0 and the target |1><1|: the error grows with T, every step pushes tau below the box
    and the clip puts it back on T_min exactly."""
    w, data, rho0, costs = decaying_level([0.5, 1.5], (0.5, 4.0), 0.0, target_level=1)
    result = qoc_amd.grape_lindblad_discrete_batch(
        1, 4, costs, 1.0, rho0, 7, np.zeros((2, 4, 1)), hamiltonian=w, lindblad_data=data,
        iteration_count=5, log_iteration_step=0, optimizer=SGD(learning_rate=0.5))
    assert routes == {"resident": 1, "host": 0}
    assert result.best_evolution_times[0] == 0.5
    assert 0.5 <= result.best_evolution_times[1] < 1.5
    assert abs(result.best_error[0] - (1 - np.exp(-GAMMA * 0.5) / 2)) < 1e-10


# ---- 6. the step kernel past a block ------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["sgd", "adam_clipped"])
def test_the_step_kernel_keeps_and_steps_tau_past_a_block_of_seeds(kind):
    """257 seeds, one thread each: best tau of the improved seeds, the update of the flagged ones -
    Adam's first step written out in NumPy, operation by operation - and the clip that follows."""
    seeds, lo, hi = 257, 0.5, 1.5
    tau0 = np.linspace(lo, hi, seeds)
    w, data, rho0, costs = decaying_level(tau0, (lo, hi), 0.1)
    improved = np.arange(seeds) % 2 == 0
    update = np.arange(seeds) % 3 != 0
    rate, beta_1, beta_2, epsilon = 0.4, 0.9, 0.999, 1e-8
    eng = Engine(0)
    try:
        device.LindbladEvaluator(1.0, rho0, 3, hamiltonian=w, lindblad_data=data, control_count=1,
                                 control_eval_count=3, costs=costs, backend=eng)
        eng.lindblad_upload_controls(np.zeros((seeds, 3, 1)))
        eng.lindblad_opt_begin()
        eng.lindblad_opt_clip(np.full(1, 10.0))
        eng.eval_lindblad_resident(True)
        tau, g = eng.lindblad_sweep_download_durations()
        assert np.array_equal(tau, tau0)
        if kind == "sgd":
            eng.lindblad_opt_step(0, improved, update, rate)
            step = rate * g
        else:
            bound = float(np.median(np.abs(g)))  # (clips the gradients of half the seeds)
            eng.lindblad_opt_step(1, improved, update, rate, beta_1, beta_2, epsilon, 1 - beta_1,
                                  1 - beta_2, bound)
            gc = np.clip(g, -bound, bound)
            assert np.any(gc != g) and np.any(gc == g)
            m = beta_1 * np.zeros(seeds) + (1 - beta_1) * gc
            v = beta_2 * np.zeros(seeds) + (1 - beta_2) * (gc * gc)
            step = rate * ((m / (1 - beta_1)) / (np.sqrt(v / (1 - beta_2)) + epsilon))
        stepped = eng.lindblad_sweep_download_durations(want_grad=False)[0]
        best = eng.lindblad_opt_download_best_durations()
        with pytest.raises(QocxError, match="evaluation with gradients"):
            eng.lindblad_sweep_download_durations()
        eng.lindblad_opt_clip(np.full(1, 10.0))
        clipped = eng.lindblad_sweep_download_durations(want_grad=False)[0]
    finally:
        eng.close()
    want = np.where(update, tau0 - step, tau0)
    assert np.array_equal(stepped, want)
    assert np.any(want < lo) or np.any(want > hi)
    assert np.array_equal(best, np.where(improved, tau0, 0.0))
    assert np.array_equal(clipped, clip(want, lo, hi))
    assert stepped[256] != tau0[256] and best[256] == tau0[256]  # the seed past the block


# ---- 7. the resident route against the host loop -------------------------------------------------------

class HostAdam(Adam):  # not type(...) is Adam: takes the host loop
    pass


class HostSGD(SGD):
    pass


OPTIMIZERS = {"adam": (lambda: Adam(learning_rate=5e-2), lambda: HostAdam(learning_rate=5e-2)),
              "sgd": (lambda: SGD(learning_rate=0.5), lambda: HostSGD(learning_rate=0.5))}


def searching(w, weight=0.0):
    """The duration sweep of route_problem() as a search inside 0.4 to 1.5 reference times."""
    ref = w.reference_time
    return LindbladSweep.duration_search(
        w._source, w.evolution_times, ref, (0.4 * ref, 1.5 * ref), weight,
        control_scales=w._user_scales, perturbations=w._extra_perturbations,
        offsets=w._user_offsets[:, 1:], rate_scales=w._user_rates)


def run_both(routes, optimizer, w, data, head, start, **kw):
    resident, host = OPTIMIZERS[optimizer]
    kw = dict(dict(iteration_count=6, log_iteration_step=0, lindblad_data=data, hamiltonian=w), **kw)
    a = qoc_amd.grape_lindblad_discrete_batch(*head, start.copy(), optimizer=resident(), **kw)
    assert routes == {"resident": 1, "host": 0}
    b = qoc_amd.grape_lindblad_discrete_batch(*head, start.copy(), optimizer=host(), **kw)
    assert routes == {"resident": 1, "host": 1}
    return a, b


def assert_bit_identical(a, b):
    for s in range(len(a.best_error)):
        print("seed", s, "best_error", abs(a.best_error[s] - b.best_error[s]), "T",
              a.best_evolution_times[s], b.best_evolution_times[s])
    assert np.array_equal(a.best_error, b.best_error)
    assert np.array_equal(a.best_iteration, b.best_iteration)
    assert np.array_equal(a.iterations_run, b.iterations_run)
    assert np.array_equal(a.best_evolution_times, b.best_evolution_times)
    for s in range(len(a.best_error)):
        assert np.array_equal(a.best_controls[s], b.best_controls[s])
        assert np.array_equal(a.best_final_densities[s], b.best_final_densities[s])
    for key in ("control_scales", "offsets", "rate_scales", "evolution_time_gradients"):
        assert np.array_equal(a.sweep_sensitivities[key], b.sweep_sensitivities[key])


VARIANTS = ("plain", "sine_basis", "control_variation", "complex", "priced", "stopped_seed")


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("optimizer", ["adam", "sgd"])
def test_resident_route_equals_host_loop_with_tau_as_a_parameter(routes, optimizer, variant):
    """Bit for bit: both loops hand the sub-division rule the same control maxima and the same
    tau_b * ||L0_b||, so they launch the same groups. The complex case keeps its bounds where no
    clip acts, as on the plain problem (the host clips the modulus in NumPy, the device in its own
    kernel). With costs of the controls both loops add the value of the engine's kernel
    (LindbladEvaluator._device_control_costs): NumPy's ControlVariation.cost() rounds the same number
    differently, which showed in the last place of best_error."""
    complex_controls = variant == "complex"
    plain, data, head, rng = route_problem(complex_controls=complex_controls)
    K, Nc, costs, T, init, N = head
    start_times = plain.evolution_times.copy()
    kw = dict(max_control_norms=np.full(K, 50.0 if complex_controls else 1.0))
    weight = 0.05 if variant == "priced" else 0.0
    if complex_controls:
        u0 = 0.3 * (rng.standard_normal((B, Nc, K)) + 1j * rng.standard_normal((B, Nc, K)))
        kw["complex_controls"] = True
    elif variant == "sine_basis":
        basis = ControlBasis.sine(Nc, 3)
        u0 = 0.3 * rng.standard_normal((B, 3, K))
        for s in range(B):
            u0[s] *= min(1.0, 0.9 / np.max(np.abs(basis.expand(u0[s]))))
        kw["control_basis"] = basis
    else:
        u0 = np.clip(0.6 * rng.standard_normal((B, Nc, K)), -1, 1)
    if variant == "control_variation":
        head = (K, Nc, costs + [ControlVariation(K, Nc, cost_multiplier=0.4, order=1)], T, init, N)
    w = searching(plain, weight)
    stopped = None
    if variant == "stopped_seed":
        ev = device.LindbladEvaluator(T, init, N, hamiltonian=w, lindblad_data=data,
                                      control_count=K, control_eval_count=Nc, costs=costs)
        errors = ev.evaluate_batch(u0)[0]
        order = np.argsort(errors)
        stopped = int(order[0])
        kw["min_error"] = 0.5 * (errors[order[0]] + errors[order[1]])
    a, b = run_both(routes, optimizer, w, data, head, u0, **kw)
    assert_bit_identical(a, b)
    assert np.any(a.best_iteration > 0)
    started = (start_times / T) * T
    assert np.any(a.best_evolution_times != started)
    lo, hi = w.time_bounds
    assert np.all((a.best_evolution_times >= lo) & (a.best_evolution_times <= hi))
    assert a.sweep_sensitivities["rate_scales"] is not None
    if variant == "sine_basis":
        for s in range(B):
            assert np.array_equal(a.best_coefficients[s], b.best_coefficients[s])
    if stopped is not None:  # stopped by min_error at iteration 0: its tau never moved
        assert a.iterations_run[stopped] == 1 and a.best_iteration[stopped] == 0
        assert a.best_evolution_times[stopped] == started[stopped]
        assert np.any(a.iterations_run > 1)


# ---- 8. the engine's refusals; a fixed sweep afterwards -------------------------------------------------

def set_drift_problem(eng, case, dissipators=None, operators=None, costs=None):
    """The problem of a duration sweep by hand: h0 = 0 and the drift as the one fixed channel."""
    g = gh.lindblad_generators(case) + [case.h0]
    eng.set_lindblad_problem(
        case.n, case.initial_densities.shape[0], len(g), case.Nc, case.N, case.T,
        np.zeros((case.n, case.n), dtype=np.complex128), g,
        case.dissipators if dissipators is None else dissipators,
        case.operators if operators is None else operators, case.initial_densities,
        costs=gh.lindblad_device_costs(case) if costs is None else costs,
        cost_eval_step=case.cost_eval_step)


def test_engine_refusals():
    case = sized_case(*TAGS["n4_l2"])
    K, L = case.K, 2
    tau, ones = np.array([0.7, 1.2]), np.ones((2, 1))
    scales, rates = np.ones((2, K)), np.ones((2, L))
    u = pulses(case, 801, seeds=2)
    eng = Engine(0)
    try:
        setter = eng.lindblad_sweep_set_durations
        good = (tau, None, ones, None, 0.5, 1.5)
        # no sweep; a sweep without rates; a problem whose own h0 is not zero
        set_drift_problem(eng, case)
        with pytest.raises(QocxError, match="no sweep set") as info:
            setter(*good)
        assert info.value.code == ERR_STATE
        with pytest.raises(QocxError, match="no durations set") as info:
            eng.lindblad_sweep_download_durations(want_grad=False)
        assert info.value.code == ERR_STATE
        eng.set_lindblad_sweep(scales, ones, None)
        with pytest.raises(QocxError, match="per-seed rates") as info:
            setter(*good)
        assert info.value.code == ERR_STATE
        gh.setup_lindblad_engine(eng, case)
        eng.set_lindblad_sweep(scales, None, rates)
        with pytest.raises(QocxError, match="h0 is zero") as info:
            setter(tau, None, None, None, 0.5, 1.5)
        assert info.value.code == ERR_STATE
        # five operators
        five = sized_case(4, 5)
        set_drift_problem(eng, five)
        eng.set_lindblad_sweep(scales, ones, np.ones((2, 5)))
        with pytest.raises(QocxError, match="1 .. 4 Lindblad operators") as info:
            setter(*good)
        assert info.value.code == ERR_ARG
        # the box, the price, the durations, the rate factors, the drift channel
        set_drift_problem(eng, case)
        eng.set_lindblad_sweep(scales, ones, rates)
        for bad in ((0.0, 1.5, 0.0), (1.5, 0.5, 0.0), (0.5, np.inf, 0.0), (0.5, 1.5, -1.0),
                    (0.5, 1.5, np.nan)):
            assert code_of(setter, tau, None, ones, None, *bad) == ERR_ARG
        assert code_of(setter, [0.7, np.nan], None, ones, None, 0.5, 1.5) == ERR_ARG
        assert code_of(setter, tau, None, ones, -rates, 0.5, 1.5) == ERR_ARG
        assert code_of(setter, tau, None, None, None, 0.5, 1.5) == ERR_ARG
        # set; gradients need an evaluation with gradients; L-BFGS is refused
        setter(*good)
        assert np.array_equal(eng.lindblad_sweep_download_durations(want_grad=False)[0], tau)
        assert code_of(eng.lindblad_sweep_download_durations) == ERR_STATE
        eng.lindblad_upload_controls(u)
        eng.eval_lindblad_resident(False)
        assert code_of(eng.lindblad_sweep_download_durations) == ERR_STATE
        eng.lindblad_opt_begin()
        with pytest.raises(QocxError, match="duration search") as info:
            eng.lindblad_opt_lbfgs_begin(5)
        assert info.value.code == ERR_STATE
        with pytest.raises(QocxError, match="gradients to step with"):
            eng.lindblad_opt_step(0, np.ones(2, bool), np.ones(2, bool), 0.1)
        eng.eval_lindblad_resident(True)
        assert np.all(np.isfinite(eng.lindblad_sweep_download_durations()[1]))
        # an evaluation with gradients that cannot run two-sided - a second cost, here a step cost -
        # fails by name and leaves no gradient; without gradients it runs
        step_case = cases_mod.lindblad_case_by_name("lindblad_n4")
        assert len(step_case.cost_specs) > 1 and 1 <= len(step_case.dissipators) <= 4
        set_drift_problem(eng, step_case)
        Ls = len(step_case.dissipators)
        eng.set_lindblad_sweep(np.ones((2, step_case.K)), ones, np.ones((2, Ls)))
        setter(*good)
        us = pulses(step_case, 802, seeds=2, amplitude=0.3)
        with pytest.raises(QocxError, match="did not run two-sided") as info:
            eng.evaluate_lindblad(us)
        assert info.value.code == ERR_STATE
        assert code_of(eng.lindblad_sweep_download_durations) == ERR_STATE
        eng.lindblad_upload_controls(us)
        with pytest.raises(QocxError, match="did not run two-sided"):
            eng.eval_lindblad_resident(True)
        assert code_of(eng.lindblad_download_results) == ERR_STATE
        assert code_of(eng.lindblad_sweep_download_durations) == ERR_STATE
        cost = eng.evaluate_lindblad(us, want_grad=False)[0]
        assert np.all(np.isfinite(cost))
        # a new sweep clears the search
        eng.set_lindblad_sweep(np.ones((2, step_case.K)), ones, np.ones((2, Ls)))
        with pytest.raises(QocxError, match="no durations set"):
            eng.lindblad_sweep_download_durations(want_grad=False)
        # stage tables
        td = cases_mod.lindblad_case_by_name("lindblad_timedep")
        device.LindbladEvaluator(
            td.T, td.initial_densities, td.N,
            hamiltonian=LindbladSweep(td.hamiltonian(), control_scales=np.ones((2, td.K))),
            lindblad_data=td.lindblad_data(), control_count=td.K, control_eval_count=td.Nc,
            costs=product_cost_list(td), backend=eng, control_bounds=np.ones(td.K))
        with pytest.raises(QocxError, match="stage tables") as info:
            setter(tau, None, None, None, 0.5, 1.5)
        assert info.value.code == ERR_STATE
    finally:
        eng.close()


def test_a_fixed_duration_sweep_after_a_search_is_what_a_fresh_engine_gives(routes):
    plain, data, head, rng = route_problem()
    K, Nc = head[0], head[1]
    u0 = np.clip(0.6 * rng.standard_normal((B, Nc, K)), -1, 1)
    kw = dict(iteration_count=4, log_iteration_step=0, max_control_norms=np.full(K, 1.0),
              lindblad_data=data)
    shared = Engine(0)
    helpers.set_backend_factory(lambda: shared)
    try:
        searched = qoc_amd.grape_lindblad_discrete_batch(
            *head, u0.copy(), hamiltonian=searching(plain, 0.05),
            optimizer=Adam(learning_rate=5e-2), **kw)
        after = qoc_amd.grape_lindblad_discrete_batch(
            *head, u0.copy(), hamiltonian=plain, optimizer=Adam(learning_rate=5e-2), **kw)
    finally:
        helpers.set_backend_factory(None)
        shared.close()
    fresh = qoc_amd.grape_lindblad_discrete_batch(
        *head, u0.copy(), hamiltonian=plain, optimizer=Adam(learning_rate=5e-2), **kw)
    assert routes == {"resident": 3, "host": 0}
    assert searched.best_evolution_times is not None and after.best_evolution_times is None
    assert np.array_equal(after.best_error, fresh.best_error)
    assert np.array_equal(after.best_iteration, fresh.best_iteration)
    for s in range(B):
        assert np.array_equal(after.best_controls[s], fresh.best_controls[s])
        assert np.array_equal(after.best_final_densities[s], fresh.best_final_densities[s])
    for key in ("control_scales", "offsets", "rate_scales", "evolution_time_gradients"):
        assert np.array_equal(after.sweep_sensitivities[key], fresh.sweep_sensitivities[key])
