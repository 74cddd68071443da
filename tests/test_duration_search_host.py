"""CPU tests of the duration search of a sweep (HamiltonianSweep.durations(time_bounds=...), no GPU):
the constructor's checks, slice, a two-level system whose error and time gradient are known in closed
form, the batch driver's host loop against GRAPE written out by hand on the oracle with the
parameters [u, tau], the clip of tau, a search that finds the pi-pulse time, and the routing of
LBFGS. The stand-in backend is SweepStandIn of tests/test_sweep_host.py with the durations calls in
NumPy, in the order qocx_duration.hip states."""

import numpy as np
import pytest

import qoc_amd
from oracle import qoc_numpy as onp
from qoc_amd.core import batch, device
from qoc_amd.standard import (LBFGS, Adam, ControlNorm, HamiltonianSweep, LindbladSweep,
                              TargetStateInfidelity)
from tests import cases as cases_mod
from tests import helpers
from tests.test_sweep_host import SweepStandIn, _system


class DurationStandIn(SweepStandIn):
    """SweepStandIn plus the duration search: tau clipped to its box, the tables tau * base tables
    (one product each), the gradient g = 0.0; g += s0 * dE/ds (k ascending); g += delta0 * dE/ddelta
    (j ascending); g += weight, and weight * tau added to the cost."""

    def set_sweep(self, scales, offsets):
        super().set_sweep(scales, offsets)
        self.dur = None
        self.tau_grad = None

    def sweep_set_durations(self, tau, base_scales, base_offsets, tau_min, tau_max,
                            time_weight=0.0):
        scales, offsets = self.swp
        tau = np.minimum(np.maximum(np.array(tau, dtype=np.float64), tau_min), tau_max)
        s0 = (np.ones(scales.shape) if base_scales is None
              else np.asarray(base_scales, dtype=np.float64))
        d0 = np.asarray(base_offsets, dtype=np.float64)
        assert s0.shape == scales.shape and d0.shape == offsets.shape and tau.shape == (len(s0),)
        self.dur = (tau, s0, d0, float(time_weight))
        self.swp = (tau[:, None] * s0, tau[:, None] * d0)
        self.tau_grad = None

    def download_results(self, want_grad=True, want_final=True):
        cost, grads, final = super().download_results(want_grad, want_final)
        if self.dur is None:
            return cost, grads, final
        tau, s0, d0, weight = self.dur
        self.tau_grad = None
        if grads is not None:
            ss, os_ = self.sweep_sensitivities()
            g = np.zeros(len(tau))
            for k in range(s0.shape[1]):
                g = g + s0[:, k] * ss[:, k]
            for j in range(d0.shape[1]):
                g = g + d0[:, j] * os_[:, j]
            self.tau_grad = g + weight
        return cost + weight * tau, grads, final

    def sweep_download_durations(self, want_grad=True):
        if want_grad and self.tau_grad is None:
            raise RuntimeError("duration gradients need an evaluation with gradients")
        return self.dur[0].copy(), self.tau_grad.copy() if want_grad else None


class Routes(object):
    """Counts the calls of the two loops of core/batch.py, as tests/test_gpu_sweep.py does."""

    def __enter__(self):
        self.resident = self.host = 0
        self._saved = (batch.run_batch_resident, batch.run_batch_host)

        def resident(*a, **kw):
            self.resident += 1
            return self._saved[0](*a, **kw)

        def host(*a, **kw):
            self.host += 1
            return self._saved[1](*a, **kw)
        batch.run_batch_resident, batch.run_batch_host = resident, host
        return self

    def __exit__(self, *exc):
        batch.run_batch_resident, batch.run_batch_host = self._saved


def _run(backend_factory, *args, **kw):
    helpers.set_backend_factory(backend_factory)
    try:
        return qoc_amd.grape_schroedinger_discrete_batch(*args, **kw)
    finally:
        helpers.set_backend_factory(None)


# ---- the constructor --------------------------------------------------------------------------------

@pytest.mark.parametrize("kw, error, fragment", [
    (dict(time_bounds=(1.0, np.inf)), ValueError, "time_bounds must be finite"),
    (dict(time_bounds=(np.nan, 2.0)), ValueError, "time_bounds must be finite"),
    (dict(time_bounds=(2.0, 1.0)), ValueError, "ordered"),
    (dict(time_bounds=(0.0, 2.0)), ValueError, "ordered"),
    (dict(time_bounds=(1.2, 2.0)), ValueError, "inside time_bounds"),
    (dict(time_bounds=(0.5, 1.4)), ValueError, "inside time_bounds"),
    (dict(time_weight=0.1), ValueError, "time_weight needs time_bounds"),
    (dict(time_bounds=(0.5, 2.0), time_weight=-0.1), ValueError, "time_weight must be finite"),
    (dict(time_bounds=(0.5, 2.0), time_weight=np.nan), ValueError, "time_weight must be finite"),
])
def test_durations_rejects_bad_search_arguments(kw, error, fragment):
    linear, _ = _system()
    with pytest.raises(error, match=fragment):
        HamiltonianSweep.durations(linear, [1.0, 1.5], 1.0, **kw)


def test_a_lindblad_sweep_refuses_the_search_and_says_why():
    linear, _ = _system()
    with pytest.raises(NotImplementedError, match="built on the host from tau_b"):
        LindbladSweep.durations(linear, [1.0, 1.5], 1.0, time_bounds=(0.5, 2.0))
    assert LindbladSweep.durations(linear, [1.0, 1.5], 1.0).searches_duration is False


def test_a_backend_without_the_call_is_refused_before_it_sees_a_problem():
    n, K, N, Nc = 4, 2, 7, 4
    linear, _ = _system(n, K)
    w = HamiltonianSweep.durations(linear, [0.5, 1.0], 1.0, time_bounds=(0.2, 2.0))
    psi0 = cases_mod.column_states(np.eye(n)[:, :1])
    backend = SweepStandIn()
    with pytest.raises(NotImplementedError, match="sweep_set_durations"):
        device.SchroedingerEvaluator(1.0, w, psi0, N, control_count=K, control_eval_count=Nc,
                                     costs=[TargetStateInfidelity(psi0)], backend=backend)
    assert backend.received == [] and not hasattr(backend, "dims")


def test_the_sweep_carries_the_search_and_slice_keeps_it():
    linear, _ = _system()
    times = np.array([0.6, 1.0, 1.7])
    plain = HamiltonianSweep.durations(linear, times, 2.0)
    assert plain.searches_duration is False and plain.time_bounds is None
    assert "searches_duration" not in vars(plain) and "time_bounds" not in vars(plain)
    w = HamiltonianSweep.durations(linear, times, 2.0, time_bounds=(0.5, 3), time_weight=0.25)
    assert w.searches_duration is True and w.time_bounds == (0.5, 3.0) and w.time_weight == 0.25
    assert w.tau_bounds == (0.25, 1.5)
    for name in ("offsets", "evolution_times", "_tau", "_user_offsets"):  # otherwise the plain sweep
        assert np.array_equal(getattr(w, name), getattr(plain, name))
    part = w.slice(1, 3)
    assert part.searches_duration and part.time_bounds == (0.5, 3.0) and part.time_weight == 0.25
    assert np.array_equal(part.evolution_times, times[1:])
    u = np.array([0.3, -0.2])
    assert np.array_equal(w.member(2)(u, 0.0), plain.member(2)(u, 0.0))  # the starting duration


# ---- the two-level known answer -----------------------------------------------------------------------

SX = np.array([[0, 1], [1, 0]], dtype=np.complex128)
OMEGA = 1.0


def two_level(u, t):
    return (OMEGA / 2) * u[0] * SX


def two_level_evaluator(times, reference_time, backend, bounds=(0.5, 4.0), weight=0.0, N=11,
                        Nc=5):
    w = HamiltonianSweep.durations(two_level, times, reference_time, time_bounds=bounds,
                                   time_weight=weight)
    psi0 = cases_mod.column_states(np.eye(2)[:, :1])
    target = cases_mod.column_states(np.eye(2)[:, 1:])
    return device.SchroedingerEvaluator(
        reference_time, w, psi0, N, control_count=1, control_eval_count=Nc,
        costs=[TargetStateInfidelity(target)], backend=backend)


@pytest.mark.parametrize("weight", [0.0, 0.3])
def test_two_level_errors_and_time_gradients_are_the_closed_form(weight):
    """|0> -> |1> under (Omega / 2) u sigma_x with u = 1: the error after T is cos^2(Omega T / 2)
    and its derivative -(Omega / 2) sin(Omega T); a step of a constant H under M2 is exact."""
    times, ref = np.array([1.2, 2.0, 2.6]), 2.0
    ev = two_level_evaluator(times, ref, DurationStandIn(), weight=weight)
    with pytest.raises(ValueError, match="evaluation with gradients"):
        ev.evolution_time_gradients()
    errors, _, _, _ = ev.evaluate_batch(np.ones((3, 5, 1)))
    want = np.cos(OMEGA * times / 2) ** 2 + weight * times / ref
    want_grad = -(OMEGA / 2) * np.sin(OMEGA * times) + weight / ref
    print("errors", errors - want, "gradients", ev.evolution_time_gradients() - want_grad)
    assert np.max(np.abs(errors - want)) < 1e-9
    assert np.max(np.abs(ev.evolution_time_gradients() - want_grad)) < 1e-9
    assert np.array_equal(ev.evolution_times(), times)
    ev.set_evolution_times([0.1, 2.0, 9.0])  # clipped to the box
    assert np.array_equal(ev.evolution_times(), [0.5, 2.0, 4.0])
    errors, _, _, _ = ev.evaluate_batch(np.ones((3, 5, 1)), want_grad=False)
    clipped = np.array([0.5, 2.0, 4.0])
    assert np.max(np.abs(errors - np.cos(clipped / 2) ** 2 - weight * clipped / ref)) < 1e-9
    with pytest.raises(ValueError, match="evaluation with gradients"):
        ev.evolution_time_gradients()


def test_the_price_of_time_is_added_after_the_costs_of_the_controls():
    n, K, N, Nc, B, T = 4, 2, 7, 4, 3, 0.6
    linear, rng = _system(n, K, seed=5)
    times = T * np.array([0.7, 1.0, 1.2])
    psi0 = cases_mod.column_states(np.eye(n)[:, :1])
    target = cases_mod.column_states(np.roll(np.eye(n), 1, axis=0)[:, :1])
    norm = ControlNorm(K, Nc, cost_multiplier=0.3)
    kw = dict(control_count=K, control_eval_count=Nc, backend=None)
    u = 0.4 * rng.standard_normal((B, Nc, K))
    out = {}
    for weight in (0.0, 0.2):
        w = HamiltonianSweep.durations(linear, times, T, time_bounds=(0.1, 2.0),
                                       time_weight=weight)
        kw["backend"] = DurationStandIn()
        ev = device.SchroedingerEvaluator(T, w, psi0, N, costs=[TargetStateInfidelity(target), norm],
                                          **kw)
        out[weight] = (ev.evaluate_batch(u)[0], ev.duration_gradients())
    tau = times / T
    assert np.array_equal(out[0.2][0], out[0.0][0] + 0.2 * tau)  # (state + controls) + time
    assert np.array_equal(out[0.2][1], out[0.0][1] + 0.2)


# ---- the batch driver ---------------------------------------------------------------------------------

def _search_problem(weight=0.0):
    n, K, N, Nc, T = 4, 2, 9, 5, 0.8
    linear, rng = _system(n, K, seed=9)
    times = T * np.array([0.5, 1.0, 1.3])
    w = HamiltonianSweep.durations(linear, times, T, time_bounds=(0.3 * T, 1.5 * T),
                                   time_weight=weight)
    psi0 = cases_mod.column_states(np.eye(n)[:, :2])
    target = cases_mod.column_states(cases_mod.random_unitary(rng, n)[:, :2])
    u0 = np.clip(0.4 * rng.standard_normal((3, Nc, K)), -0.9, 0.9)
    return linear, w, (n, K, N, Nc, T), psi0, target, u0


@pytest.mark.parametrize("weight", [0.0, 0.15])
def test_host_loop_is_grape_by_hand_on_the_parameters_u_and_tau(weight):
    """Seed b by hand: the plain (K + 1)-channel problem r -> sum_k r_k G_k + r_K H0 on the oracle at
    r = [tau u, tau], the chain rule to (u, tau), Adam on the vector [u, tau]."""
    linear, w, (n, K, N, Nc, T), psi0, target, u0 = _search_problem(weight)
    iterations, adam = 5, Adam()
    result = _run(DurationStandIn, K, Nc, [TargetStateInfidelity(target)], T, w, psi0, N, u0,
                  iteration_count=iterations, log_iteration_step=0, optimizer=adam)
    zero = np.zeros(K)

    def wide(r, t):  # the last channel is the drift
        return linear(r[:K], t) - linear(zero, t) + r[K] * linear(zero, t)

    problem = onp.SchroedingerProblem(T, wide, psi0, N, control_eval_count=Nc,
                                      costs=[onp.TargetStateInfidelity(target)],
                                      control_count=K + 1)
    lo, hi = w.tau_bounds
    moved = False
    for b in range(3):
        x = np.concatenate([u0[b].reshape(-1), [w.evolution_times[b] / T]])
        m, v = np.zeros_like(x), np.zeros_like(x)
        best = (np.inf, None, None, -1)
        for it in range(iterations):
            u = x[:-1].reshape(Nc, K)
            np.clip(u, -1.0, 1.0, out=u)  # max_control_norms default to 1: in place
            x[-1] = min(max(x[-1], lo), hi)
            tau = x[-1]
            r = np.concatenate([tau * u, np.full((Nc, 1), tau)], axis=1)
            error, g, _ = onp.evaluate_with_grad(problem, r)
            g = np.real(g)
            error = error + weight * tau
            if error < best[0]:
                best = (error, u.copy(), tau, it)
            grad = np.concatenate([(tau * g[:, :K]).reshape(-1),
                                   [np.sum(u * g[:, :K]) + np.sum(g[:, K]) + weight]])
            m = adam.beta_1 * m + (1 - adam.beta_1) * grad
            v = adam.beta_2 * v + (1 - adam.beta_2) * grad ** 2
            m_hat, v_hat = m / (1 - adam.beta_1 ** (it + 1)), v / (1 - adam.beta_2 ** (it + 1))
            x = x - adam.learning_rate * m_hat / (np.sqrt(v_hat) + adam.epsilon)
        assert result.best_iteration[b] == best[3]
        assert abs(result.best_error[b] - best[0]) < 1e-12
        assert np.max(np.abs(result.best_controls[b] - best[1])) < 1e-10
        assert abs(result.best_evolution_times[b] - best[2] * T) < 1e-12
        moved = moved or result.best_evolution_times[b] != w.evolution_times[b]
    assert moved
    sens = result.sweep_sensitivities  # at the best controls AND the best durations
    ev = device.SchroedingerEvaluator(T, w, psi0, N, control_count=K, control_eval_count=Nc,
                                      costs=[TargetStateInfidelity(target)],
                                      backend=DurationStandIn())
    ev.set_evolution_times(result.best_evolution_times)
    ev.evaluate_batch(np.stack(result.best_controls))
    again = ev.sweep_sensitivities()
    for key in ("control_scales", "offsets", "evolution_time_gradients"):
        assert np.max(np.abs(sens[key] - again[key])) < 1e-12


def test_tau_is_clipped_in_place_every_iteration():
    """Seed 0 starts at T_max with a gradient that points outward (the error falls with T there):
    every step moves tau past the box, every iteration evaluates it at T_max exactly."""
    seen = []

    class Recording(DurationStandIn):
        def sweep_set_durations(self, tau, *a, **kw):
            super().sweep_set_durations(tau, *a, **kw)
            seen.append((np.array(tau), self.dur[0].copy()))

    ref = 2.0
    w = HamiltonianSweep.durations(two_level, [2.0, 1.5], ref, time_bounds=(1.0, 2.0))
    psi0 = cases_mod.column_states(np.eye(2)[:, :1])
    target = cases_mod.column_states(np.eye(2)[:, 1:])
    result = _run(Recording, 1, 5, [TargetStateInfidelity(target)], ref, w, psi0, 11,
                  np.ones((2, 5, 1)), iteration_count=6, log_iteration_step=0,
                  optimizer=Adam(learning_rate=0.05))
    in_loop = seen[1:7]  # (the first call is the evaluator's own, the last the sensitivities')
    assert len(seen) == 8
    for given, kept in in_loop:
        assert given[0] == 1.0 and kept[0] == 1.0  # handed over already clipped: tau_max exactly
        assert 0.5 <= kept[1] <= 1.0
    assert in_loop[-1][1][1] > in_loop[0][1][1]  # the free seed moves towards longer times
    assert result.best_evolution_times[0] == 2.0
    assert result.best_evolution_times[1] > 1.5


def test_the_search_finds_the_pi_pulse_time():
    """u is saturated at max_control_norms = 1, so a fixed T = 2 cannot do better than cos^2(1); the
    search lengthens the pulse towards T = pi, where the error vanishes."""
    ref = 2.0
    psi0 = cases_mod.column_states(np.eye(2)[:, :1])
    target = cases_mod.column_states(np.eye(2)[:, 1:])
    args = (1, 5, [TargetStateInfidelity(target)], ref)
    kw = dict(iteration_count=40, log_iteration_step=0, optimizer=Adam(learning_rate=0.05),
              max_control_norms=np.array([1.0]))
    fixed = _run(SweepStandIn, *args, HamiltonianSweep.durations(two_level, [2.0], ref), psi0, 11,
                 np.ones((1, 5, 1)), **kw)
    search = _run(DurationStandIn, *args,
                  HamiltonianSweep.durations(two_level, [2.0], ref, time_bounds=(1.0, 5.0)),
                  psi0, 11, np.ones((1, 5, 1)), **kw)
    print("fixed", fixed.best_error, "search", search.best_error, search.best_evolution_times)
    assert abs(fixed.best_error[0] - np.cos(1.0) ** 2) < 1e-9
    assert search.best_error[0] < 0.1 * fixed.best_error[0]
    assert abs(search.best_evolution_times[0] - np.pi) < 0.5
    assert fixed.best_evolution_times is None


def test_lbfgs_with_a_search_takes_the_host_loop_and_lowers_the_error():
    linear, w, (n, K, N, Nc, T), psi0, target, u0 = _search_problem()

    class ResidentLooking(DurationStandIn):
        """Everything resident_route asks a backend for - so only the search keeps LBFGS off it."""
        opt_step = opt_begin_complex = opt_lbfgs_step = set_control_costs = None

    args = (K, Nc, [TargetStateInfidelity(target)], T, w, psi0, N, u0)
    with Routes() as routes:
        result = _run(ResidentLooking, *args, iteration_count=8, log_iteration_step=0,
                      optimizer=LBFGS())
    assert (routes.resident, routes.host) == (0, 1)
    start = _run(DurationStandIn, *args, iteration_count=1, log_iteration_step=0,
                 optimizer=LBFGS())
    print("LBFGS", start.best_error, "->", result.best_error)
    assert np.all(result.best_error < start.best_error)
    assert np.all(np.isfinite(result.best_evolution_times))
    lo, hi = w.time_bounds
    assert np.all((result.best_evolution_times >= lo) & (result.best_evolution_times <= hi))
    # ... while the same backend with Adam would have been given the resident loop
    pstate = type("P", (), dict(impose_control_conditions=None, duration_search=object()))()
    ev = device.SchroedingerEvaluator(T, w, psi0, N, control_count=K, control_eval_count=Nc,
                                      costs=[TargetStateInfidelity(target)],
                                      backend=ResidentLooking())
    params = np.zeros((3, Nc * K))
    assert batch.resident_route(batch.batched_stepper(Adam(), params), Adam(), pstate, ev, 3)
    assert not batch.resident_route(batch.batched_stepper(LBFGS(), params), LBFGS(), pstate, ev, 3)
    pstate.duration_search = None
    assert batch.resident_route(batch.batched_stepper(LBFGS(), params), LBFGS(), pstate, ev, 3)
