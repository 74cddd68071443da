"""CPU tests of the duration search of a Lindblad sweep (LindbladSweep.duration_search, no GPU): the
constructors' checks, the refusals of LindbladEvaluator before a backend sees anything, slice, the
batch driver's host loop against GRAPE written out by hand on the parameters [u, tau] with the
fixed-duration sweep as its evaluation, the clip of tau, the routing of LBFGS and the price of time.
The stand-in backend is LindbladSweepStandIn of tests/lindblad_sweep_model.py with the three durations
calls in NumPy, in the order qocx_lindblad_duration.hip states."""

import os
import re

import numpy as np
import pytest

import qoc_amd
from qoc_amd import engine
from qoc_amd.core import batch, device
from qoc_amd.standard import (LBFGS, Adam, ControlBandwidthMax, ControlNorm, ForbidDensities,
                              HamiltonianSweep, LindbladSweep, TargetDensityInfidelity)
from tests import helpers
from tests.lindblad_sweep_model import LindbladSweepStandIn
from tests.test_duration_search_host import Routes
from tests.test_lindblad_sweep_host import _densities, _open_system
from tests.test_sweep_host import _system

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class LindbladDurationStandIn(LindbladSweepStandIn):
    """LindbladSweepStandIn plus the duration search: tau clipped to its box, the three tables tau *
    base tables (one product each), rate sensitivities in every evaluation with gradients, the
    gradient g = 0.0; g += s0 * dE/ds (k ascending); g += delta0 * dE/ddelta (j ascending);
    g += c0 * dE/dc (l ascending); g += weight, and weight * tau added to the cost."""

    def set_lindblad_sweep(self, scales, offsets, rate_scales=None):
        super().set_lindblad_sweep(scales, offsets, rate_scales)
        self.dur = None
        self.tau_grad = None

    def lindblad_sweep_set_durations(self, tau, base_scales, base_offsets, base_rate_scales,
                                     tau_min, tau_max, time_weight=0.0):
        self.log.append("lindblad_sweep_set_durations")
        scales, offsets, rates = self.swp
        assert rates is not None, "a duration search needs per-seed rates"
        tau = np.minimum(np.maximum(np.array(tau, dtype=np.float64), tau_min), tau_max)
        s0 = (np.ones(scales.shape) if base_scales is None
              else np.asarray(base_scales, dtype=np.float64))
        d0 = np.asarray(base_offsets, dtype=np.float64)
        c0 = (np.ones(rates.shape) if base_rate_scales is None
              else np.asarray(base_rate_scales, dtype=np.float64))
        assert s0.shape == scales.shape and d0.shape == offsets.shape and c0.shape == rates.shape
        assert tau.shape == (len(s0),)
        self.dur = (tau, s0, d0, c0, float(time_weight))
        self.swp = (tau[:, None] * s0, tau[:, None] * d0, tau[:, None] * c0)
        self.tau_grad = None

    def evaluate_lindblad(self, controls, want_grad=True, want_final=True):
        if getattr(self, "dur", None) is None:
            return super().evaluate_lindblad(controls, want_grad, want_final)
        asked, self.want_rates = self.want_rates, True
        try:
            cost, grads, final = super().evaluate_lindblad(controls, want_grad, want_final)
        finally:
            self.want_rates = asked
        tau, s0, d0, c0, weight = self.dur
        self.tau_grad = None
        if grads is not None:
            log = len(self.log)
            ss, os_, rs = self.lindblad_sweep_sensitivities()
            del self.log[log:]
            g = np.zeros(len(tau))
            for k in range(s0.shape[1]):
                g = g + s0[:, k] * ss[:, k]
            for j in range(d0.shape[1]):
                g = g + d0[:, j] * os_[:, j]
            for l in range(c0.shape[1]):
                g = g + c0[:, l] * rs[:, l]
            self.tau_grad = g + weight
        return cost + weight * tau, grads, final

    def lindblad_sweep_download_durations(self, want_grad=True):
        if want_grad and self.tau_grad is None:
            raise RuntimeError("duration gradients need an evaluation with gradients")
        return self.dur[0].copy(), self.tau_grad.copy() if want_grad else None

    def lindblad_opt_download_best_durations(self):
        raise AssertionError("the stand-in has no resident driver")


def _run(backend_factory, *args, **kw):
    helpers.set_backend_factory(backend_factory)
    try:
        return qoc_amd.grape_lindblad_discrete_batch(*args, **kw)
    finally:
        helpers.set_backend_factory(None)


# ---- the constructors ---------------------------------------------------------------------------------

@pytest.mark.parametrize("bounds, kw, fragment", [
    ((1.0, np.inf), {}, "time_bounds must be finite"),
    ((np.nan, 2.0), {}, "time_bounds must be finite"),
    ((2.0, 1.0), {}, "ordered"),
    ((0.0, 2.0), {}, "ordered"),
    ((1.2, 2.0), {}, "inside time_bounds"),
    ((0.5, 1.4), {}, "inside time_bounds"),
    (None, {}, "time_bounds must be"),
    ((0.5, 2.0), dict(time_weight=-0.1), "time_weight must be finite"),
    ((0.5, 2.0), dict(time_weight=np.nan), "time_weight must be finite"),
    ((0.5, 2.0), dict(rate_scales=-np.ones((2, 2))), "rate_scales must be >= 0"),
    ((0.5, 2.0), dict(rate_scales=np.ones((3, 2))), "rate_scales are for 3 seeds"),
])
def test_duration_search_rejects_bad_arguments(bounds, kw, fragment):
    linear, _ = _system()
    with pytest.raises(ValueError, match=fragment):
        LindbladSweep.duration_search(linear, [1.0, 1.5], 1.0, bounds, **kw)


def test_the_hamiltonian_alias_builds_what_durations_builds():
    linear, rng = _system()
    times, s0 = np.array([0.6, 1.0, 1.7]), 1 + 0.1 * rng.standard_normal((3, 2))
    a = HamiltonianSweep.duration_search(linear, times, 2.0, (0.5, 3), 0.25, control_scales=s0)
    b = HamiltonianSweep.durations(linear, times, 2.0, control_scales=s0, time_bounds=(0.5, 3),
                                   time_weight=0.25)
    assert type(a) is HamiltonianSweep and a.searches_duration
    assert set(vars(a)) == set(vars(b))
    for name, value in vars(b).items():
        if callable(value):
            continue
        got = getattr(a, name)
        assert (np.array_equal(got, value) if isinstance(value, np.ndarray) else got == value), name
    u = np.array([0.3, -0.2])
    assert np.array_equal(a.member(1)(u, 0.0), b.member(1)(u, 0.0))
    with pytest.raises(ValueError, match="time_bounds must be"):
        HamiltonianSweep.duration_search(linear, times, 2.0, None)


def test_durations_still_refuses_time_bounds_and_names_the_new_constructor():
    linear, _ = _system()
    with pytest.raises(NotImplementedError, match="built on the host from tau_b") as info:
        LindbladSweep.durations(linear, [1.0, 1.5], 1.0, time_bounds=(0.5, 2.0))
    assert "LindbladSweep.duration_search" in str(info.value)
    with pytest.raises(NotImplementedError, match="duration_search"):
        LindbladSweep.durations(linear, [1.0, 1.5], 1.0, time_weight=0.1)


def test_the_sweep_carries_the_search_and_slice_keeps_it_with_the_rates():
    linear, _ = _system()
    times = np.array([0.6, 1.0, 1.7])
    c0 = np.array([[1.0, 1.0], [0.5, 2.0], [1.5, 0.7]])
    plain = LindbladSweep.durations(linear, times, 2.0, rate_scales=c0)
    w = LindbladSweep.duration_search(linear, times, 2.0, (0.5, 3), 0.25, rate_scales=c0)
    assert isinstance(w, LindbladSweep) and w.searches_duration and not plain.searches_duration
    assert w.time_bounds == (0.5, 3.0) and w.time_weight == 0.25 and w.tau_bounds == (0.25, 1.5)
    for name in ("offsets", "evolution_times", "_tau", "_user_offsets", "rate_scales",
                 "_user_rates"):  # otherwise the fixed sweep
        assert np.array_equal(getattr(w, name), getattr(plain, name))
    assert np.array_equal(w.base_rates(2), c0)
    assert LindbladSweep.duration_search(linear, times, 2.0, (0.5, 3)).base_rates(2) is None
    with pytest.raises(ValueError, match=r"\(B, L\) with L = 3"):
        w.base_rates(3)
    part = w.slice(1, 3)
    assert part.searches_duration and part.time_bounds == (0.5, 3.0) and part.time_weight == 0.25
    assert np.array_equal(part.evolution_times, times[1:])
    assert np.array_equal(part.rate_scales, w.rate_scales[1:])
    assert np.array_equal(part.base_rates(2), c0[1:])

    class Comm(object):
        rank, world = 1, 2
    ranked = batch.rank_sweep(w, 3, Comm())
    assert ranked.searches_duration and ranked.seed_count == 1
    assert np.array_equal(ranked.base_rates(2), c0[2:])


# ---- refusals before the backend receives anything ----------------------------------------------------

def test_the_evaluator_refuses_what_cannot_run_two_sided_before_the_backend_sees_it():
    n, K, N, Nc, T = 4, 2, 6, 4, 0.8
    linear, data, gammas, ops, rng = _open_system(n, K)
    init, targ = _densities(n, rng)
    target = TargetDensityInfidelity(targ)
    w = LindbladSweep.duration_search(linear, [0.5, 1.0], T, (0.2, 2.0))

    def refused(fragment, costs=(target,), data=data, sweep=w, backend=None):
        backend = LindbladDurationStandIn() if backend is None else backend
        with pytest.raises(NotImplementedError, match=fragment):
            device.LindbladEvaluator(T, init, N, hamiltonian=sweep, lindblad_data=data,
                                     control_count=K, control_eval_count=Nc, costs=list(costs),
                                     backend=backend)
        assert backend.log == [] and backend.received == []

    refused("exactly one cost of the densities", costs=(target, target))
    refused("exactly one cost of the densities", costs=())
    refused("exactly one cost of the densities", costs=(ForbidDensities(targ[:, None], N),))
    refused("exactly one cost of the densities",
            costs=(target, ForbidDensities(targ[:, None], N)))
    refused("use the\\s+Schroedinger search", data=lambda t: (np.zeros(0), np.zeros((0, n, n))))
    five = np.stack([ops[0]] * 5)
    refused("1 to 4 Lindblad operators", data=lambda t: (np.full(5, 0.1), five))
    refused("ControlBandwidthMax", costs=(target, ControlBandwidthMax(K, Nc, T, np.full(K, 5.0))))
    refused("lindblad_sweep_set_durations", backend=LindbladSweepStandIn())
    moving, *_ = _open_system(n, K, time_dependent=True)
    refused("time-independent system",
            sweep=LindbladSweep.duration_search(moving, [0.5, 1.0], T, (0.2, 2.0)))
    # ... and what it takes: the one cost, with a cost of the controls beside it
    backend = LindbladDurationStandIn()
    ev = device.LindbladEvaluator(T, init, N, hamiltonian=w, lindblad_data=data, control_count=K,
                                  control_eval_count=Nc, costs=[target, ControlNorm(K, Nc)],
                                  backend=backend)
    assert backend.log == ["set_lindblad_problem", "set_lindblad_sweep",
                           "lindblad_sweep_set_durations"]
    assert np.array_equal(ev.evolution_times(), [0.5, 1.0])
    with pytest.raises(ValueError, match="evaluation with gradients"):
        ev.duration_gradients()
    plain = device.LindbladEvaluator(
        T, init, N, hamiltonian=LindbladSweep.durations(linear, [0.5, 1.0], T), lindblad_data=data,
        control_count=K, control_eval_count=Nc, costs=[target], backend=LindbladDurationStandIn())
    with pytest.raises(ValueError, match="duration search"):
        plain.set_durations([1.0, 1.0])


# ---- the batch driver ---------------------------------------------------------------------------------

def _search_problem(weight=0.0, seed=9):
    n, K, N, Nc, B, T = 4, 2, 6, 4, 3, 0.8
    linear, data, gammas, ops, rng = _open_system(n, K, seed=seed)
    c0 = np.array([[1.0, 1.0], [0.5, 2.0], [1.5, 0.7]])
    s0 = 1 + 0.1 * rng.standard_normal((B, K))
    times = T * np.array([0.5, 1.0, 1.3])
    w = LindbladSweep.duration_search(linear, times, T, (0.3 * T, 1.5 * T), weight,
                                      control_scales=s0, rate_scales=c0)
    init, targ = _densities(n, rng)
    u0 = np.clip(0.4 * rng.standard_normal((B, Nc, K)), -0.9, 0.9)
    return linear, data, w, (s0, c0), (K, Nc, [TargetDensityInfidelity(targ)], T, init, N), u0


@pytest.mark.parametrize("weight", [0.0, 0.15])
def test_host_loop_is_grape_by_hand_on_the_parameters_u_and_tau(weight):
    """Seed b by hand: every iteration evaluates the FIXED-duration sweep of that one seed at the
    current tau (LindbladSweep.durations on the plain stand-in, rate sensitivities on), takes
    dE/dtau = T * evolution_time_gradients from it, and steps Adam on the vector [u, tau]."""
    linear, data, w, (s0, c0), head, u0 = _search_problem(weight)
    K, Nc, costs, T, init, N = head
    iterations, adam = 4, Adam()
    result = _run(LindbladDurationStandIn, *head, u0, hamiltonian=w, lindblad_data=data,
                  iteration_count=iterations, log_iteration_step=0, optimizer=adam)
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
            one = LindbladSweep.durations(linear, [tau * T], T, control_scales=s0[b:b + 1],
                                          rate_scales=c0[b:b + 1])
            ev = device.LindbladEvaluator(T, init, N, hamiltonian=one, lindblad_data=data,
                                          control_count=K, control_eval_count=Nc, costs=costs,
                                          backend=LindbladSweepStandIn())
            ev.want_rate_sensitivities(True)
            errors, grads, _, _ = ev.evaluate_batch(u[None])
            tau_grad = ev.sweep_sensitivities()["evolution_time_gradients"][0] * T + weight
            error = errors[0] + weight * tau
            if error < best[0]:
                best = (error, u.copy(), tau, it)
            grad = np.concatenate([grads[0].reshape(-1), [tau_grad]])
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
    ev = device.LindbladEvaluator(T, init, N, hamiltonian=w, lindblad_data=data, control_count=K,
                                  control_eval_count=Nc, costs=costs,
                                  backend=LindbladDurationStandIn())
    ev.set_evolution_times(result.best_evolution_times)
    ev.evaluate_batch(np.stack(result.best_controls))
    again = ev.sweep_sensitivities()
    for key in ("control_scales", "offsets", "rate_scales", "evolution_time_gradients"):
        assert np.max(np.abs(sens[key] - again[key])) < 1e-12
    # evolution_time_gradients of the evaluator: the sweep's own plus the price of time
    assert np.max(np.abs(ev.evolution_time_gradients()
                         - (again["evolution_time_gradients"] + weight / T))) < 1e-12


def test_tau_is_clipped_in_place_every_iteration():
    """The excited state decays and the target IS the excited state, so the error grows with T and the
    gradient points below the box for seed 0, which starts at T_min: every step moves tau past the
    box, every iteration evaluates it at T_min exactly."""
    seen = []

    class Recording(LindbladDurationStandIn):
        def lindblad_sweep_set_durations(self, tau, *a, **kw):
            super().lindblad_sweep_set_durations(tau, *a, **kw)
            seen.append((np.array(tau), self.dur[0].copy()))

    sz = np.diag([1.0, -1.0]).astype(np.complex128)
    lower = np.array([[0, 1], [0, 0]], dtype=np.complex128)
    w = LindbladSweep.duration_search(lambda u, t: u[0] * sz, [0.5, 1.5], 1.0, (0.5, 4.0))
    excited = np.diag([0.0, 1.0]).astype(np.complex128)[None]
    iterations = 5
    result = _run(Recording, 1, 3, [TargetDensityInfidelity(excited)], 1.0, excited, 5,
                  np.zeros((2, 3, 1)), hamiltonian=w,
                  lindblad_data=lambda t: (np.array([0.7]), lower[None]),
                  iteration_count=iterations, log_iteration_step=0,
                  optimizer=Adam(learning_rate=0.05))
    # (the first call is the evaluator's own, the last the sensitivities')
    assert len(seen) == iterations + 2
    in_loop = seen[1:iterations + 1]
    for given, kept in in_loop:
        assert given[0] == 0.5 and kept[0] == 0.5  # handed over already clipped: T_min exactly
        assert 0.5 <= kept[1] <= 1.5
    assert in_loop[-1][1][1] < in_loop[0][1][1]  # the free seed moves towards shorter times
    assert result.best_evolution_times[0] == 0.5
    assert result.best_evolution_times[1] < 1.5


def test_lbfgs_with_a_search_takes_the_host_loop_and_lowers_the_error():
    linear, data, w, _, head, u0 = _search_problem()
    K, Nc, costs, T, init, N = head

    class ResidentLooking(LindbladDurationStandIn):
        """Everything resident_route asks a backend for - so only the search keeps LBFGS off it."""
        lindblad_opt_step = lindblad_opt_begin_complex = lindblad_opt_lbfgs_step = None
        set_control_costs = None

    kw = dict(hamiltonian=w, lindblad_data=data, log_iteration_step=0, optimizer=LBFGS())
    with Routes() as routes:
        result = _run(ResidentLooking, *head, u0, iteration_count=6, **kw)
    assert (routes.resident, routes.host) == (0, 1)
    start = _run(LindbladDurationStandIn, *head, u0, iteration_count=1, **kw)
    print("LBFGS", start.best_error, "->", result.best_error)
    assert np.all(result.best_error < start.best_error)
    lo, hi = w.time_bounds
    assert np.all((result.best_evolution_times >= lo) & (result.best_evolution_times <= hi))
    # ... while the same backend with Adam would have been given the resident loop
    ev = device.LindbladEvaluator(T, init, N, hamiltonian=w, lindblad_data=data, control_count=K,
                                  control_eval_count=Nc, costs=costs, backend=ResidentLooking())
    pstate = type("P", (), dict(impose_control_conditions=None, duration_search=ev))()
    params = np.zeros((3, Nc * K))
    assert batch.resident_route(batch.batched_stepper(Adam(), params), Adam(), pstate, ev, 3)
    assert not batch.resident_route(batch.batched_stepper(LBFGS(), params), LBFGS(), pstate, ev, 3)


def test_best_error_includes_the_price_of_time_added_after_the_costs_of_the_controls():
    linear, data, _, (s0, c0), head, u0 = _search_problem()
    K, Nc, costs, T, init, N = head
    costs = costs + [ControlNorm(K, Nc, cost_multiplier=0.3)]
    times = T * np.array([0.5, 1.0, 1.3])
    out = {}
    for weight in (0.0, 0.2):
        w = LindbladSweep.duration_search(linear, times, T, (0.3 * T, 1.5 * T), weight,
                                          control_scales=s0, rate_scales=c0)
        ev = device.LindbladEvaluator(T, init, N, hamiltonian=w, lindblad_data=data,
                                      control_count=K, control_eval_count=Nc, costs=costs,
                                      backend=LindbladDurationStandIn())
        out[weight] = (ev.evaluate_batch(u0)[0], ev.duration_gradients())
    tau = times / T
    assert np.array_equal(out[0.2][0], out[0.0][0] + 0.2 * tau)  # (state + controls) + time
    assert np.array_equal(out[0.2][1], out[0.0][1] + 0.2)
    # one iteration of the driver: its best error is that of the starting point, price included
    w = LindbladSweep.duration_search(linear, times, T, (0.3 * T, 1.5 * T), 0.2,
                                      control_scales=s0, rate_scales=c0)
    result = _run(LindbladDurationStandIn, K, Nc, costs, T, init, N, u0, hamiltonian=w,
                  lindblad_data=data, iteration_count=1, log_iteration_step=0, optimizer=Adam())
    assert np.array_equal(result.best_error, out[0.2][0])
    assert np.array_equal(result.best_evolution_times, tau * T)


def test_a_search_takes_the_costs_of_the_controls_from_a_backend_that_evaluates_them():
    """Where the resident route could run, evaluate_batch adds the costs of the controls as that route
    does: the backend's own evaluation of the descriptors, set for the call and cleared after it, one
    sum onto the error and one onto the gradient, the price of time after them. A fixed-duration sweep
    on the same backend, and a search on a backend without the calls, keep NumPy's cost()."""
    linear, data, w, (s0, c0), head, u0 = _search_problem(0.2)
    K, Nc, costs, T, init, N = head
    norm = ControlNorm(K, Nc, cost_multiplier=0.3)

    class Costing(LindbladDurationStandIn):
        lindblad_opt_step = lindblad_opt_begin_complex = None  # (what resident_capable asks for)

        def set_control_costs(self, path, complex_controls, descriptors):
            self.log.append("set_control_costs %d" % len(descriptors))

        def eval_control_costs(self, path, controls, want_grad=True):
            self.log.append("eval_control_costs grad=%d" % bool(want_grad))
            controls = np.asarray(controls)
            return (np.full(len(controls), 0.125),
                    np.full(controls.shape, 0.5) if want_grad else None)

    def evaluate(sweep, backend, want_grad=True):
        ev = device.LindbladEvaluator(T, init, N, hamiltonian=sweep, lindblad_data=data,
                                      control_count=K, control_eval_count=Nc, costs=costs + [norm],
                                      backend=backend)
        return ev.evaluate_batch(u0, want_grad=want_grad)
    plain = evaluate(w, LindbladDurationStandIn())
    free = _search_problem(0.0)[2]  # (the same sweep without a price: the state cost alone)
    bare = device.LindbladEvaluator(T, init, N, hamiltonian=free, lindblad_data=data, control_count=K,
                                    control_eval_count=Nc, costs=costs,
                                    backend=LindbladDurationStandIn()).evaluate_batch(u0)
    backend = Costing()
    got = evaluate(w, backend)
    assert backend.log[-4:] == ["evaluate_lindblad grad=1", "set_control_costs 1",
                                "eval_control_costs grad=1", "set_control_costs 0"]
    tau = w.evolution_times / T
    assert np.array_equal(got[0], (bare[0] + 0.125) + 0.2 * tau)
    assert np.array_equal(got[1], bare[1] + 0.5)
    assert not np.array_equal(got[0], plain[0])
    backend = Costing()
    assert evaluate(w, backend, want_grad=False)[1] is None
    assert backend.log[-2] == "eval_control_costs grad=0"
    fixed = LindbladSweep.durations(linear, w.evolution_times, T, control_scales=s0, rate_scales=c0)
    backend = Costing()
    evaluate(fixed, backend)
    assert not [entry for entry in backend.log if "control_costs" in entry]


# ---- the ABI ------------------------------------------------------------------------------------------

NEW_SYMBOLS = ("qocx_lindblad_sweep_set_durations", "qocx_lindblad_sweep_download_durations",
               "qocx_lindblad_opt_download_best_durations")


def test_the_new_symbols_are_in_the_header_the_binding_and_the_library():
    header = open(os.path.join(ROOT, "include", "qocx.h")).read()
    lib = engine.load_library()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint %s\(qocx_ctx\* ctx" % name, header), name
        assert name in engine.SIGNATURES and hasattr(lib, name), name
    assert len(engine.SIGNATURES["qocx_lindblad_sweep_set_durations"][1]) == 8
    for name in ("lindblad_sweep_set_durations", "lindblad_sweep_download_durations",
                 "lindblad_opt_download_best_durations"):
        assert callable(getattr(engine.Engine, name))
