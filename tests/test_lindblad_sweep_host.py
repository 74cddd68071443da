"""CPU tests of qoc_amd.standard.LindbladSweep and its host routing (no GPU): construction and the
refusals by name, the algebra of a duration sweep against the oracles, the NumPy
restatement of the rate sensitivities (tests/lindblad_sweep_model.py) against central differences,
evolution_time_gradients against central differences in the duration, both routes of the batch
driver on a stand-in backend, and the new ABI symbols."""

import os
import re

import numpy as np
import pytest

import qoc_amd
from oracle import qoc_lindblad_numpy as ol
from qoc_amd import engine
from qoc_amd.core import device
from qoc_amd.models.cost import Cost
from qoc_amd.standard import (LBFGS, SGD, Adam, ControlBandwidthMax, ControlNorm,
                              HamiltonianEnsemble, HamiltonianSweep, LindbladSweep,
                              QuadraticHamiltonian, TargetDensityInfidelity, TargetStateInfidelity)
from tests import cases as cases_mod
from tests import gpu_helpers as gh
from tests import helpers
from tests import lindblad_model as lm
from tests import lindblad_sweep_model as sm
from tests.lindblad_sweep_model import LindbladSweepStandIn
from tests.oracle_backend import OracleBackend

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _open_system(n=4, K=2, seed=3, complex_controls=False, time_dependent=False, L=2):
    """A decaying oscillator with random drives: (hamiltonian, lindblad_data, gammas, ops, rng)."""
    rng = np.random.default_rng(seed)
    a = cases_mod.annihilation(n)
    ad = a.conj().T
    h0 = 0.6 * cases_mod.gue(rng, n)
    g_re = [0.5 * cases_mod.gue(rng, n) for _ in range(K)]
    g_im = [0.5 * cases_mod.gue(rng, n) for _ in range(K)]
    ops = np.stack([a / np.sqrt(n - 1), ad @ a / (n - 1), (a + 1j * ad @ a) / (n - 1)][:L])
    gammas = np.array([0.3, 0.2, 0.15])[:L]

    def linear(u, t):
        out = h0 * (1 + 0.3 * np.cos(1.7 * t)) if time_dependent else h0
        for k in range(K):
            out = out + (u[k].real * g_re[k] + u[k].imag * g_im[k] if complex_controls
                         else u[k] * g_re[k])
        return out
    return linear, (lambda t: (gammas, ops)), gammas, ops, rng


def _densities(n, rng, S=1):
    init = np.stack([cases_mod.random_density(rng, n) for _ in range(S)])
    targ = np.stack([cases_mod.random_density(rng, n) for _ in range(S)])
    return init, targ


def _evaluator(w, data, init, costs, T=0.8, N=6, K=2, Nc=4, backend=None, **kw):
    return device.LindbladEvaluator(
        T, init, N, hamiltonian=w, lindblad_data=data, control_count=K, control_eval_count=Nc,
        costs=costs, backend=LindbladSweepStandIn() if backend is None else backend, **kw)


# ---- 1. construction and refusals ---------------------------------------------------------------------

def test_construction_reads_the_seed_count_from_any_table_and_slices_the_rates():
    linear, data, gammas, ops, rng = _open_system()
    c = np.array([[0.5, 1.0], [1.0, 2.0], [2.0, 0.25]])
    w = LindbladSweep(linear, rate_scales=c)
    assert isinstance(w, HamiltonianSweep) and w.seed_count == 3 and w.has_rates
    assert w.control_scales is None and w.offsets is None and not w.time_scaled
    assert np.array_equal(w.resolved_rate_scales(2), c)
    d = np.stack([cases_mod.gue(rng, 4)])
    w = LindbladSweep(linear, perturbations=d, offsets=np.array([[0.1], [0.2], [0.3]]),
                      control_scales=np.ones((3, 2)), rate_scales=c)
    assert w.seed_count == 3 and "rate_scales 3x2" in repr(w)
    part = w.slice(1, 3)
    assert isinstance(part, LindbladSweep) and part.seed_count == 2
    assert np.array_equal(part.rate_scales, c[1:]) and np.array_equal(part.offsets, w.offsets[1:])
    gam, op = part.member_lindblad_data(1, data)(0.3)
    assert np.array_equal(gam, c[2] * gammas) and op is ops
    u = rng.standard_normal(2)
    assert np.array_equal(part.member(0)(u, 0.1), w.member(1)(u, 0.1))
    plain = LindbladSweep(linear, control_scales=np.ones((2, 2)))
    assert not plain.has_rates and plain.resolved_rate_scales(2) is None
    assert plain.member_lindblad_data(0, data) is data


@pytest.mark.parametrize("kw, fragment", [
    (dict(rate_scales=np.ones((2, 2)), control_scales=np.ones((3, 2))), "disagree on the seed count"),
    (dict(rate_scales=-np.ones((2, 2))), "rate_scales must be >= 0"),
    (dict(rate_scales=np.array([[1.0, np.inf]])), "rate_scales is not finite"),
    (dict(rate_scales=np.ones(3)), "rate_scales must have 2 dimensions"),
    (dict(rate_scales=np.zeros((0, 2))), "at least one seed"),
    (dict(), "needs offsets or control_scales"),
])
def test_constructor_rejects_bad_arguments(kw, fragment):
    with pytest.raises(ValueError, match=re.escape(fragment)):
        LindbladSweep(lambda u, t: np.eye(3), **kw)


def test_durations_multiplies_the_rates_by_tau():
    linear, data, gammas, ops, rng = _open_system()
    times, ref = np.array([0.4, 0.8, 1.2]), 0.8
    tau = times / ref
    w = LindbladSweep.durations(linear, times, ref)
    assert isinstance(w, LindbladSweep) and w.time_scaled and w.has_rates and w.rate_scales is None
    assert np.array_equal(w.resolved_rate_scales(2), np.repeat(tau[:, None], 2, axis=1))
    assert np.array_equal(w.offsets[:, 0], tau)
    c0 = np.array([[1.0, 2.0], [0.5, 1.0], [3.0, 0.1]])
    w = LindbladSweep.durations(linear, times, ref, rate_scales=c0,
                                control_scales=np.ones((3, 2)))
    assert np.array_equal(w.rate_scales, tau[:, None] * c0)
    assert np.array_equal(w.slice(1, 2).rate_scales, tau[1:2, None] * c0[1:2])
    gam, _ = w.member_lindblad_data(2, data)(0.0)
    assert np.array_equal(gam, tau[2] * c0[2] * gammas)
    with pytest.raises(ValueError, match="rate_scales are for 2 seeds, evolution_times for 3"):
        LindbladSweep.durations(linear, times, ref, rate_scales=np.ones((2, 2)))
    with pytest.raises(ValueError, match=r"rate_scales must be \(B, L\) with L = 3"):
        w.resolved_rate_scales(3)
    # the rate part of the chain rule: sum_l dE/dc_bl c0_bl / reference_time on top of the sweep's
    s, o, r = rng.standard_normal((3, 2)), rng.standard_normal((3, 1)), rng.standard_normal((3, 2))
    base = HamiltonianSweep.time_gradients(w, s, o)
    assert np.array_equal(w.time_gradients(s, o, r), base + np.sum(r * c0, axis=1) / ref)
    assert np.array_equal(w.time_gradients(s, o), base)


class _UserCost(Cost):
    name = "user"

    def cost(self, controls, densities, step):
        return float(np.real(densities[0, 0, 0]))


def test_refusals_by_name():
    n, K, N, Nc = 4, 2, 6, 4
    linear, data, gammas, ops, rng = _open_system(n, K)
    init, targ = _densities(n, rng)
    costs = [TargetDensityInfidelity(targ)]
    rates = np.array([[0.5, 1.0], [2.0, 1.0]])
    w = LindbladSweep(linear, control_scales=np.ones((2, K)), rate_scales=rates)
    make = lambda sweep, data=data, costs=costs, **kw: _evaluator(  # noqa: E731
        sweep, data, init, costs, N=N, K=K, Nc=Nc, **kw)
    # the single-problem entry points name member(b); save files go with them
    args = (0.8, init, N)
    with pytest.raises(NotImplementedError, match=r"evolve_lindblad_discrete.*member\(b\)"):
        qoc_amd.evolve_lindblad_discrete(*args, controls=np.zeros((Nc, K)), costs=costs,
                                         hamiltonian=w, lindblad_data=data)
    with pytest.raises(NotImplementedError, match=r"grape_lindblad_discrete.*member\(b\)"):
        qoc_amd.grape_lindblad_discrete(K, Nc, costs, *args, hamiltonian=w, lindblad_data=data)
    with pytest.raises(NotImplementedError, match="save files"):
        qoc_amd.grape_lindblad_discrete(K, Nc, costs, *args, hamiltonian=w, lindblad_data=data,
                                        save_file_path="/nonexistent/x.h5")
    # the Schroedinger entry points: nothing to scale
    psi0 = cases_mod.column_states(np.eye(n)[:, :1])
    tcost = [TargetStateInfidelity(psi0)]
    with pytest.raises(ValueError, match="nothing to scale"):
        device.SchroedingerEvaluator(0.8, w, psi0, N, control_count=K, control_eval_count=Nc,
                                     costs=tcost, backend=OracleBackend())
    with pytest.raises(ValueError, match="nothing to scale"):
        qoc_amd.evolve_schroedinger_discrete(0.8, w, psi0, N, controls=np.zeros((Nc, K)))
    with pytest.raises(ValueError, match="nothing to scale"):
        qoc_amd.grape_schroedinger_discrete(K, Nc, tcost, 0.8, w, psi0, N)
    with pytest.raises(ValueError, match="nothing to scale"):
        qoc_amd.grape_schroedinger_discrete_batch(K, Nc, tcost, 0.8, w, psi0, N,
                                                  np.zeros((2, Nc, K)))
    # inside an ensemble
    with pytest.raises(NotImplementedError, match="inside a HamiltonianEnsemble"):
        HamiltonianEnsemble(w, control_scales=np.ones((2, K)))
    # user costs without a device descriptor
    with pytest.raises(NotImplementedError, match="without a device descriptor"):
        make(w, costs=[_UserCost()])
    # bases
    quad = QuadraticHamiltonian(linear, [(0, 0, np.eye(n))])
    with pytest.raises(NotImplementedError, match="QuadraticHamiltonian"):
        make(LindbladSweep(quad, rate_scales=rates))
    with pytest.raises(ValueError, match="callable"):  # a sweep is no callable, nor is an ensemble
        LindbladSweep(LindbladSweep(linear, rate_scales=rates), rate_scales=rates)
    with pytest.raises(ValueError, match="callable"):
        LindbladSweep(HamiltonianEnsemble(linear, control_scales=np.ones((2, K))), rate_scales=rates)
    inner = LindbladSweep(linear, rate_scales=rates)
    inner.hamiltonian = HamiltonianSweep(linear, control_scales=np.ones((2, K)))  # (set from outside)
    with pytest.raises(NotImplementedError, match="sweep x ensemble"):
        make(inner)
    with pytest.raises(NotImplementedError, match="plain hamiltonian"):
        LindbladSweep.durations(quad, [0.5, 1.0], 1.0)
    nonlinear = lambda u, t: linear(u, t) + u[0] ** 2 * np.eye(n)  # noqa: E731
    with pytest.raises(NotImplementedError, match="linear in the controls"):
        make(LindbladSweep(nonlinear, rate_scales=rates))
    # K_r + J > 8 real channels
    wide = LindbladSweep(linear, perturbations=np.stack([np.eye(n)] * 7), offsets=np.ones((2, 7)))
    with pytest.raises(NotImplementedError, match=r"K_r \+ J = 2 \+ 7"):
        make(wide)
    # ControlBandwidthMax with a duration sweep
    dur = LindbladSweep.durations(linear, [0.5, 1.0], 0.8)
    with pytest.raises(NotImplementedError, match="ControlBandwidthMax"):
        make(dur, costs=costs + [ControlBandwidthMax(K, Nc, 0.8, np.full(K, 5.0))])
    # with rates: a time-dependent base, drive or lindblad_data - before the backend sees a problem
    moving, *_ = _open_system(n, K, time_dependent=True)
    moving_data = lambda t: (gammas * (1 + 0.1 * t), ops)  # noqa: E731
    for sweep, dat, who in (
            (LindbladSweep(moving, rate_scales=rates), data, "the hamiltonian"),
            (LindbladSweep(linear, rate_scales=rates), moving_data, "lindblad_data"),
            (LindbladSweep.durations(moving, [0.5, 1.0], 0.8), data, "the hamiltonian"),
            (LindbladSweep.durations(linear, [0.5, 1.0], 0.8), moving_data, "lindblad_data")):
        backend = LindbladSweepStandIn()
        with pytest.raises(NotImplementedError, match="time-independent system.*" + who):
            make(sweep, data=dat, backend=backend)
        assert backend.log == []
    # ... without rates the time-dependent drive is fine (one set of stage tables serves every seed)
    backend = LindbladSweepStandIn()
    make(LindbladSweep(moving, control_scales=np.ones((2, K))), backend=backend,
         control_bounds=np.ones(K))
    assert backend.log == ["set_lindblad_problem", "set_lindblad_sweep"]
    assert backend.received[0][3] is None
    # a second dimension other than L
    with pytest.raises(ValueError, match=r"rate_scales must be \(B, L\) with L = 2"):
        make(LindbladSweep(linear, rate_scales=np.ones((2, 3))))
    # a backend without the setter; no controls; a wrong batch
    with pytest.raises(NotImplementedError, match="set_lindblad_sweep"):
        make(w, backend=OracleBackend())
    with pytest.raises(NotImplementedError, match="at least one control"):
        device.LindbladEvaluator(0.8, init, N, hamiltonian=w, lindblad_data=data, costs=costs,
                                 backend=LindbladSweepStandIn())
    ev = make(w)
    with pytest.raises(ValueError, match="exactly that many"):
        ev.evaluate_batch(np.zeros((3, Nc, K)))
    helpers.set_backend_factory(LindbladSweepStandIn)
    try:
        with pytest.raises(ValueError, match="exactly that many seeds"):
            qoc_amd.grape_lindblad_discrete_batch(K, Nc, costs, *args, np.zeros((3, Nc, K)),
                                                  hamiltonian=w, lindblad_data=data)
    finally:
        helpers.set_backend_factory(None)


def test_a_plain_sweep_stays_refused_on_the_lindblad_path():
    linear, data, gammas, ops, rng = _open_system()
    init, targ = _densities(4, rng)
    w = HamiltonianSweep(linear, control_scales=np.ones((2, 2)))
    with pytest.raises(NotImplementedError, match="dissipation rates.*LindbladSweep"):
        _evaluator(w, data, init, [TargetDensityInfidelity(targ)])
    with pytest.raises(NotImplementedError, match="dissipation rates"):
        qoc_amd.grape_lindblad_discrete_batch(2, 4, [], 0.8, init, 6, np.zeros((2, 4, 2)),
                                              hamiltonian=w, lindblad_data=data)


def test_costs_may_be_empty():
    linear, data, gammas, ops, rng = _open_system()
    init, _ = _densities(4, rng)
    ev = _evaluator(LindbladSweep(linear, rate_scales=np.array([[1.0, 1.0], [2.0, 0.5]])),
                    data, init, [])
    errors, grads, finals, _ = ev.evaluate_batch(0.3 * rng.standard_normal((2, 4, 2)))
    assert np.array_equal(errors, np.zeros(2)) and finals.shape == (2, 1, 4, 4)


# ---- 2. durations builds the right seed ------------------------------------------------------------

def test_a_duration_seed_is_the_unscaled_system_on_its_own_time():
    """member(b) with member_lindblad_data(b, .) on reference_time against the user's system (with its
    own scales, offsets and rate factors) on T_b, at 1e-12, the bound of the Schroedinger duration
    sweep against its oracle (tests/test_sweep_host.py). The oracle here is the fixed-step
    integrator of the oracle backend (tests/lindblad_model.py) on one frozen grid: scaling the
    Lindbladian is scaling time exactly for it, as for the expm oracle of the Schroedinger test
    (observed: 2e-16 .. 1e-15). The adaptive reference integrator (oracle/qoc_lindblad_numpy.py) is
    not invariant under the scaling - its initial-step rule reads the time scale, so the two runs
    take different step sequences (492 against 558 right-hand sides) and differ by 1.7e-12 ..
    1.1e-11 on these shapes, its own noise; it agrees bit for bit where tau_b = 1. It is held to the
    forward parity gate of DESIGN.md section 9 (cost 1e-9, densities 1e-8) as a second check."""
    n, K, N, Nc, ref, ksub = 4, 2, 6, 4, 0.8, 4
    linear, data, gammas, ops, rng = _open_system(n, K, seed=21)
    init, targ = _densities(n, rng)
    times = ref * np.array([0.6, 1.0, 1.5])
    s0 = 1 + 0.1 * rng.standard_normal((3, K))
    c0 = np.array([[1.0, 1.0], [0.5, 2.0], [1.5, 0.7]])
    dmat, d0 = cases_mod.gue(rng, n)[None], 0.2 * rng.standard_normal((3, 1))
    w = LindbladSweep.durations(linear, times, ref, control_scales=s0, perturbations=dmat,
                                offsets=d0, rate_scales=c0)
    u = 0.5 * rng.standard_normal((Nc, K))
    costs = [ol.TargetDensityInfidelity(targ)]

    def structured(hamiltonian, lindblad_data):
        zero = np.zeros(K)
        h0 = hamiltonian(zero, 0.0)
        return lm.StructuredLindblad(h0, [hamiltonian(np.eye(K)[k], 0.0) - h0 for k in range(K)],
                                     *lindblad_data(0.0))

    def model(T, hamiltonian, lindblad_data):
        err, _, dens = lm.evaluate_with_grad(structured(hamiltonian, lindblad_data), u, init, T, N,
                                             costs, want_grad=False, subdivision=ksub)
        return err, dens

    def reference(T, hamiltonian, lindblad_data):
        problem = ol.LindbladProblem(T, init, N, hamiltonian=hamiltonian,
                                     lindblad_data=lindblad_data, control_eval_count=Nc,
                                     costs=costs, control_count=K)
        return ol.evaluate(problem, u)
    for b in range(3):
        seed = (ref, w.member(b), w.member_lindblad_data(b, data))
        user = (times[b], lambda v, t, b=b: linear(s0[b] * v, t) + d0[b, 0] * dmat[0],
                lambda t, b=b: (c0[b] * gammas, ops))
        (got, dens), (want, want_dens) = model(*seed), model(*user)
        (r_got, r_dens), (r_want, r_want_dens) = reference(*seed), reference(*user)
        print("seed", b, "model", abs(got - want), np.max(np.abs(dens - want_dens)),
              "reference", abs(r_got - r_want), np.max(np.abs(r_dens - r_want_dens)))
        assert abs(got - want) < 1e-12 and np.max(np.abs(dens - want_dens)) < 1e-12
        assert abs(r_got - r_want) < 1e-9 and np.max(np.abs(r_dens - r_want_dens)) < 1e-8
        assert abs(got - r_got) < 1e-9  # (the two oracles describe the same system)


# ---- 3. the model's rate derivative -------------------------------------------------------------------

@pytest.mark.parametrize("name", ["lindblad_n4", "lindblad_n4_complex"])
def test_the_model_rate_derivative_agrees_with_central_differences(name):
    """tests/lindblad_sweep_model.rate_sensitivities against (E(c + h e_l) - E(c - h e_l)) / 2h of
    lindblad_model's own cost on a frozen grid (three pieces per system step). The step was chosen
    by a scan on the CPU: |fd - model| over both fixtures and every l was
        h = 1e-2: 9.3e-10   1e-3: 9.3e-12   1e-4: 4.3e-13   1e-5: 4.1e-12   1e-6: 5.4e-11
    (lindblad_n4: 2.9e-13, 3.5e-13; lindblad_n4_complex: 4.3e-13 at h = 1e-4), so h = 1e-4 and the
    bound is ten times the worst, 4.3e-12; the derivatives themselves are 7e-6 .. 4e-4."""
    case = cases_mod.lindblad_case_by_name(name)
    costs = [getattr(ol, k)(**kw) for k, kw in case.cost_specs]
    system = lm.StructuredLindblad(case.h0, gh.lindblad_generators(case), case.dissipators,
                                   case.operators)
    u = gh.real_controls(case, case.controls[0])
    L = len(case.dissipators)
    c0 = np.array([1.3, 0.7])[:L]
    args = (u, case.initial_densities, case.T, case.N, costs, case.cost_eval_step)
    err, sens = sm.rate_sensitivities(system, *args, subdivision=3, factors=c0)

    def cost(c):
        return lm.evaluate_with_grad(sm.scaled_system(system, c), *args, want_grad=False,
                                     subdivision=3)[0]
    assert err == cost(c0)
    h = 1e-4
    for l in range(L):
        step = np.zeros(L)
        step[l] = h
        fd = (cost(c0 + step) - cost(c0 - step)) / (2 * h)
        print(name, l, "model", sens[l], "fd - model", fd - sens[l])
        assert abs(sens[l]) > 1e-6
        assert abs(fd - sens[l]) < 4.3e-12


# ---- 4. evolution_time_gradients ---------------------------------------------------------------------

def test_time_gradients_agree_with_central_differences_in_the_duration():
    """dE_b/dT_b from the sensitivities of ONE evaluation at the reference time (the stand-in: the
    model of test 3 on a frozen grid of four pieces per system step) against the central difference
    of the model's cost of member b's unscaled system on T_b +- eps, same grid. eps was scanned on the
    CPU: |fd - chain rule| over the three seeds was
        eps / T_b = 1e-2: 2.7e-8   1e-3: 2.7e-10   1e-4: 3.2e-12   1e-5: 8.1e-12   1e-6: 3.7e-11
    (at 1e-4: 1.2e-12, 3.2e-12, 5.8e-13), so eps = 1e-4 T_b and the bound is ten times the worst,
    3.2e-11; the gradients are 3e-4 .. 3e-3."""
    n, K, N, Nc, ref, ksub = 4, 2, 6, 4, 0.8, 4
    linear, data, gammas, ops, rng = _open_system(n, K, seed=33)
    init, targ = _densities(n, rng)
    times = ref * np.array([0.6, 1.0, 1.4])
    s0 = 1 + 0.1 * rng.standard_normal((3, K))
    c0 = np.array([[1.0, 1.0], [0.5, 2.0], [1.5, 0.7]])
    w = LindbladSweep.durations(linear, times, ref, control_scales=s0, rate_scales=c0)
    backend = LindbladSweepStandIn()
    ev = _evaluator(w, data, init, [TargetDensityInfidelity(targ)], T=ref, N=N, K=K, Nc=Nc,
                    backend=backend)
    backend.lb_subdivision = ksub
    u = 0.5 * rng.standard_normal((3, Nc, K))
    ev.want_rate_sensitivities(True)
    errors, _, _, _ = ev.evaluate_batch(u)
    sens = ev.sweep_sensitivities()
    ev.want_rate_sensitivities(False)
    assert sens["rate_scales"].shape == (3, 2) and sens["control_scales"].shape == (3, K)
    grads = sens["evolution_time_gradients"]
    assert np.array_equal(grads, w.time_gradients(sens["control_scales"], sens["offsets"],
                                                  sens["rate_scales"]))
    zero = np.zeros(K)
    h0 = linear(zero, 0.0)
    g = [linear(np.eye(K)[k], 0.0) - h0 for k in range(K)]
    costs = [ol.TargetDensityInfidelity(targ)]

    def model_error(b, T):
        system = lm.StructuredLindblad(h0, g, c0[b] * gammas, ops)
        return lm.evaluate_with_grad(system, s0[b] * u[b], init, T, N, costs, want_grad=False,
                                     subdivision=ksub)[0]
    for b, T in enumerate(times):
        assert abs(errors[b] - model_error(b, T)) < 1e-13
        eps = 1e-4 * T
        fd = (model_error(b, T + eps) - model_error(b, T - eps)) / (2 * eps)
        print("T", T, "fd", fd, "chain rule", grads[b], "diff", fd - grads[b])
        assert abs(fd) > 1e-4
        assert abs(fd - grads[b]) < 3.2e-11
    # without the request the rate entries are None, not garbage
    ev.evaluate_batch(u)
    sens = ev.sweep_sensitivities()
    assert sens["rate_scales"] is None and sens["evolution_time_gradients"] is None
    assert sens["control_scales"].shape == (3, K)


# ---- 5. the routes of the batch driver on a stand-in --------------------------------------------------

def _batch_problem(seed=9, durations=True):
    n, K, N, Nc, B, T = 4, 2, 6, 4, 3, 0.8
    linear, data, gammas, ops, rng = _open_system(n, K, seed=seed)
    c0 = np.array([[1.0, 1.0], [0.5, 2.0], [1.5, 0.7]])
    if durations:
        w = LindbladSweep.durations(linear, T * np.array([0.5, 1.0, 1.3]), T, rate_scales=c0)
    else:
        w = LindbladSweep(linear, perturbations=cases_mod.gue(rng, n)[None],
                          offsets=0.3 * rng.standard_normal((B, 1)),
                          control_scales=1 + 0.05 * rng.standard_normal((B, K)), rate_scales=c0)
    init, targ = _densities(n, rng)
    costs = [TargetDensityInfidelity(targ), ControlNorm(K, Nc, cost_multiplier=0.05)]
    u0 = np.clip(0.4 * rng.standard_normal((B, Nc, K)), -0.9, 0.9)
    return w, data, (K, Nc, costs, T, init, N), u0


@pytest.mark.parametrize("optimizer, durations", [
    (Adam(), True), (SGD(learning_rate=0.05), False), (LBFGS(), True)])
def test_host_loop_walks_the_single_seed_trajectories_of_the_members(optimizer, durations):
    w, data, head, u0 = _batch_problem(durations=durations)
    kw = dict(iteration_count=4, log_iteration_step=0, optimizer=optimizer)
    backends = []

    def factory():
        backends.append(LindbladSweepStandIn())
        return backends[-1]
    helpers.set_backend_factory(factory)
    try:
        full = qoc_amd.grape_lindblad_discrete_batch(*head, u0, hamiltonian=w, lindblad_data=data,
                                                     **kw)
    finally:
        helpers.set_backend_factory(None)
    assert full.member_errors == [None] * 3
    assert full.best_final_densities[0].shape == (1, 4, 4)
    sens = full.sweep_sensitivities
    assert sens["control_scales"].shape == (3, 2) and sens["rate_scales"].shape == (3, 2)
    assert np.all(np.isfinite(sens["rate_scales"]))
    assert ("evolution_time_gradients" in sens) == durations
    if durations:
        assert sens["evolution_time_gradients"].shape == (3,)
    # the calls: the problem, the sweep, one evaluation per iteration, then the one evaluation with
    # rate sensitivities after the loop
    log = backends[0].log
    assert log[:2] == ["set_lindblad_problem", "set_lindblad_sweep"]
    assert log[-4:] == ["want_rates 1", "evaluate_lindblad grad=1", "lindblad_sweep_sensitivities",
                        "want_rates 0"]
    assert set(log[2:-4]) == {"evaluate_lindblad grad=1"}
    helpers.set_backend_factory(OracleBackend)
    try:
        for b in range(3):
            one = qoc_amd.grape_lindblad_discrete(
                *head, hamiltonian=w.member(b), lindblad_data=w.member_lindblad_data(b, data),
                initial_controls=u0[b], **kw)
            assert one.best_iteration == full.best_iteration[b]
            assert abs(one.best_error - full.best_error[b]) < 1e-12
            assert np.max(np.abs(one.best_controls - full.best_controls[b])) < 1e-10
    finally:
        helpers.set_backend_factory(None)


class ResidentStandIn(LindbladSweepStandIn):
    """The stand-in with the resident driver's calls of the Lindblad prefix (SGD only, real
    controls, no costs of the controls)."""

    def lindblad_upload_controls(self, controls):
        self.log.append("lindblad_upload_controls")
        self.res = np.array(controls, dtype=np.float64)

    def lindblad_opt_begin(self):
        self.log.append("lindblad_opt_begin")
        self.best, self.best_final = self.res.copy(), None

    def lindblad_opt_clip(self, max_norms):
        self.log.append("lindblad_opt_clip")
        engine.host_clip_controls(self.res, max_norms)

    def eval_lindblad_resident(self, want_grad=True):
        self.log.append("eval_lindblad_resident")
        self.res_out = LindbladSweepStandIn.evaluate_lindblad(self, self.res, want_grad)
        self.log.pop()

    def lindblad_download_costs(self):
        self.log.append("lindblad_download_costs")
        return self.res_out[0].copy()

    def lindblad_opt_step(self, kind, improved, update, learning_rate, *rest, **kw):
        self.log.append("lindblad_opt_step")
        assert kind == 0
        improved, update = np.asarray(improved, bool), np.asarray(update, bool)
        self.best[improved] = self.res[improved]
        if self.best_final is None:
            self.best_final = np.zeros_like(self.res_out[2])
        self.best_final[improved] = self.res_out[2][improved]
        self.res[update] -= learning_rate * self.res_out[1][update]

    def lindblad_opt_download_best(self):
        self.log.append("lindblad_opt_download_best")
        return self.best.copy(), self.best_final.copy()


def test_resident_route_makes_the_calls_of_the_host_loop_in_order():
    w, data, head, u0 = _batch_problem(durations=True)
    K, Nc, costs, T, init, N = head
    head = (K, Nc, costs[:1], T, init, N)  # (the device cost alone)
    kw = dict(iteration_count=3, log_iteration_step=0, optimizer=SGD(learning_rate=0.05),
              hamiltonian=w, lindblad_data=data, max_control_norms=np.full(K, 0.95))
    runs = {}
    for name, cls in (("host", LindbladSweepStandIn), ("resident", ResidentStandIn)):
        made = []

        def factory(cls=cls, made=made):
            made.append(cls())
            return made[-1]
        helpers.set_backend_factory(factory)
        try:
            runs[name] = (qoc_amd.grape_lindblad_discrete_batch(*head, u0, **kw), made[0].log)
        finally:
            helpers.set_backend_factory(None)
    (host, host_log), (res, res_log) = runs["host"], runs["resident"]
    tail = ["want_rates 1", "evaluate_lindblad grad=1", "lindblad_sweep_sensitivities", "want_rates 0"]
    assert host_log == ["set_lindblad_problem", "set_lindblad_sweep"] + 3 * [
        "evaluate_lindblad grad=1"] + tail
    assert res_log == (["set_lindblad_problem", "set_lindblad_sweep", "lindblad_upload_controls",
                        "lindblad_opt_begin"]
                       + 3 * ["lindblad_opt_clip", "eval_lindblad_resident",
                              "lindblad_download_costs", "lindblad_opt_step"]
                       + ["lindblad_opt_download_best"] + tail)
    assert np.array_equal(host.best_iteration, res.best_iteration)
    assert np.max(np.abs(host.best_error - res.best_error)) < 1e-14
    for b in range(3):
        assert np.max(np.abs(host.best_controls[b] - res.best_controls[b])) < 1e-14
    for key in ("control_scales", "offsets", "rate_scales", "evolution_time_gradients"):
        assert np.max(np.abs(host.sweep_sensitivities[key] - res.sweep_sensitivities[key])) < 1e-12


def test_every_rank_takes_its_block_of_the_sweep():
    """rank_sweep hands a rank sweep.slice(lo, hi), rates included."""
    from qoc_amd.core import batch

    class Comm(object):
        rank, world = 1, 2
    w, data, head, u0 = _batch_problem(durations=True)
    part = batch.rank_sweep(w, 3, Comm())
    assert isinstance(part, LindbladSweep) and part.seed_count == 1
    assert np.array_equal(part.rate_scales, w.rate_scales[2:])
    assert np.array_equal(part.evolution_times, w.evolution_times[2:])


# ---- the ABI ------------------------------------------------------------------------------------------

NEW_SYMBOLS = ("qocx_lindblad_set_sweep", "qocx_lindblad_sweep_download_sensitivities",
               "qocx_lindblad_sweep_want_rate_sensitivities")


def test_the_new_symbols_are_in_the_header_the_binding_and_the_library():
    header = open(os.path.join(ROOT, "include", "qocx.h")).read()
    lib = engine.load_library()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint %s\(qocx_ctx\* ctx" % name, header), name
        assert name in engine.SIGNATURES and hasattr(lib, name), name
    assert len(engine.SIGNATURES["qocx_lindblad_set_sweep"][1]) == 6
    assert len(engine.SIGNATURES["qocx_lindblad_sweep_download_sensitivities"][1]) == 4
    assert "gradients with respect to delta or to the rates below\n * (a sweep has them" in header
