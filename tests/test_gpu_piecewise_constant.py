"""
GPU tests (-m gpu) of InterpolationPolicy.PIECEWISE_CONSTANT on the engine: the tables
qocx_set_schroedinger_problem / qocx_set_lindblad_problem build under
qocx_set_interpolation_policy, read by every kernel route, against the two references of
tests/piecewise_constant.py.

Reference A (the oracle on the control-free closure of the pulse; gradient by central differences,
h = 1e-5) at the project's gates - DESIGN section 10: states and cost 1e-10, gradient against
differences 1e-7 of its largest entry; section 9: Lindblad densities 1e-8, cost 1e-9, gradient the
gate tests/test_gpu_lindblad.py applies to differences of the reference's forward pass: 3e-7 of
max |g| on Richardson-extrapolated quotients. Reference B (the linear twin, M2, N - 1 = Nc) on
the device itself: states 1e-12, gradient 1e-10 relative.

Shapes: K = 2, S <= 2, B = 2 - a quiet seed (amplitude 0.05) and a loud one (amplitude 2).
"""

import numpy as np
import pytest

import qoc_amd
from oracle import qoc_lindblad_numpy as ol
from oracle import qoc_numpy as onp
from qoc_amd.core import device
from qoc_amd.core.common import clip_control_norms
from qoc_amd.engine import COST_TARGET_COHERENT, QocxError
from qoc_amd.models import InterpolationPolicy, MagnusPolicy
from qoc_amd.standard import (LBFGS, Adam, ControlBasis, HamiltonianEnsemble, QuadraticHamiltonian,
                              TargetDensityInfidelity, TargetStateInfidelity)
from qoc_amd.standard.costs import ControlVariation, ForbidStates, TargetStateInfidelityTime
from tests import cases as cases_mod
from tests import gpu_helpers as gh
from tests import helpers
from tests import piecewise_constant as pc
from tests.test_gpu_lbfgs import assert_same_runs, routes  # noqa: F401

pytestmark = pytest.mark.gpu

PWC = InterpolationPolicy.PIECEWISE_CONSTANT
K = 2
DT = 0.3


@pytest.fixture(autouse=True)
def real_engine():
    helpers.set_backend_factory(None)
    yield
    helpers.set_backend_factory(None)


@pytest.fixture
def engine():
    from qoc_amd.engine import Engine
    out = Engine(0)
    yield out
    out.close()


def seeds(Nc, seed, complex_controls=False, channels=K):
    """(2, Nc, K): a quiet and a loud pulse."""
    rng = np.random.default_rng(seed)
    u = rng.standard_normal((2, Nc, channels))
    if complex_controls:
        u = u + 1j * rng.standard_normal((2, Nc, channels))
    return u * np.array([0.05, 2.0])[:, None, None]


def assert_matches_reference_a(ev, hamiltonian, pulses, T, psi0, N, ocosts, magnus,
                               cost_eval_step=1, grad_seeds=(0, 1)):
    """grad_seeds: the seeds whose gradient is checked against differences of Reference A (2 Nc K
    oracle passes each)."""
    errors, grads, finals, _ = ev.evaluate_batch(pulses)
    for b, c in enumerate(pulses):
        want_grad = b in grad_seeds
        err, fin = pc.reference_a(hamiltonian, c, T, psi0, N, ocosts, magnus, cost_eval_step)
        print("seed", b, "cost", errors[b] - err, "states", np.max(np.abs(finals[b] - fin)))
        assert abs(errors[b] - err) < 1e-10
        assert np.max(np.abs(finals[b] - fin)) < 1e-10
        if want_grad:
            ref = pc.reference_a_gradient(hamiltonian, c, T, psi0, N, ocosts, magnus, cost_eval_step)
            scale = np.max(np.abs(ref))
            print("seed", b, "max |g|", scale, "max |g - fd|", np.max(np.abs(grads[b] - ref)))
            assert scale > 1e-6
            assert np.max(np.abs(grads[b] - ref)) < 1e-7 * scale
    return errors, grads, finals


# ---- the engine against Reference A on every kernel route --------------------------------------------

ENGINE_CASES = [
    (4, "M2", 6, 6),
    (8, "M2", 18, 6),    # pack8, three steps per slice
    (16, "M6", 7, 3),    # unaligned: the nodes of a step in two slices
    (20, "M4", 7, 3),    # step table, two- and three-wave K1a
    (32, "M2", 8, 8),
    (40, "M6", 6, 3),    # four-wave K1a
    (72, "M2", 7, 3),    # general path
]


@pytest.mark.parametrize("n, magnus, nsteps, Nc", ENGINE_CASES)
def test_engine_against_reference_a(n, magnus, nsteps, Nc):
    N, T = nsteps + 1, DT * nsteps
    h = pc.system(n, K, seed=100 + n)
    psi0, target = pc.states(n, 2, seed=200 + n)
    ev = device.SchroedingerEvaluator(
        T, h, psi0, N, control_count=K, control_eval_count=Nc,
        costs=[TargetStateInfidelity(target)], magnus_policy=getattr(MagnusPolicy, magnus),
        interpolation_policy=PWC)
    assert ev.opaque_hamiltonian is None and ev.linearized_hamiltonian is None
    # (n >= 40: the oracle takes 0.3 s per pass - differences for the loud seed only)
    assert_matches_reference_a(ev, h, seeds(Nc, 300 + n), T, psi0, N,
                               [onp.TargetStateInfidelity(target)], magnus,
                               grad_seeds=(0, 1) if n < 40 else (1,))


def test_time_dependent_drive_operators():
    """G_k(t) and H0(t) tables per node together with slice indices per node (n = 16, M6)."""
    n, nsteps, Nc = 16, 7, 3
    N, T = nsteps + 1, DT * nsteps
    h = pc.system(n, K, seed=116, drive_frequency=2.3)
    psi0, target = pc.states(n, 2, seed=216)
    ev = device.SchroedingerEvaluator(T, h, psi0, N, control_count=K, control_eval_count=Nc,
                                      costs=[TargetStateInfidelity(target)],
                                      magnus_policy=MagnusPolicy.M6, interpolation_policy=PWC)
    assert_matches_reference_a(ev, h, seeds(Nc, 316), T, psi0, N,
                               [onp.TargetStateInfidelity(target)], "M6")


def test_step_costs_and_the_unit_adjoint_route():
    n, nsteps, Nc = 8, 18, 6
    N, T = nsteps + 1, DT * nsteps
    h = pc.system(n, K, seed=108)
    psi0, target = pc.states(n, 2, seed=208)
    forbidden = np.stack([pc.states(n, 2, seed=209)[1], pc.states(n, 2, seed=210)[1]])
    costs = [ForbidStates(forbidden, N, cost_eval_step=3),
             TargetStateInfidelityTime(N, target, cost_eval_step=3)]
    ocosts = [onp.ForbidStates(forbidden, N, cost_eval_step=3),
              onp.TargetStateInfidelityTime(N, target, cost_eval_step=3)]
    ev = device.SchroedingerEvaluator(T, h, psi0, N, control_count=K, control_eval_count=Nc,
                                      costs=costs, cost_eval_step=3, interpolation_policy=PWC)
    assert_matches_reference_a(ev, h, seeds(Nc, 308), T, psi0, N, ocosts, "M2", cost_eval_step=3)
    # one final target, one state, one control array at a time: the unit adjoint
    ev = device.SchroedingerEvaluator(T, h, psi0[:1], N, control_count=K, control_eval_count=Nc,
                                      costs=[TargetStateInfidelity(target[:1])],
                                      interpolation_policy=PWC, latency_mode=True)
    for c in seeds(Nc, 308):
        assert_matches_reference_a(ev, h, c[None], T, psi0[:1], N,
                                   [onp.TargetStateInfidelity(target[:1])], "M2")


@pytest.mark.parametrize("latency", [False, True])
def test_latency_mode_at_n20(latency):
    n, nsteps, Nc = 20, 7, 3
    N, T = nsteps + 1, DT * nsteps
    h = pc.system(n, K, seed=120)
    psi0, target = pc.states(n, 2, seed=220)
    ev = device.SchroedingerEvaluator(T, h, psi0, N, control_count=K, control_eval_count=Nc,
                                      costs=[TargetStateInfidelity(target)],
                                      interpolation_policy=PWC, latency_mode=latency)
    for c in seeds(Nc, 320):
        assert_matches_reference_a(ev, h, c[None], T, psi0, N,
                                   [onp.TargetStateInfidelity(target)], "M2")


def test_complex_controls():
    n, nsteps, Nc = 16, 7, 3
    N, T = nsteps + 1, DT * nsteps
    h = pc.system(n, K, seed=117)
    psi0, target = pc.states(n, 2, seed=217)
    ev = device.SchroedingerEvaluator(T, h, psi0, N, control_count=K, control_eval_count=Nc,
                                      complex_controls=True, costs=[TargetStateInfidelity(target)],
                                      magnus_policy=MagnusPolicy.M6, interpolation_policy=PWC)
    assert_matches_reference_a(ev, h, seeds(Nc, 317, complex_controls=True), T, psi0, N,
                               [onp.TargetStateInfidelity(target)], "M6")


def test_quadratic_hamiltonian():
    n, nsteps, Nc = 24, 7, 3
    N, T = nsteps + 1, DT * nsteps
    rng = np.random.default_rng(124)
    h = QuadraticHamiltonian(pc.system(n, K, seed=124),
                             [(0, 0, pc.hermitian(rng, n, 0.3)), (0, 1, pc.hermitian(rng, n, 0.2))])
    psi0, target = pc.states(n, 2, seed=224)
    ev = device.SchroedingerEvaluator(T, h, psi0, N, control_count=K, control_eval_count=Nc,
                                      costs=[TargetStateInfidelity(target)],
                                      interpolation_policy=PWC)
    assert ev.quadratic_terms is not None and ev.opaque_hamiltonian is None
    assert_matches_reference_a(ev, h, seeds(Nc, 324), T, psi0, N,
                               [onp.TargetStateInfidelity(target)], "M2")


def test_hamiltonian_ensemble():
    n, nsteps, Nc, M = 8, 18, 6, 3
    N, T = nsteps + 1, DT * nsteps
    rng = np.random.default_rng(130)
    e = HamiltonianEnsemble(pc.system(n, K, seed=130),
                            perturbations=np.stack([pc.hermitian(rng, n, 0.3)]),
                            offsets=0.5 * rng.standard_normal((M, 1)),
                            control_scales=1 + 0.05 * rng.standard_normal((M, K)),
                            weights=rng.uniform(0.2, 1.0, M))
    psi0, target = pc.states(n, 2, seed=230)
    ev = device.SchroedingerEvaluator(T, e, psi0, N, control_count=K, control_eval_count=Nc,
                                      costs=[TargetStateInfidelity(target)],
                                      interpolation_policy=PWC)
    pulses = seeds(Nc, 330)
    errors, grads, finals, _ = ev.evaluate_batch(pulses)
    members = ev.member_errors()
    ocosts = [onp.TargetStateInfidelity(target)]
    for b, c in enumerate(pulses):
        total, gsum = 0.0, np.zeros_like(c)
        for m in range(M):
            err, fin = pc.reference_a(e.member(m), c, T, psi0, N, ocosts)
            assert abs(members[b, m] - err) < 1e-10
            assert np.max(np.abs(finals[b, m] - fin)) < 1e-10
            total += e.weights[m] * err
            gsum += e.weights[m] * pc.reference_a_gradient(e.member(m), c, T, psi0, N, ocosts)
        assert abs(errors[b] - np.dot(e.weights, members[b])) < 1e-14  # the reduction
        assert abs(errors[b] - total) < 1e-10
        assert np.max(np.abs(grads[b] - gsum)) < 1e-7 * np.max(np.abs(gsum))


def test_m2_explicit_generator_route():
    """A callable with an epsilon^2 term under M2: the host samples the slices' generators
    (structure.sample_generators with piecewise-constant rows), the engine takes them as they are
    and the host folds the cotangents back through the same rows."""
    n, nsteps, Nc = 8, 7, 3
    N, T = nsteps + 1, DT * nsteps
    base = pc.system(n, K, seed=140)
    q = pc.hermitian(np.random.default_rng(141), n, 0.4)
    h = lambda u, t: base(u, t) + (0.0 if u is None else u[0] ** 2) * q  # noqa: E731
    psi0, target = pc.states(n, 2, seed=240)
    ev = device.SchroedingerEvaluator(T, h, psi0, N, control_count=K, control_eval_count=Nc,
                                      costs=[TargetStateInfidelity(target)],
                                      interpolation_policy=PWC)
    assert ev.opaque_hamiltonian is not None
    assert_matches_reference_a(ev, h, seeds(Nc, 340), T, psi0, N,
                               [onp.TargetStateInfidelity(target)], "M2")


# ---- Reference B: the linear twin on the device ------------------------------------------------------

@pytest.mark.parametrize("n", [20, 72])
def test_linear_twin_on_the_device(n):
    Nc = 6
    N, T = Nc + 1, DT * Nc
    h = pc.system(n, K, seed=150 + n)
    psi0, target = pc.states(n, 2, seed=250 + n)
    common = dict(control_count=K, costs=[TargetStateInfidelity(target)])
    pulses = 0.7 * np.random.default_rng(350 + n).standard_normal((2, Nc, K))
    piecewise = device.SchroedingerEvaluator(T, h, psi0, N, control_eval_count=Nc,
                                             interpolation_policy=PWC, **common)
    e_p, g_p, f_p, _ = piecewise.evaluate_batch(pulses)
    twins = np.stack([pc.linear_twin(c)[0] for c in pulses])
    linear = device.SchroedingerEvaluator(T, h, psi0, N, control_eval_count=Nc + 1, **common)
    e_l, g_l, f_l, _ = linear.evaluate_batch(twins)
    J = pc.linear_twin(pulses[0])[1]
    for b in range(2):
        mapped = J.T @ g_l[b]
        print("states", np.max(np.abs(f_p[b] - f_l[b])), "gradient",
              np.max(np.abs(g_p[b] - mapped)) / np.max(np.abs(mapped)))
        assert np.max(np.abs(f_p[b] - f_l[b])) < 1e-12 and abs(e_p[b] - e_l[b]) < 1e-12
        assert np.max(np.abs(g_p[b] - mapped)) < 1e-10 * np.max(np.abs(mapped))


# ---- bounds ------------------------------------------------------------------------------------------

def test_a_one_slice_spike_keeps_its_digits(engine):
    """Nc = N, M2, n = 20: the shape at which a LINEAR problem bounds the step generators by the
    mean of neighbouring knots. Here a step reads one slice: the spike's own bound decides its
    Pade order."""
    n, Nc = 20, 8
    N = Nc
    h = pc.system(n, K, seed=160)
    psi0, target = pc.states(n, 2, seed=260)
    pulse = np.full((Nc, K), 0.4)
    pulse[4] = 4.0  # ten times its neighbours
    h0 = np.asarray(h(np.zeros(K), 0.0))
    g = np.stack([np.asarray(h(np.eye(K)[k], 0.0)) - h0 for k in range(K)])
    # dt such that the mean of the spike and a neighbour, (0.4 + 4) / 2 = 2.2 per control, is bounded
    # below theta_5 and the spike itself above it: theta_5 = dt (||H0||_1 + 3.1 sum_k ||G_k||_1)
    theta_5 = 2.539398330063230e-01
    g_sum = sum(np.linalg.norm(g[k], 1) for k in range(K))
    dt = theta_5 / (np.linalg.norm(h0, 1) + 3.1 * g_sum)
    assert dt * (np.linalg.norm(h0, 1) + 2.2 * g_sum) < 0.9 * theta_5
    T = dt * (N - 1)
    engine.set_schroedinger_problem(
        n, 2, K, Nc, N, T, h0[None], g[None], psi0[:, :, 0],
        costs=[dict(kind=COST_TARGET_COHERENT, step_cost=0, scale=1.0, vectors=target[:, :, 0])],
        interpolation="piecewise_constant")
    cost, grads, final = engine.evaluate(pulse[None])
    orders = engine.pade_orders()
    ocosts = [onp.TargetStateInfidelity(target)]
    err, fin = pc.reference_a(h, pulse, T, psi0, N, ocosts)
    ref = pc.reference_a_gradient(h, pulse, T, psi0, N, ocosts)
    print("orders", orders, "cost", cost[0] - err, "states", np.max(np.abs(final[0] - fin[:, :, 0])))
    assert abs(cost[0] - err) < 1e-10 and np.max(np.abs(final[0] - fin[:, :, 0])) < 1e-10
    assert np.max(np.abs(grads[0] - ref)) < 1e-7 * np.max(np.abs(ref))
    # the spike's own bound dt (||H0||_1 + sum_k 4 ||G_k||_1) lies above theta_5 = 0.2539...: the
    # steps that read the spike (slice 4: the steps whose midpoint lies in it) are above order 5
    spike_bound = dt * (np.linalg.norm(h0, 1) + 4.0 * g_sum)
    assert spike_bound > 1.1 * theta_5
    in_spike = sum(1 for j in range(N - 1) if pc.slice_of((j + 0.5) * dt, Nc, T) == 4)
    assert in_spike >= 1
    assert sum(count for order, count in orders.items() if order > 5) >= in_spike


def test_opt_clip_then_eval_resident_equals_the_host_clipped_upload(engine):
    n, nsteps, Nc = 20, 7, 3
    N, T = nsteps + 1, DT * nsteps
    h = pc.system(n, K, seed=161)
    psi0, target = pc.states(n, 2, seed=261)
    h0 = np.asarray(h(np.zeros(K), 0.0))
    g = np.stack([np.asarray(h(np.eye(K)[k], 0.0)) - h0 for k in range(K)])
    engine.set_schroedinger_problem(
        n, 2, K, Nc, N, T, h0[None], g[None], psi0[:, :, 0],
        costs=[dict(kind=COST_TARGET_COHERENT, step_cost=0, scale=1.0, vectors=target[:, :, 0])],
        interpolation="piecewise_constant")
    pulses = seeds(Nc, 361)
    norms = np.full(K, 1.5)  # at the scale of the controls: the loud seed is clipped
    clipped = pulses.copy()
    for c in clipped:
        clip_control_norms(c, norms)
    assert not np.array_equal(clipped, pulses)
    engine.upload_controls(clipped)
    engine.eval_resident(True)
    host = engine.download_results()
    engine.upload_controls(pulses)
    engine.opt_begin()
    engine.opt_clip(norms)
    engine.eval_resident(True)
    resident = engine.download_results()
    for a, b in zip(host, resident):
        assert np.array_equal(a, b)


# ---- Lindblad ----------------------------------------------------------------------------------------

def lindblad_setup(n, L, Nc, seed, drive_frequency=None):
    # (drive operators of norm 3: a gradient large against the noise of the reference's differences)
    h = pc.system(n, K, seed=seed, drive_frequency=drive_frequency, drive_norm=3.0)
    data, rho0, target = pc.lindblad_system(n, L, seed + 1)
    pulses = seeds(Nc, seed + 2)
    pulses[1] *= 0.5  # (amplitude 1: the reference's adaptive integrator stays quick)
    return h, data, rho0, target, pulses


def lindblad_evaluator(h, data, rho0, target, N, Nc, T):
    n = rho0.shape[1]
    return device.LindbladEvaluator(T, rho0, N, hamiltonian=h, lindblad_data=data,
                                    control_count=K, control_eval_count=Nc,
                                    costs=[TargetDensityInfidelity(target, cost_multiplier=n)],
                                    interpolation_policy=PWC)


def assert_gradient_matches_differences(grads, cost_of, c, seed, slice_length):
    """The gate tests/test_gpu_lindblad.py applies to differences of the reference's forward pass
    (stored entries, 3e-7 of max |g|, on a gradient with max |g| >= 1e-2). The quotients are
    extrapolated twice (error O(h^6)) at the step h = 0.1 / slice_length, where h times the slice's
    phase ||G|| T / Nc = 3 slice_length is 0.3. Noise: the reference's forward reproduces itself to
    1.2e-11 (measured: the same pulse displaced by 1e-13), times cost_multiplier = n <= 20 and
    ~6 / h in the extrapolated quotient: 7e-9 at h = 0.2, a tenth of the gate at max |g| = 0.2.
    Truncation: the reference's own quotients at h and h / 2 agree to 2e-8 .. 8e-8 of max |g| on
    these problems (at twice the step to 7e-7: the sixth power)."""
    idx = np.random.default_rng(9100 + seed).choice(c.size, size=3, replace=False)
    fd = pc.richardson_differences(cost_of, c, idx, h=0.1 / slice_length)
    scale = np.max(np.abs(grads))
    dev = np.max(np.abs(grads.ravel()[idx] - fd)) / scale
    print("max |g|", scale, "gradient against differences", dev)
    assert scale > 1e-2
    assert dev < 3e-7


def assert_lindblad_matches_reference_a(ev, h, data, rho0, target, pulses, N, T):
    ocosts = [ol.TargetDensityInfidelity(target, cost_multiplier=rho0.shape[1])]
    errors, grads, finals, _ = ev.evaluate_batch(pulses)
    for b, c in enumerate(pulses):
        err, fin = pc.lindblad_reference_a(h, c, T, rho0, N, ocosts, data)
        print("seed", b, "cost", errors[b] - err, "densities", np.max(np.abs(finals[b] - fin)))
        assert abs(errors[b] - err) < 1e-9
        assert np.max(np.abs(finals[b] - fin)) < 1e-8
        assert_gradient_matches_differences(
            grads[b], lambda x: pc.lindblad_reference_a(h, x, T, rho0, N, ocosts, data)[0], c, b,
            T / c.shape[0])


@pytest.mark.parametrize("n, L, nsteps, Nc", [
    (4, 2, 4, 4),     # multi-wave
    (16, 1, 6, 3),
    (20, 2, 3, 3),    # lindblad_4t
])
def test_lindblad_against_reference_a(n, L, nsteps, Nc):
    N, T = nsteps + 1, 0.25 * nsteps
    h, data, rho0, target, pulses = lindblad_setup(n, L, Nc, seed=400 + n)
    ev = lindblad_evaluator(h, data, rho0, target, N, Nc, T)
    assert not ev.time_dependent
    assert_lindblad_matches_reference_a(ev, h, data, rho0, target, pulses, N, T)


def test_lindblad_time_dependent_hamiltonian_tables():
    """H0(t) and G_k(t): tables at the stage times of Nc + 1 knots."""
    n, L, nsteps, Nc = 4, 1, 4, 2
    N, T = nsteps + 1, 0.25 * nsteps
    h, data, rho0, target, pulses = lindblad_setup(n, L, Nc, seed=450, drive_frequency=2.3)
    ev = lindblad_evaluator(h, data, rho0, target, N, Nc, T)
    assert ev.time_dependent
    assert_lindblad_matches_reference_a(ev, h, data, rho0, target, pulses, N, T)


def test_lindblad_unaligned_against_the_aligned_evaluation():
    """N - 1 = 4 over Nc = 3 slices: the edges fall inside system steps, where the reference's
    integrator would cross them. The same pulse with N - 1 = 12 has them on system steps."""
    n, L, Nc = 4, 2, 3
    T = 1.0
    h, data, rho0, target, pulses = lindblad_setup(n, L, Nc, seed=460)
    coarse = lindblad_evaluator(h, data, rho0, target, 5, Nc, T)
    fine = lindblad_evaluator(h, data, rho0, target, 13, Nc, T)
    e_c, g_c, f_c, _ = coarse.evaluate_batch(pulses)
    e_f, _, f_f, _ = fine.evaluate_batch(pulses, want_grad=False)
    for b, c in enumerate(pulses):
        print("seed", b, "cost", e_c[b] - e_f[b], "densities", np.max(np.abs(f_c[b] - f_f[b])))
        assert abs(e_c[b] - e_f[b]) < 1e-9 and np.max(np.abs(f_c[b] - f_f[b])) < 1e-8
        assert_gradient_matches_differences(
            g_c[b], lambda x: fine.evaluate_batch(x[None], want_grad=False)[0][0], c, b, T / Nc)


def stark(base, q):
    return lambda u, t: base(u, t) + (0.0 if u is None else u[0] ** 2) * q


def test_lindblad_frozen_controls_and_tangent_routes():
    """A callable with an epsilon^2 term on the Lindblad path, aligned: evolve folds the pulse into
    a time-dependent Hamiltonian sampled slice by slice, GRAPE hands the engine the tangent at the
    slices' values. A stage ON a slice edge belongs to the slice of its sub-interval."""
    n, L, nsteps, Nc = 4, 1, 4, 2
    N, T = nsteps + 1, 0.25 * nsteps
    base, data, rho0, target, pulses = lindblad_setup(n, L, Nc, seed=470)
    h = stark(base, pc.hermitian(np.random.default_rng(471), n, 0.4))
    ocosts = [ol.TargetDensityInfidelity(target, cost_multiplier=n)]
    c = pulses[1]
    err, fin = pc.lindblad_reference_a(h, c, T, rho0, N, ocosts, data)
    result = qoc_amd.evolve_lindblad_discrete(T, rho0, N, controls=c, hamiltonian=h,
                                              costs=[TargetDensityInfidelity(target,
                                                                             cost_multiplier=n)],
                                              lindblad_data=data, interpolation_policy=PWC)
    print("frozen: cost", result.error - err, "densities",
          np.max(np.abs(result.final_densities - fin)))
    assert abs(result.error - err) < 1e-9
    assert np.max(np.abs(result.final_densities - fin)) < 1e-8
    ev = lindblad_evaluator(h, data, rho0, target, N, Nc, T)
    assert ev.linearized_hamiltonian is not None
    assert_lindblad_matches_reference_a(ev, h, data, rho0, target, pulses[1:], N, T)


# ---- the resident multi-start route against the host loop --------------------------------------------

class HostAdam(Adam):  # not type(...) is Adam: the host loop
    pass


class HostLBFGS(LBFGS):
    pass


def both_routes(run, args, u0, routes, make, host, **kw):
    kw = dict(dict(iteration_count=3, log_iteration_step=0, interpolation_policy=PWC), **kw)
    before = dict(routes)
    a = run(*args, u0.copy(), optimizer=make(), **kw)
    assert routes == {"resident": before["resident"] + 1, "host": before["host"]}
    b = run(*args, u0.copy(), optimizer=host(), **kw)
    assert routes == {"resident": before["resident"] + 1, "host": before["host"] + 1}
    return a, b


OPTIMIZERS = [(lambda: Adam(learning_rate=2e-2), lambda: HostAdam(learning_rate=2e-2)),
              (LBFGS, HostLBFGS)]


@pytest.mark.parametrize("make, host", OPTIMIZERS)
@pytest.mark.parametrize("variant", ["variation", "basis"])
def test_resident_schroedinger_route_walks_the_host_loop(routes, make, host, variant):  # noqa: F811
    n, nsteps, Nc = 8, 18, 6
    N, T = nsteps + 1, DT * nsteps
    h = pc.system(n, K, seed=508)
    psi0, target = pc.states(n, 2, seed=608)
    costs = [TargetStateInfidelity(target)]
    kw = dict(max_control_norms=np.full(K, 0.6))
    if variant == "variation":
        costs.append(ControlVariation(K, Nc, cost_multiplier=0.1, max_control_norms=np.full(K, 0.6)))
        u0 = np.clip(0.3 * np.random.default_rng(708).standard_normal((2, Nc, K)), -0.6, 0.6)
    else:
        kw["control_basis"] = ControlBasis.sine(Nc, 3)
        u0 = 0.2 * np.random.default_rng(709).standard_normal((2, 3, K))
    args = (K, Nc, costs, T, h, psi0, N)
    a, b = both_routes(qoc_amd.grape_schroedinger_discrete_batch, args, u0, routes, make, host, **kw)
    assert_same_runs(a, b)
    assert np.any(a.best_iteration > 0)


@pytest.mark.parametrize("make, host", OPTIMIZERS)
@pytest.mark.parametrize("variant", ["plain", "basis"])
def test_resident_lindblad_route_walks_the_host_loop(routes, make, host, variant):  # noqa: F811
    n, L, nsteps, Nc = 4, 2, 4, 4
    N, T = nsteps + 1, 0.25 * nsteps
    h, data, rho0, target, _ = lindblad_setup(n, L, Nc, seed=520)
    kw = dict(hamiltonian=h, lindblad_data=data, max_control_norms=np.full(K, 2.0))
    if variant == "plain":
        u0 = np.clip(0.8 * np.random.default_rng(720).standard_normal((2, Nc, K)), -2.0, 2.0)
    else:
        kw["control_basis"] = ControlBasis.sine(Nc, 3)
        u0 = 0.4 * np.random.default_rng(721).standard_normal((2, 3, K))
    args = (K, Nc, [TargetDensityInfidelity(target)], T, rho0, N)
    a, b = both_routes(qoc_amd.grape_lindblad_discrete_batch, args, u0, routes, make, host, **kw)
    assert_same_runs(a, b, finals="best_final_densities")
    assert np.any(a.best_iteration > 0)


# ---- the ABI call, and LINEAR untouched ---------------------------------------------------------------

def test_set_interpolation_policy_rejects_other_values(engine):
    for bad in (0, 3, -1):
        with pytest.raises(QocxError):
            engine.set_interpolation_policy(bad)
    with pytest.raises(ValueError):
        engine.set_interpolation_policy("cubic")
    for good in (2, 1, "piecewise_constant", "linear", PWC, InterpolationPolicy.LINEAR):
        engine.set_interpolation_policy(good)
    assert engine._lib.qocx_set_interpolation_policy(engine._ctx, 7) != 0  # the ABI itself
    assert engine._lib.qocx_set_interpolation_policy(engine._ctx, 1) == 0


def test_linear_bits_are_untouched():
    from qoc_amd.engine import Engine
    case = cases_mod.case_by_name("c3_subset")
    u = gh.real_controls(case, np.stack(case.controls[:2]))

    def run(engine, prepare):
        prepare(engine)
        gh.setup_engine(engine, case)  # (sets the problem without the interpolation argument ...
        return engine.evaluate(u)

    outs = []
    # (a fresh Engine never makes the ABI call for a linear problem; the second context makes it)
    for prepare in (lambda e: None,
                    lambda e: e._check(e._lib.qocx_set_interpolation_policy(e._ctx, 1))):
        eng = Engine(0)
        outs.append(run(eng, prepare))
        eng.close()
    # a context switched to piecewise constant and back reproduces them, and differs in between
    eng = Engine(0)
    h0, g = gh.sample_hamiltonian(case)
    descs, _ = gh.device_costs(case)
    head = (case.n, case.S, case.K, case.Nc, case.N, case.T, h0, g, case.initial_states[:, :, 0])
    eng.set_schroedinger_problem(*head, costs=descs, interpolation="piecewise_constant")
    between = eng.evaluate(u)
    outs.append(run(eng, lambda e: None))  # ... which is LINEAR again)
    eng.close()
    for out in outs[1:]:
        for a, b in zip(outs[0], out):
            assert np.array_equal(a, b)
    assert not np.array_equal(between[0], outs[0][0])
