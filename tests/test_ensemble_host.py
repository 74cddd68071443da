"""CPU tests of qoc_amd.standard.HamiltonianEnsemble and its host routing (no GPU): the
constructor's checks, member(m), a stand-in backend that takes ensembles (where the evaluator must
hand over the (K_r + J)-channel problem and reduce nothing itself), the rejections, and the ABI."""

import numpy as np
import pytest

import qoc_amd
from oracle import qoc_numpy as onp
from qoc_amd import engine
from qoc_amd.core import device
from qoc_amd.models import MagnusPolicy
from qoc_amd.models.cost import Cost
from qoc_amd.standard import (ControlNorm, ForbidStates, HamiltonianEnsemble,
                              QuadraticHamiltonian, TargetStateInfidelity,
                              TargetStateInfidelityTime)
from tests import cases as cases_mod
from tests import helpers
from tests.oracle_backend import OracleBackend


def _system(n=5, K=2, seed=3, complex_controls=False, time_dependent=False):
    rng = np.random.default_rng(seed)
    h0 = cases_mod.gue(rng, n)
    g_re = [cases_mod.gue(rng, n) for _ in range(K)]
    g_im = [cases_mod.gue(rng, n) for _ in range(K)]

    def linear(u, t):
        out = h0 * (1 + 0.3 * np.cos(1.7 * t)) if time_dependent else h0
        if u is None:
            return out
        for k in range(K):
            out = out + (u[k].real * g_re[k] + u[k].imag * g_im[k] if complex_controls
                         else u[k] * g_re[k])
        return out
    return linear, rng


def _ensemble(linear, rng, n, K, M=3, J=2):
    d = np.stack([cases_mod.gue(rng, n) for _ in range(J)]) if J else None
    return HamiltonianEnsemble(
        linear, perturbations=d, offsets=0.3 * rng.standard_normal((M, J)) if J else None,
        control_scales=1 + 0.05 * rng.standard_normal((M, K)), weights=rng.uniform(0.2, 1.0, M))


# ---- the constructor ------------------------------------------------------------------------------

_D = np.stack([np.eye(3), np.diag([1.0, -1.0, 0.0])])


@pytest.mark.parametrize("kw, fragment", [
    (dict(offsets=np.zeros((2, 2))), "offsets need perturbations"),
    (dict(perturbations=_D), "perturbations need offsets"),
    (dict(perturbations=_D, offsets=np.zeros((2, 3))), "J = 2"),
    (dict(perturbations=np.ones((2, 3, 2)), offsets=np.zeros((2, 2))), "(J, n, n)"),
    (dict(perturbations=_D, offsets=np.zeros(2)), "offsets must have 2 dimensions"),
    (dict(perturbations=_D, offsets=np.zeros((3, 2)), weights=np.ones(2)), "disagree"),
    (dict(control_scales=np.ones((4, 1)), weights=np.ones(3)), "disagree"),
    (dict(weights=np.array([0.5, -0.1])), "weights must be >= 0"),
    (dict(weights=np.array([0.5, np.nan])), "weights is not finite"),
    (dict(control_scales=np.array([[1.0, np.inf]])), "control_scales is not finite"),
    (dict(perturbations=_D * np.nan, offsets=np.zeros((1, 2))), "perturbations is not finite"),
    (dict(weights=np.zeros(0)), "at least one member"),
    (dict(), "needs offsets, control_scales or weights"),
])
def test_constructor_rejects_bad_arguments(kw, fragment):
    with pytest.raises(ValueError, match=fragment.replace("(", r"\(").replace(")", r"\)")):
        HamiltonianEnsemble(lambda u, t: np.eye(3), **kw)


def test_constructor_reads_m_and_defaults_the_weights():
    with pytest.raises(ValueError, match="callable"):
        HamiltonianEnsemble(np.eye(3), weights=np.ones(2))
    e = HamiltonianEnsemble(lambda u, t: np.eye(3), perturbations=_D, offsets=np.zeros((4, 2)))
    assert e.member_count == 4 and e.perturbation_count == 2 and e.hilbert_size == 3
    assert np.array_equal(e.weights, np.full(4, 0.25))
    assert not callable(e)
    e = HamiltonianEnsemble(lambda u, t: np.eye(3), control_scales=np.ones((2, 5)))
    assert e.member_count == 2 and e.perturbation_count == 0
    with pytest.raises(ValueError, match=r"control_scales must be \(M, control_count\)"):
        e.real_channel_scales(4, False)
    assert e.real_channel_scales(5, True).shape == (2, 10)
    with pytest.raises(IndexError):
        e.member(2)


@pytest.mark.parametrize("complex_controls", [False, True])
def test_member_is_the_scaled_base_plus_the_offsets(complex_controls):
    n, K, M, J = 4, 3, 3, 2
    linear, rng = _system(n, K, seed=7, complex_controls=complex_controls, time_dependent=True)
    e = _ensemble(linear, rng, n, K, M, J)
    for m in range(M):
        h = e.member(m)
        for _ in range(3):
            u = rng.standard_normal(K)
            if complex_controls:
                u = u + 1j * rng.standard_normal(K)
            t = rng.uniform(0, 2)
            want = linear(e.control_scales[m] * u, t) + sum(
                e.offsets[m, j] * e.perturbations[j] for j in range(J))
            assert np.allclose(h(u, t), want, rtol=0, atol=1e-14)


# ---- a stand-in backend WITH the entry point ------------------------------------------------------

class EnsembleStandIn(OracleBackend):
    """The oracle backend plus set_ensemble: it expands the seeds into their members on the host,
    evaluates the (K_r + J)-channel problem it was given, and reduces the member results as the
    engine does (weighted sum in member order, gradients of the fixed channels dropped)."""

    def __init__(self):
        super().__init__()
        self.received = []
        self.ens = None

    def set_schroedinger_problem(self, *a, **kw):
        super().set_schroedinger_problem(*a, **kw)
        self.ens = None

    def set_ensemble(self, scales, offsets, weights):
        n, S, K, Nc, N = self.dims
        weights = np.asarray(weights, dtype=np.float64)
        M = weights.shape[0]
        J = 0 if offsets is None else np.asarray(offsets).shape[1]
        scales = np.ones((M, K - J)) if scales is None else np.asarray(scales, dtype=np.float64)
        offsets = np.zeros((M, 0)) if offsets is None else np.asarray(offsets, dtype=np.float64)
        assert scales.shape == (M, K - J) and offsets.shape == (M, J)
        self.received.append((self.dims, scales.copy(), offsets.copy(), weights.copy()))
        self.ens = (scales, offsets, weights)

    def upload_controls(self, controls):
        n, S, K, Nc, N = self.dims
        scales, offsets, weights = self.ens
        kr, M = scales.shape[1], len(weights)
        u = np.asarray(controls, dtype=np.float64).reshape(-1, Nc, kr)
        items = np.empty((u.shape[0], M, Nc, K))
        items[..., :kr] = scales[None, :, None, :] * u[:, None]
        items[..., kr:] = offsets[None, :, None, :]
        self.seeds = u.shape[0]
        super().upload_controls(items.reshape(-1, Nc, K))

    def download_results(self, want_grad=True, want_final=True):
        n, S, K, Nc, N = self.dims
        scales, offsets, weights = self.ens
        kr, M, B = scales.shape[1], len(weights), self.seeds
        cost, grads, final = super().download_results(want_grad, want_final)
        self.members = cost.reshape(B, M)
        seed_cost = np.zeros(B)
        for m in range(M):
            seed_cost += weights[m] * self.members[:, m]
        seed_grads = None
        if grads is not None:
            g = grads.reshape(B, M, Nc, K)[..., :kr]
            seed_grads = np.zeros((B, Nc, kr))
            for m in range(M):
                seed_grads += (weights[m] * scales[m]) * g[:, m]
        return seed_cost, seed_grads, None if final is None else final.reshape(B, M, S, n)

    def ensemble_member_costs(self):
        return self.members


def _oracle_member(e, m, T, psi0, N, Nc, K, costs, complex_controls):
    return onp.SchroedingerProblem(T, e.member(m), psi0, N, control_eval_count=Nc, costs=costs,
                                   complex_controls=complex_controls, control_count=K)


@pytest.mark.parametrize("complex_controls, time_dependent, step_costs, magnus", [
    (False, False, False, MagnusPolicy.M2),
    (True, True, False, MagnusPolicy.M2),
    (False, True, True, MagnusPolicy.M4),
    (True, False, True, MagnusPolicy.M6),
])
def test_stand_in_reduces_the_weighted_member_evaluations(complex_controls, time_dependent,
                                                          step_costs, magnus):
    n, K, N, Nc, S, M, J, B, T = 4, 2, 9, 5, 2, 3, 2, 2, 0.8
    linear, rng = _system(n, K, seed=31, complex_controls=complex_controls,
                          time_dependent=time_dependent)
    e = _ensemble(linear, rng, n, K, M, J)
    psi0 = cases_mod.column_states(np.eye(n)[:, :S])
    target = cases_mod.column_states(cases_mod.random_unitary(rng, n)[:, :S])
    if step_costs:
        forbid = cases_mod.column_states(np.eye(n)[:, S:S + 1])[None].repeat(S, axis=0)
        costs = [ForbidStates(forbid, N), TargetStateInfidelityTime(N, target)]
        ocosts = [onp.ForbidStates(forbid, N), onp.TargetStateInfidelityTime(N, target)]
    else:
        costs, ocosts = [TargetStateInfidelity(target)], [onp.TargetStateInfidelity(target)]
    backend = EnsembleStandIn()
    ev = device.SchroedingerEvaluator(
        T, e, psi0, N, control_count=K, control_eval_count=Nc, complex_controls=complex_controls,
        costs=costs, magnus_policy=magnus, backend=backend)
    kr = K * (2 if complex_controls else 1)
    assert ev.ensemble is e and ev.opaque_hamiltonian is None
    assert ev.linearized_hamiltonian is None
    (dims, scales, offsets, weights), = backend.received
    assert dims[2] == kr + J
    assert np.array_equal(scales, e.real_channel_scales(K, complex_controls))
    assert np.array_equal(offsets, e.offsets) and np.array_equal(weights, e.weights)
    # the problem's last J channels are the D_j (at every probe time)
    t = 0.37
    h0 = backend.problem.hamiltonian(np.zeros(kr + J), t)
    for j in range(J):
        unit = np.zeros(kr + J)
        unit[kr + j] = 1.0
        assert np.allclose(backend.problem.hamiltonian(unit, t) - h0, e.perturbations[j],
                           rtol=0, atol=1e-13)
    u = 0.5 * rng.standard_normal((B, Nc, K))
    if complex_controls:
        u = u + 0.5j * rng.standard_normal((B, Nc, K))
    errors, grads, finals, _ = ev.evaluate_batch(u)
    assert finals.shape == (B, M, S, n, 1)
    members = ev.member_errors()
    assert members.shape == (B, M)
    for b in range(B):
        want_err, want_grad = 0.0, 0.0
        for m in range(M):
            p = _oracle_member(e, m, T, psi0, N, Nc, K, ocosts, complex_controls)
            p.magnus_policy = magnus.short
            err, gr, fin = onp.evaluate_with_grad(p, u[b])
            assert abs(members[b, m] - err) < 1e-12
            assert np.max(np.abs(finals[b, m] - fin)) < 1e-12
            want_err += e.weights[m] * err
            want_grad = want_grad + e.weights[m] * gr
        assert abs(errors[b] - want_err) < 1e-12
        if not complex_controls:
            want_grad = np.real(want_grad)
        assert np.max(np.abs(grads[b] - want_grad)) < 1e-12


def test_costs_of_the_controls_are_added_once_per_seed():
    n, K, N, Nc, M = 4, 2, 7, 4, 3
    linear, rng = _system(n, K, seed=5)
    e = _ensemble(linear, rng, n, K, M, J=1)
    psi0 = cases_mod.column_states(np.eye(n)[:, :1])
    target = cases_mod.column_states(np.roll(np.eye(n), 1, axis=0)[:, :1])
    norm = ControlNorm(K, Nc, cost_multiplier=0.3)
    kw = dict(control_count=K, control_eval_count=Nc)
    plain = device.SchroedingerEvaluator(0.6, e, psi0, N, costs=[TargetStateInfidelity(target)],
                                         backend=EnsembleStandIn(), **kw)
    with_norm = device.SchroedingerEvaluator(
        0.6, e, psi0, N, costs=[TargetStateInfidelity(target), norm], backend=EnsembleStandIn(),
        **kw)
    assert with_norm.host_costs == [norm]
    u = 0.4 * rng.standard_normal((2, Nc, K))
    e0, g0, _, _ = plain.evaluate_batch(u)
    e1, g1, _, _ = with_norm.evaluate_batch(u)
    for b in range(2):
        assert abs(e1[b] - (e0[b] + norm.cost(u[b], None, N - 1))) < 1e-14
        assert np.max(np.abs(g1[b] - (g0[b] + norm.controls_bar(u[b], None, N - 1)))) < 1e-14


def test_entry_points_return_member_axes_and_member_errors():
    n, K, N, Nc, M, S = 4, 2, 7, 4, 3, 2
    linear, rng = _system(n, K, seed=9)
    e = _ensemble(linear, rng, n, K, M, J=2)
    psi0 = cases_mod.column_states(np.eye(n)[:, :S])
    target = cases_mod.column_states(np.roll(np.eye(n), 1, axis=0)[:, :S])
    costs = [TargetStateInfidelity(target)]
    u = np.clip(0.4 * rng.standard_normal((Nc, K)), -0.9, 0.9)
    helpers.set_backend_factory(EnsembleStandIn)
    try:
        r = qoc_amd.evolve_schroedinger_discrete(0.6, e, psi0, N, controls=u, costs=costs)
        assert r.final_states.shape == (M, S, n, 1) and r.member_errors.shape == (M,)
        assert abs(r.error - np.dot(e.weights, r.member_errors)) < 1e-14
        g = qoc_amd.grape_schroedinger_discrete(
            K, Nc, costs, 0.6, e, psi0, N, initial_controls=u, iteration_count=3,
            log_iteration_step=0)
        assert g.best_final_states.shape == (M, S, n, 1)
        assert abs(g.best_error - np.dot(e.weights, g.member_errors)) < 1e-14
        u0 = np.clip(0.4 * rng.standard_normal((2, Nc, K)), -0.9, 0.9)
        gb = qoc_amd.grape_schroedinger_discrete_batch(
            K, Nc, costs, 0.6, e, psi0, N, u0, iteration_count=3, log_iteration_step=0)
        for b in range(2):
            assert gb.best_final_states[b].shape == (M, S, n, 1)
            assert abs(gb.best_error[b] - np.dot(e.weights, gb.member_errors[b])) < 1e-14
        assert np.array_equal(gb.best.member_errors, gb.member_errors[int(np.argmin(gb.best_error))])
    finally:
        helpers.set_backend_factory(None)


# ---- rejections -----------------------------------------------------------------------------------

class _UserCost(Cost):
    name = "user"

    def cost(self, controls, states, step):
        return float(np.abs(states[0, 0, 0]) ** 2)


def test_rejections():
    n, K, N, Nc = 4, 2, 7, 4
    linear, rng = _system(n, K, seed=13)
    e = _ensemble(linear, rng, n, K, 2, J=1)
    psi0 = cases_mod.column_states(np.eye(n)[:, :1])
    target = cases_mod.column_states(np.roll(np.eye(n), 1, axis=0)[:, :1])
    costs = [TargetStateInfidelity(target)]
    kw = dict(control_count=K, control_eval_count=Nc)
    with pytest.raises(NotImplementedError, match="set_ensemble"):
        device.SchroedingerEvaluator(0.6, e, psi0, N, costs=costs, backend=OracleBackend(), **kw)
    nonlinear = HamiltonianEnsemble(lambda u, t: linear(u, t) + u[0] ** 2 * np.eye(n),
                                    weights=np.ones(2))
    with pytest.raises(NotImplementedError, match="linear in the controls"):
        device.SchroedingerEvaluator(0.6, nonlinear, psi0, N, costs=costs,
                                     backend=EnsembleStandIn(), **kw)
    quad = HamiltonianEnsemble(QuadraticHamiltonian(linear, [(0, 0, np.eye(n))]),
                               weights=np.ones(2))
    with pytest.raises(NotImplementedError, match="linear in the controls"):
        device.SchroedingerEvaluator(0.6, quad, psi0, N, costs=costs, backend=EnsembleStandIn(),
                                     **kw)
    with pytest.raises(NotImplementedError, match="device"):
        device.SchroedingerEvaluator(0.6, e, psi0, N, costs=costs + [_UserCost()],
                                     backend=EnsembleStandIn(), **kw)
    with pytest.raises(NotImplementedError, match="at least one control"):
        device.SchroedingerEvaluator(0.6, e, psi0, N, costs=costs, backend=EnsembleStandIn())
    with pytest.raises(ValueError, match="control_scales"):
        device.SchroedingerEvaluator(0.6, e, psi0, N, costs=costs, backend=EnsembleStandIn(),
                                     control_count=K + 1, control_eval_count=Nc)
    with pytest.raises(ValueError, match="perturbations are 4 x 4"):
        device.SchroedingerEvaluator(0.6, e, cases_mod.column_states(np.eye(5)[:, :1]), N,
                                     costs=costs, backend=EnsembleStandIn(), **kw)
    u = np.clip(0.3 * rng.standard_normal((Nc, K)), -0.9, 0.9)
    with pytest.raises(NotImplementedError, match="save"):
        qoc_amd.evolve_schroedinger_discrete(0.6, e, psi0, N, controls=u, costs=costs,
                                             save_file_path="unused.h5")
    with pytest.raises(NotImplementedError, match="save"):
        qoc_amd.grape_schroedinger_discrete(K, Nc, costs, 0.6, e, psi0, N, initial_controls=u,
                                            save_file_path="unused.h5")
    rho0 = np.eye(n, dtype=np.complex128)[None] / n
    with pytest.raises(NotImplementedError, match="Lindblad"):
        qoc_amd.evolve_lindblad_discrete(0.6, rho0, N, controls=u, hamiltonian=e)
    with pytest.raises(NotImplementedError, match="Lindblad"):
        qoc_amd.grape_lindblad_discrete(K, Nc, [], 0.6, rho0, N, hamiltonian=e,
                                        initial_controls=u)
    with pytest.raises(NotImplementedError, match="Lindblad"):
        qoc_amd.grape_lindblad_discrete_batch(K, Nc, [], 0.6, rho0, N, u[None], hamiltonian=e)


def test_the_abi_declares_the_entry_points():
    lib = engine.load_library()
    for name in ("qocx_set_ensemble", "qocx_ensemble_download_members"):
        assert name in engine.SIGNATURES
        assert hasattr(lib, name)
    assert hasattr(engine.Engine, "set_ensemble")
    assert hasattr(engine.Engine, "ensemble_member_costs")
