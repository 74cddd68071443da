"""CPU tests of HamiltonianEnsemble on the Lindblad path (no GPU): a stand-in backend with
set_lindblad_ensemble (where the evaluator must hand over the (K_r + J)-channel problem and reduce
nothing itself), the evaluator and the three entry points with real and complex controls and a
time-dependent base, the rejections, and the ABI.

Member references: the plain Lindblad problem of ensemble.member(m) - sum_j delta_mj D_j folded into
the Hamiltonian - through the same NumPy model of the device algorithm (tests/lindblad_model.py).
An ensemble item carries the D_j as control channels instead, so the two integrate on different
sub-interval grids; each is a converged fixed-step DOP853 (1e-10 against the
reference), hence 1e-9 on costs and densities and 1e-8 on gradients here. What the stand-in and the
evaluator add on top (weighted sums) is held to rounding: 1e-13.
"""

import numpy as np
import pytest

import qoc_amd
from qoc_amd import engine
from qoc_amd.core import device
from qoc_amd.models.cost import Cost
from qoc_amd.standard import (Adam, ControlNorm, HamiltonianEnsemble, QuadraticHamiltonian,
                              TargetDensityInfidelity)
from tests import cases as cases_mod
from tests import helpers
from tests.oracle_backend import OracleBackend
from tests.test_lindblad_host_api import product_cost_list


class LindbladEnsembleStandIn(OracleBackend):
    """The oracle backend plus set_lindblad_ensemble: it expands the seeds into their members on
    the host, evaluates every item of the (K_r + J)-channel problem it was given through the
    oracle, and reduces the member results as the engine does (weighted sum in member order,
    gradients of the fixed channels dropped)."""

    def __init__(self):
        super().__init__()
        self.problems = []   # (positional arguments, keywords) of every set_lindblad_problem
        self.received = []   # (K of the problem, scales, offsets, weights) of every ensemble
        self.ens = None

    def set_lindblad_problem(self, *a, **kw):
        super().set_lindblad_problem(*a, **kw)
        self.problems.append((a, kw))
        self.ens = None

    def set_lindblad_ensemble(self, scales, offsets, weights):
        K = self.lb["K"]
        weights = np.asarray(weights, dtype=np.float64)
        M = weights.shape[0]
        J = 0 if offsets is None else np.asarray(offsets).shape[1]
        scales = np.ones((M, K - J)) if scales is None else np.asarray(scales, dtype=np.float64)
        offsets = np.zeros((M, 0)) if offsets is None else np.asarray(offsets, dtype=np.float64)
        assert scales.shape == (M, K - J) and offsets.shape == (M, J)
        self.received.append((K, scales.copy(), offsets.copy(), weights.copy()))
        self.ens = (scales, offsets, weights)

    def evaluate_lindblad(self, controls, want_grad=True, want_final=True):
        if self.ens is None:
            return super().evaluate_lindblad(controls, want_grad, want_final)
        p = self.lb
        scales, offsets, weights = self.ens
        kr, M, K, Nc = scales.shape[1], len(weights), p["K"], p["Nc"]
        u = np.asarray(controls, dtype=np.float64).reshape(-1, Nc, kr)
        B = u.shape[0]
        items = np.empty((B, M, Nc, K))
        items[..., :kr] = scales[None, :, None, :] * u[:, None]
        items[..., kr:] = offsets[None, :, None, :]
        cost, grads, final = super().evaluate_lindblad(items.reshape(-1, Nc, K), want_grad,
                                                       want_final)
        self.members = cost.reshape(B, M)
        self.item_grads = None if grads is None else grads.reshape(B, M, Nc, K)
        if self.keep:
            self.lb_steps = list(np.stack(self.lb_steps).reshape(
                (B, M) + self.lb_steps[0].shape))
        seed_cost = np.zeros(B)
        for m in range(M):
            seed_cost += weights[m] * self.members[:, m]
        seed_grads = None
        if grads is not None:
            seed_grads = np.zeros((B, Nc, kr))
            for m in range(M):
                seed_grads += (weights[m] * scales[m]) * self.item_grads[:, m, :, :kr]
        return seed_cost, seed_grads, final.reshape((B, M) + final.shape[1:])

    def lindblad_ensemble_member_costs(self):
        return self.members


def _ensemble(case, rng, M=3, J=2, scales=True):
    d = np.stack([0.5 * cases_mod.gue(rng, case.n) for _ in range(J)]) if J else None
    return HamiltonianEnsemble(
        case.hamiltonian(), perturbations=d,
        offsets=0.3 * rng.standard_normal((M, J)) if J else None,
        control_scales=1 + 0.05 * rng.standard_normal((M, case.K)) if scales else None,
        weights=rng.uniform(0.2, 1.0, M))


def _evaluator(case, hamiltonian, backend, costs=None, **kw):
    return device.LindbladEvaluator(
        case.T, case.initial_densities, case.N, hamiltonian=hamiltonian,
        lindblad_data=case.lindblad_data(), control_count=case.K, control_eval_count=case.Nc,
        complex_controls=case.complex_controls,
        costs=product_cost_list(case) if costs is None else costs,
        cost_eval_step=case.cost_eval_step, backend=backend, **kw)


def _seeds(case, rng, B, sigma=0.4):
    u = sigma * rng.standard_normal((B, case.Nc, case.K))
    if case.complex_controls:
        u = u + 1j * sigma * rng.standard_normal((B, case.Nc, case.K))
    return u


@pytest.mark.parametrize("name", ["lindblad_n4", "lindblad_n4_complex", "lindblad_timedep"])
def test_evaluator_reduces_the_weighted_member_evaluations(name):
    """Real controls with step costs, complex controls, and a time-dependent base (stage tables)."""
    case = cases_mod.lindblad_case_by_name(name)
    rng = np.random.default_rng(41)
    M, J, B = 3, 2, 2
    e = _ensemble(case, rng, M, J)
    backend = LindbladEnsembleStandIn()
    ev = _evaluator(case, e, backend)
    kr = case.K * (2 if case.complex_controls else 1)
    assert ev.ensemble is e and ev.linearized_hamiltonian is None
    assert ev.time_dependent == (case.time_mod is not None)
    u = _seeds(case, rng, B)
    errors, grads, finals, _ = ev.evaluate_batch(u)
    K, scales, offsets, weights = backend.received[-1]
    assert K == kr + J
    assert np.array_equal(scales, e.real_channel_scales(case.K, case.complex_controls))
    assert np.array_equal(offsets, e.offsets) and np.array_equal(weights, e.weights)
    # the problem's last J channels are the D_j
    g = np.asarray(backend.problems[-1][0][7])
    assert g.shape[0] == kr + J and np.array_equal(g[kr:], e.perturbations)
    S, n = case.initial_densities.shape[0], case.n
    assert finals.shape == (B, M, S, n, n)
    members = ev.member_errors()
    assert members.shape == (B, M)
    assert grads.shape == u.shape and np.iscomplexobj(grads) == case.complex_controls
    member_evs = [_evaluator(case, e.member(m), OracleBackend()) for m in range(M)]
    for b in range(B):
        want_err, want_grad = 0.0, 0.0
        for m in range(M):
            err, gr, fin, _ = member_evs[m].evaluate(u[b])
            assert abs(members[b, m] - err) < 1e-9
            assert np.max(np.abs(finals[b, m] - fin)) < 1e-9
            want_err += e.weights[m] * err
            want_grad = want_grad + e.weights[m] * gr  # (d/du of member(m): s_mk dc/dr)
        assert abs(errors[b] - want_err) < 1e-9
        assert abs(errors[b] - np.dot(e.weights, members[b])) < 1e-13
        assert np.max(np.abs(grads[b] - want_grad)) < 1e-8
        # the gradient is sum_m w_m s_mk dc_(b,m)/dr of the items the backend evaluated
        item = backend.item_grads[b][..., :kr]
        folded = sum(e.weights[m] * scales[m] * item[m] for m in range(M))
        folded = folded[..., 0::2] + 1j * folded[..., 1::2] if case.complex_controls else folded
        assert np.max(np.abs(grads[b] - folded)) < 1e-13


def test_step_densities_carry_the_member_axis():
    case = cases_mod.lindblad_case_by_name("lindblad_n4")
    rng = np.random.default_rng(42)
    e = _ensemble(case, rng, M=2, J=1)
    ev = _evaluator(case, e, LindbladEnsembleStandIn())
    u = _seeds(case, rng, 2)
    _, _, finals, steps = ev.evaluate_batch(u, want_grad=False, want_step_densities=True)
    S, n = case.initial_densities.shape[0], case.n
    assert steps.shape == (2, 2, case.N, S, n, n)
    assert np.max(np.abs(steps[:, :, -1] - finals)) < 1e-13


def test_time_dependent_drive_repeats_the_perturbations_in_every_stage_table():
    """G_k(t): the host samples g at the stage times and appends the D_j to every table; the
    bounds that size the fixed grid are the items' (bound_k max_m |s_mk|, max_m |delta_mj|)."""
    case = cases_mod.lindblad_case_by_name("lindblad_timedep")
    rng = np.random.default_rng(43)
    base = case.hamiltonian()
    zero = np.zeros(case.K)

    def driven(u, t):  # the first drive operator breathes
        unit = np.array([1.0] + [0.0] * (case.K - 1))
        return base(u, t) + 0.2 * np.cos(2.3 * t) * u[0] * (base(unit, t) - base(zero, t))
    M, J = 2, 1
    d = np.stack([3.0 * cases_mod.gue(rng, case.n)])
    offsets = np.array([[0.9], [-1.4]])
    scales = np.array([[1.0, 1.0], [2.5, 0.5]])
    e = HamiltonianEnsemble(driven, perturbations=d, offsets=offsets, control_scales=scales,
                            weights=np.array([0.5, 0.5]))
    backend = LindbladEnsembleStandIn()
    bounds = np.array([1.2, 0.7])
    ev = _evaluator(case, e, backend, control_bounds=bounds)
    args, kw = backend.problems[-1]
    assert backend.ens is not None  # (set again after the problem with its tables)
    g_stages = np.asarray(kw["g_stages"])
    assert g_stages.shape[1] == case.K + J
    assert np.array_equal(g_stages[:, case.K:], np.broadcast_to(d[None], g_stages[:, case.K:].shape))
    assert not np.array_equal(g_stages[0, 0], g_stages[5, 0])
    assert np.array_equal(ev._item_bounds(bounds), np.array([1.2 * 2.5, 0.7 * 1.0, 1.4]))
    # the grid covers the largest item: the seeds' bounds alone would give a coarser one
    plain = LindbladEnsembleStandIn()
    _evaluator(case, driven, plain, control_bounds=bounds)
    assert kw["fixed_subdivision"] > plain.problems[-1][1]["fixed_subdivision"]
    u = np.clip(_seeds(case, rng, 1), -0.7, 0.7)
    errors, _, finals, _ = ev.evaluate_batch(u)
    assert len(backend.problems) == 1  # the tables were wide enough: not rebuilt
    for m in range(M):
        err, _, fin, _ = _evaluator(case, e.member(m), OracleBackend()).evaluate(u[0])
        assert abs(ev.member_errors()[0, m] - err) < 1e-9
        assert np.max(np.abs(finals[0, m] - fin)) < 1e-9


def test_costs_of_the_controls_are_added_once_per_seed():
    case = cases_mod.lindblad_case_by_name("lindblad_n4")
    rng = np.random.default_rng(44)
    e = _ensemble(case, rng, M=3, J=1)
    norm = ControlNorm(case.K, case.Nc, cost_multiplier=0.3)
    costs = product_cost_list(case)
    plain = _evaluator(case, e, LindbladEnsembleStandIn(), costs=costs)
    with_norm = _evaluator(case, e, LindbladEnsembleStandIn(), costs=costs + [norm])
    assert with_norm.host_costs == [norm]
    u = _seeds(case, rng, 2)
    e0, g0, _, _ = plain.evaluate_batch(u)
    e1, g1, _, _ = with_norm.evaluate_batch(u)
    for b in range(2):
        assert abs(e1[b] - (e0[b] + norm.cost(u[b], None, case.N - 1))) < 1e-14
        assert np.max(np.abs(g1[b] - (g0[b] + norm.controls_bar(u[b], None, case.N - 1)))) < 1e-14


@pytest.mark.parametrize("name", ["lindblad_n4", "lindblad_n4_complex", "lindblad_timedep"])
def test_entry_points_return_member_axes_and_member_errors(name):
    case = cases_mod.lindblad_case_by_name(name)
    rng = np.random.default_rng(45)
    M = 3
    e = _ensemble(case, rng, M, J=2)
    S, n = case.initial_densities.shape[0], case.n
    costs = product_cost_list(case)
    u = 0.5 * _seeds(case, rng, 1)[0]
    kw = dict(cost_eval_step=case.cost_eval_step, hamiltonian=e,
              lindblad_data=case.lindblad_data())
    helpers.set_backend_factory(LindbladEnsembleStandIn)
    try:
        r = qoc_amd.evolve_lindblad_discrete(case.T, case.initial_densities, case.N, controls=u,
                                             costs=costs, **kw)
        assert r.final_densities.shape == (M, S, n, n) and r.member_errors.shape == (M,)
        assert abs(r.error - np.dot(e.weights, r.member_errors)) < 1e-13
        member = qoc_amd.evolve_lindblad_discrete(
            case.T, case.initial_densities, case.N, controls=u, costs=costs,
            **dict(kw, hamiltonian=e.member(1)))
        assert abs(member.error - r.member_errors[1]) < 1e-9
        gkw = dict(kw, complex_controls=case.complex_controls, iteration_count=3,
                   log_iteration_step=0, optimizer=Adam(learning_rate=1e-2))
        g = qoc_amd.grape_lindblad_discrete(case.K, case.Nc, costs, case.T,
                                            case.initial_densities, case.N, initial_controls=u,
                                            **gkw)
        assert g.best_final_densities.shape == (M, S, n, n)
        assert abs(g.best_error - np.dot(e.weights, g.member_errors)) < 1e-13
        u0 = 0.5 * _seeds(case, rng, 2)
        gb = qoc_amd.grape_lindblad_discrete_batch(case.K, case.Nc, costs, case.T,
                                                   case.initial_densities, case.N, u0, **gkw)
        for b in range(2):
            assert gb.best_final_densities[b].shape == (M, S, n, n)
            assert abs(gb.best_error[b] - np.dot(e.weights, gb.member_errors[b])) < 1e-13
        assert np.array_equal(gb.best.member_errors, gb.member_errors[int(np.argmin(gb.best_error))])
        # seed 0 of the batch walks the single-seed trajectory
        one = qoc_amd.grape_lindblad_discrete(case.K, case.Nc, costs, case.T,
                                              case.initial_densities, case.N,
                                              initial_controls=u0[0], **gkw)
        assert abs(one.best_error - gb.best_error[0]) < 1e-13
        assert np.max(np.abs(one.member_errors - gb.member_errors[0])) < 1e-13
    finally:
        helpers.set_backend_factory(None)


# ---- rejections -----------------------------------------------------------------------------------

class _UserCost(Cost):
    name = "user"

    def cost(self, controls, densities, step):
        return float(np.real(densities[0, 0, 0]))


def test_rejections():
    case = cases_mod.lindblad_case_by_name("lindblad_n4")
    rng = np.random.default_rng(46)
    e = _ensemble(case, rng, M=2, J=1)
    n, K = case.n, case.K
    linear = case.hamiltonian()
    costs = product_cost_list(case)
    # K_r + J > 8: the Lindblad engine's channel limit, named
    wide = HamiltonianEnsemble(
        linear, perturbations=np.stack([cases_mod.gue(rng, n) for _ in range(7)]),
        offsets=np.zeros((2, 7)))
    with pytest.raises(NotImplementedError, match=r"Lindblad engine takes up to 8 .* 2 \+ 7"):
        _evaluator(case, wide, LindbladEnsembleStandIn())
    fits = HamiltonianEnsemble(
        linear, perturbations=np.stack([cases_mod.gue(rng, n) for _ in range(6)]),
        offsets=np.zeros((2, 6)))
    assert _evaluator(case, fits, LindbladEnsembleStandIn()).device_k == 8
    # a base that is not linear in the controls, a QuadraticHamiltonian base, frozen controls
    nonlinear = HamiltonianEnsemble(lambda u, t: linear(u, t) + u[0] ** 2 * np.eye(n),
                                    weights=np.ones(2))
    with pytest.raises(NotImplementedError, match="linear in the controls"):
        _evaluator(case, nonlinear, LindbladEnsembleStandIn())
    quad = HamiltonianEnsemble(QuadraticHamiltonian(linear, [(0, 0, np.eye(n))]),
                               weights=np.ones(2))
    with pytest.raises(NotImplementedError, match="linear in the controls"):
        _evaluator(case, quad, LindbladEnsembleStandIn())
    with pytest.raises(NotImplementedError, match="linear in the controls"):
        _evaluator(case, e, LindbladEnsembleStandIn(), need_gradients=False,
                   frozen_controls=case.controls[0])
    # quadratic_scales come with a QuadraticHamiltonian base only: refused with it
    scaled = HamiltonianEnsemble(QuadraticHamiltonian(linear, [(0, 0, np.eye(n))]),
                                 weights=np.ones(2), quadratic_scales=np.ones((2, 1)))
    with pytest.raises(NotImplementedError, match="linear in the controls"):
        _evaluator(case, scaled, LindbladEnsembleStandIn())
    # a cost without a device descriptor; a backend without the entry point; no controls
    with pytest.raises(NotImplementedError, match="device"):
        _evaluator(case, e, LindbladEnsembleStandIn(), costs=costs + [_UserCost()])
    with pytest.raises(NotImplementedError, match="set_lindblad_ensemble"):
        _evaluator(case, e, OracleBackend())
    with pytest.raises(NotImplementedError, match="at least one control"):
        device.LindbladEvaluator(case.T, case.initial_densities, case.N, hamiltonian=e,
                                 lindblad_data=case.lindblad_data(), costs=costs,
                                 backend=LindbladEnsembleStandIn())
    with pytest.raises(ValueError, match="perturbations are 4 x 4"):
        device.LindbladEvaluator(case.T, np.eye(5, dtype=np.complex128)[None] / 5, case.N,
                                 hamiltonian=e, control_count=K, control_eval_count=case.Nc,
                                 costs=[TargetDensityInfidelity(np.eye(5)[None] / 5)],
                                 backend=LindbladEnsembleStandIn())
    # no costs: nothing to weigh - refused before a backend is made (none is installed here)
    with pytest.raises(NotImplementedError, match="Lindblad path needs at least one cost"):
        device.LindbladEvaluator(case.T, case.initial_densities, case.N, hamiltonian=e,
                                 control_count=K, control_eval_count=case.Nc, costs=[])
    u = case.controls[0]
    args = (K, case.Nc, costs, case.T, case.initial_densities, case.N)
    # save files: refused before the file is touched and before a backend is made
    with pytest.raises(NotImplementedError, match="save"):
        qoc_amd.evolve_lindblad_discrete(case.T, case.initial_densities, case.N, controls=u,
                                         costs=costs, hamiltonian=e, save_file_path="unused.h5")
    with pytest.raises(NotImplementedError, match="save"):
        qoc_amd.grape_lindblad_discrete(*args, hamiltonian=e, initial_controls=u,
                                        save_file_path="unused.h5")
    for call in (
            lambda: qoc_amd.evolve_lindblad_discrete(case.T, case.initial_densities, case.N,
                                                     controls=u, hamiltonian=e),
            lambda: qoc_amd.grape_lindblad_discrete(K, case.Nc, [], *args[3:], hamiltonian=e,
                                                    initial_controls=u),
            lambda: qoc_amd.grape_lindblad_discrete_batch(K, case.Nc, [], *args[3:], u[None],
                                                          hamiltonian=e)):
        with pytest.raises(NotImplementedError, match="Lindblad path needs at least one cost"):
            call()


def test_the_abi_declares_the_entry_points():
    lib = engine.load_library()
    for name in ("qocx_lindblad_set_ensemble", "qocx_lindblad_ensemble_download_members"):
        assert name in engine.SIGNATURES
        assert hasattr(lib, name)
    vp, i32, dp = engine._VP, engine._I32, engine._c_double_p
    assert engine.SIGNATURES["qocx_lindblad_set_ensemble"] == (
        engine.ctypes.c_int, [vp, i32, i32, dp, dp, dp])
    assert engine.SIGNATURES["qocx_lindblad_set_ensemble"] == engine.SIGNATURES["qocx_set_ensemble"]
    assert engine.SIGNATURES["qocx_lindblad_ensemble_download_members"] == (
        engine.ctypes.c_int, [vp, dp])
    assert hasattr(engine.Engine, "set_lindblad_ensemble")
    assert hasattr(engine.Engine, "lindblad_ensemble_member_costs")
