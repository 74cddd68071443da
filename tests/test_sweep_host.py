"""CPU tests of qoc_amd.standard.HamiltonianSweep and its host routing (no GPU): the constructor's
checks, member(b), slice, the algebra of a duration sweep, a stand-in backend that takes sweeps
(where the evaluator must hand over the (K_r + J)-channel problem and the per-seed tables), the
batch driver's host loop against single-seed GRAPE on member(b), rank slicing, and the refusals."""

import os
import socket
import sys

import numpy as np
import pytest

import qoc_amd
from oracle import qoc_numpy as onp
from qoc_amd import engine, parallel
from qoc_amd.core import device
from qoc_amd.models import MagnusPolicy
from qoc_amd.models.cost import Cost
from qoc_amd.standard import (LBFGS, SGD, Adam, ControlBandwidthMax, ControlNorm,
                              HamiltonianEnsemble, HamiltonianSweep, QuadraticHamiltonian,
                              TargetStateInfidelity)
from tests import cases as cases_mod
from tests import helpers
from tests.oracle_backend import OracleBackend

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _system(n=4, K=2, seed=3, complex_controls=False, time_dependent=False):
    rng = np.random.default_rng(seed)
    h0 = cases_mod.gue(rng, n)
    g_re = [cases_mod.gue(rng, n) for _ in range(K)]
    g_im = [cases_mod.gue(rng, n) for _ in range(K)]

    def linear(u, t):
        out = h0 * (1 + 0.3 * np.cos(1.7 * t)) if time_dependent else h0
        for k in range(K):
            out = out + (u[k].real * g_re[k] + u[k].imag * g_im[k] if complex_controls
                         else u[k] * g_re[k])
        return out
    return linear, rng


def _sweep(linear, rng, n, K, B=3, J=2):
    d = np.stack([cases_mod.gue(rng, n) for _ in range(J)]) if J else None
    return HamiltonianSweep(
        linear, perturbations=d, offsets=0.3 * rng.standard_normal((B, J)) if J else None,
        control_scales=1 + 0.05 * rng.standard_normal((B, K)))


class SweepStandIn(OracleBackend):
    """The oracle backend plus set_sweep: it expands seed b into item b on the host, evaluates the
    (K_r + J)-channel problem it was given and takes the items' results back to the seeds as the
    engine does (grad_b = s_b * item gradient, the fixed channels dropped; the sensitivities are the
    plain sums over the knots)."""

    def __init__(self):
        super().__init__()
        self.received = []
        self.swp = None

    def set_schroedinger_problem(self, *a, **kw):
        super().set_schroedinger_problem(*a, **kw)
        self.swp = None

    def set_sweep(self, scales, offsets):
        n, S, K, Nc, N = self.dims
        J = 0 if offsets is None else np.asarray(offsets).shape[1]
        B = len(scales) if scales is not None else len(offsets)
        scales = np.ones((B, K - J)) if scales is None else np.asarray(scales, dtype=np.float64)
        offsets = np.zeros((B, 0)) if offsets is None else np.asarray(offsets, dtype=np.float64)
        assert scales.shape == (B, K - J) and offsets.shape == (B, J)
        self.received.append((self.dims, scales.copy(), offsets.copy()))
        self.swp = (scales, offsets)

    def upload_controls(self, controls):
        n, S, K, Nc, N = self.dims
        scales, offsets = self.swp
        kr = scales.shape[1]
        u = np.asarray(controls, dtype=np.float64).reshape(-1, Nc, kr)
        assert u.shape[0] == scales.shape[0], "a sweep takes exactly its own seed count"
        items = np.empty((u.shape[0], Nc, K))
        items[..., :kr] = scales[:, None, :] * u
        items[..., kr:] = offsets[:, None, :]
        self.seed_controls = u
        super().upload_controls(items)

    def download_results(self, want_grad=True, want_final=True):
        scales, offsets = self.swp
        kr = scales.shape[1]
        cost, grads, final = super().download_results(want_grad, want_final)
        self.item_grads = grads
        return cost, None if grads is None else scales[:, None, :] * grads[..., :kr], final

    def sweep_sensitivities(self):
        kr = self.swp[0].shape[1]
        g = self.item_grads
        return (np.sum(self.seed_controls * g[..., :kr], axis=1), np.sum(g[..., kr:], axis=1))


# ---- the constructor ------------------------------------------------------------------------------

_D = np.stack([np.eye(3), np.diag([1.0, -1.0, 0.0])])


@pytest.mark.parametrize("kw, fragment", [
    (dict(offsets=np.zeros((2, 2))), "offsets need perturbations"),
    (dict(perturbations=_D), "perturbations need offsets"),
    (dict(perturbations=_D, offsets=np.zeros((2, 3))), "J = 2"),
    (dict(perturbations=np.ones((2, 3, 2)), offsets=np.zeros((2, 2))), "(J, n, n)"),
    (dict(perturbations=_D, offsets=np.zeros(2)), "offsets must have 2 dimensions"),
    (dict(perturbations=_D, offsets=np.zeros((3, 2)), control_scales=np.ones((2, 1))), "disagree"),
    (dict(control_scales=np.array([[1.0, np.inf]])), "control_scales is not finite"),
    (dict(perturbations=_D, offsets=np.array([[0.0, np.nan]])), "offsets is not finite"),
    (dict(perturbations=_D * np.nan, offsets=np.zeros((1, 2))), "perturbations is not finite"),
    (dict(control_scales=np.zeros((0, 2))), "at least one seed"),
    (dict(), "needs offsets or control_scales"),
])
def test_constructor_rejects_bad_arguments(kw, fragment):
    with pytest.raises(ValueError, match=fragment.replace("(", r"\(").replace(")", r"\)")):
        HamiltonianSweep(lambda u, t: np.eye(3), **kw)


def test_constructor_reads_b_and_the_object_is_not_callable():
    with pytest.raises(ValueError, match="callable"):
        HamiltonianSweep(np.eye(3), control_scales=np.ones((2, 1)))
    w = HamiltonianSweep(lambda u, t: np.eye(3), perturbations=_D, offsets=np.zeros((4, 2)))
    assert w.seed_count == 4 and w.perturbation_count == 2 and w.hilbert_size == 3
    assert not callable(w) and not w.time_scaled and w.evolution_times is None
    w = HamiltonianSweep(lambda u, t: np.eye(3), control_scales=np.ones((2, 5)))
    assert w.seed_count == 2 and w.perturbation_count == 0
    with pytest.raises(ValueError, match=r"control_scales must be \(B, control_count\)"):
        w.real_channel_scales(4, False)
    assert w.real_channel_scales(5, True).shape == (2, 10)
    with pytest.raises(IndexError):
        w.member(2)
    with pytest.raises(IndexError):
        w.slice(1, 1)
    with pytest.raises(ValueError, match="duration sweep"):
        w.time_gradients(np.zeros((2, 5)), np.zeros((2, 0)))


@pytest.mark.parametrize("complex_controls", [False, True])
def test_member_is_the_scaled_base_plus_the_offsets_and_slice_keeps_it(complex_controls):
    n, K, B, J = 4, 3, 4, 2
    linear, rng = _system(n, K, seed=7, complex_controls=complex_controls, time_dependent=True)
    w = _sweep(linear, rng, n, K, B, J)
    part = w.slice(1, 3)
    assert part.seed_count == 2
    assert np.array_equal(part.offsets, w.offsets[1:3])
    assert np.array_equal(part.control_scales, w.control_scales[1:3])
    for b in range(B):
        h = w.member(b)
        for _ in range(3):
            u = rng.standard_normal(K)
            if complex_controls:
                u = u + 1j * rng.standard_normal(K)
            t = rng.uniform(0, 2)
            want = linear(w.control_scales[b] * u, t) + sum(
                w.offsets[b, j] * w.perturbations[j] for j in range(J))
            assert np.allclose(h(u, t), want, rtol=0, atol=1e-14)
            if 1 <= b < 3:
                assert np.array_equal(part.member(b - 1)(u, t), h(u, t))


# ---- duration sweeps --------------------------------------------------------------------------------

@pytest.mark.parametrize("kw, fragment", [
    (dict(evolution_times=[1.0, 0.0]), "evolution_times must be > 0"),
    (dict(evolution_times=[1.0, np.inf]), "evolution_times is not finite"),
    (dict(evolution_times=[]), "at least one seed"),
    (dict(evolution_times=[1.0], reference_time=0.0), "reference_time"),
    (dict(evolution_times=[1.0], control_scales=np.ones((2, 2))), "control_scales are for 2 seeds"),
    (dict(evolution_times=[1.0], perturbations=np.eye(4)[None], offsets=np.zeros((2, 1))),
     "offsets are for 2 seeds"),
])
def test_durations_rejects_bad_arguments(kw, fragment):
    linear, _ = _system()
    kw.setdefault("reference_time", 1.0)
    with pytest.raises(ValueError, match=fragment):
        HamiltonianSweep.durations(linear, **kw)


def test_durations_rejects_a_time_dependent_hamiltonian():
    n, K, N, Nc = 4, 2, 7, 4
    linear, _ = _system(n, K, time_dependent=True)
    with pytest.raises(ValueError, match="time-independent"):  # the control count is known here
        HamiltonianSweep.durations(linear, [0.5, 1.0], 1.0, control_scales=np.ones((2, K)))
    w = HamiltonianSweep.durations(linear, [0.5, 1.0], 1.0)  # ... and here only with the problem
    psi0 = cases_mod.column_states(np.eye(n)[:, :1])
    with pytest.raises(ValueError, match="time-independent"):
        device.SchroedingerEvaluator(1.0, w, psi0, N, control_count=K, control_eval_count=Nc,
                                     costs=[TargetStateInfidelity(psi0)], backend=SweepStandIn())
    with pytest.raises(NotImplementedError, match="plain hamiltonian"):
        HamiltonianSweep.durations(QuadraticHamiltonian(linear, []), [1.0], 1.0)


@pytest.mark.parametrize("complex_controls, scaled", [(False, False), (True, True)])
def test_a_duration_member_is_tau_times_the_hamiltonian(complex_controls, scaled):
    n, K = 5, 2
    linear, rng = _system(n, K, seed=11, complex_controls=complex_controls)
    times, ref = np.array([0.4, 0.9, 1.0, 1.7]), 1.0
    w = HamiltonianSweep.durations(linear, times, ref)
    assert w.time_scaled and np.array_equal(w.evolution_times, times) and w.reference_time == ref
    assert w.perturbation_count == 1 and np.array_equal(w.offsets[:, 0], times / ref)
    for b in range(len(times)):
        for _ in range(3):
            u = rng.standard_normal(K) + (1j * rng.standard_normal(K) if complex_controls else 0)
            want = (times[b] / ref) * linear(u, 0.3)
            assert helpers.rel_err(w.member(b)(u, 0.3), want) < 1e-15
    if scaled:  # user scales and further offsets are multiplied by tau as well
        s0, d0 = 1 + 0.1 * rng.standard_normal((4, K)), 0.2 * rng.standard_normal((4, 1))
        dmat = cases_mod.gue(rng, n)[None]
        w = HamiltonianSweep.durations(linear, times, ref, control_scales=s0, perturbations=dmat,
                                       offsets=d0)
        tau = times / ref
        assert np.array_equal(w.control_scales, tau[:, None] * s0)
        assert np.array_equal(w.offsets, np.concatenate([tau[:, None], tau[:, None] * d0], axis=1))
        assert w.perturbations.shape == (2, n, n)  # resolved: the control count was known
        u = rng.standard_normal(K) + 1j * rng.standard_normal(K)
        want = tau[2] * (linear(s0[2] * u, 0.0) + d0[2, 0] * dmat[0])
        assert helpers.rel_err(w.member(2)(u, 0.0), want) < 1e-15
        part = w.slice(2, 4)
        assert np.array_equal(part.evolution_times, times[2:])
        assert np.array_equal(part.member(0)(u, 0.0), w.member(2)(u, 0.0))


def test_time_gradients_agree_with_central_differences_of_the_oracle_in_the_duration():
    """c2_transmon at two durations: dE_b/dT_b from the sensitivities of ONE evaluation at the
    reference time against (E(T_b + h) - E(T_b - h)) / 2h of the oracle run for T_b, h = 1e-4 T_b."""
    case = cases_mod.case_c2_transmon()
    ref = case.T
    times = ref * np.array([0.8, 1.3])
    w = HamiltonianSweep.durations(case.hamiltonian(), times, ref)
    target = case.cost_specs[0][1]["target_states"]
    ev = device.SchroedingerEvaluator(
        ref, w, case.initial_states, case.N, control_count=case.K, control_eval_count=case.Nc,
        costs=[TargetStateInfidelity(target)], backend=SweepStandIn())
    u = case.controls[0]
    errors, _, _, _ = ev.evaluate_batch(np.stack([u, u]))
    sens = ev.sweep_sensitivities()
    assert sens["control_scales"].shape == (2, case.K) and sens["offsets"].shape == (2, 1)
    grads = sens["evolution_time_gradients"]
    assert np.array_equal(grads, w.time_gradients(sens["control_scales"], sens["offsets"]))

    def oracle_error(T):
        problem = onp.SchroedingerProblem(
            T, case.hamiltonian(), case.initial_states, case.N, control_eval_count=case.Nc,
            costs=[onp.TargetStateInfidelity(target)], control_count=case.K)
        return onp.evaluate(problem, u)[0]

    for b, T in enumerate(times):
        assert abs(errors[b] - oracle_error(T)) < 1e-12
        h = 1e-4 * T
        fd = (oracle_error(T + h) - oracle_error(T - h)) / (2 * h)
        print("T", T, "fd", fd, "chain rule", grads[b])
        assert abs(fd) > 1e-5
        assert abs(fd - grads[b]) < 1e-8 * max(1.0, abs(fd) / 1e-3)


# ---- the evaluator on a stand-in backend -----------------------------------------------------------

@pytest.mark.parametrize("complex_controls, time_dependent, magnus", [
    (False, False, MagnusPolicy.M2),
    (True, True, MagnusPolicy.M2),
    (False, True, MagnusPolicy.M4),
    (True, False, MagnusPolicy.M6),
])
def test_stand_in_evaluates_every_seed_on_its_own_system(complex_controls, time_dependent, magnus):
    n, K, N, Nc, S, B, J, T = 4, 2, 9, 5, 2, 3, 2, 0.8
    linear, rng = _system(n, K, seed=31, complex_controls=complex_controls,
                          time_dependent=time_dependent)
    w = _sweep(linear, rng, n, K, B, J)
    psi0 = cases_mod.column_states(np.eye(n)[:, :S])
    target = cases_mod.column_states(cases_mod.random_unitary(rng, n)[:, :S])
    backend = SweepStandIn()
    ev = device.SchroedingerEvaluator(
        T, w, psi0, N, control_count=K, control_eval_count=Nc, complex_controls=complex_controls,
        costs=[TargetStateInfidelity(target)], magnus_policy=magnus, backend=backend)
    kr = K * (2 if complex_controls else 1)
    assert ev.sweep is w and ev.ensemble is None and ev.opaque_hamiltonian is None
    (dims, scales, offsets), = backend.received
    assert dims[2] == kr + J
    assert np.array_equal(scales, w.real_channel_scales(K, complex_controls))
    assert np.array_equal(offsets, w.offsets)
    h0 = backend.problem.hamiltonian(np.zeros(kr + J), 0.37)
    for j in range(J):  # the problem's last J channels are the D_j
        unit = np.zeros(kr + J)
        unit[kr + j] = 1.0
        assert np.allclose(backend.problem.hamiltonian(unit, 0.37) - h0, w.perturbations[j],
                           rtol=0, atol=1e-13)
    u = 0.5 * rng.standard_normal((B, Nc, K))
    if complex_controls:
        u = u + 0.5j * rng.standard_normal((B, Nc, K))
    with pytest.raises(ValueError, match="exactly that many"):
        ev.evaluate_batch(u[:2])
    errors, grads, finals, _ = ev.evaluate_batch(u)
    assert finals.shape == (B, S, n, 1)
    sens = ev.sweep_sensitivities()
    assert sens["control_scales"].shape == (B, K) and sens["offsets"].shape == (B, J)
    assert "evolution_time_gradients" not in sens
    for b in range(B):
        p = onp.SchroedingerProblem(T, w.member(b), psi0, N, control_eval_count=Nc,
                                    costs=[onp.TargetStateInfidelity(target)],
                                    complex_controls=complex_controls, control_count=K)
        p.magnus_policy = magnus.short
        err, gr, fin = onp.evaluate_with_grad(p, u[b])
        assert abs(errors[b] - err) < 1e-12
        assert np.max(np.abs(finals[b] - fin)) < 1e-12
        assert np.max(np.abs(grads[b] - (gr if complex_controls else np.real(gr)))) < 1e-12
    # d error_b / d s_bk by central differences of the members' oracle errors
    h = 1e-6
    for b, k in ((0, 0), (B - 1, K - 1)):
        vals = []
        for sign in (1, -1):
            s = w.control_scales.copy()
            s[b, k] += sign * h
            moved = HamiltonianSweep(linear, w.perturbations, w.offsets, s)
            p = onp.SchroedingerProblem(T, moved.member(b), psi0, N, control_eval_count=Nc,
                                        costs=[onp.TargetStateInfidelity(target)],
                                        complex_controls=complex_controls, control_count=K)
            p.magnus_policy = magnus.short
            vals.append(onp.evaluate(p, u[b])[0])
        assert abs((vals[0] - vals[1]) / (2 * h) - sens["control_scales"][b, k]) < 1e-8


def test_costs_of_the_controls_act_on_the_seeds_own_controls():
    n, K, N, Nc, B = 4, 2, 7, 4, 3
    linear, rng = _system(n, K, seed=5)
    w = _sweep(linear, rng, n, K, B, J=1)
    psi0 = cases_mod.column_states(np.eye(n)[:, :1])
    target = cases_mod.column_states(np.roll(np.eye(n), 1, axis=0)[:, :1])
    norm = ControlNorm(K, Nc, cost_multiplier=0.3)
    kw = dict(control_count=K, control_eval_count=Nc)
    plain = device.SchroedingerEvaluator(0.6, w, psi0, N, costs=[TargetStateInfidelity(target)],
                                         backend=SweepStandIn(), **kw)
    with_norm = device.SchroedingerEvaluator(
        0.6, w, psi0, N, costs=[TargetStateInfidelity(target), norm], backend=SweepStandIn(), **kw)
    assert with_norm.host_costs == [norm]
    u = 0.4 * rng.standard_normal((B, Nc, K))
    e0, g0, _, _ = plain.evaluate_batch(u)
    e1, g1, _, _ = with_norm.evaluate_batch(u)
    for b in range(B):
        assert abs(e1[b] - (e0[b] + norm.cost(u[b], None, N - 1))) < 1e-14
        assert np.max(np.abs(g1[b] - (g0[b] + norm.controls_bar(u[b], None, N - 1)))) < 1e-14
    for key in ("control_scales", "offsets"):  # the tables do not enter the control costs
        assert np.array_equal(plain.sweep_sensitivities()[key], with_norm.sweep_sensitivities()[key])


# ---- the batch driver --------------------------------------------------------------------------------

def _batch_problem(seed=9, durations=True):
    n, K, N, Nc, B, T = 4, 2, 9, 5, 3, 0.8
    linear, rng = _system(n, K, seed=seed)
    if durations:
        w = HamiltonianSweep.durations(linear, T * np.array([0.5, 1.0, 1.3]), T)
    else:
        w = _sweep(linear, rng, n, K, B, J=1)
    psi0 = cases_mod.column_states(np.eye(n)[:, :2])
    target = cases_mod.column_states(cases_mod.random_unitary(rng, n)[:, :2])
    costs = [TargetStateInfidelity(target), ControlNorm(K, Nc, cost_multiplier=0.05)]
    u0 = np.clip(0.4 * rng.standard_normal((B, Nc, K)), -0.9, 0.9)
    return w, (K, Nc, costs, T), (psi0, N), u0


@pytest.mark.parametrize("optimizer, durations", [
    (Adam(), True), (SGD(learning_rate=0.05), False), (LBFGS(), True)])
def test_host_loop_walks_the_single_seed_trajectories_of_the_members(optimizer, durations):
    w, head, tail, u0 = _batch_problem(durations=durations)
    kw = dict(iteration_count=5, log_iteration_step=0, optimizer=optimizer)
    helpers.set_backend_factory(SweepStandIn)
    try:
        full = qoc_amd.grape_schroedinger_discrete_batch(*head, w, *tail, u0, **kw)
    finally:
        helpers.set_backend_factory(None)
    sens = full.sweep_sensitivities
    assert sens["control_scales"].shape == (3, 2) and np.all(np.isfinite(sens["offsets"]))
    assert ("evolution_time_gradients" in sens) == durations
    if durations:
        assert sens["evolution_time_gradients"].shape == (3,)
    helpers.set_backend_factory(OracleBackend)
    try:
        for b in range(3):
            one = qoc_amd.grape_schroedinger_discrete(
                *head, w.member(b), *tail, initial_controls=u0[b], **kw)
            assert one.best_iteration == full.best_iteration[b]
            assert abs(one.best_error - full.best_error[b]) < 1e-12
            assert np.max(np.abs(one.best_controls - full.best_controls[b])) < 1e-10
    finally:
        helpers.set_backend_factory(None)


def test_the_batch_needs_one_system_per_seed():
    w, head, tail, u0 = _batch_problem()
    helpers.set_backend_factory(SweepStandIn)
    try:
        with pytest.raises(ValueError, match="exactly that many seeds"):
            qoc_amd.grape_schroedinger_discrete_batch(*head, w, *tail, u0[:2], iteration_count=1,
                                                      log_iteration_step=0)
    finally:
        helpers.set_backend_factory(None)


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _rank_main(rank, world, port, out_dir):
    sys.path.insert(0, ROOT)
    import torch
    import torch.distributed as dist

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank),
                      WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)

    class GlooComm(object):
        def __init__(self):
            self.rank, self.world = rank, world

        def _reduce(self, array, op):
            t = torch.from_numpy(np.ascontiguousarray(array, dtype=np.float64))
            dist.all_reduce(t, op=op)
            return t.numpy()

        def allreduce_sum(self, array):
            return self._reduce(array, dist.ReduceOp.SUM)

        def allreduce_max(self, array):
            return self._reduce(array, dist.ReduceOp.MAX)

        def barrier(self):
            dist.barrier()

    w, head, tail, u0 = _batch_problem()
    helpers.set_backend_factory(SweepStandIn)
    out = qoc_amd.grape_schroedinger_discrete_batch(
        *head, w, *tail, u0, iteration_count=4, log_iteration_step=0, comm=GlooComm())
    np.savez(os.path.join(out_dir, "rank%d.npz" % rank), best_error=out.best_error,
             controls=np.stack(out.best_controls), global_best=out.global_best_error,
             time_gradients=out.sweep_sensitivities["evolution_time_gradients"])
    dist.destroy_process_group()


def test_every_rank_optimises_its_block_of_the_sweep(tmp_path):
    import torch.multiprocessing as mp
    world, port = 2, _free_port()
    mp.spawn(_rank_main, args=(world, port, str(tmp_path)), nprocs=world, join=True)
    w, head, tail, u0 = _batch_problem()
    helpers.set_backend_factory(SweepStandIn)
    try:
        full = qoc_amd.grape_schroedinger_discrete_batch(
            *head, w, *tail, u0, iteration_count=4, log_iteration_step=0)
    finally:
        helpers.set_backend_factory(None)
    for r in range(world):
        lo, hi = parallel.shard_bounds(3, r, world)
        out = np.load(os.path.join(str(tmp_path), "rank%d.npz" % r))
        assert np.array_equal(out["best_error"], full.best_error[lo:hi])
        assert np.array_equal(out["controls"], np.stack(full.best_controls[lo:hi]))
        assert np.array_equal(out["time_gradients"],
                              full.sweep_sensitivities["evolution_time_gradients"][lo:hi])
        assert float(out["global_best"]) == float(np.min(full.best_error))


# ---- refusals ---------------------------------------------------------------------------------------

class _UserCost(Cost):
    name = "user"

    def cost(self, controls, states, step):
        return float(np.abs(states[0, 0, 0]) ** 2)


def test_refusals():
    n, K, N, Nc = 4, 2, 7, 4
    linear, rng = _system(n, K, seed=13)
    w = _sweep(linear, rng, n, K, 2, J=1)
    psi0 = cases_mod.column_states(np.eye(n)[:, :1])
    target = cases_mod.column_states(np.roll(np.eye(n), 1, axis=0)[:, :1])
    costs = [TargetStateInfidelity(target)]
    kw = dict(control_count=K, control_eval_count=Nc)
    make = lambda sweep, backend=None, **more: device.SchroedingerEvaluator(  # noqa: E731
        0.6, sweep, psi0, N, backend=backend if backend is not None else SweepStandIn(),
        **dict(dict(costs=costs, **kw), **more))
    with pytest.raises(NotImplementedError, match="set_sweep"):
        make(w, OracleBackend())
    scales = np.ones((2, K))
    with pytest.raises(NotImplementedError, match="linear in the controls"):
        make(HamiltonianSweep(lambda u, t: linear(u, t) + u[0] ** 2 * np.eye(n),
                              control_scales=scales))
    with pytest.raises(NotImplementedError, match="QuadraticHamiltonian"):
        make(HamiltonianSweep(QuadraticHamiltonian(linear, [(0, 0, np.eye(n))]),
                              control_scales=scales))
    ensemble = HamiltonianEnsemble(linear, weights=np.ones(2))
    with pytest.raises(ValueError, match="callable"):  # an ensemble is no callable
        HamiltonianSweep(ensemble, control_scales=scales)
    with pytest.raises(NotImplementedError, match="inside a HamiltonianEnsemble"):
        HamiltonianEnsemble(w, weights=np.ones(2))
    with pytest.raises(NotImplementedError, match="without a device descriptor"):
        make(w, costs=costs + [_UserCost()])
    with pytest.raises(NotImplementedError, match="at least one control"):
        device.SchroedingerEvaluator(0.6, w, psi0, N, costs=costs, backend=SweepStandIn())
    with pytest.raises(ValueError, match="control_scales"):
        make(w, control_count=K + 1)
    with pytest.raises(ValueError, match="perturbations are 4 x 4"):
        device.SchroedingerEvaluator(0.6, w, cases_mod.column_states(np.eye(5)[:, :1]), N,
                                     costs=costs, backend=SweepStandIn(), **kw)
    timed = HamiltonianSweep.durations(linear, [0.3, 0.6], 0.6)
    bandwidth = ControlBandwidthMax(K, Nc, 0.6, np.full(K, 2.0))
    with pytest.raises(NotImplementedError, match="ControlBandwidthMax"):
        make(timed, costs=costs + [bandwidth])
    make(w, costs=costs + [bandwidth])  # (its bins are those of the one evolution time here)
    u = np.clip(0.3 * rng.standard_normal((Nc, K)), -0.9, 0.9)
    with pytest.raises(NotImplementedError, match=r"member\(b\)"):
        qoc_amd.evolve_schroedinger_discrete(0.6, w, psi0, N, controls=u, costs=costs)
    with pytest.raises(NotImplementedError, match=r"member\(b\)"):
        qoc_amd.grape_schroedinger_discrete(K, Nc, costs, 0.6, w, psi0, N, initial_controls=u)
    with pytest.raises(NotImplementedError, match=r"member\(b\)"):  # save files go with them
        qoc_amd.grape_schroedinger_discrete(K, Nc, costs, 0.6, w, psi0, N, initial_controls=u,
                                            save_file_path="unused.h5")
    rho0 = np.eye(n, dtype=np.complex128)[None] / n
    with pytest.raises(NotImplementedError, match="dissipation rates"):
        qoc_amd.evolve_lindblad_discrete(0.6, rho0, N, controls=u, hamiltonian=w)
    with pytest.raises(NotImplementedError, match="dissipation rates"):
        qoc_amd.grape_lindblad_discrete(K, Nc, [], 0.6, rho0, N, hamiltonian=w, initial_controls=u)
    with pytest.raises(NotImplementedError, match="dissipation rates"):
        qoc_amd.grape_lindblad_discrete_batch(K, Nc, [], 0.6, rho0, N, u[None], hamiltonian=w)
    with pytest.raises(NotImplementedError, match="dissipation rates"):
        device.LindbladEvaluator(0.6, rho0, N, hamiltonian=w, control_count=K,
                                 control_eval_count=Nc, backend=SweepStandIn())


def test_the_abi_declares_the_entry_points():
    lib = engine.load_library()
    for name in ("qocx_set_sweep", "qocx_sweep_download_sensitivities"):
        assert name in engine.SIGNATURES
        assert hasattr(lib, name)
    assert hasattr(engine.Engine, "set_sweep")
    assert hasattr(engine.Engine, "sweep_sensitivities")
