"""
CPU tests of InterpolationPolicy.PIECEWISE_CONSTANT: the enum and its save-file string, the
interpolation rows of qoc_amd/core/structure.py, the six entry points on a stand-in backend that
implements the policy by the control-free closure of Reference A (tests/piecewise_constant.py), the
host routes of callables that are not linear in the controls, the identities of a pulse constant
over a step, and LINEAR left as it was. The engine's tables and kernels run in
tests/test_gpu_piecewise_constant.py - the Lindblad frozen-controls and tangent routes too: the
NumPy model of the Lindblad device algorithm (tests/lindblad_model.py) interpolates linearly only.
Gates: DESIGN section 10 (states and cost 1e-10, gradient against differences 1e-7) and section 9
(Lindblad densities 1e-8, cost 1e-9).
"""

import copy
import sys

import numpy as np
import pytest

import qoc_amd
from oracle import qoc_lindblad_numpy as ol
from oracle import qoc_numpy as onp
from qoc_amd.core import device, structure
from qoc_amd.models import InterpolationPolicy, MagnusPolicy
from qoc_amd.standard import Adam, TargetDensityInfidelity, TargetStateInfidelity
from tests import cases as cases_mod
from tests import fake_h5py, helpers
from tests import piecewise_constant as pc
from tests.oracle_backend import OracleBackend
from tests.test_host_api import product_cost_list

PWC = InterpolationPolicy.PIECEWISE_CONSTANT


class PiecewiseBackend(OracleBackend):
    """OracleBackend + interpolation="piecewise_constant": every control array is folded into the
    control-free closure of Reference A and evaluated by the oracle; gradients are central
    differences of that forward pass. Structured problems only (what the entry points set)."""

    def set_schroedinger_problem(self, *args, interpolation="linear", **kw):
        super().set_schroedinger_problem(*args, **kw)
        self.pwc = interpolation == "piecewise_constant"
        self.interpolations = getattr(self, "interpolations", []) + [interpolation]

    def _folded(self, u):
        n, S, K, Nc, N = self.dims
        folded = copy.copy(self.problem)
        folded.hamiltonian = pc.closure(self.problem.hamiltonian, u, self.problem.evolution_time)
        folded.control_eval_count = folded.control_count = 0
        return folded

    def eval_resident(self, want_grad=True):
        n, S, K, Nc, N = self.dims
        if not self.pwc or K == 0:
            return super().eval_resident(want_grad)
        assert getattr(self, "inj", None) is None
        self.calls += 1
        self.cost, self.grads, self.final, self.steps = [], [], [], []
        for u in self.controls:
            inter = []
            err, fin = onp.evaluate(self._folded(u), None, intermediate=inter)
            self.cost.append(err)
            self.final.append(np.asarray(fin)[:, :, 0])
            if self.keep:
                self.steps.append(np.stack(inter)[:, :, :, 0])
            if want_grad:
                self.grads.append(pc.central_differences(
                    lambda x: onp.evaluate(self._folded(x), None)[0], u))

    def set_lindblad_problem(self, n, S, K, Nc, N, T, h0, g, dissipators, operators,
                             initial_densities, interpolation="linear", **kw):
        self.lb_pwc = interpolation == "piecewise_constant"
        self.interpolations = getattr(self, "interpolations", []) + [interpolation]
        if not self.lb_pwc:
            return super().set_lindblad_problem(n, S, K, Nc, N, T, h0, g, dissipators, operators,
                                                initial_densities, **kw)
        assert not kw.get("fixed_subdivision"), "static problems only"
        from tests.oracle_backend import _DensityDescriptorCost
        h0 = np.asarray(h0, dtype=np.complex128).reshape(n, n)
        g = np.asarray(g, dtype=np.complex128).reshape(K, n, n)
        self.lb = dict(
            K=K, Nc=Nc, N=N, T=T, ces=kw.get("cost_eval_step", 1),
            hamiltonian=lambda u, t: h0 + sum(u[k] * g[k] for k in range(K)),
            data=(lambda t: (dissipators, operators)) if operators is not None else None,
            rho0=np.asarray(initial_densities, dtype=np.complex128).reshape(S, n, n),
            costs=[_DensityDescriptorCost(c, S, n) for c in kw.get("costs", ())])

    def evaluate_lindblad(self, controls, want_grad=True, want_final=True):
        if not self.lb_pwc:
            return super().evaluate_lindblad(controls, want_grad, want_final)
        p = self.lb
        assert not self.keep and getattr(self, "lb_inj", None) is None
        self.calls += 1

        def forward(u):
            return pc.lindblad_reference_a(p["hamiltonian"], u, p["T"], p["rho0"], p["N"],
                                           p["costs"], p["data"], p["ces"])
        batch = np.asarray(controls, dtype=np.float64).reshape(-1, p["Nc"], p["K"])
        out = [forward(u) for u in batch]
        grads = None
        if want_grad:
            grads = np.stack([pc.central_differences(lambda x: forward(x)[0], u, h=1e-4)
                              for u in batch])
        return (np.array([o[0] for o in out], dtype=np.float64), grads,
                np.stack([o[1] for o in out]))


@pytest.fixture(autouse=True)
def piecewise_engine(monkeypatch):
    monkeypatch.setitem(sys.modules, "h5py", fake_h5py)
    fake_h5py.STORE.clear()
    helpers.set_backend_factory(PiecewiseBackend)
    yield
    helpers.set_backend_factory(None)


# ---- a small problem: n = 5, K = 2, Nc = 6 ---------------------------------------------------------

N_HILBERT, K, NC, T = 5, 2, 6, 3.0
HAMILTONIAN = pc.system(N_HILBERT, K, seed=11)
PSI0, TARGET = pc.states(N_HILBERT, 2, seed=12)
PULSE = 0.7 * np.random.default_rng(13).standard_normal((NC, K))


def schroedinger_args(N):
    return (K, NC, [TargetStateInfidelity(TARGET)], T, HAMILTONIAN, PSI0, N)


def oracle_costs():
    return [onp.TargetStateInfidelity(TARGET)]


class Probe(object):
    """Optimizer plugin: the gradient at the start and central differences of the error through
    the driver's own callbacks (tests/test_control_basis_host.py)."""

    def __init__(self, step=pc.FD_STEP):
        self.step = step

    def run(self, function, iteration_count, initial_params, jacobian, args=()):
        x = np.array(initial_params, dtype=np.float64)
        self.grads = np.array(jacobian(x.copy(), *args)[0])
        self.differences = np.zeros_like(x)
        for i in range(len(x)):
            up, down = x.copy(), x.copy()
            up[i] += self.step
            down[i] -= self.step
            self.differences[i] = (function(up, *args)[0] - function(down, *args)[0]) / (2 * self.step)


# ---- the enum ----------------------------------------------------------------------------------------

def test_enum_member_label_and_save_file_string(tmp_path):
    assert PWC.value == 2 and InterpolationPolicy(2) is PWC
    assert str(PWC) == repr(PWC) == "interpolation_piecewise_constant"
    assert InterpolationPolicy.LINEAR.value == 1
    assert str(InterpolationPolicy.LINEAR) == "interpolation_linear"
    assert (PWC.short, InterpolationPolicy.LINEAR.short) == ("piecewise_constant", "linear")
    path = str(tmp_path / "evolve.h5")
    qoc_amd.evolve_schroedinger_discrete(T, HAMILTONIAN, PSI0, 7, controls=PULSE,
                                         interpolation_policy=PWC, save_file_path=path)
    assert str(fake_h5py.STORE[path]["interpolation_policy"].array) == \
        "interpolation_piecewise_constant"
    path = str(tmp_path / "evolve_linear.h5")
    qoc_amd.evolve_schroedinger_discrete(T, HAMILTONIAN, PSI0, 7, controls=PULSE,
                                         save_file_path=path)
    assert str(fake_h5py.STORE[path]["interpolation_policy"].array) == "interpolation_linear"


# ---- structure.interpolation_rows / controls_at ------------------------------------------------------

def test_rows_and_controls_at_under_both_policies():
    rng = np.random.default_rng(1)
    c = rng.standard_normal((NC, K)) + 1j * rng.standard_normal((NC, K))
    edge = 2 * T / NC  # an interior slice edge: right-continuous
    times = [0.0, 0.2, np.nextafter(edge, 0.0), edge, np.nextafter(edge, T), T - 1e-9, T]
    rows = structure.interpolation_rows(T, NC, times, PWC)
    assert list(rows[0]) == [0, 0, 1, 2, 2, NC - 1, NC - 1] and np.array_equal(rows[0], rows[1])
    assert np.array_equal(structure.controls_at(c, rows, times), c[rows[0]])  # bit for bit
    assert np.array_equal(structure.controls_at(c.real, rows, times), c.real[rows[0]])
    # the transpose gives row i1 the whole cotangent (weight 1 - 0, and 0 on the same row)
    i1, i2, x1, x2 = rows
    assert np.all((np.asarray(times) - x1) / (x2 - x1) == 0.0)
    # LINEAR: the default, the reference's rule, knots at j T / (Nc - 1)
    lin = structure.interpolation_rows(T, NC, times)
    for a, b in zip(lin, structure.interpolation_rows(T, NC, times, InterpolationPolicy.LINEAR)):
        assert np.array_equal(a, b)
    assert list(lin[0]) == [0, 0, 1, 1, 1, NC - 2, NC - 2]
    assert list(lin[1]) == [1, 1, 2, 2, 2, NC - 1, NC - 1]
    u = structure.controls_at(c.real, lin, times)
    assert np.array_equal(u[0], c.real[0]) and np.allclose(u[-1], c.real[-1], atol=1e-15)
    assert np.allclose(u[1], c.real[0] + (c.real[1] - c.real[0]) * 0.2 / (T / (NC - 1)))


def test_lindblad_stage_rows_take_the_slice_of_the_sub_interval():
    """Stage times of two sub-intervals that meet ON a slice edge: the last stage of the first one
    (c = 1, t = edge) stays in its slice, the first stage of the second one is in the next."""
    stage_times = device.make_backend().lindblad_stage_times(T, 4, NC + 1, 1, 1)
    count = structure.LINDBLAD_STAGES
    assert len(stage_times) % count == 0
    groups = stage_times.reshape(-1, count)
    # 3 system steps x 6 slices: cut at the slice edges, 2 sub-intervals per step
    assert groups.shape[0] == NC
    assert np.allclose(groups[:, 0], np.arange(NC) * T / NC) and np.allclose(groups[:, -1],
                                                                            (np.arange(NC) + 1) * T / NC)
    rows = structure.lindblad_stage_rows(T, NC, stage_times, PWC)
    assert np.array_equal(rows[0], np.repeat(np.arange(NC), count))
    by_time = structure.interpolation_rows(T, NC, stage_times, PWC)[0]
    assert by_time[count - 1] == 1 and rows[0][count - 1] == 0  # what by-time lookup gets wrong
    lin = structure.lindblad_stage_rows(T, NC, stage_times)
    for a, b in zip(lin, structure.interpolation_rows(T, NC, stage_times)):
        assert np.array_equal(a, b)


# ---- the entry points on the stand-in backend --------------------------------------------------------

@pytest.mark.parametrize("magnus", ["M2", "M4", "M6"])
def test_evolve_schroedinger_gives_the_closure_oracles_error(magnus):
    N = 8  # unaligned: 7 steps over 6 slices, the M4 / M6 nodes of a step in two slices
    result = qoc_amd.evolve_schroedinger_discrete(
        T, HAMILTONIAN, PSI0, N, controls=PULSE, costs=[TargetStateInfidelity(TARGET)],
        interpolation_policy=PWC, magnus_policy=getattr(MagnusPolicy, magnus))
    err, fin = pc.reference_a(HAMILTONIAN, PULSE, T, PSI0, N, oracle_costs(), magnus)
    assert abs(result.error - err) < 1e-10
    assert np.max(np.abs(result.final_states - fin)) < 1e-10
    linear = qoc_amd.evolve_schroedinger_discrete(
        T, HAMILTONIAN, PSI0, N, controls=PULSE, costs=[TargetStateInfidelity(TARGET)],
        magnus_policy=getattr(MagnusPolicy, magnus))
    assert abs(linear.error - err) > 1e-4  # the two policies are different pulses


def test_grape_schroedinger_gradient_matches_differences():
    probe = Probe()
    qoc_amd.grape_schroedinger_discrete(*schroedinger_args(8), initial_controls=PULSE.copy(),
                                        optimizer=probe, interpolation_policy=PWC,
                                        max_control_norms=np.full(K, 5.0), log_iteration_step=0)
    scale = np.max(np.abs(probe.grads))
    print("max |g|", scale, "max |g - fd|", np.max(np.abs(probe.grads - probe.differences)))
    assert scale > 1e-3 and np.all(probe.grads.reshape(NC, K) != 0)  # every row carries gradient
    assert np.max(np.abs(probe.grads - probe.differences)) <= 1e-7 * scale
    ref = pc.reference_a_gradient(HAMILTONIAN, PULSE, T, PSI0, 8, oracle_costs())
    assert np.max(np.abs(probe.grads.reshape(NC, K) - ref)) <= 1e-7 * scale


def test_grape_schroedinger_descends_and_batch_equals_single_runs():
    seeds = np.stack([PULSE, 0.3 * PULSE[::-1]])
    kw = dict(interpolation_policy=PWC, iteration_count=3, log_iteration_step=0,
              max_control_norms=np.full(K, 5.0))
    out = qoc_amd.grape_schroedinger_discrete_batch(
        *schroedinger_args(7), seeds.copy(), optimizer=Adam(learning_rate=2e-2), **kw)
    for b in range(2):
        single = qoc_amd.grape_schroedinger_discrete(
            *schroedinger_args(7), initial_controls=seeds[b].copy(),
            optimizer=Adam(learning_rate=2e-2), **kw)
        assert single.best_error == out.best_error[b]
        assert np.array_equal(single.best_controls, out.best_controls[b])
        assert np.array_equal(single.best_final_states, out.best_final_states[b])
        first = pc.reference_a(HAMILTONIAN, seeds[b], T, PSI0, 7, oracle_costs())[0]
        assert single.best_error < first and single.best_iteration > 0


LB_N, LB_NC = 3, 2
LB_HAMILTONIAN = pc.system(LB_N, 2, seed=21)
LB_DATA, LB_RHO0, LB_TARGET = pc.lindblad_system(LB_N, 1, seed=22)
LB_PULSE = 0.6 * np.random.default_rng(23).standard_normal((LB_NC, 2))
LB_T = 1.0


def lindblad_args(N):
    return (2, LB_NC, [TargetDensityInfidelity(LB_TARGET)], LB_T, LB_RHO0, N)


def test_lindblad_entry_points_on_the_closure_oracle():
    """Aligned (N - 1 = 4 = 2 Nc): the reference's integrator restarts at every system step."""
    N = 5
    costs = [ol.TargetDensityInfidelity(LB_TARGET)]
    err, fin = pc.lindblad_reference_a(LB_HAMILTONIAN, LB_PULSE, LB_T, LB_RHO0, N, costs, LB_DATA)
    result = qoc_amd.evolve_lindblad_discrete(
        LB_T, LB_RHO0, N, controls=LB_PULSE, costs=[TargetDensityInfidelity(LB_TARGET)],
        hamiltonian=LB_HAMILTONIAN, lindblad_data=LB_DATA, interpolation_policy=PWC)
    assert abs(result.error - err) < 1e-9
    assert np.max(np.abs(result.final_densities - fin)) < 1e-8
    kw = dict(hamiltonian=LB_HAMILTONIAN, lindblad_data=LB_DATA, interpolation_policy=PWC,
              iteration_count=2, log_iteration_step=0, max_control_norms=np.full(2, 5.0))
    seeds = np.stack([LB_PULSE, -0.5 * LB_PULSE])
    out = qoc_amd.grape_lindblad_discrete_batch(*lindblad_args(N), seeds.copy(),
                                                optimizer=Adam(learning_rate=5e-2), **kw)
    for b in range(2):
        single = qoc_amd.grape_lindblad_discrete(*lindblad_args(N), initial_controls=seeds[b].copy(),
                                                 optimizer=Adam(learning_rate=5e-2), **kw)
        assert single.best_error == out.best_error[b]
        assert np.array_equal(single.best_controls, out.best_controls[b])
    assert abs(out.best_error[0] - err) < 1e-9 or out.best_error[0] < err


def test_lindblad_evaluator_asks_for_the_stage_times_of_one_knot_more():
    asked = []

    class Recording(PiecewiseBackend):
        def lindblad_stage_times(self, *args):
            asked.append(args)
            return OracleBackend.lindblad_stage_times(*args)

    for policy, knots in ((InterpolationPolicy.LINEAR, LB_NC), (PWC, LB_NC + 1)):
        del asked[:]
        backend = Recording()
        device.LindbladEvaluator(LB_T, LB_RHO0, 5, hamiltonian=LB_HAMILTONIAN, lindblad_data=LB_DATA,
                                 control_count=2, control_eval_count=LB_NC,
                                 costs=[TargetDensityInfidelity(LB_TARGET)],
                                 interpolation_policy=policy, backend=backend)
        assert asked and all(a[2] == knots for a in asked)
        assert backend.interpolations == [policy.short]


def test_a_backend_without_the_policy_is_an_error_not_a_fallback():
    with pytest.raises(NotImplementedError):
        device.SchroedingerEvaluator(T, HAMILTONIAN, PSI0, 7, control_count=K,
                                     control_eval_count=NC, interpolation_policy=PWC,
                                     backend=OracleBackend())
    with pytest.raises(NotImplementedError):
        device.LindbladEvaluator(LB_T, LB_RHO0, 5, hamiltonian=LB_HAMILTONIAN, control_count=2,
                                 control_eval_count=LB_NC, interpolation_policy=PWC,
                                 backend=OracleBackend())


# ---- callables that are not linear in the controls ---------------------------------------------------

def stark_hamiltonian():
    """H0 + u_0 G_0 + u_1 G_1 + u_0^2 Q: the epsilon^2 term."""
    rng = np.random.default_rng(31)
    q = pc.hermitian(rng, N_HILBERT, 0.5)
    return lambda u, t: HAMILTONIAN(u, t) + (0.0 if u is None else u[0] ** 2) * q


def test_m2_generator_route_under_the_policy():
    """sample_generators / generator_gradients with piecewise-constant rows: the generators are
    those of the slices, and the chain rule through them matches differences (the check of
    tests/test_host_api.py::test_opaque_generator_gradients_against_finite_differences). The
    engine's share of the route runs in tests/test_gpu_piecewise_constant.py."""
    h = stark_hamiltonian()
    N = 8
    dt = T / (N - 1)
    times = [j * dt + 0.5 * dt for j in range(N - 1)]
    ev = device.SchroedingerEvaluator(T, h, PSI0, N, control_count=K, control_eval_count=NC,
                                      interpolation_policy=PWC)
    assert ev.opaque_hamiltonian is not None
    assert np.array_equal(ev._rows[0], [pc.slice_of(t, NC, T) for t in times])
    gens, u = structure.sample_generators(h, PULSE, ev._rows, times, dt, N_HILBERT)
    fold = pc.closure(h, PULSE, T)
    for j, t in enumerate(times):
        assert np.array_equal(gens[j], dt * (-1j * fold(None, t)))
    rng = np.random.default_rng(8)
    weights = rng.standard_normal(gens.shape) + 1j * rng.standard_normal(gens.shape)

    def cost(c):
        ip = np.sum(np.conj(weights) * structure.sample_generators(h, c, ev._rows, times, dt,
                                                                   N_HILBERT)[0], axis=(1, 2))
        return float(np.sum(np.abs(ip) ** 2)), 2 * ip[:, None, None] * weights
    grads = structure.generator_gradients(h, PULSE, ev._rows, times, dt, cost(PULSE)[1], False)
    fd = pc.central_differences(lambda c: cost(c)[0], PULSE)
    assert np.max(np.abs(grads - fd)) < 1e-7 * np.max(np.abs(fd))


def test_m4_tangent_route_against_reference_a():
    h = stark_hamiltonian()
    N = 8
    ev = device.SchroedingerEvaluator(T, h, PSI0, N, control_count=K, control_eval_count=NC,
                                      costs=[TargetStateInfidelity(TARGET)],
                                      magnus_policy=MagnusPolicy.M4, interpolation_policy=PWC)
    assert ev.linearized_hamiltonian is not None
    error, grads, final, _ = ev.evaluate(PULSE)
    err, fin = pc.reference_a(h, PULSE, T, PSI0, N, oracle_costs(), "M4")
    ref = pc.reference_a_gradient(h, PULSE, T, PSI0, N, oracle_costs(), "M4")
    print("error", error - err, "gradient", np.max(np.abs(grads - ref)) / np.max(np.abs(ref)))
    assert abs(error - err) < 1e-10 and np.max(np.abs(final - fin)) < 1e-10
    assert np.max(np.abs(grads - ref)) < 1e-7 * np.max(np.abs(ref))


# ---- identities of a pulse that is constant over every step ------------------------------------------

def evolve_final(N, magnus):
    return qoc_amd.evolve_schroedinger_discrete(
        T, HAMILTONIAN, PSI0, N, controls=PULSE, interpolation_policy=PWC,
        magnus_policy=getattr(MagnusPolicy, magnus)).final_states


def test_aligned_magnus_orders_coincide_and_so_do_steps_per_slice():
    """A system constant in time and slice edges on system steps: the step generator is constant
    over the step, so the Pade step is the slice's exact propagator under M2, M4 and M6, and r
    steps per slice multiply to one step per slice."""
    one = evolve_final(NC + 1, "M2")
    for magnus in ("M4", "M6"):
        assert np.max(np.abs(evolve_final(NC + 1, magnus) - one)) < 1e-12
    assert np.max(np.abs(evolve_final(3 * NC + 1, "M2") - one)) < 1e-12
    assert np.max(np.abs(evolve_final(2 * NC + 1, "M6") - one)) < 1e-12


# ---- LINEAR is untouched -----------------------------------------------------------------------------

def test_other_policies_still_raise():
    case = cases_mod.case_by_name("ctrlcosts_r")
    for policy in ("cubic", 2, "interpolation_piecewise_constant"):
        with pytest.raises(NotImplementedError):
            qoc_amd.evolve_schroedinger_discrete(case.T, case.hamiltonian(), case.initial_states,
                                                 case.N, controls=case.controls[0],
                                                 interpolation_policy=policy)
        with pytest.raises(NotImplementedError):
            qoc_amd.evolve_lindblad_discrete(LB_T, LB_RHO0, 5, controls=LB_PULSE,
                                             hamiltonian=LB_HAMILTONIAN, interpolation_policy=policy)


def test_linear_given_explicitly_gives_the_bits_of_the_default():
    case = cases_mod.case_by_name("ctrlcosts_r")
    common = dict(control_count=case.K, control_eval_count=case.Nc,
                  complex_controls=case.complex_controls, costs=product_cost_list(case),
                  cost_eval_step=case.cost_eval_step)
    outs = []
    for kw in ({}, dict(interpolation_policy=InterpolationPolicy.LINEAR)):
        backend = OracleBackend()  # takes no interpolation keyword: LINEAR must not send one
        ev = device.SchroedingerEvaluator(case.T, case.hamiltonian(), case.initial_states, case.N,
                                          backend=backend, **common, **kw)
        outs.append(ev.evaluate(case.controls[0]))
    assert outs[0][0] == outs[1][0]
    assert np.array_equal(outs[0][1], outs[1][1]) and np.array_equal(outs[0][2], outs[1][2])
