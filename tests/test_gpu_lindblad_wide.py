"""
GPU tests (-m gpu) of the Lindblad engine at 33 <= n <= 64: the sixteen-wave kernel of
qoc_amd/csrc/qocx_lindblad16t.hip behind the knob lindblad_wide / the keyword wide=True.

The cases are the table of tests/lindblad_wide_cases.py, the smallest shapes at which this kernel can
still go wrong (3 or 4 system steps, 2 seeds): tile edges and pad tiles (n = 33, 47, 48, 49, 64), 1 and
2 densities, 0 ... 8 operators, 1 ... 8 controls, both cost kinds with a ragged step cost, a
non-Hermitian h0, two sub-division groups in one batch, recomputed stage values, host cotangents, knots
and slice edges inside steps. Every case is held to the NumPy model of the scheme at the gates of
tests/test_gpu_lindblad.py::test_lindblad_edge_shapes_against_model; three cases to the exact
superoperator reference; one to the oracle's adaptive integrator (the forward parity of DESIGN.md 9);
then the public API with wide=True and the engine's refusals by name.

Without the kernel every test here fails: at set_lindblad_problem (QocxError, hilbert_size must be in
1..32) or at the evaluator (NotImplementedError).
"""

import numpy as np
import pytest

import qoc_amd
from oracle import qoc_lindblad_numpy as ol
from qoc_amd.core import batch as batch_mod
from qoc_amd.standard import Adam, HamiltonianEnsemble, LindbladSweep, TargetDensityInfidelity
from tests import cases as cases_mod
from tests import gpu_helpers as gh
from tests import helpers
from tests import lindblad_exact as ex
from tests import lindblad_wide_cases as wc

pytestmark = pytest.mark.gpu

# device against model (test_lindblad_edge_shapes_against_model)
GATE_COST = 1e-12
GATE_DENSITIES = 1e-12
GATE_GRADIENT = 1e-10        # of max(max |g|, 1e-3)
# device against exact: per quantity ten times the worst model-against-exact error over EXACT_NAMES or
# the constant of tests/lindblad_exact.py, whichever is larger. Measured on the CPU by
# tools/measure_lindblad_wide_exact.py -> profiles/lindblad_wide_exact.jsonl: cost 0, densities 1.1e-14
# (exact_n36_l1_s2_k1), gradient 6.5e-13 of the largest entry (exact_n33_forbid): ten times each stays
# below its constant, so the constants hold.
EXACT_GATES = {"cost": ex.GATE_COST, "densities": ex.GATE_DENSITIES, "gradient": ex.GATE_GRADIENT}
PWC = "piecewise_constant"


@pytest.fixture(autouse=True)
def real_engine():
    helpers.set_backend_factory(None)
    yield
    helpers.set_backend_factory(None)


@pytest.fixture(scope="module")
def engine():
    from qoc_amd.engine import Engine
    e = Engine(0)
    e.set_knob("lindblad_wide", 1)
    yield e
    e.close()


def set_problem(engine, case, **kw):
    L = 0 if case.operators is None else len(case.operators)
    engine.set_lindblad_problem(
        case.n, case.S, len(case.g), case.Nc, case.N, case.T, case.h0, case.g,
        case.gammas if L else None, case.operators if L else None, case.rho0,
        costs=gh.lindblad_device_costs(case), cost_eval_step=case.ces,
        interpolation=PWC if case.kind == "plain" else "linear", **kw)


def device_results(engine, case, debug=None):
    set_problem(engine, case)
    try:
        if debug is not None:
            engine.debug_lindblad_knobs(*debug)
        if case.bars:
            engine.set_density_cotangents(case.bar_steps, case.bar_values)
        cost, grads, final = engine.evaluate_lindblad(case.controls)
    finally:
        engine.debug_lindblad_knobs(0, 256, 0)
        engine.set_density_cotangents(None, None)
    return dict(cost=cost, grad=grads, final=final)


def assert_at_model_gates(name, got, want):
    cost = float(np.max(np.abs(got["cost"] - want["cost"])))
    dens = float(np.max(np.abs(got["final"] - want["final"])))
    grad = max(float(np.max(np.abs(got["grad"][b] - want["grad"][b]))
                     / max(np.max(np.abs(want["grad"][b])), 1e-3)) for b in range(len(want["cost"])))
    print(name, "cost %.3g densities %.3g gradient %.3g (of the largest entry)" % (cost, dens, grad))
    assert cost <= GATE_COST, (cost, GATE_COST)
    assert dens <= GATE_DENSITIES, (dens, GATE_DENSITIES)
    assert grad <= GATE_GRADIENT, (grad, GATE_GRADIENT)


@pytest.mark.parametrize("name", wc.NAMES)
def test_the_wide_kernel_against_the_model(engine, name):
    case = wc.build(name)
    want = wc.model_results(name)
    got = device_results(engine, case, case.debug)
    # the gradient carries a signal (small: the costs divide every overlap by n)
    assert np.max(np.abs(want["grad"])) > 1e-5
    assert_at_model_gates(name, got, want)
    if case.debug is not None:
        # recomputed stage values come out of the same forward_stages as kept ones: cost and final
        # densities bit for bit (the gradient, which sums in the same order, within the gate above)
        kept = device_results(engine, case)
        assert np.array_equal(got["cost"], kept["cost"])
        assert np.array_equal(got["final"], kept["final"])
        assert_at_model_gates(name + " (kept)", kept, want)
    if case.bars:  # the cotangents reach the gradient
        plain = device_results(engine, wc.SimpleNamespace(**dict(vars(case), bars=False)))
        assert np.max(np.abs(plain["grad"] - got["grad"])) > 1e-3 * np.max(np.abs(got["grad"]))
    if case.amplitudes is not None:
        # 1 and >= 2 sub-intervals per step in one batch, and the engine cuts the model's grid
        set_problem(engine, case)
        counts = []
        for b in range(case.controls.shape[0]):
            engine.evaluate_lindblad(case.controls[b:b + 1], want_grad=False)
            counts.append(engine.lindblad_last_subintervals())
        print("sub-intervals per seed", counts)
        assert counts == wc.grid_counts(case)
        assert counts[0] == case.N - 1 and counts[1] >= 2 * (case.N - 1)


def test_want_grad_zero_and_step_densities(engine):
    """The forward pass alone (want_grad = 0) gives the cost and final densities of the full evaluation
    bit for bit, and the densities at the system steps end in the final ones."""
    case = wc.build("n40_costs_ces1")
    full = device_results(engine, case)
    set_problem(engine, case)
    cost, grads, final = engine.evaluate_lindblad(case.controls, want_grad=False)
    assert grads is None
    assert np.array_equal(cost, full["cost"]) and np.array_equal(final, full["final"])
    model_step2 = wc.lm.evaluate_with_grad(
        wc.system_of(case), case.controls[1], case.rho0, case.T, case.N, wc.case_costs(case), case.ces,
        want_grad=False, stop_step=2, piecewise_constant=True)[2]
    engine.set_keep_step_states(True)
    try:
        engine.evaluate_lindblad(case.controls, want_grad=False)
        steps = engine.download_step_densities()
    finally:
        engine.set_keep_step_states(False)
    assert steps.shape == (2, case.N, case.S, case.n, case.n)
    assert np.array_equal(steps[:, 0], np.broadcast_to(case.rho0, steps[:, 0].shape))
    assert np.array_equal(steps[:, -1], final)
    assert np.max(np.abs(steps[1, 2] - model_step2)) <= GATE_DENSITIES


@pytest.mark.parametrize("name", wc.EXACT_NAMES)
def test_the_wide_kernel_against_the_exact_reference(engine, name):
    case = wc.build(name)
    want = wc.exact_results(name)
    errors = wc.compare(device_results(engine, case), want)
    print(name, errors)
    for key in sorted(errors):
        assert errors[key] <= EXACT_GATES[key], (key, errors[key], EXACT_GATES[key])


def qubit_mode(levels=17, seed=11, N=6, T=1.5):
    """A qubit and a `levels`-level mode (n = 2 levels) with a, a^H a as operators, one drive on each."""
    n = 2 * levels
    a = np.kron(np.eye(2), cases_mod.annihilation(levels))
    sm = np.kron(np.array([[0, 1], [0, 0]], dtype=np.complex128), np.eye(levels))
    num = a.conj().T @ a
    h0 = 0.5 * (sm.conj().T @ sm) + 0.05 * num + 0.3 * (sm.conj().T @ a + a.conj().T @ sm)
    drives = [sm + sm.conj().T, 0.3 * (a + a.conj().T)]
    ops = np.stack([a, num])
    gammas = np.array([0.02, 0.005])
    rho0 = np.zeros((1, n, n), dtype=np.complex128)
    rho0[0, 0, 0] = 1
    targ = np.zeros((1, n, n), dtype=np.complex128)
    targ[0, levels, levels] = 1
    controls = 0.5 * np.random.default_rng(seed).standard_normal((N, 2))

    def hamiltonian(u, t):
        return h0 + u[0] * drives[0] + u[1] * drives[1]

    def lindblad_data(t):
        return gammas, ops
    return wc.SimpleNamespace(n=n, N=N, T=T, rho0=rho0, targ=targ, controls=controls,
                              hamiltonian=hamiltonian, lindblad_data=lindblad_data, drives=drives)


def test_forward_parity_with_the_adaptive_integrator_at_n40(engine):
    """n = 40, N = 5: against the oracle's restatement of the reference's adaptive integrator
    (oracle/qoc_lindblad_numpy.py), densities 1e-8 and cost 1e-9."""
    q = qubit_mode(levels=20, N=5, T=1.0)
    result = qoc_amd.evolve_lindblad_discrete(
        q.T, q.rho0, q.N, controls=q.controls, costs=[TargetDensityInfidelity(q.targ)],
        hamiltonian=q.hamiltonian, lindblad_data=q.lindblad_data, wide=True)
    problem = ol.LindbladProblem(q.T, q.rho0, q.N, hamiltonian=q.hamiltonian, lindblad_data=q.lindblad_data,
                                 control_eval_count=q.N, costs=[ol.TargetDensityInfidelity(q.targ)],
                                 control_count=2)
    err, fin = ol.evaluate(problem, q.controls)
    print("cost", abs(result.error - err), "densities", np.max(np.abs(result.final_densities - fin)))
    assert abs(result.error - err) < 1e-9
    assert np.max(np.abs(result.final_densities - fin)) < 1e-8


def test_a_seed_does_not_depend_on_its_neighbours(engine):
    case = wc.build("n40_subdivisions")
    rng = np.random.default_rng(77)
    others = 0.7 * rng.standard_normal((4, case.Nc, case.K))
    batch = np.concatenate([others[:2], case.controls[1:2], others[2:]])
    set_problem(engine, case)
    alone = engine.evaluate_lindblad(case.controls[1:2])
    among = engine.evaluate_lindblad(batch)
    for x, y in zip(alone, among):
        assert np.array_equal(x[0], y[2])


@pytest.fixture
def routes(monkeypatch):
    """Counts the runs of each route of the multi-start loop."""
    taken = {"resident": 0, "host": 0}
    resident, host = batch_mod.run_batch_resident, batch_mod.run_batch_host

    def run_resident(*a, **k):
        taken["resident"] += 1
        return resident(*a, **k)

    def run_host(*a, **k):
        taken["host"] += 1
        return host(*a, **k)
    monkeypatch.setattr(batch_mod, "run_batch_resident", run_resident)
    monkeypatch.setattr(batch_mod, "run_batch_host", run_host)
    return taken


class PluginAdam(Adam):  # not type(...) is Adam: takes the host loop
    pass


def test_the_public_api_at_n34(routes):
    """A qubit and a 17-level mode, wide=True: evolve against the oracle, GRAPE, the resident multi-start
    route against the host loop, an ensemble without rates against plain evaluations of its members, a
    sweep with control_scales and offsets against member(b)."""
    q = qubit_mode()
    costs = [TargetDensityInfidelity(q.targ)]
    common = dict(hamiltonian=q.hamiltonian, lindblad_data=q.lindblad_data, wide=True)
    with pytest.raises(NotImplementedError, match="hilbert_size <= 32"):
        qoc_amd.evolve_lindblad_discrete(q.T, q.rho0, q.N, controls=q.controls, costs=costs,
                                         hamiltonian=q.hamiltonian, lindblad_data=q.lindblad_data)
    result = qoc_amd.evolve_lindblad_discrete(q.T, q.rho0, q.N, controls=q.controls, costs=costs, **common)
    problem = ol.LindbladProblem(q.T, q.rho0, q.N, hamiltonian=q.hamiltonian, lindblad_data=q.lindblad_data,
                                 control_eval_count=q.N, costs=[ol.TargetDensityInfidelity(q.targ)],
                                 control_count=2)
    err, fin = ol.evaluate(problem, q.controls)
    assert abs(result.error - err) < 1e-9
    assert np.max(np.abs(result.final_densities - fin)) < 1e-8

    args = (2, q.N, costs, q.T, q.rho0, q.N)
    kw = dict(log_iteration_step=0, max_control_norms=np.full(2, 3.0), **common)
    grape = qoc_amd.grape_lindblad_discrete(*args, initial_controls=q.controls.copy(), iteration_count=3,
                                            optimizer=Adam(learning_rate=5e-2), **kw)
    assert grape.best_error < result.error

    u0 = 0.5 * np.random.default_rng(5).standard_normal((3, q.N, 2))
    a = qoc_amd.grape_lindblad_discrete_batch(*args, u0.copy(), iteration_count=3,
                                              optimizer=Adam(learning_rate=5e-2), **kw)
    b = qoc_amd.grape_lindblad_discrete_batch(*args, u0.copy(), iteration_count=3,
                                              optimizer=PluginAdam(learning_rate=5e-2), **kw)
    assert routes == {"resident": 1, "host": 1}
    assert np.array_equal(a.best_error, b.best_error)
    assert np.array_equal(a.best_iteration, b.best_iteration)
    for s in range(3):
        assert np.array_equal(a.best_controls[s], b.best_controls[s])
        assert np.array_equal(a.best_final_densities[s], b.best_final_densities[s])
    assert np.all(a.best_error < np.array([qoc_amd.evolve_lindblad_discrete(
        q.T, q.rho0, q.N, controls=u0[s], costs=costs, **common).error for s in range(3)]))

    rng = np.random.default_rng(8)
    detune = np.kron(np.diag([0.0, 1.0]), np.eye(q.n // 2)).astype(np.complex128)
    ensemble = HamiltonianEnsemble(q.hamiltonian, perturbations=[detune], offsets=[[-0.1], [0.15]],
                                   control_scales=1 + 0.05 * rng.standard_normal((2, 2)),
                                   weights=[0.4, 0.6])
    er = qoc_amd.evolve_lindblad_discrete(q.T, q.rho0, q.N, controls=q.controls, costs=costs,
                                          hamiltonian=ensemble, lindblad_data=q.lindblad_data, wide=True)
    assert er.final_densities.shape == (2,) + q.rho0.shape
    for m in range(2):
        one = qoc_amd.evolve_lindblad_discrete(q.T, q.rho0, q.N, controls=q.controls, costs=costs,
                                               hamiltonian=ensemble.member(m),
                                               lindblad_data=q.lindblad_data, wide=True)
        assert abs(er.member_errors[m] - one.error) < 1e-12
        assert np.max(np.abs(er.final_densities[m] - one.final_densities)) < 1e-12
    assert abs(er.error - (0.4 * er.member_errors[0] + 0.6 * er.member_errors[1])) < 1e-12

    sweep = LindbladSweep(q.hamiltonian, perturbations=[detune], offsets=[[-0.1], [0.0], [0.15]],
                          control_scales=1 + 0.05 * rng.standard_normal((3, 2)))
    sw = qoc_amd.grape_lindblad_discrete_batch(*args, u0.copy(), iteration_count=2,
                                               optimizer=Adam(learning_rate=5e-2),
                                               **dict(kw, hamiltonian=sweep))
    assert sw.sweep_sensitivities["rate_scales"] is None
    assert sw.sweep_sensitivities.get("evolution_time_gradients") is None
    assert sw.sweep_sensitivities["control_scales"].shape == (3, 2)
    for s in range(3):
        one = qoc_amd.evolve_lindblad_discrete(q.T, q.rho0, q.N, controls=sw.best_controls[s], costs=costs,
                                               hamiltonian=sweep.member(s), lindblad_data=q.lindblad_data,
                                               wide=True)
        assert abs(sw.best_error[s] - one.error) < 1e-12
        assert np.max(np.abs(sw.best_final_densities[s] - one.final_densities)) < 1e-12


def test_engine_refusals_by_name():
    """With the knob at 1: what has kernels of its own at n <= 32 only is refused by name before any state is
    touched, n = 65 is refused, and n = 33 is refused again once the knob is back at 0."""
    from qoc_amd.engine import Engine, QocxError
    case = wc.build("n33_s2_k1_l1")
    e = Engine(0)
    try:
        with pytest.raises(QocxError, match="1..32"):
            set_problem(e, case)
        e.set_knob("lindblad_wide", 1)
        set_problem(e, case)
        times = Engine.lindblad_stage_times(case.T, case.N, case.Nc + 1, case.K, 2)
        with pytest.raises(QocxError, match="stage tables .* hilbert_size > 32"):
            set_problem(e, case, fixed_subdivision=2, h0_stages=np.stack([case.h0 for _ in times]))
        # the refused problem left the one before in place
        assert e.evaluate_lindblad(case.controls)[0].shape == (2,)
        e.set_lindblad_ensemble(np.ones((2, 1)), None, np.array([0.5, 0.5]))
        with pytest.raises(QocxError, match="per-member rates .* hilbert_size > 32"):
            e.set_lindblad_ensemble_rates(np.ones((2, 1)))
        set_problem(e, case)
        with pytest.raises(QocxError, match="per-seed rates .* hilbert_size > 32"):
            e.set_lindblad_sweep(np.ones((2, 1)), None, np.ones((2, 1)))
        e.set_lindblad_sweep(np.ones((2, 1)), None, None)
        with pytest.raises(QocxError, match="rate sensitivities .* hilbert_size > 32"):
            e.lindblad_sweep_want_rate_sensitivities(True)
        with pytest.raises(QocxError, match="per-seed durations .* hilbert_size > 32"):
            e.lindblad_sweep_set_durations(np.ones(2), np.ones((2, 1)), None, None, 0.5, 1.5, 0.0)
        big = wc.SimpleNamespace(**dict(vars(case), n=65, h0=np.zeros((65, 65)), g=[np.eye(65)],
                                        operators=None, gammas=None,
                                        rho0=np.stack([np.eye(65) / 65] * 2), cost_specs=[]))
        with pytest.raises(QocxError, match="1..64"):
            set_problem(e, big)
        e.set_knob("lindblad_wide", 0)
        with pytest.raises(QocxError, match="1..32"):
            set_problem(e, case)
    finally:
        e.close()
