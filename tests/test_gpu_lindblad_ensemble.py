"""
GPU tests (-m gpu) of HamiltonianEnsemble on the Lindblad path (qocx_lindblad_set_ensemble):

a. a member is, bit for bit, the plain (K_r + J)-channel Lindblad problem on host-expanded
   controls - through qocx_eval_lindblad and through the resident calls - and the seeds' costs and
   gradients are the fold of the members' in member order with one fma per member;
b. members against the CPU references, at the gates tests/test_gpu_lindblad.py holds the plain path
   to: the NumPy model of the device algorithm on the (K_r + J)-channel system (cost and final
   densities 1e-12, gradients 1e-10 of max |g| with a floor of 1e-3) and the reference integrator
   on the member problem with sum_j delta_mj D_j folded into the Hamiltonian (cost 1e-9, final
   densities 1e-8);
c. every item picks its own sub-division count: the members of one seed fall into different
   groups and no result depends on the batch neighbours;
d. the degenerate ensemble (M = 1, J = 0, s = 1, w = 1) is the plain problem, bit for bit;
e. multi-start GRAPE: the resident route against the host loop and single-seed runs (best_error
   1e-12, best_controls 1e-10 relative, member_errors 1e-12);
f. the engine's rejections.
"""

from fractions import Fraction

import numpy as np
import pytest

import qoc_amd
from oracle import qoc_lindblad_numpy as ol
from qoc_amd.core import batch as batch_mod
from qoc_amd.core import device
from qoc_amd.engine import Engine, QocxError
from qoc_amd.standard import LBFGS, Adam, ControlBasis, HamiltonianEnsemble
from qoc_amd.standard.costs import ControlVariation
from tests import cases as cases_mod
from tests import gpu_helpers as gh
from tests import helpers
from tests import lindblad_model as lm
from tests.test_lindblad_host_api import product_cost_list

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def real_engine():
    helpers.set_backend_factory(None)
    yield
    helpers.set_backend_factory(None)


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


class RecordingEngine(Engine):
    """The engine, remembering the arguments of the last set_lindblad_problem: the plain
    (K_r + J)-channel problem is set from the very arrays the ensemble's problem was set from."""

    def set_lindblad_problem(self, *a, **kw):
        self.last_problem = (a, kw)
        Engine.set_lindblad_problem(self, *a, **kw)


def k6_case():
    """n = 4 with six controls: with J = 2 the K = 8 edge of the Lindblad engine."""
    return cases_mod.lindblad_case("lindblad_n4_k6", n=4, N=7, S=1, K=6, seeds=2, h_seed=76,
                                   Nc=4, T=0.6, sigma=0.3)


def case_of(name):
    return k6_case() if name == "lindblad_n4_k6" else cases_mod.lindblad_case_by_name(name)


def make_ensemble(case, M, J, seed, offset_scale=0.3, d_scale=0.5):
    rng = np.random.default_rng(seed)
    d = np.stack([d_scale * cases_mod.gue(rng, case.n) for _ in range(J)]) if J else None
    return HamiltonianEnsemble(
        case.hamiltonian(), perturbations=d,
        offsets=offset_scale * rng.standard_normal((M, J)) if J else None,
        control_scales=1 + 0.05 * rng.standard_normal((M, case.K)),
        weights=rng.uniform(0.2, 1.0, M))


def make_evaluator(case, hamiltonian, backend, **kw):
    return device.LindbladEvaluator(
        case.T, case.initial_densities, case.N, hamiltonian=hamiltonian,
        lindblad_data=case.lindblad_data(), control_count=case.K, control_eval_count=case.Nc,
        complex_controls=case.complex_controls, costs=product_cost_list(case),
        cost_eval_step=case.cost_eval_step, backend=backend, **kw)


def expand(e, u):
    """Seeds (B, Nc, K_r) -> items (B, M, Nc, K_r + J): one product, one rounding."""
    M, J = e.member_count, e.perturbation_count
    B, Nc, kr = u.shape
    items = np.empty((B, M, Nc, kr + J))
    scales = np.ones((M, kr)) if e.control_scales is None else e.control_scales
    items[..., :kr] = scales[None, :, None, :] * u[:, None]
    if J:
        items[..., kr:] = e.offsets[None, :, None, :]
    return items


def fma_fold(terms):
    """acc = fma(a_m, x_m, acc) over m from 0.0, exactly: every step rounds the exact a x + acc
    once, as the reduce kernel's fma does."""
    acc = 0.0
    for a, x in terms:
        acc = float(Fraction(float(a)) * Fraction(float(x)) + Fraction(acc))
    return acc


def folded(e, member_cost, item_grads):
    """The seeds' costs and gradients as ensemble_reduce_kernel forms them from the items'."""
    B, M = member_cost.shape
    cost = np.array([fma_fold((e.weights[m], member_cost[b, m]) for m in range(M))
                     for b in range(B)])
    kr = e.control_scales.shape[1]
    grads = np.empty(item_grads.shape[:1] + item_grads.shape[2:3] + (kr,))
    for idx in np.ndindex(*grads.shape):
        b, j, k = idx
        grads[idx] = fma_fold((e.weights[m] * e.control_scales[m, k], item_grads[b, m, j, k])
                              for m in range(M))
    return cost, grads


SHAPES = {  # name: (M, J) - the stage loops named in the module docstring's (a)
    "lindblad_n4": (3, 2),       # n <= 16 stage loops, ForbidDensities step costs
    "lindblad_wc_n16": (3, 1),   # four waves, two-sided
    "lindblad_n20": (2, 1),      # the tile-per-wave kernel
    "lindblad_timedep": (2, 1),  # stage tables, fixed grid
    "lindblad_n4_k6": (2, 2),    # K_r + J = 8
}
_RUNS = {}


def run_shape(name):
    """One ensemble evaluation and the plain evaluation of its expanded items, shared by the tests
    of (a) and (b): the reference is computed once and left unchanged."""
    if name in _RUNS:
        return _RUNS[name]
    case = case_of(name)
    M, J = SHAPES[name]
    e = make_ensemble(case, M, J, seed=300 + len(name))
    u = 0.4 * np.random.default_rng(17).standard_normal((2, case.Nc, case.K))
    engine = RecordingEngine(0)
    try:
        ev = make_evaluator(case, e, engine)
        errors, grads, finals, _ = ev.evaluate_batch(u)  # (time dependent: sets the tables)
        members = ev.member_errors()
        ens_host = engine.evaluate_lindblad(u)
        members_host = engine.lindblad_ensemble_member_costs()
        engine.lindblad_upload_controls(u)
        engine.eval_lindblad_resident(True)
        ens_resident = engine.lindblad_download_results()
        members_resident = engine.lindblad_ensemble_member_costs()
        resident_costs = engine.lindblad_download_costs()
        # the plain (K_r + J)-channel problem from the same arrays, on host-expanded controls
        a, kw = engine.last_problem
        Engine.set_lindblad_problem(engine, *a, **kw)
        items = expand(e, u)
        plain = engine.evaluate_lindblad(items.reshape((-1,) + items.shape[2:]))
    finally:
        engine.close()
    _RUNS[name] = dict(case=case, e=e, u=u, items=items, evaluator=(errors, grads, finals, members),
                       host=ens_host + (members_host,),
                       resident=ens_resident + (members_resident,),
                       resident_costs=resident_costs, plain=plain, problem=(a, kw))
    return _RUNS[name]


# ---- a. members are the plain expanded problem ------------------------------------------------------

@pytest.mark.parametrize("name", sorted(SHAPES))
def test_members_are_the_plain_problem_on_expanded_controls(name):
    r = run_shape(name)
    case, e, u = r["case"], r["e"], r["u"]
    M, J = SHAPES[name]
    B, kr = u.shape[0], case.K
    S, n = case.initial_densities.shape[0], case.n
    assert r["problem"][0][2] == kr + J
    assert (r["problem"][1].get("fixed_subdivision", 0) > 0) == (case.time_mod is not None)
    p_cost, p_grads, p_final = r["plain"]
    p_cost = p_cost.reshape(B, M)
    p_grads = p_grads.reshape(B, M, case.Nc, kr + J)
    p_final = p_final.reshape(B, M, S, n, n)
    want_cost, want_grads = folded(e, p_cost, p_grads)
    for cost, grads, final, members in (r["host"], r["resident"]):
        assert final.shape == (B, M, S, n, n) and grads.shape == (B, case.Nc, kr)
        assert np.array_equal(members, p_cost)
        assert np.array_equal(final, p_final)
        # the seeds' results are the fold of the plain items' in member order, one fma each: equal
        # reduced gradients for every member weighting the items enter with
        assert np.array_equal(cost, want_cost)
        assert np.array_equal(grads, want_grads)
        sum_cost = np.sum(e.weights[None] * p_cost, axis=1)
        sum_grads = np.sum((e.weights[:, None] * e.control_scales)[None, :, None, :]
                           * p_grads[..., :kr], axis=1)
        assert np.max(np.abs(cost - sum_cost) / np.abs(sum_cost)) < 1e-14
        assert np.max(np.abs(grads - sum_grads)) < 1e-14 * np.max(np.abs(sum_grads))
    assert np.array_equal(r["resident_costs"], want_cost)
    # ... and what the evaluator hands on is the engine's
    errors, grads, finals, members = r["evaluator"]
    assert np.array_equal(errors, want_cost) and np.array_equal(grads, want_grads)
    assert np.array_equal(finals, p_final) and np.array_equal(members, p_cost)


def test_one_hot_weights_return_the_items_own_gradients():
    """scales = 1 and w = e_m: the reduced gradient IS item m's, so the items' gradients equal the
    plain problem's bit for bit."""
    case = cases_mod.lindblad_case_by_name("lindblad_wc_n16")
    rng = np.random.default_rng(23)
    M, J = 3, 1
    d = np.stack([0.5 * cases_mod.gue(rng, case.n)])
    offsets = 0.3 * rng.standard_normal((M, J))
    u = 0.4 * rng.standard_normal((2, case.Nc, case.K))
    engine = RecordingEngine(0)
    try:
        got = []
        for m in range(M):
            e = HamiltonianEnsemble(case.hamiltonian(), perturbations=d, offsets=offsets,
                                    weights=np.eye(M)[m])
            ev = make_evaluator(case, e, engine)
            got.append(ev.evaluate_batch(u)[1])
        a, kw = engine.last_problem
        Engine.set_lindblad_problem(engine, *a, **kw)
        items = expand(e, u)
        _, p_grads, _ = engine.evaluate_lindblad(items.reshape((-1,) + items.shape[2:]))
    finally:
        engine.close()
    p_grads = p_grads.reshape(2, M, case.Nc, case.K + J)
    for m in range(M):
        assert np.array_equal(got[m], p_grads[:, m, :, :case.K])


# ---- b. members against the CPU references ----------------------------------------------------------

@pytest.mark.parametrize("name", ["lindblad_n4", "lindblad_wc_n16"])
def test_members_match_the_device_model_and_the_reference_integrator(name):
    r = run_shape(name)
    case, e, u, items = r["case"], r["e"], r["u"], r["items"]
    M, J = SHAPES[name]
    kr = case.K
    _, _, final, members = r["host"]
    p_grads = r["plain"][1].reshape(u.shape[0], M, case.Nc, kr + J)
    costs = [getattr(ol, k)(**kw) for k, kw in case.cost_specs]
    system = lm.StructuredLindblad(case.h0, gh.lindblad_generators(case) + list(e.perturbations),
                                   case.dissipators, case.operators)
    b = 1
    # (the model takes seconds per member at n = 16: there the last member, every member at n = 4;
    # the reference integrator on every member of both)
    for m in range(M):
        if case.n < 16 or m == M - 1:
            m_err, m_grads, m_final = lm.evaluate_with_grad(
                system, items[b, m], case.initial_densities, case.T, case.N, costs,
                case.cost_eval_step)
            scale = max(np.max(np.abs(m_grads)), 1e-3)
            print(name, m, "model:", abs(members[b, m] - m_err),
                  np.max(np.abs(final[b, m] - m_final)), np.max(np.abs(p_grads[b, m] - m_grads)) / scale)
            assert abs(members[b, m] - m_err) < 1e-12
            assert np.max(np.abs(final[b, m] - m_final)) < 1e-12
            assert np.max(np.abs(p_grads[b, m] - m_grads)) / scale < 1e-10
        problem = ol.LindbladProblem(
            case.T, case.initial_densities, case.N, hamiltonian=e.member(m),
            lindblad_data=case.lindblad_data(), control_eval_count=case.Nc, costs=costs,
            cost_eval_step=case.cost_eval_step, control_count=case.K)
        o_err, o_final = ol.evaluate(problem, u[b])
        print(name, m, "reference:", abs(members[b, m] - o_err),
              np.max(np.abs(final[b, m] - o_final)))
        assert abs(members[b, m] - o_err) < 1e-9
        assert np.max(np.abs(final[b, m] - o_final)) < 1e-8


# ---- c. sub-division groups -------------------------------------------------------------------------

def test_items_of_one_seed_take_their_own_subdivision_counts():
    case = cases_mod.lindblad_case_by_name("lindblad_n4")
    rng = np.random.default_rng(29)
    M, J = 3, 1
    d = np.stack([cases_mod.gue(rng, case.n)])
    d = d / np.linalg.norm(d[0], 2)
    e = HamiltonianEnsemble(case.hamiltonian(), perturbations=d,
                            offsets=np.array([[0.0], [15.0], [40.0]]),
                            control_scales=np.array([[1.0, 1.0], [1.1, 0.9], [0.9, 1.2]]),
                            weights=np.array([0.5, 0.3, 0.2]))
    base = 0.3 * rng.standard_normal((case.Nc, case.K))
    u = np.stack([base, 6.0 * base, 20.0 * base])  # three seeds of different amplitude
    # the precondition, from the model of the device's rule: the members of every seed differ in
    # their sub-division counts, and so do the seeds
    system = lm.StructuredLindblad(case.h0, gh.lindblad_generators(case) + list(d),
                                   case.dissipators, case.operators)
    items = expand(e, u)
    dt = case.T / (case.N - 1)
    counts = np.array([[int(np.ceil(system.norm_bound(np.max(np.abs(items[b, m]), axis=0))
                                    * dt / 0.4)) for m in range(M)] for b in range(3)])
    grids = np.array([[len(lm.substep_grid(case.T, case.N, case.Nc, system.norm_bound(
        np.max(np.abs(items[b, m]), axis=0)))[0]) for m in range(M)] for b in range(3)])
    assert all(len(set(counts[b])) == M for b in range(3)), counts
    assert len(set(counts[:, 0])) == 3 and np.all(grids >= counts)
    engine = Engine(0)
    try:
        ev = make_evaluator(case, e, engine)
        full = ev.evaluate_batch(u)[:3] + (ev.member_errors(),)
        subintervals = engine.lindblad_last_subintervals()
        alone, alone_sub = [], 0
        for b in range(3):
            alone.append(ev.evaluate_batch(u[b:b + 1])[:3] + (ev.member_errors(),))
            alone_sub += engine.lindblad_last_subintervals()
        engine.lindblad_upload_controls(u[::-1])
        engine.eval_lindblad_resident(True)
        resident = engine.lindblad_download_results() + (engine.lindblad_ensemble_member_costs(),)
    finally:
        engine.close()
    assert subintervals == alone_sub  # (every item ran on the grid it runs on alone)
    for b in range(3):
        for x, y in zip(full, alone[b]):
            assert np.array_equal(x[b], y[0])
        for x, y in zip(full, resident):
            assert np.array_equal(x[b], y[2 - b])


# ---- d. the degenerate ensemble ---------------------------------------------------------------------

@pytest.mark.parametrize("name", ["lindblad_n4", "lindblad_wc_n16"])
def test_degenerate_ensemble_is_the_plain_problem(name):
    case = cases_mod.lindblad_case_by_name(name)
    u = np.stack(case.controls)
    engine = Engine(0)
    try:
        gh.setup_lindblad_engine(engine, case)
        plain = engine.evaluate_lindblad(u)
        engine.set_lindblad_ensemble(np.ones((1, case.K)), None, np.ones(1))
        host = engine.evaluate_lindblad(u)
        members = engine.lindblad_ensemble_member_costs()
        engine.lindblad_upload_controls(u)
        engine.eval_lindblad_resident(True)
        resident = engine.lindblad_download_results()
    finally:
        engine.close()
    for out in (host, resident):
        assert np.array_equal(out[0], plain[0]) and np.array_equal(out[1], plain[1])
        assert np.array_equal(out[2][:, 0], plain[2]) and out[2].shape[1] == 1
    assert np.array_equal(members[:, 0], plain[0])


# ---- e. multi-start ---------------------------------------------------------------------------------

class HostAdam(Adam):  # not type(...) is Adam: the host loop
    pass


class HostLBFGS(LBFGS):
    pass


OPTIMIZERS = {
    "adam": (lambda: Adam(learning_rate=2e-2), lambda: HostAdam(learning_rate=2e-2)),
    "lbfgs": (LBFGS, HostLBFGS),
}


def rel_err(a, b):
    return np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(np.max(np.abs(np.asarray(b))), 1e-300)


def assert_close_runs(a, b, seeds, M, shape):
    for s in range(seeds):
        assert a.best_iteration[s] == b.best_iteration[s]
        assert abs(a.best_error[s] - b.best_error[s]) < 1e-12
        assert rel_err(a.best_controls[s], b.best_controls[s]) < 1e-10
        assert np.max(np.abs(a.member_errors[s] - b.member_errors[s])) < 1e-12
        assert a.best_final_densities[s].shape == (M,) + shape
        assert a.member_errors[s].shape == (M,)


def multistart(routes, optimizer, case, e, u0, iterations=4, single=True, more_costs=(), **extra):
    resident, host = OPTIMIZERS[optimizer]
    costs = product_cost_list(case) + list(more_costs)
    args = (case.K, case.Nc, costs, case.T, case.initial_densities, case.N)
    kw = dict(cost_eval_step=case.cost_eval_step, hamiltonian=e,
              lindblad_data=case.lindblad_data(), log_iteration_step=0,
              iteration_count=iterations, complex_controls=case.complex_controls, **extra)
    a = qoc_amd.grape_lindblad_discrete_batch(*args, u0.copy(), optimizer=resident(), **kw)
    assert routes == {"resident": 1, "host": 0}
    b = qoc_amd.grape_lindblad_discrete_batch(*args, u0.copy(), optimizer=host(), **kw)
    assert routes == {"resident": 1, "host": 1}
    B, M = u0.shape[0], e.member_count
    assert_close_runs(a, b, B, M, case.initial_densities.shape)
    for s in range(B if not more_costs else 0):  # (costs of the controls come on top)
        assert abs(a.best_error[s] - np.dot(e.weights, a.member_errors[s])) < 1e-12
    if single:
        for s in range(B):
            one = qoc_amd.grape_lindblad_discrete(*args, initial_controls=u0[s].copy(),
                                                  optimizer=resident(), **kw)
            assert one.best_iteration == a.best_iteration[s]
            assert abs(one.best_error - a.best_error[s]) < 1e-12
            assert rel_err(a.best_controls[s], one.best_controls) < 1e-10
            assert np.max(np.abs(one.member_errors - a.member_errors[s])) < 1e-12
    return a, b


@pytest.mark.parametrize("optimizer", ["adam", "lbfgs"])
def test_resident_route_equals_host_loop_and_single_seed_runs(routes, optimizer):
    case = cases_mod.lindblad_case_by_name("lindblad_n4")
    e = make_ensemble(case, 3, 2, seed=51)
    u0 = np.clip(0.5 * np.random.default_rng(52).standard_normal((3, case.Nc, case.K)), -0.8, 0.8)
    a, _ = multistart(routes, optimizer, case, e, u0, max_control_norms=np.full(case.K, 0.8))
    assert np.any(a.best_iteration > 0)


def test_resident_route_with_a_sine_basis_and_a_control_cost_on_the_device(routes):
    case = cases_mod.lindblad_case_by_name("lindblad_n4")
    e = make_ensemble(case, 3, 2, seed=53)
    basis = ControlBasis.sine(case.Nc, 4)
    c0 = 0.2 * np.random.default_rng(54).standard_normal((3, 4, case.K))
    for b in range(3):
        c0[b] *= min(1.0, 0.75 / np.max(np.abs(basis.expand(c0[b]))))
    a, b = multistart(routes, "adam", case, e, c0, single=False, control_basis=basis,
                      max_control_norms=np.full(case.K, 0.8),
                      more_costs=[ControlVariation(case.K, case.Nc, cost_multiplier=0.4, order=1)])
    for s in range(3):
        assert a.best_coefficients[s].shape == (4, case.K)
        assert rel_err(a.best_coefficients[s], b.best_coefficients[s]) < 1e-10
        variation = ControlVariation(case.K, case.Nc, cost_multiplier=0.4, order=1).cost(
            a.best_controls[s], None, case.N - 1)
        assert variation > 0  # once per seed, on the seed's pulse:
        assert abs(a.best_error[s] - variation - np.dot(e.weights, a.member_errors[s])) < 1e-12


def test_resident_route_with_complex_controls(routes):
    case = cases_mod.lindblad_case_by_name("lindblad_n4_complex")
    e = make_ensemble(case, 2, 1, seed=55)
    rng = np.random.default_rng(56)
    u0 = 0.3 * (rng.standard_normal((3, case.Nc, case.K))
                + 1j * rng.standard_normal((3, case.Nc, case.K)))
    a, _ = multistart(routes, "adam", case, e, u0, max_control_norms=np.full(case.K, 2.0))
    assert all(np.iscomplexobj(c) for c in a.best_controls)


# ---- f. the engine's rejections ---------------------------------------------------------------------

def test_engine_rejections():
    case = k6_case()
    engine = Engine(0)
    rng = np.random.default_rng(61)
    try:
        # K_r + J = 9: the problem setter's limit (QOCX_LINDBLAD_MAX_K = 8)
        g9 = gh.lindblad_generators(case) + [cases_mod.gue(rng, case.n) for _ in range(3)]
        with pytest.raises(QocxError, match="control_count must be in 0..8") as err:
            engine.set_lindblad_problem(
                case.n, 1, 9, case.Nc, case.N, case.T, case.h0, g9, case.dissipators,
                case.operators, case.initial_densities, costs=gh.lindblad_device_costs(case))
        assert err.value.code == -1
        gh.setup_lindblad_engine(engine, case)  # K = 6
        with pytest.raises(QocxError, match="no ensemble set") as err:
            engine.lindblad_ensemble_member_costs()
        assert err.value.code == -3
        with pytest.raises(QocxError, match="fixed < control_count") as err:
            engine.set_lindblad_ensemble(None, np.zeros((2, 6)), np.ones(2))
        assert err.value.code == -1
        bad = np.ones((2, 5))
        bad[1, 3] = np.inf
        with pytest.raises(QocxError, match="non-finite ensemble control scale"):
            engine.set_lindblad_ensemble(bad, np.zeros((2, 1)), np.ones(2))
        with pytest.raises(QocxError, match="non-finite ensemble offset"):
            engine.set_lindblad_ensemble(None, np.array([[0.0], [np.nan]]), np.ones(2))
        with pytest.raises(QocxError, match="weights must be finite and >= 0"):
            engine.set_lindblad_ensemble(None, np.zeros((2, 1)), np.array([1.0, -0.5]))
        engine.set_lindblad_ensemble(None, np.zeros((2, 1)), np.ones(2))
        with pytest.raises(QocxError, match="no evaluation results"):
            engine.lindblad_ensemble_member_costs()
        bars = np.zeros((2, 1, 1, case.n, case.n), dtype=np.complex128)
        with pytest.raises(QocxError, match="not taken with an ensemble") as err:
            engine.set_density_cotangents([case.N - 1], bars)
        assert err.value.code == -3
        engine.set_density_cotangents(None, None)  # clearing is always fine
        # after the refusals the ensemble still evaluates; a new problem clears it
        u = 0.2 * rng.standard_normal((2, case.Nc, 5))
        cost, grads, final = engine.evaluate_lindblad(u)
        assert grads.shape == u.shape and final.shape == (2, 2, 1, case.n, case.n)
        assert np.all(np.isfinite(cost)) and np.all(np.isfinite(grads))
        gh.setup_lindblad_engine(engine, case)
        with pytest.raises(QocxError, match="no ensemble set"):
            engine.lindblad_ensemble_member_costs()
    finally:
        engine.close()
