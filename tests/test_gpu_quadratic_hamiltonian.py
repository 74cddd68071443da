"""
GPU tests (-m gpu) of Hamiltonians quadratic in the controls on the device
(qoc_amd.standard.QuadraticHamiltonian -> qocx_set_quadratic_terms): the engine evaluates
H = H0(t) + sum_k r_k G_k(t) + sum r_k r_l Q_kl as linear in the effective controls (r_k, r_k r_l)
on the wavefront route (n <= 64) and the general route (n > 64), and the user's callable is not
called during an evaluation.
"""

import copy

import numpy as np
import pytest

import qoc_amd
import qoc_amd.standard.costs as product_costs
from oracle import qoc_numpy as onp
from qoc_amd import engine as engine_mod
from qoc_amd.core import batch as batch_mod
from qoc_amd.core import device
from qoc_amd.standard import SGD, Adam, QuadraticHamiltonian
from tests import cases as cases_mod
from tests import helpers
from tests.helpers import golden, rel_err

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


class Counted(object):
    def __init__(self, fn):
        self.fn, self.calls = fn, 0

    def __call__(self, *a):
        self.calls += 1
        return self.fn(*a)


def product_cost_list(case):
    return [getattr(product_costs, kind)(**kw) for kind, kw in case.cost_specs]


def quadratic_of_case(case):
    """The fixture's Hamiltonian rebuilt as linear part + (k, k, quad_k) terms (complex
    controls: (2k, 2k, Q) and (2k + 1, 2k + 1, Q), |u_k|^2 = Re^2 + Im^2)."""
    lin = copy.copy(case)
    lin.quad = None
    terms = []
    for k, q in enumerate(case.quad):
        if case.complex_controls:
            terms += [(2 * k, 2 * k, q), (2 * k + 1, 2 * k + 1, q)]
        else:
            terms.append((k, k, q))
    counted = Counted(lin.hamiltonian())
    return QuadraticHamiltonian(counted, terms), counted


# ---- the reference's fixtures of quadratic Hamiltonians ------------------------------------------

@pytest.mark.parametrize("name", ["opaque_eps2_real", "opaque_stark_complex", "opaque_eps2_n36"])
def test_reference_fixtures_on_the_quadratic_route(name):
    """The gates of tests/test_gpu_api.py::test_opaque_hamiltonian_on_gpu: reference forward
    1e-10, gradients 1e-8 vs AD and 1e-7 vs finite differences of the reference forward."""
    case = cases_mod.case_by_name(name)
    g = golden(name)
    h, counted = quadratic_of_case(case)
    ev = device.SchroedingerEvaluator(
        case.T, h, case.initial_states, case.N, control_count=case.K,
        control_eval_count=case.Nc, complex_controls=case.complex_controls,
        costs=product_cost_list(case), cost_eval_step=case.cost_eval_step)
    assert ev.opaque_hamiltonian is None and ev.linearized_hamiltonian is None
    assert ev.quadratic_terms is not None
    counted.calls = 0
    errors, grads, finals, _ = ev.evaluate_batch(np.stack(case.controls), want_grad=True)
    assert counted.calls == 0
    for b in range(len(case.controls)):
        assert abs(errors[b] - g["error"][b]) < 1e-10
        assert rel_err(finals[b], g["final_states"][b]) < 1e-10
        assert rel_err(grads[b], g["grads_ad"][b]) < 1e-8
        scale = np.max(np.abs(g["grads_ad"][b]))
        assert np.max(np.abs(np.asarray(grads[b]).flat[g["fd_index"][b]] - g["grads_fd"][b])) / scale < 1e-7
    # the single-evaluation entry point (latency mode) on the same route
    result = qoc_amd.evolve_schroedinger_discrete(
        case.T, h, case.initial_states, case.N, controls=case.controls[0],
        cost_eval_step=case.cost_eval_step, costs=product_cost_list(case))
    assert abs(result.error - g["error"][0]) < 1e-10
    assert rel_err(result.final_states, g["final_states"][0]) < 1e-10


# ---- other shapes: cross pairs, non-Hermitian Q, both adjoints, the general route ---------------

def shaped_problem(n, step_cost, K=3, N=21, Nc=8, seed=0, time_dependent=False):
    """A transmon-like linear part (complex-Hermitian drives) with a square, a cross pair and a
    non-Hermitian Q on a Hermitian linear part."""
    rng = np.random.default_rng(1000 + n + seed)
    h0 = cases_mod.gue(rng, n)
    gs = [cases_mod.gue(rng, n) for _ in range(K)]

    def linear(u, t):
        out = h0 * (1 + 0.25 * np.sin(2.1 * t)) if time_dependent else h0
        for k in range(K):
            out = out + u[k] * gs[k]
        return out
    nonherm = 0.3 * (rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))) / np.sqrt(n)
    terms = [(0, 0, 0.6 * cases_mod.gue(rng, n)), (0, 2, 0.5 * cases_mod.gue(rng, n)),
             (1, 2, nonherm)]
    S = 2
    psi0 = cases_mod.column_states(np.eye(n)[:, :S])
    target = cases_mod.column_states(cases_mod.random_unitary(rng, n)[:, :S])
    T = 0.06 * (N - 1)
    if step_cost:
        costs = [product_costs.TargetStateInfidelityTime(N, target)]
        ocosts = [onp.TargetStateInfidelityTime(N, target)]
    else:
        costs = [product_costs.TargetStateInfidelity(target)]
        ocosts = [onp.TargetStateInfidelity(target)]
    controls = 0.7 * rng.standard_normal((3, Nc, K))
    controls[1] *= 0.05
    return dict(linear=linear, terms=terms, psi0=psi0, T=T, N=N, Nc=Nc, K=K, costs=costs,
                ocosts=ocosts, controls=controls)


def oracle_forward(p, h, u):
    problem = onp.SchroedingerProblem(p["T"], h, p["psi0"], p["N"], control_eval_count=p["Nc"],
                                      costs=p["ocosts"], control_count=p["K"])
    return onp.evaluate(problem, u)


@pytest.mark.parametrize("n", [24, 72])
@pytest.mark.parametrize("step_cost", [False, True])
def test_shapes_against_the_oracle_and_the_opaque_route(n, step_cost):
    p = shaped_problem(n, step_cost, time_dependent=(n == 24))
    counted = Counted(p["linear"])
    h = QuadraticHamiltonian(counted, p["terms"])
    plain = lambda u, t: h(u, t)  # noqa: E731 - today's opaque route on the same function
    kw = dict(control_count=p["K"], control_eval_count=p["Nc"], costs=p["costs"])
    ev = device.SchroedingerEvaluator(p["T"], h, p["psi0"], p["N"], **kw)
    ev_opaque = device.SchroedingerEvaluator(p["T"], plain, p["psi0"], p["N"], **kw)
    assert ev.opaque_hamiltonian is None and ev_opaque.opaque_hamiltonian is plain
    counted.calls = 0
    errors, grads, finals, _ = ev.evaluate_batch(p["controls"])
    assert counted.calls == 0
    _, grads_opaque, _, _ = ev_opaque.evaluate_batch(p["controls"])
    rng = np.random.default_rng(n)
    for b in range(len(p["controls"])):
        u = p["controls"][b]
        err, fin = oracle_forward(p, h, u)
        assert abs(errors[b] - err) < 1e-10
        assert np.max(np.abs(finals[b] - fin)) < 1e-10
        assert rel_err(grads[b], grads_opaque[b]) < 1e-8
        scale = np.max(np.abs(grads[b]))
        for _ in range(3):  # central differences of the oracle forward
            i, k = rng.integers(p["Nc"]), rng.integers(p["K"])
            step = 1e-5
            up, down = u.copy(), u.copy()
            up[i, k] += step
            down[i, k] -= step
            fd = (oracle_forward(p, h, up)[0] - oracle_forward(p, h, down)[0]) / (2 * step)
            assert abs(grads[b][i, k] - fd) / scale < 1e-7


def test_batch_equals_single_bit_for_bit():
    """Seeds of very different amplitude in one batch: each seed's results equal its own
    one-seed evaluation bit for bit (the route depends on the problem, not on the batch)."""
    p = shaped_problem(24, False, seed=3)
    h = QuadraticHamiltonian(p["linear"], p["terms"])
    u = p["controls"].copy()
    u[0] *= 0.01
    u[2] *= 3.0
    ev = device.SchroedingerEvaluator(p["T"], h, p["psi0"], p["N"], control_count=p["K"],
                                      control_eval_count=p["Nc"], costs=p["costs"])
    errors, grads, finals, _ = ev.evaluate_batch(u)
    for b in range(3):
        e1, g1, f1, _ = ev.evaluate_batch(u[b:b + 1])
        assert e1[0] == errors[b]
        assert np.array_equal(g1[0], grads[b])
        assert np.array_equal(f1[0], finals[b])


# ---- multi-start GRAPE ---------------------------------------------------------------------------

class PluginAdam(Adam):  # not type(...) is Adam: takes the host loop
    pass


class PluginSGD(SGD):
    pass


def test_multistart_runs_resident_and_equals_host_loop_and_single_runs(routes):
    p = shaped_problem(24, False, seed=5, N=31, Nc=10)
    h = QuadraticHamiltonian(p["linear"], p["terms"])
    B = 5
    u0 = np.clip(0.6 * np.random.default_rng(93).standard_normal((B, p["Nc"], p["K"])), -1, 1)
    args = (p["K"], p["Nc"], p["costs"], p["T"], h, p["psi0"], p["N"])
    kw = dict(iteration_count=5, log_iteration_step=0, max_control_norms=np.full(p["K"], 1.0))
    a = qoc_amd.grape_schroedinger_discrete_batch(*args, u0.copy(),
                                                  optimizer=Adam(learning_rate=5e-2), **kw)
    assert routes == {"resident": 1, "host": 0}
    b = qoc_amd.grape_schroedinger_discrete_batch(*args, u0.copy(),
                                                  optimizer=PluginAdam(learning_rate=5e-2), **kw)
    assert routes == {"resident": 1, "host": 1}
    assert np.array_equal(a.best_error, b.best_error)
    assert np.array_equal(a.best_iteration, b.best_iteration)
    for s in range(B):
        assert np.array_equal(a.best_controls[s], b.best_controls[s])
        assert np.array_equal(a.best_final_states[s], b.best_final_states[s])
    for s in range(B):
        one = qoc_amd.grape_schroedinger_discrete_batch(*args, u0[s:s + 1].copy(),
                                                        optimizer=Adam(learning_rate=5e-2), **kw)
        assert one.best_error[0] == a.best_error[s]
        assert np.array_equal(one.best_controls[0], a.best_controls[s])
        assert np.array_equal(one.best_final_states[0], a.best_final_states[s])
        ref = qoc_amd.grape_schroedinger_discrete(*args, initial_controls=u0[s].copy(),
                                                  optimizer=Adam(learning_rate=5e-2), **kw)
        assert ref.best_iteration == a.best_iteration[s]
        assert abs(ref.best_error - a.best_error[s]) < 1e-12
        assert rel_err(a.best_controls[s], ref.best_controls) < 1e-10
    assert routes["host"] == 1 and routes["resident"] == 1 + B


# ---- norm bounds between knots -------------------------------------------------------------------

def crossing_problem(n):
    """r_0 goes 0 -> a and r_1 a -> 0 over one knot interval: r_0 r_1 is 0 at both knots and
    a^2 / 4 in the middle, where Q_01 dominates the step generator."""
    rng = np.random.default_rng(77 + n)
    h0 = 0.2 * cases_mod.gue(rng, n)
    gs = [0.01 * cases_mod.gue(rng, n) for _ in range(2)]
    q = 3.0 * cases_mod.gue(rng, n)
    a = 4.0
    N, Nc, T = 3, 2, 2.0
    controls = np.array([[0.0, a], [a, 0.0]])[None]
    psi0 = cases_mod.column_states(np.eye(n)[:, :2])
    target = cases_mod.column_states(np.roll(np.eye(n), 1, axis=0)[:, :2])
    linear = lambda u, t: h0 + u[0] * gs[0] + u[1] * gs[1]  # noqa: E731
    h = QuadraticHamiltonian(linear, [(0, 1, q)])
    dt = T / (N - 1)
    one = lambda m: np.max(np.sum(np.abs(m), axis=0))  # noqa: E731
    knot_bound = dt * (one(h0) + a * max(one(gs[0]), one(gs[1])))
    mid = dt * one(h(np.array([a / 4, 3 * a / 4]), 0.0))  # the first step's midpoint
    # a bound taken at the knots alone would under-count the squarings the midpoints need
    assert onp.pade_scale_count(knot_bound) < onp.pade_scale_count(mid)
    return dict(h=h, psi0=psi0, target=target, N=N, Nc=Nc, T=T, controls=controls, a=a)


@pytest.mark.parametrize("n", [6, 24, 72])
def test_norm_bound_between_knots_on_upload_and_after_clip(n):
    p = crossing_problem(n)
    problem = onp.SchroedingerProblem(p["T"], p["h"], p["psi0"], p["N"], control_eval_count=p["Nc"],
                                      costs=[onp.TargetStateInfidelity(p["target"])], control_count=2)
    err, fin = onp.evaluate(problem, p["controls"][0])
    ev = device.SchroedingerEvaluator(
        p["T"], p["h"], p["psi0"], p["N"], control_count=2, control_eval_count=p["Nc"],
        costs=[product_costs.TargetStateInfidelity(p["target"])])
    errors, _, finals, _ = ev.evaluate_batch(p["controls"], want_grad=False)
    assert abs(errors[0] - err) < 1e-10
    assert np.max(np.abs(finals[0] - fin)) < 1e-10
    # the resident driver's path: controls twice as large, clipped on the device to a
    backend = ev.backend
    backend.upload_controls(2 * p["controls"])
    backend.opt_begin()
    backend.opt_clip(np.full(2, p["a"]))
    backend.eval_resident(False)
    cost, _, final = backend.download_results(want_grad=False)
    assert abs(cost[0] - err) < 1e-10
    assert np.max(np.abs(final[0] - fin[:, :, 0])) < 1e-10


# ---- rejections ----------------------------------------------------------------------------------

def test_engine_rejects_bad_quadratic_terms():
    eng = engine_mod.Engine(0)
    n, K, N = 4, 2, 5
    rng = np.random.default_rng(1)
    h0, g = cases_mod.gue(rng, n), np.stack([cases_mod.gue(rng, n) for _ in range(K)])
    psi0 = np.eye(n, dtype=np.complex128)[:1]
    q = cases_mod.gue(rng, n)[None]
    try:
        eng.set_schroedinger_problem(n, 1, K, N, N, 1.0, h0[None], g[None], psi0,
                                     magnus_policy="M4")
        with pytest.raises(engine_mod.QocxError, match="M2"):
            eng.set_quadratic_terms([[0, 1]], q)
        eng.set_schroedinger_problem(n, 1, K, N, N, 1.0, h0[None], g[None], psi0)
        with pytest.raises(engine_mod.QocxError, match="<= 64"):
            eng.set_quadratic_terms([[0, 1]] * 63, np.repeat(q, 63, axis=0))
        with pytest.raises(engine_mod.QocxError, match="0 <= k <= l"):
            eng.set_quadratic_terms([[1, 0]], q)
        with pytest.raises(engine_mod.QocxError, match="0 <= k <= l"):
            eng.set_quadratic_terms([[0, 2]], q)
        eng.set_quadratic_terms([[0, 1]] * 62, np.repeat(q, 62, axis=0))  # K + 62 = 64: taken
        eng.set_quadratic_terms([], None)  # and cleared
    finally:
        eng.close()
