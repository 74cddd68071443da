"""
GPU tests (-m gpu) of the costs of the controls alone on the device (qocx_set_control_costs,
qoc_amd/csrc/qocx_ctrlcost.hip) and of complex controls in the resident multi-start drivers
(qocx_opt_begin_complex): the kernels against the four Python classes, batch invariance, the runs
that used to take the host loop, the collective and the bits of everything else.

Gates of the kernels against the classes (eps = 2^-52, T = number of terms a sum runs over): costs
to 4 T eps relative; gradients of ControlNorm / ControlArea to 8 eps of the largest entry, of
ControlVariation to 16 * 2^order * eps; ControlBandwidthMax cost to Nc eps and gradient to
(Nc + 8) eps. Bandwidth cases have at least two bins per control: with a single bin the cost is
identically 1 and the gradient of both sides is rounding noise around zero, which has no largest
entry to compare with.

Why Nc + 8 for the bandwidth gradient: Nc eps bounds a length-Nc dot product with twiddles good to
eps, but around its two dot products the formula rounds about eight more times per entry (modulus,
the sum and the maximum it is divided by, the weight and its correction at the maximum, weight times
bin, the quotient by the modulus through a reciprocal, the final scaling), which matters where Nc
itself is 2 or 3. Measured on the inputs of this file at Nc = 2, 3 (37 seeds): controls_bar() itself
- NumPy's FFT - is 1.5 to 3.1 eps of the largest entry away from a numpy.longdouble direct DFT of
the same formula, the twiddle-product formulation 1.4 to 3.2 eps, and the device 2.6 to 4.1 eps from
controls_bar(), against Nc eps = 2 or 3 eps. At Nc = 64 / 1001 the device is 5 / 21 eps from it.

ControlArea adds the knots in the order of numpy.sum(controls / max, axis=0) - knot by knot for
several controls, NumPy's pairwise scheme for one complex control, which is one contiguous column -
because the direction sum / |sum| of a complex control inherits the relative error of the sum: on
the inputs here a knot-by-knot sum is 84 eps from controls_bar() for one complex control at
Nc = 1001, and an exactly rounded sum 35 eps for four (NumPy's own error); in NumPy's order 2 eps.
"""

import numpy as np
import pytest

import qoc_amd
import qoc_amd.standard.costs as product_costs
from qoc_amd import engine as engine_mod
from qoc_amd.core import batch as batch_mod
from qoc_amd.core import structure
from qoc_amd.standard import Adam, QuadraticHamiltonian
from qoc_amd.standard.costs import (ControlArea, ControlBandwidthMax, ControlNorm,
                                    ControlVariation)
from tests import cases as cases_mod
from tests import gpu_helpers as gh
from tests import helpers
from tests.helpers import rel_err
from tests.test_gpu_ensemble import transmon_ensemble
from tests.test_gpu_quadratic_hamiltonian import shaped_problem
from tests.test_lindblad_host_api import product_cost_list

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
SCH, LIN = engine_mod.PATH_SCHROEDINGER, engine_mod.PATH_LINDBLAD


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


@pytest.fixture(scope="module")
def engine():
    eng = engine_mod.Engine(0)
    yield eng
    eng.close()


def tiny_problem(eng, kr, Nc, n=2, N=3, T=1.0):
    """A Schroedinger problem that only fixes the control layout (Nc knots, kr channels)."""
    rng = np.random.default_rng(kr + Nc)
    h0 = cases_mod.gue(rng, n)
    g = np.stack([cases_mod.gue(rng, n) for _ in range(kr)])
    target = dict(kind=engine_mod.COST_TARGET_COHERENT, step_cost=False, scale=1.0,
                  vectors=np.eye(n)[1:2])
    eng.set_schroedinger_problem(n, 1, kr, Nc, N, T, h0[None], g[None], np.eye(n)[:1],
                                 costs=[target])


def bandwidths(K, Nc, T):
    """max_bandwidths with at least two DFT bins at or above them for every control (all bins at
    Nc = 2, 3; at Nc = 3 the one positive bin alone would be a single-bin set)."""
    if Nc <= 3:
        return np.full(K, -1e9)
    freqs = np.fft.fftfreq(Nc, d=T / (Nc - 1))
    return np.array([freqs[Nc // 4 + k] - (1e-9 if k % 2 else 0.0) for k in range(K)])


def random_controls(rng, B, Nc, K, cplx, sigma=1.0):
    u = sigma * rng.standard_normal((B, Nc, K))
    return u + 1j * sigma * rng.standard_normal((B, Nc, K)) if cplx else u


def check_class(eng, cost, u, cplx, terms, grad_gate, cost_gate=None, label=""):
    """The kernels on the descriptor of `cost` against cost.cost() / controls_bar() for every seed
    of u (B x Nc x K); prints the figures, then asserts the gates."""
    B, Nc, K = u.shape
    desc = cost.control_descriptor(K, Nc, cplx)
    assert desc is not None
    eng.set_control_costs(SCH, cplx, [desc])
    value, grad = eng.eval_control_costs(SCH, structure.to_real_controls(u, cplx))
    only_value, none = eng.eval_control_costs(SCH, structure.to_real_controls(u, cplx), False)
    assert none is None and np.array_equal(only_value, value)
    dev_cost = dev_grad = 0.0
    for b in range(B):
        want = cost.cost(u[b], None, 0)
        want_grad = structure.to_real_controls(cost.controls_bar(u[b], None, 0), cplx)
        dev_cost = max(dev_cost, abs(value[b] - want) / abs(want))
        dev_grad = max(dev_grad, np.max(np.abs(grad[b] - want_grad)) / np.max(np.abs(want_grad)))
    cost_gate = 4 * terms * EPS if cost_gate is None else cost_gate
    print("{} {} B={} Nc={} K={} cplx={}: cost {:.2f} eps (gate {:.0f}), gradient {:.2f} eps "
          "(gate {:.0f})".format(type(cost).__name__, label, B, Nc, K, int(cplx), dev_cost / EPS,
                                 cost_gate / EPS, dev_grad / EPS, grad_gate / EPS))
    assert dev_cost <= cost_gate, (type(cost).__name__, label, dev_cost / EPS)
    assert dev_grad <= grad_gate, (type(cost).__name__, label, dev_grad / EPS)


# ---- 6. the kernels against the four classes -------------------------------------------------------

@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("K", [1, 4])
@pytest.mark.parametrize("Nc", [2, 3, 64, 1001])
@pytest.mark.parametrize("B", [1, 37])
def test_kernels_equal_the_python_classes(engine, B, Nc, K, cplx):
    T = 3.0
    tiny_problem(engine, K * (2 if cplx else 1), Nc, T=T)
    rng = np.random.default_rng(1000 * B + 10 * Nc + 2 * K + cplx)
    u = random_controls(rng, B, Nc, K, cplx)
    mx, w = rng.uniform(0.5, 2.0, K), rng.uniform(0.1, 2.0, K)
    channels = K * (2 if cplx else 1)
    check_class(engine, ControlNorm(K, Nc, control_weights=w, cost_multiplier=0.3,
                                    max_control_norms=mx), u, cplx, Nc * channels, 8 * EPS)
    check_class(engine, ControlNorm(K, Nc), u, cplx, Nc * channels, 8 * EPS, label="plain")
    check_class(engine, ControlArea(K, Nc, cost_multiplier=1.7, max_control_norms=mx), u, cplx,
                Nc * K, 8 * EPS)
    for order in (1, 2, 3):
        if order < Nc:
            check_class(engine, ControlVariation(K, Nc, cost_multiplier=0.9, max_control_norms=mx,
                                                 order=order),
                        u, cplx, (Nc - order) * channels, 16 * 2 ** order * EPS,
                        label="order {}".format(order))
    bandwidth = ControlBandwidthMax(K, Nc, T, bandwidths(K, Nc, T), cost_multiplier=1.3)
    assert all(len(b) >= 2 for b in bandwidth.control_descriptor(K, Nc, cplx)["bins"])
    check_class(engine, bandwidth, u, cplx, None, (Nc + 8) * EPS, cost_gate=Nc * EPS)


def test_zero_area_sum_and_tied_maximum(engine):
    Nc, K = 4, 2
    tiny_problem(engine, K, Nc)
    u = np.array([[[1.0, 0.3], [-1.0, 0.2], [0.5, -0.1], [-0.5, 0.4]]])
    area = ControlArea(K, Nc, max_control_norms=np.array([2.0, 1.0]))
    engine.set_control_costs(SCH, False, [area.control_descriptor(K, Nc, False)])
    value, grad = engine.eval_control_costs(SCH, u)
    assert np.all(grad[0, :, 0] == 0.0)
    assert np.max(np.abs(grad[0] - area.controls_bar(u[0], None, 0))) <= 8 * EPS * np.max(np.abs(grad))
    assert abs(value[0] - area.cost(u[0], None, 0)) <= 4 * Nc * K * EPS * value[0]
    # a pulse at the first knot: every bin has the same modulus, the first one is "the" maximum
    Nc = 8
    tiny_problem(engine, 1, Nc)
    u = np.zeros((1, Nc, 1))
    u[0, 0, 0] = 0.7
    bandwidth = ControlBandwidthMax(1, Nc, 1.0, [-1e9])
    engine.set_control_costs(SCH, False, [bandwidth.control_descriptor(1, Nc, False)])
    value, grad = engine.eval_control_costs(SCH, u)
    want = bandwidth.controls_bar(u[0], None, 0)
    assert abs(value[0] - 1.0) <= Nc * EPS
    assert np.max(np.abs(want)) > 0.1
    assert np.max(np.abs(grad[0] - want)) <= Nc * EPS * np.max(np.abs(want))


def all_costs(K, Nc, T, rng):
    mx, w = rng.uniform(0.5, 2.0, K), rng.uniform(0.1, 2.0, K)
    return [ControlVariation(K, Nc, cost_multiplier=0.9, max_control_norms=mx, order=2),
            ControlBandwidthMax(K, Nc, T, bandwidths(K, Nc, T), cost_multiplier=1.3),
            ControlNorm(K, Nc, control_weights=w, cost_multiplier=0.3, max_control_norms=mx),
            ControlArea(K, Nc, cost_multiplier=1.7, max_control_norms=mx),
            ControlBandwidthMax(K, Nc, T, np.full(K, -1e9), cost_multiplier=0.2)]


# ---- 7. batch invariance ---------------------------------------------------------------------------

@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("Nc, K", [(64, 1), (1001, 4), (4000, 2)])
def test_a_seed_does_not_depend_on_its_batch(engine, Nc, K, cplx):
    """(Nc = 4000: the twiddle table stays in HBM instead of LDS.)"""
    T = 2.0
    tiny_problem(engine, K * (2 if cplx else 1), Nc, T=T)
    rng = np.random.default_rng(7 + Nc + cplx)
    costs = all_costs(K, Nc, T, rng)
    engine.set_control_costs(SCH, cplx, [c.control_descriptor(K, Nc, cplx) for c in costs])
    u = structure.to_real_controls(random_controls(rng, 37, Nc, K, cplx), cplx)
    value, grad = engine.eval_control_costs(SCH, u)
    for b in (0, 7, 8, 36):
        one_value, one_grad = engine.eval_control_costs(SCH, u[b:b + 1])
        assert one_value[0] == value[b]
        assert np.array_equal(one_grad[0], grad[b])
    want = sum(c.cost(structure.from_real_gradients(u[5], cplx), None, 0) for c in costs)
    assert abs(value[5] - want) <= 1e-12 * abs(want)


# ---- 8. multi-start runs that took the host loop ----------------------------------------------------

class PluginAdam(Adam):  # not type(...) is Adam: takes the host loop
    pass


def both_routes(run, args, u0, routes, **kw):
    kw = dict(dict(iteration_count=5, log_iteration_step=0), **kw)
    a = run(*args, u0.copy(), optimizer=Adam(learning_rate=5e-2), **kw)
    assert routes == {"resident": 1, "host": 0}
    b = run(*args, u0.copy(), optimizer=PluginAdam(learning_rate=5e-2), **kw)
    assert routes == {"resident": 1, "host": 1}
    return a, b


def assert_equal_to_rounding(a, b, seeds):
    assert np.array_equal(a.best_iteration, b.best_iteration)
    assert np.array_equal(a.iterations_run, b.iterations_run)
    for s in range(seeds):
        print("seed {}: best_error {:.3e} apart, best_controls {:.3e} relative".format(
            s, abs(a.best_error[s] - b.best_error[s]), rel_err(a.best_controls[s], b.best_controls[s])))
    for s in range(seeds):
        assert abs(a.best_error[s] - b.best_error[s]) < 1e-12
        assert rel_err(a.best_controls[s], b.best_controls[s]) < 1e-10


def shaping_costs(K, Nc, T):
    freqs = np.fft.fftfreq(Nc, d=T / (Nc - 1))
    return [ControlVariation(K, Nc, cost_multiplier=0.4, order=2),
            ControlBandwidthMax(K, Nc, T, np.full(K, freqs[Nc // 3]), cost_multiplier=0.3)]


@pytest.mark.parametrize("kind", ["linear", "ensemble", "quadratic"])
def test_schroedinger_with_shaping_costs_runs_resident(kind, routes):
    n, N, Nc, B = 24, 31, 10, 4
    if kind == "ensemble":
        K, T = 3, 1.5
        hamiltonian, rng = transmon_ensemble(n, K, M=3, J=1, seed=5, complex_controls=False)
        psi0 = cases_mod.column_states(np.eye(n)[:, :2])
        target = cases_mod.column_states(cases_mod.random_unitary(rng, n)[:, :2])
        state_costs = [product_costs.TargetStateInfidelity(target)]
    else:
        p = shaped_problem(n, False, seed=5, N=N, Nc=Nc)
        K, T, psi0, state_costs = p["K"], p["T"], p["psi0"], p["costs"]
        hamiltonian = (QuadraticHamiltonian(p["linear"], p["terms"]) if kind == "quadratic"
                       else p["linear"])
    costs = state_costs + shaping_costs(K, Nc, T)
    u0 = np.clip(0.6 * np.random.default_rng(93).standard_normal((B, Nc, K)), -1, 1)
    args = (K, Nc, costs, T, hamiltonian, psi0, N)
    a, b = both_routes(qoc_amd.grape_schroedinger_discrete_batch, args, u0, routes,
                       max_control_norms=np.full(K, 1.0))
    assert_equal_to_rounding(a, b, B)
    for s in range(B):
        assert np.max(np.abs(a.best_final_states[s] - b.best_final_states[s])) < 1e-10
        if kind == "ensemble":
            assert np.max(np.abs(a.member_errors[s] - b.member_errors[s])) < 1e-10
    # the control costs are part of the errors, and gone from the engine after the run
    plain = qoc_amd.grape_schroedinger_discrete_batch(
        K, Nc, state_costs, T, hamiltonian, psi0, N, u0.copy(), optimizer=Adam(learning_rate=5e-2),
        iteration_count=1, log_iteration_step=0, max_control_norms=np.full(K, 1.0))
    first = qoc_amd.grape_schroedinger_discrete_batch(
        *args, u0.copy(), optimizer=Adam(learning_rate=5e-2), iteration_count=1,
        log_iteration_step=0, max_control_norms=np.full(K, 1.0))
    for s in range(B):
        shaping = sum(c.cost(u0[s], None, N - 1) for c in costs[len(state_costs):])
        assert shaping > 1e-3
        assert abs(first.best_error[s] - plain.best_error[s] - shaping) < 1e-12


def test_lindblad_with_norm_and_area_runs_resident(routes):
    case = cases_mod.lindblad_case_by_name("lindblad_wc_n16")
    mx = np.full(case.K, 1.0)
    costs = product_cost_list(case) + [
        ControlNorm(case.K, case.Nc, cost_multiplier=0.5, max_control_norms=mx),
        ControlArea(case.K, case.Nc, cost_multiplier=0.3, max_control_norms=mx)]
    args = (case.K, case.Nc, costs, case.T, case.initial_densities, case.N)
    kw = dict(cost_eval_step=case.cost_eval_step, hamiltonian=case.hamiltonian(),
              lindblad_data=case.lindblad_data(), max_control_norms=mx)
    u0 = np.clip(0.9 * np.random.default_rng(92).standard_normal((6, case.Nc, case.K)), -1, 1)
    a, b = both_routes(qoc_amd.grape_lindblad_discrete_batch, args, u0, routes,
                       **kw)
    assert_equal_to_rounding(a, b, 6)
    for s in range(6):
        assert np.max(np.abs(a.best_final_densities[s] - b.best_final_densities[s])) < 1e-10


def complex_problem(n=24, K=2, N=31, Nc=10, seed=3):
    rng = np.random.default_rng(700 + seed)
    h0 = cases_mod.gue(rng, n)
    g_re = [cases_mod.gue(rng, n) for _ in range(K)]
    g_im = [cases_mod.gue(rng, n) for _ in range(K)]

    def hamiltonian(u, t):
        out = h0
        for k in range(K):
            out = out + u[k].real * g_re[k] + u[k].imag * g_im[k]
        return out
    psi0 = cases_mod.column_states(np.eye(n)[:, :2])
    target = cases_mod.column_states(cases_mod.random_unitary(rng, n)[:, :2])
    return (K, Nc, [product_costs.TargetStateInfidelity(target)], 0.06 * (N - 1), hamiltonian,
            psi0, N), rng


def test_complex_controls_run_resident_bit_for_bit(routes):
    """No control cost and no entry ever at max_control_norms: the evaluation kernels and the
    optimizer arithmetic are the same on both routes."""
    args, rng = complex_problem()
    K, Nc, B = args[0], args[1], 4
    u0 = 0.3 * random_controls(rng, B, Nc, K, True)
    a, b = both_routes(qoc_amd.grape_schroedinger_discrete_batch, args, u0, routes,
                       complex_controls=True,
                       max_control_norms=np.full(K, 10.0))
    assert np.array_equal(a.best_error, b.best_error)
    assert np.array_equal(a.best_iteration, b.best_iteration)
    assert np.any(a.best_iteration > 0)
    for s in range(B):
        assert np.iscomplexobj(a.best_controls[s]) and a.best_controls[s].shape == (Nc, K)
        assert np.array_equal(a.best_controls[s], b.best_controls[s])
        assert np.array_equal(a.best_final_states[s], b.best_final_states[s])


@pytest.mark.parametrize("with_costs", [False, True])
def test_complex_controls_with_an_active_clip(with_costs, routes):
    args, rng = complex_problem(seed=4)
    K, Nc, B = args[0], args[1], 4
    mx = np.array([0.5, 0.8])
    if with_costs:
        args = args[:2] + (args[2] + shaping_costs(K, Nc, args[3]),) + args[3:]
    u0 = 0.25 * random_controls(rng, B, Nc, K, True)
    u0[np.abs(u0) > 0.45] *= 0.5
    # moduli next to the bound, many phases: Adam steps of 5e-2 take some of them beyond it. (The
    # phases advance by no multiple of 2 pi / Nc: a pure DFT harmonic would leave nothing but
    # rounding noise in the penalised bins, and the bandwidth cost - a ratio of those - undefined.)
    u0[0, :, 0] = 0.499 * np.exp(1.3j * np.arange(Nc) + 0.3j)
    u0[1, :, 1] = 0.799 * np.exp(-0.7j * np.arange(Nc) + 0.1j)
    a, b = both_routes(qoc_amd.grape_schroedinger_discrete_batch, args, u0, routes,
                       complex_controls=True, max_control_norms=mx)
    assert_equal_to_rounding(a, b, B)
    later = [s for s in (0, 1) if a.best_iteration[s] > 0]
    assert later  # (best controls that went through a clip ...)
    at_bound = sum(int(np.sum(np.abs(np.abs(a.best_controls[s]) - mx) <= 4 * EPS)) for s in later)
    assert at_bound > 0  # (... which acted)
    for s in range(B):
        assert np.all(np.abs(a.best_controls[s]) <= mx * (1 + 4 * EPS))


def test_lindblad_complex_controls_run_resident(routes):
    n, K, N, Nc = 4, 1, 9, 5
    rng = np.random.default_rng(12)
    h0, g_re, g_im = (cases_mod.gue(rng, n) for _ in range(3))
    lower = np.diag(np.sqrt(np.arange(1, n)), 1).astype(np.complex128)

    def hamiltonian(u, t):
        return h0 + u[0].real * g_re + u[0].imag * g_im
    rho0 = np.zeros((1, n, n), dtype=np.complex128)
    rho0[0, 0, 0] = 1.0
    target = np.zeros((1, n, n), dtype=np.complex128)
    target[0, 1, 1] = 1.0
    mx = np.array([0.6])
    costs = [product_costs.TargetDensityInfidelity(target),
             ControlNorm(K, Nc, cost_multiplier=0.2, max_control_norms=mx)]
    args = (K, Nc, costs, 1.0, rho0, N)
    u0 = 0.3 * random_controls(rng, 3, Nc, K, True)
    u0[0, :, 0] = 0.599 * np.exp(2j * np.pi * np.arange(Nc) / Nc)
    a, b = both_routes(qoc_amd.grape_lindblad_discrete_batch, args, u0, routes,
                       complex_controls=True, hamiltonian=hamiltonian,
                       lindblad_data=lambda t: (np.array([0.05]), lower[None]),
                       max_control_norms=mx)
    assert_equal_to_rounding(a, b, 3)
    for s in range(3):
        assert np.iscomplexobj(a.best_controls[s])
        assert np.all(np.abs(a.best_controls[s]) <= mx * (1 + 4 * EPS))


# ---- 9, 10. the collective; nothing else changes ----------------------------------------------------

def engine_problem(eng, ensemble):
    n, S, kr, Nc, N, T = 6, 2, 4, 8, 13, 1.2
    rng = np.random.default_rng(31)
    J = 1 if ensemble else 0
    h0 = cases_mod.gue(rng, n)
    g = np.stack([cases_mod.gue(rng, n) for _ in range(kr + J)])
    target = dict(kind=engine_mod.COST_TARGET_COHERENT, step_cost=False, scale=1.0,
                  vectors=cases_mod.random_unitary(rng, n)[:, :S].T)
    eng.set_schroedinger_problem(n, S, kr + J, Nc, N, T, h0[None], g[None], np.eye(n)[:S],
                                 costs=[target])
    if ensemble:
        eng.set_ensemble(1 + 0.1 * rng.standard_normal((3, kr)), 0.4 * rng.standard_normal((3, 1)),
                         np.array([0.5, 0.3, 0.2]))
    costs = all_costs(kr, Nc, T, rng)
    return [c.control_descriptor(kr, Nc, False) for c in costs], 0.5 * rng.standard_normal((5, Nc, kr))


@pytest.mark.parametrize("ensemble", [False, True])
def test_control_costs_are_one_addition_and_change_nothing_else(engine, ensemble):
    descs, u = engine_problem(engine, ensemble)
    engine.upload_controls(u)
    engine.eval_resident(True)
    cost0, grad0, final0 = engine.download_results()
    engine.set_control_costs(SCH, False, descs)
    extra_cost, extra_grad = engine.eval_control_costs(SCH, u)
    assert np.all(extra_cost > 1e-3)
    engine.eval_resident(True)
    cost1, grad1, final1 = engine.download_results()
    assert np.array_equal(final1, final0)
    assert np.array_equal(cost1, cost0 + extra_cost)
    assert np.array_equal(grad1, grad0 + extra_grad)
    assert np.array_equal(engine.download_costs(), cost1)
    # 9. the collective sums the totals
    total, total_grad = engine.reduce_results()
    assert abs(total - np.sum(cost1)) <= 8 * EPS * np.sum(np.abs(cost1))
    assert np.max(np.abs(total_grad - np.sum(grad1, axis=0))) <= 8 * EPS * np.max(
        np.sum(np.abs(grad1), axis=0))
    assert abs(total - np.sum(cost0)) > 1e-3
    engine.eval_resident(False)  # without gradients: the same totals
    assert np.array_equal(engine.download_results(want_grad=False)[0], cost1)
    # cleared again: the bits of before
    engine.set_control_costs(SCH, False, [])
    engine.eval_resident(True)
    for x, y in zip(engine.download_results(), (cost0, grad0, final0)):
        assert np.array_equal(x, y)


def test_host_buffer_entry_points_ignore_the_control_costs(engine):
    descs, u = engine_problem(engine, False)
    lib, ctx = engine._lib, engine._ctx
    import ctypes
    dp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))  # noqa: E731
    out = []
    for with_costs in (False, True):
        engine.set_control_costs(SCH, False, descs if with_costs else [])
        cost, grad = np.empty(5), np.empty(u.shape)
        assert lib.qocx_eval_schroedinger(ctx, 5, dp(u), 1, dp(cost), dp(grad), None) == 0
        out.append((cost, grad))
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])
    engine.set_control_costs(SCH, False, [])


def test_lindblad_control_costs_are_one_addition_and_change_nothing_else(engine):
    case = cases_mod.lindblad_case_by_name("lindblad_n4")
    gh.setup_lindblad_engine(engine, case)
    kr = len(gh.lindblad_generators(case))
    rng = np.random.default_rng(5)
    u = 0.4 * rng.standard_normal((3, case.Nc, kr))
    mx = np.full(kr, 1.5)
    descs = [ControlNorm(kr, case.Nc, cost_multiplier=0.5, max_control_norms=mx).control_descriptor(
        kr, case.Nc, False), ControlArea(kr, case.Nc, max_control_norms=mx).control_descriptor(
        kr, case.Nc, False)]
    engine.lindblad_upload_controls(u)
    engine.eval_lindblad_resident(True)
    cost0, grad0, final0 = engine.lindblad_download_results()
    engine.set_control_costs(LIN, False, descs)
    extra_cost, extra_grad = engine.eval_control_costs(LIN, u)
    engine.eval_lindblad_resident(True)
    cost1, grad1, final1 = engine.lindblad_download_results()
    assert np.array_equal(final1, final0)
    assert np.array_equal(cost1, cost0 + extra_cost) and np.all(extra_cost > 1e-3)
    assert np.array_equal(grad1, grad0 + extra_grad)
    assert np.array_equal(engine.evaluate_lindblad(u)[0], cost0)  # (host buffers: without them)
    engine.set_control_costs(LIN, False, [])
    engine.eval_lindblad_resident(True)
    for x, y in zip(engine.lindblad_download_results(), (cost0, grad0, final0)):
        assert np.array_equal(x, y)


def test_engine_rejects_bad_control_costs(engine):
    Nc, K = 6, 2
    tiny_problem(engine, K, Nc)
    ok = dict(kind=engine_mod.CONTROL_NORM, multiplier=1.0)
    bad = [dict(kind=9, multiplier=1.0),
           dict(kind=engine_mod.CONTROL_VARIATION, multiplier=1.0, order=0),
           dict(kind=engine_mod.CONTROL_VARIATION, multiplier=1.0, order=Nc),
           dict(kind=engine_mod.CONTROL_AREA, multiplier=1.0),
           dict(kind=engine_mod.CONTROL_NORM, multiplier=np.inf),
           dict(kind=engine_mod.CONTROL_NORM, multiplier=1.0, max_norms=[1.0, np.nan]),
           dict(kind=engine_mod.CONTROL_BANDWIDTH_MAX, multiplier=1.0, bins=[[1, 2], []]),
           dict(kind=engine_mod.CONTROL_BANDWIDTH_MAX, multiplier=1.0, bins=[[1, 2], [Nc]]),
           dict(kind=engine_mod.CONTROL_BANDWIDTH_MAX, multiplier=1.0, bins=[[2, 1], [0]])]
    for desc in bad:
        with pytest.raises(engine_mod.QocxError) as err:
            engine.set_control_costs(SCH, False, [ok, desc])
        assert err.value.code == -1, desc
    with pytest.raises(engine_mod.QocxError):  # nothing set after a rejection
        engine.eval_control_costs(SCH, np.zeros((1, Nc, K)))
    tiny_problem(engine, 3, Nc)
    with pytest.raises(engine_mod.QocxError) as err:  # complex controls need channel pairs
        engine.set_control_costs(SCH, True, [ok])
    assert err.value.code == -1
    engine.set_schroedinger_problem(2, 1, 0, 0, 3, 1.0, np.eye(2)[None], None, np.eye(2)[:1],
                                    costs=[dict(kind=0, step_cost=False, scale=1.0,
                                                vectors=np.eye(2)[1:2])])
    with pytest.raises(engine_mod.QocxError) as err:  # a problem without controls
        engine.set_control_costs(SCH, False, [ok])
    assert err.value.code == -1
