"""
GPU tests (-m gpu) of Hamiltonian sweeps on the device (qoc_amd.standard.HamiltonianSweep ->
qocx_set_sweep): seed b is item b, the plain (K_r + J)-channel problem on the controls
[s_b * u_b, delta_b] - bit for bit -, its gradient comes back as s_bk * g_item, and the
sensitivities are the sums of qocx_sweep.hip in their documented order.
"""

import numpy as np
import pytest

import qoc_amd
import qoc_amd.standard.costs as product_costs
from oracle import qoc_numpy as onp
from qoc_amd import engine as engine_mod
from qoc_amd.core import batch as batch_mod
from qoc_amd.core import device
from qoc_amd.models import InterpolationPolicy, MagnusPolicy
from qoc_amd.standard import LBFGS, SGD, Adam, ControlBasis, ControlVariation, HamiltonianSweep
from tests import cases as cases_mod
from tests import helpers
from tests import piecewise_constant as pc
from tests.helpers import rel_err

pytestmark = pytest.mark.gpu

LANES = 64  # QOCX_SWEEP_LANES: the partial sums of one sensitivity (qocx_sweep.hip)
ERR_STATE = -3  # QOCX_ERR_STATE (include/qocx.h)


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


# ---- 1. the engine: every seed against the plain expanded problem, bit for bit ---------------------

def engine_problem(n, magnus="M2", time_dependent=False, S=1, kr=3, J=2, B=3, N=21, Nc=8,
                   interpolation="linear", seed=0):
    rng = np.random.default_rng(700 + n + 7 * seed)
    nodes = {"M2": 1, "M4": 2, "M6": 3}[magnus]
    nt = (N - 1) * nodes if time_dependent else 1
    h0 = cases_mod.gue(rng, n)
    gs = np.stack([cases_mod.gue(rng, n) for _ in range(kr)])
    d = np.stack([0.5 * cases_mod.gue(rng, n) for _ in range(J)]) if J else np.zeros((0, n, n))
    wobble = 1 + 0.2 * np.sin(np.linspace(0, 3, nt)) if time_dependent else np.ones(1)
    h0_t = wobble[:, None, None] * h0[None]
    g_t = np.concatenate([np.repeat(gs[None], nt, axis=0), np.repeat(d[None], nt, axis=0)], axis=1)
    psi0 = np.eye(n, dtype=np.complex128)[:S]
    target = cases_mod.column_states(cases_mod.random_unitary(rng, n)[:, :S])
    descs = [product_costs.TargetStateInfidelity(target).device_descriptor(S, n)]
    # seeds with loud and quiet systems: scales from 0.5 to 1.4, so that the seeds of one call
    # differ in their Pade orders and squarings
    scales = np.linspace(0.5, 1.4, B)[:, None] * (1 + 0.05 * rng.standard_normal((B, kr)))
    offsets = 0.4 * rng.standard_normal((B, J)) if J else None
    u = 0.6 * rng.standard_normal((B, Nc, kr))
    return dict(n=n, S=S, K=kr + J, kr=kr, J=J, B=B, N=N, Nc=Nc, T=0.05 * (N - 1), h0=h0_t,
                g=g_t, psi0=psi0, descs=descs, magnus=magnus, scales=scales, offsets=offsets, u=u,
                interpolation=interpolation)


def expand(p):
    items = np.empty((p["B"], p["Nc"], p["K"]))
    items[..., :p["kr"]] = p["scales"][:, None, :] * p["u"]
    if p["J"]:
        items[..., p["kr"]:] = p["offsets"][:, None, :]
    return items


def make_engine(p):
    eng = engine_mod.Engine(0)
    eng.set_schroedinger_problem(p["n"], p["S"], p["K"], p["Nc"], p["N"], p["T"], p["h0"], p["g"],
                                 p["psi0"], costs=p["descs"], magnus_policy=p["magnus"],
                                 interpolation=p["interpolation"])
    return eng


def ordered_sum(terms):
    """The summation order of qocx_sweep.hip over the knots (axis 0): LANES partial sums over the
    knots l, l + LANES, ... ascending from +0.0, then the halving tree."""
    terms = np.asarray(terms, dtype=np.float64)
    partial = np.zeros((LANES,) + terms.shape[1:])
    for j in range(terms.shape[0]):
        partial[j % LANES] = partial[j % LANES] + terms[j]
    half = LANES // 2
    while half >= 1:
        partial = partial[:half] + partial[half:2 * half]
        half //= 2
    return partial[0]


ENGINE_CASES = {
    # the matrix kernels: n <= 16, <= 32, <= 64 and the general path; M4 / M6 at two sizes
    "n3": dict(n=3), "n16": dict(n=16), "n24": dict(n=24), "n40": dict(n=40),
    "n80_general": dict(n=80, N=6, Nc=6, B=2),
    "n3_M4": dict(n=3, magnus="M4"), "n24_M4": dict(n=24, magnus="M4"),
    "n3_M6": dict(n=3, magnus="M6"), "n24_M6": dict(n=24, magnus="M6"),
    # the shapes at which the three sweep kernels can go wrong
    "one_seed": dict(n=3, B=1),
    "scales_only_315_elements": dict(n=3, B=5, Nc=9, kr=7, J=0),  # crosses a 256-thread block
    "offsets_only_fewest_knots": dict(n=3, kr=1, J=3, Nc=2),
    "one_knot_past_the_lanes": dict(n=3, Nc=LANES + 1, N=LANES + 1),
    "complex_pairs": dict(n=16, kr=4, J=1),   # K_r = 2 K: Re / Im channels share a scale
    "time_dependent_base": dict(n=3, time_dependent=True),
    "piecewise_constant": dict(n=16, N=8, Nc=3, interpolation="piecewise_constant"),
}


@pytest.mark.parametrize("name", sorted(ENGINE_CASES))
def test_a_seed_is_the_plain_expanded_problem_bit_for_bit(name):
    p = engine_problem(**ENGINE_CASES[name])
    if name == "complex_pairs":
        p["scales"] = np.repeat(p["scales"][:, :2], 2, axis=1)
    swp, plain = make_engine(p), make_engine(p)
    try:
        swp.set_sweep(p["scales"], p["offsets"])
        swp.upload_controls(p["u"])
        swp.eval_resident(True)
        cost, grads, final = swp.download_results()
        scale_sens, offset_sens = swp.sweep_sensitivities()
        orders = swp.pade_orders()
        plain.upload_controls(expand(p))
        plain.eval_resident(True)
        pcost, pgrads, pfinal = plain.download_results()
        porders = plain.pade_orders()
    finally:
        swp.close()
        plain.close()
    B, kr, Nc = p["B"], p["kr"], p["Nc"]
    assert grads.shape == (B, Nc, kr) and final.shape == (B, p["S"], p["n"])
    assert scale_sens.shape == (B, kr) and offset_sens.shape == (B, p["J"])
    assert orders == porders
    assert np.array_equal(cost, pcost)
    assert np.array_equal(final, pfinal)
    assert np.array_equal(grads, p["scales"][:, None, :] * pgrads[..., :kr])
    assert np.any(pgrads != 0.0)
    for b in range(B):
        assert np.array_equal(scale_sens[b], ordered_sum(p["u"][b] * pgrads[b, :, :kr]))
        assert np.array_equal(offset_sens[b], ordered_sum(pgrads[b, :, kr:]))


def test_degenerate_sweep_is_the_plain_batch():
    p = engine_problem(24, J=0, B=3)
    swp, plain = make_engine(p), make_engine(p)
    try:
        swp.set_sweep(np.ones((3, p["kr"])), None)
        c1, g1, f1 = swp.evaluate(p["u"])
        c0, g0, f0 = plain.evaluate(p["u"])
    finally:
        swp.close()
        plain.close()
    assert np.array_equal(c1, c0) and np.array_equal(g1, g0) and np.array_equal(f1, f0)


def test_reduce_results_and_the_resident_clip_act_on_the_seeds():
    p = engine_problem(24, B=3)
    eng = make_engine(p)
    try:
        eng.set_sweep(p["scales"], p["offsets"])
        eng.upload_controls(p["u"])
        eng.eval_resident(True)
        cost, grads, _ = eng.download_results()
        total, total_g = eng.reduce_results()
        assert abs(total - np.sum(cost)) <= 1e-14 * abs(total)
        assert rel_err(total_g, np.sum(grads, axis=0)) < 1e-14
        # clip on the device: the next evaluation expands the clipped seed controls, and the
        # sensitivities wait for it
        eng.opt_begin()
        eng.opt_clip(np.full(p["kr"], 0.3))
        with pytest.raises(engine_mod.QocxError, match="evaluation with gradients"):
            eng.sweep_sensitivities()
        eng.eval_resident(True)
        costs = eng.download_costs()
        s1, o1 = eng.sweep_sensitivities()
        c2, g2, f2 = eng.evaluate(np.clip(p["u"], -0.3, 0.3))
        s2, o2 = eng.sweep_sensitivities()
    finally:
        eng.close()
    assert np.array_equal(costs, c2) and np.array_equal(s1, s2) and np.array_equal(o1, o2)


# ---- 2. a duration sweep against the oracle ----------------------------------------------------------

def test_a_duration_sweep_of_c2_transmon_against_the_oracle_at_every_duration():
    case = cases_mod.case_c2_transmon()
    ref, B = case.T, 4
    times = ref * np.array([0.5, 0.8, 1.0, 1.3])
    h = case.hamiltonian()
    w = HamiltonianSweep.durations(h, times, ref)
    target = case.cost_specs[0][1]["target_states"]
    ev = device.SchroedingerEvaluator(
        ref, w, case.initial_states, case.N, control_count=case.K, control_eval_count=case.Nc,
        costs=[product_costs.TargetStateInfidelity(target)])
    rng = np.random.default_rng(77)
    u = np.stack([case.controls[0]] + [0.1 * rng.standard_normal((case.Nc, case.K))
                                       for _ in range(B - 1)])
    errors, grads, finals, _ = ev.evaluate_batch(u)
    sens = ev.sweep_sensitivities()
    # the expanded problem of the oracle: channels [G_0, G_1, H0] on [tau u, tau] over [0, ref]
    h0 = np.asarray(h(np.zeros(case.K), 0.0))

    def expanded(r, t):
        return (h(r[:case.K], t) - h0) + r[case.K] * h0

    for b in range(B):
        problem = onp.SchroedingerProblem(
            times[b], h, case.initial_states, case.N, control_eval_count=case.Nc,
            costs=[onp.TargetStateInfidelity(target)], control_count=case.K)
        err, gr, fin = onp.evaluate_with_grad(problem, u[b])
        assert abs(errors[b] - err) < 1e-10
        assert np.max(np.abs(finals[b] - fin)) < 1e-10
        assert rel_err(grads[b], np.real(gr)) < 1e-8
        tau = times[b] / ref
        wide = onp.SchroedingerProblem(
            ref, expanded, case.initial_states, case.N, control_eval_count=case.Nc,
            costs=[onp.TargetStateInfidelity(target)], control_count=case.K + 1)
        r = np.concatenate([tau * u[b], np.full((case.Nc, 1), tau)], axis=1)
        _, g_wide, _ = onp.evaluate_with_grad(wide, r)
        g_wide = np.real(g_wide)
        want_s = np.sum(u[b] * g_wide[:, :case.K], axis=0)
        want_d = np.sum(g_wide[:, case.K:], axis=0)
        assert rel_err(sens["control_scales"][b], want_s) < 1e-8
        assert rel_err(sens["offsets"][b], want_d) < 1e-8
        want_t = (np.sum(want_s) + want_d[0]) / ref
        assert abs(sens["evolution_time_gradients"][b] - want_t) < 1e-8 * max(
            abs(want_t), np.max(np.abs(want_s)) / ref)


# ---- 3. multi-start GRAPE: the routes ----------------------------------------------------------------

class HostAdam(Adam):  # not type(...) is Adam: takes the host loop
    pass


class HostSGD(SGD):
    pass


class HostLBFGS(LBFGS):
    pass


OPTIMIZERS = {
    "adam": (lambda: Adam(learning_rate=5e-2), lambda: HostAdam(learning_rate=5e-2)),
    "sgd": (lambda: SGD(learning_rate=0.5), lambda: HostSGD(learning_rate=0.5)),
    "lbfgs": (LBFGS, HostLBFGS),
}


def route_problem(complex_controls=False, n=16, K=2, N=21, Nc=10, S=2, B=3, T=1.2):
    rng = np.random.default_rng(1100 + n + int(complex_controls))
    h0 = cases_mod.gue(rng, n)
    g_re = [cases_mod.gue(rng, n) for _ in range(K)]
    g_im = [cases_mod.gue(rng, n) for _ in range(K)]

    def linear(u, t):
        out = h0
        for k in range(K):
            out = out + (u[k].real * g_re[k] + u[k].imag * g_im[k] if complex_controls
                         else u[k] * g_re[k])
        return out
    w = HamiltonianSweep.durations(
        linear, T * np.array([0.6, 1.0, 1.4]), T,
        control_scales=1 + 0.05 * rng.standard_normal((B, K)),
        perturbations=0.3 * cases_mod.gue(rng, n)[None], offsets=0.5 * rng.standard_normal((B, 1)))
    psi0 = cases_mod.column_states(np.eye(n)[:, :S])
    target = cases_mod.column_states(cases_mod.random_unitary(rng, n)[:, :S])
    return w, (K, Nc, [product_costs.TargetStateInfidelity(target)], T), (psi0, N), rng


def run_routes(routes, optimizer, w, head, tail, start, single=True, **kw):
    """The resident route, the host loop and (single) B single-seed runs on member(b)."""
    resident, host = OPTIMIZERS[optimizer]
    kw = dict(dict(iteration_count=5, log_iteration_step=0), **kw)
    a = qoc_amd.grape_schroedinger_discrete_batch(*head, w, *tail, start.copy(),
                                                  optimizer=resident(), **kw)
    assert routes == {"resident": 1, "host": 0}
    b = qoc_amd.grape_schroedinger_discrete_batch(*head, w, *tail, start.copy(), optimizer=host(),
                                                  **kw)
    assert routes == {"resident": 1, "host": 1}
    B = start.shape[0]
    for s in range(B if single else 0):
        one = qoc_amd.grape_schroedinger_discrete(*head, w.member(s), *tail,
                                                  initial_controls=start[s].copy(),
                                                  optimizer=resident(), **kw)
        assert one.best_iteration == a.best_iteration[s]
        assert abs(one.best_error - a.best_error[s]) < 1e-12
        assert rel_err(a.best_controls[s], one.best_controls) < 1e-10
        assert abs(one.best_error - b.best_error[s]) < 1e-12
        assert rel_err(b.best_controls[s], one.best_controls) < 1e-10
    return a, b


def assert_bit_identical(a, b):
    assert np.array_equal(a.best_error, b.best_error)
    assert np.array_equal(a.best_iteration, b.best_iteration)
    assert np.array_equal(a.iterations_run, b.iterations_run)
    for s in range(len(a.best_error)):
        assert np.array_equal(a.best_controls[s], b.best_controls[s])
        assert np.array_equal(a.best_final_states[s], b.best_final_states[s])
    for key in ("control_scales", "offsets", "evolution_time_gradients"):
        assert np.array_equal(a.sweep_sensitivities[key], b.sweep_sensitivities[key])


@pytest.mark.parametrize("optimizer", ["adam", "sgd", "lbfgs"])
def test_resident_route_equals_host_loop_and_single_seed_runs(routes, optimizer):
    w, head, tail, rng = route_problem()
    K, Nc = head[0], head[1]
    u0 = np.clip(0.6 * rng.standard_normal((3, Nc, K)), -1, 1)
    a, b = run_routes(routes, optimizer, w, head, tail, u0, max_control_norms=np.full(K, 1.0))
    assert_bit_identical(a, b)
    assert np.any(a.best_iteration > 0)
    assert a.sweep_sensitivities["control_scales"].shape == (3, K)
    assert a.sweep_sensitivities["offsets"].shape == (3, 2)  # the drift D_0 and the perturbation
    assert np.all(np.isfinite(a.sweep_sensitivities["evolution_time_gradients"]))


@pytest.mark.parametrize("optimizer", ["adam", "sgd", "lbfgs"])
def test_resident_route_with_a_sine_basis(routes, optimizer):
    w, head, tail, rng = route_problem()
    K, Nc = head[0], head[1]
    basis = ControlBasis.sine(Nc, 4)
    c0 = 0.3 * rng.standard_normal((3, 4, K))
    for s in range(3):
        c0[s] *= min(1.0, 0.9 / np.max(np.abs(basis.expand(c0[s]))))
    a, b = run_routes(routes, optimizer, w, head, tail, c0, control_basis=basis,
                      max_control_norms=np.full(K, 1.0))
    assert_bit_identical(a, b)
    for s in range(3):
        assert np.array_equal(a.best_coefficients[s], b.best_coefficients[s])


@pytest.mark.parametrize("optimizer", ["adam", "sgd", "lbfgs"])
def test_resident_route_with_control_variation(routes, optimizer):
    w, head, tail, rng = route_problem()
    K, Nc, costs, T = head
    head = (K, Nc, costs + [ControlVariation(K, Nc, cost_multiplier=0.4, order=1)], T)
    u0 = np.clip(0.6 * rng.standard_normal((3, Nc, K)), -1, 1)
    a, b = run_routes(routes, optimizer, w, head, tail, u0, max_control_norms=np.full(K, 1.0))
    for s in range(3):
        print("seed {}: best_error {:.3e} apart, best_controls {:.3e} relative".format(
            s, abs(a.best_error[s] - b.best_error[s]), rel_err(a.best_controls[s], b.best_controls[s])))
    assert_bit_identical(a, b)


def test_resident_route_with_complex_controls(routes):
    w, head, tail, rng = route_problem(complex_controls=True)
    K, Nc = head[0], head[1]
    u0 = 0.3 * (rng.standard_normal((3, Nc, K)) + 1j * rng.standard_normal((3, Nc, K)))
    a, b = run_routes(routes, "adam", w, head, tail, u0, complex_controls=True,
                      max_control_norms=np.full(K, 2.0))
    # Equal to rounding, not bit for bit: the resident route sizes the squarings by the clip bound
    # (every channel at max_control_norms, twice per complex control), the host loop by the
    # uploaded pulse, and at this shape the PLAIN problem on member(1) already parts by 1e-15 in
    # its final states between the two routes with identical controls. The gates are those of the
    # comparison with the single-seed runs.
    assert np.array_equal(a.best_iteration, b.best_iteration)
    for s in range(3):
        assert abs(a.best_error[s] - b.best_error[s]) < 1e-12
        assert rel_err(a.best_controls[s], b.best_controls[s]) < 1e-10
        assert np.max(np.abs(a.best_final_states[s] - b.best_final_states[s])) < 1e-10
    for key in ("control_scales", "offsets", "evolution_time_gradients"):
        assert rel_err(a.sweep_sensitivities[key], b.sweep_sensitivities[key]) < 1e-8
    assert all(np.iscomplexobj(c) for c in a.best_controls)
    assert a.sweep_sensitivities["control_scales"].shape == (3, K)


def test_piecewise_constant_and_m4_through_the_evaluator():
    """The evaluator's own path (probe, appended channels, set_sweep) under M4 and under
    PIECEWISE_CONSTANT: seed b against the oracle on member(b) (piecewise constant: against the
    oracle on the control-free closure of the pulse, its gradient by central differences at that
    reference's own gate of 1e-7)."""
    w, head, tail, rng = route_problem(n=6, N=9, Nc=4)
    (K, Nc, _, T), (psi0, N) = head, tail
    target = cases_mod.column_states(cases_mod.random_unitary(rng, 6)[:, :2])
    u = 0.5 * rng.standard_normal((3, Nc, K))
    ocosts = [onp.TargetStateInfidelity(target)]
    for magnus, policy in ((MagnusPolicy.M4, InterpolationPolicy.LINEAR),
                           (MagnusPolicy.M2, InterpolationPolicy.PIECEWISE_CONSTANT)):
        ev = device.SchroedingerEvaluator(
            T, w, psi0, N, control_count=K, control_eval_count=Nc, magnus_policy=magnus,
            interpolation_policy=policy, costs=[product_costs.TargetStateInfidelity(target)])
        errors, grads, finals, _ = ev.evaluate_batch(u)
        for b in range(3):
            if policy == InterpolationPolicy.LINEAR:
                problem = onp.SchroedingerProblem(
                    T, w.member(b), psi0, N, control_eval_count=Nc, costs=ocosts,
                    magnus_policy=magnus.short, control_count=K)
                err, gr, fin = onp.evaluate_with_grad(problem, u[b])
                gate = 1e-8
            else:
                err, fin = pc.reference_a(w.member(b), u[b], T, psi0, N, ocosts)
                gr = pc.reference_a_gradient(w.member(b), u[b], T, psi0, N, ocosts)
                gate = 1e-7
            assert abs(errors[b] - err) < 1e-10
            assert np.max(np.abs(finals[b] - fin)) < 1e-10
            assert rel_err(grads[b], np.real(gr)) < gate


# ---- 5. refusals of the ABI ----------------------------------------------------------------------------

def test_engine_refusals():
    p = engine_problem(3, B=3)
    eng = make_engine(p)
    try:
        with pytest.raises(engine_mod.QocxError, match="no sweep set"):
            eng._sweep = dict(B=3, J=p["J"], Kr=p["kr"])
            eng.sweep_sensitivities()
        eng.set_sweep(p["scales"], p["offsets"])
        with pytest.raises(engine_mod.QocxError, match="exactly its own seed count"):
            eng.upload_controls(p["u"][:2])
        with pytest.raises(engine_mod.QocxError, match="exactly its own seed count"):
            eng.upload_controls(np.concatenate([p["u"], p["u"]]))
        with pytest.raises(engine_mod.QocxError, match="a sweep or an ensemble") as info:
            eng.set_ensemble(None, None, np.ones(2))
        assert info.value.code == ERR_STATE
        with pytest.raises(engine_mod.QocxError, match="quadratic terms") as info:
            eng.set_quadratic_terms([[0, 0]], np.eye(3)[None])
        assert info.value.code == ERR_STATE
        bad = p["scales"].copy()
        bad[1, 0] = np.inf
        with pytest.raises(engine_mod.QocxError, match="non-finite sweep control scale"):
            eng.set_sweep(bad, p["offsets"])
        bad = p["offsets"].copy()
        bad[2, 1] = np.nan
        with pytest.raises(engine_mod.QocxError, match="non-finite sweep offset"):
            eng.set_sweep(p["scales"], bad)
        with pytest.raises(engine_mod.QocxError, match="fixed < control_count"):
            eng.set_sweep(None, np.zeros((3, p["K"])))  # no channel is left for the seeds
        # the sweep set before the refused calls still stands; no gradients, no sensitivities
        eng.upload_controls(p["u"])
        eng.eval_resident(False)
        with pytest.raises(engine_mod.QocxError, match="evaluation with gradients"):
            eng.sweep_sensitivities()
        with pytest.raises(engine_mod.QocxError, match="no ensemble set"):
            eng._ensemble = dict(M=1, J=p["J"], Kr=p["kr"])
            eng.ensemble_member_costs()
        eng._ensemble = None
        # a new problem clears the sweep; an ensemble then bars the sweep
        eng.set_schroedinger_problem(p["n"], p["S"], p["K"], p["Nc"], p["N"], p["T"], p["h0"],
                                     p["g"], p["psi0"], costs=p["descs"])
        eng.upload_controls(expand(p))
        eng.set_ensemble(None, None, np.ones(2))
        with pytest.raises(engine_mod.QocxError, match="a sweep or an ensemble") as info:
            eng.set_sweep(p["scales"], p["offsets"])
        assert info.value.code == ERR_STATE
    finally:
        eng.close()
