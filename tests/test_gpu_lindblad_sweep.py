"""
GPU tests (-m gpu) of LindbladSweep (qocx_lindblad_set_sweep, qocx_lindblad_ratesens.hip): B open
systems, each with a pulse, scales, offsets and dissipation rates of its own.

1. a seed is, bit for bit, the plain (K_r + J)-channel problem set with dissipators = c_b * gamma on
   host-expanded controls - cost, gradient (after the one product with s_bk), final densities and
   sub-division counts -, through qocx_eval_lindblad and the resident calls; with seeds in several
   sub-division groups (a launch order that is a real permutation); without rate_scales on the
   plain kernels, a time-dependent drive included;
2. degenerate sweeps: all 1 is the plain batch, swapped rows swap the seeds;
3. rate sensitivities against the NumPy model (tests/lindblad_sweep_model.py) at the gate of the
   control gradient (tests/helpers.py, lindblad_grad_close), in several pieces, and None - never
   garbage - where a piece did not run two-sided; channel sensitivities in the summation order of
   qocx_sweep.hip, bit for bit;
4. T1 decay per seed of a duration sweep, and dE_b/dT_b against the analytic value;
5. the resident route against the host loop and the single-seed runs on member(b);
6. the engine's rejections and what clears the sweep.

Shapes: N = 7 system steps and Nc = 4 (N = 4, Nc = 3 above one tile), B = 3 seeds.
"""

import ctypes

import numpy as np
import pytest

import qoc_amd
from oracle import qoc_lindblad_numpy as ol
from qoc_amd.core import device
from qoc_amd.engine import Engine, QocxError
from qoc_amd.standard import (LBFGS, Adam, ControlBasis, ControlVariation, LindbladSweep,
                              TargetDensityInfidelity)
from tests import cases as cases_mod
from tests import gpu_helpers as gh
from tests import helpers
from tests import lindblad_model as lm
from tests import lindblad_sweep_model as sm
from tests.test_gpu_lindblad_ensemble import routes  # noqa: F401 (fixture)
from tests.test_gpu_lindblad_rate_ensemble import shape_case
from tests.test_gpu_sweep import ordered_sum
from tests.test_lindblad_host_api import product_cost_list

pytestmark = pytest.mark.gpu

B = 3
ERR_ARG, ERR_STATE = -1, -3
_DP = ctypes.POINTER(ctypes.c_double)


@pytest.fixture(autouse=True)
def real_engine():
    helpers.set_backend_factory(None)
    yield
    helpers.set_backend_factory(None)


@pytest.fixture(scope="module")
def engine():
    e = Engine(0)
    yield e
    e.close()


class RecordingEngine(Engine):
    """The engine, remembering the arguments of the last set_lindblad_problem and set_lindblad_sweep."""

    def set_lindblad_problem(self, *a, interpolation="linear", **kw):
        self.last_problem = (a, dict(kw, interpolation=interpolation))
        Engine.set_lindblad_problem(self, *a, interpolation=interpolation, **kw)

    def set_lindblad_sweep(self, *a):
        self.last_sweep = a
        Engine.set_lindblad_sweep(self, *a)


def sized_case(n, L, ops="real", S=1):
    case = shape_case(n, L, ops, N=4 if n > 16 else 7, Nc=3 if n > 16 else 4)
    if S > 1:  # more densities under the one final TargetDensityInfidelity
        rng = np.random.default_rng(7000 + n)
        case.initial_densities = np.stack([cases_mod.random_density(rng, n) for _ in range(S)])
        targ = np.stack([cases_mod.random_density(rng, n) for _ in range(S)])
        case.cost_specs = [("TargetDensityInfidelity", dict(target_densities=targ))]
    return case


def sweep_for(case, seed, J=1, seeds=B, rates="distinct"):
    """Distinct scales, J fixed channels and rate factors from {0.5, 1, 2} (or none)."""
    rng = np.random.default_rng(seed)
    L = len(case.dissipators)
    d = np.stack([0.5 * cases_mod.gue(rng, case.n) for _ in range(J)]) if J else None
    c = None
    if rates == "distinct":
        c = np.array([[0.5, 1.0, 2.0][(b + l) % 3] for b in range(seeds) for l in range(L)],
                     dtype=np.float64).reshape(seeds, L)
    return LindbladSweep(case.hamiltonian(), perturbations=d,
                         offsets=0.3 * rng.standard_normal((seeds, J)) if J else None,
                         control_scales=1 + 0.05 * rng.standard_normal((seeds, case.K)),
                         rate_scales=c)


def expand(w, u):
    """Seeds (B, Nc, K_r) -> items (B, Nc, K_r + J): one product, one rounding."""
    kr, J = u.shape[2], w.perturbation_count
    items = np.empty(u.shape[:2] + (kr + J,))
    items[..., :kr] = w.control_scales[:, None, :] * u
    if J:
        items[..., kr:] = w.offsets[:, None, :]
    return items


def set_problem(engine, case, w, dissipators):
    g = gh.lindblad_generators(case) + ([] if w.perturbations is None else list(w.perturbations))
    engine.set_lindblad_problem(
        case.n, case.initial_densities.shape[0], len(g), case.Nc, case.N, case.T, case.h0, g,
        dissipators, case.operators, case.initial_densities,
        costs=gh.lindblad_device_costs(case), cost_eval_step=case.cost_eval_step)


def sweep_results(engine, case, w, u):
    """(cost, grads, final) of the sweep through qocx_eval_lindblad and through the resident calls,
    and the sub-interval total of each evaluation."""
    set_problem(engine, case, w, case.dissipators)
    engine.set_lindblad_sweep(w.control_scales, w.offsets, w.rate_scales)
    host = engine.evaluate_lindblad(u)
    total = engine.lindblad_last_subintervals()
    engine.lindblad_upload_controls(u)
    engine.eval_lindblad_resident(True)
    resident = engine.lindblad_download_results()
    assert engine.lindblad_last_subintervals() == total
    return host, resident, total


def plain_seeds(engine, case, w, u):
    """Every seed as the plain problem with dissipators = c_b * gamma on its host-expanded controls,
    alone: (cost (B,), grads (B, Nc, K), final (B, S, n, n), sub-intervals (B,))."""
    items = expand(w, u)
    outs, counts = [], []
    for b in range(u.shape[0]):
        c = np.ones(len(case.dissipators)) if w.rate_scales is None else w.rate_scales[b]
        set_problem(engine, case, w, c * case.dissipators)
        outs.append(engine.evaluate_lindblad(items[b:b + 1]))
        counts.append(engine.lindblad_last_subintervals())
    return tuple(np.concatenate([o[i] for o in outs]) for i in range(3)) + (np.array(counts),)


def assert_seeds_are_plain(w, results, plain, kr):
    p_cost, p_grads, p_final, _ = plain
    want_grads = w.control_scales[:, None, :] * p_grads[..., :kr]  # one product, one rounding
    for cost, grads, final in results:
        assert np.array_equal(cost, p_cost)
        assert np.array_equal(final, p_final)
        assert np.array_equal(grads, want_grads)


# ---- 1. a seed is the plain problem -----------------------------------------------------------------------

# tag: (n, L, operators, S, two-sided evaluation expected)
SEED_CASES = {
    "n3_l1_padded_operator": (3, 1, "real", 1, True),
    "n4_l2": (4, 2, "real", 1, True),
    "n4_l2_complex_ops": (4, 2, "random", 1, True),
    "n16_l3_s2": (16, 3, "real", 2, True),
    "n20_l2_four_tiles": (20, 2, "real", 1, True),
    "n4_l5_one_wave": (4, 5, "real", 1, False),
}


@pytest.mark.parametrize("tag", sorted(SEED_CASES))
def test_a_seed_is_the_plain_problem_with_its_rates(engine, tag):
    n, L, ops, S, two_sided = SEED_CASES[tag]
    case = sized_case(n, L, ops, S)
    w = sweep_for(case, seed=500 + len(tag))
    u = 0.5 * np.random.default_rng(501).standard_normal((B, case.Nc, case.K))
    try:
        engine.set_timing(True, only="lindblad_combine")
        engine.reset_timing()
        host, resident, total = sweep_results(engine, case, w, u)
        combined = engine.timing()["lindblad_combine"][0]
    finally:
        engine.set_timing(False)
    plain = plain_seeds(engine, case, w, u)
    assert host[2].shape == (B, S, n, n) and host[1].shape == (B, case.Nc, case.K)
    assert_seeds_are_plain(w, (host, resident), plain, case.K)
    assert total == int(np.sum(plain[3]))
    assert (combined > 0) == two_sided, combined
    # the tables reach every seed: far above any gate
    assert np.min(np.abs(np.diff(plain[0]))) > 1e-6


def test_seeds_in_different_sub_division_groups(engine):
    """Amplitudes of 4, 1.5 and 0.2: the seeds' sub-division counts fall from seed to seed, so the
    launch order (groups in ascending count) is the reverse of the seed order."""
    case = sized_case(4, 2)
    w = sweep_for(case, seed=510)
    u = np.random.default_rng(511).standard_normal((B, case.Nc, case.K))
    u *= (np.array([4.0, 1.5, 0.2]) / np.max(np.abs(u), axis=(1, 2)))[:, None, None]
    host, resident, total = sweep_results(engine, case, w, u)
    plain = plain_seeds(engine, case, w, u)
    counts = plain[3]
    print("sub-intervals per seed", counts)
    assert counts[0] > counts[1] > counts[2]
    assert total == int(np.sum(counts))
    assert_seeds_are_plain(w, (host, resident), plain, case.K)
    # ... and the rate sensitivities come back in seed order (3 below holds them to the model)
    both = rate_sensitivities(engine, case, w, u)[2]
    alone = []
    for b in range(B):
        set_problem(engine, case, w, case.dissipators)
        engine.set_lindblad_sweep(w.control_scales[b:b + 1], w.offsets[b:b + 1], w.rate_scales[b:b + 1])
        engine.lindblad_sweep_want_rate_sensitivities(True)
        engine.evaluate_lindblad(u[b:b + 1])
        alone.append(engine.lindblad_sweep_sensitivities()[2][0])
    assert np.array_equal(both, np.stack(alone))


def test_without_rate_scales_the_plain_kernels_run_and_the_drive_may_depend_on_time():
    """Through the evaluator: lindblad_timedep (stage tables, a fixed grid) and a static problem; seed
    b against the plain problem set from the very arrays the evaluator set, tables included."""
    for name in ("lindblad_timedep", "lindblad_wc_n4"):
        case = cases_mod.lindblad_case_by_name(name)
        w = sweep_for(case, seed=520, rates=None)
        u = 0.4 * np.random.default_rng(521).standard_normal((B, case.Nc, case.K))
        engine = RecordingEngine(0)
        try:
            ev = device.LindbladEvaluator(
                case.T, case.initial_densities, case.N, hamiltonian=w,
                lindblad_data=case.lindblad_data(), control_count=case.K,
                control_eval_count=case.Nc, costs=product_cost_list(case),
                cost_eval_step=case.cost_eval_step, backend=engine)
            errors, grads, finals, _ = ev.evaluate_batch(u)
            a, kw = engine.last_problem
            assert engine.last_sweep[2] is None
            assert (kw.get("fixed_subdivision", 0) > 0) == (name == "lindblad_timedep")
            items = expand(w, u)
            Engine.set_lindblad_problem(engine, *a, **kw)
            p_cost, p_grads, p_final = engine.evaluate_lindblad(items)
        finally:
            engine.close()
        assert np.array_equal(errors, p_cost) and np.array_equal(finals, p_final)
        assert np.array_equal(grads, w.control_scales[:, None, :] * p_grads[..., :case.K])


# ---- 2. degenerate sweeps -----------------------------------------------------------------------------

def test_a_sweep_of_ones_is_the_plain_batch(engine):
    case = sized_case(4, 2)
    L = len(case.dissipators)
    u = 0.5 * np.random.default_rng(531).standard_normal((B, case.Nc, case.K))
    w = LindbladSweep(case.hamiltonian(), control_scales=np.ones((B, case.K)),
                      rate_scales=np.ones((B, L)))
    host, resident, _ = sweep_results(engine, case, w, u)
    gh.setup_lindblad_engine(engine, case)
    plain = engine.evaluate_lindblad(u)
    for got in (host, resident):
        for x, y in zip(got, plain):
            assert np.array_equal(x, y)


def test_swapped_rows_swap_the_seeds(engine):
    for n in (4, 20):
        case = sized_case(n, 2)
        w = sweep_for(case, seed=540)
        row = 0.5 * np.random.default_rng(541).standard_normal((case.Nc, case.K))
        u = np.stack([row] * B)  # the same pulse on every seed: the seeds differ by their tables alone
        first = sweep_results(engine, case, w, u)[:2]
        order = [1, 2, 0]
        swapped_w = LindbladSweep(case.hamiltonian(), perturbations=w.perturbations,
                                  offsets=w.offsets[order], control_scales=w.control_scales[order],
                                  rate_scales=w.rate_scales[order])
        swapped = sweep_results(engine, case, swapped_w, u)[:2]
        for a, b in zip(first, swapped):
            for x, y in zip(a, b):
                assert np.array_equal(x[order], y)
            assert np.min(np.abs(np.diff(a[0]))) > 1e-6


# ---- 3. rate sensitivities ----------------------------------------------------------------------------

_SENS = {}


def sensitivity_run(tag):
    """One evaluation with rate sensitivities (two seeds) and the model's, computed once, shared."""
    if tag in _SENS:
        return _SENS[tag]
    n, L, ops, S = {"n4_l1": (4, 1, "real", 1), "n4_l2": (4, 2, "real", 1),
                    "n16_l3_s2_complex_ops": (16, 3, "random", 2),
                    "n20_l2": (20, 2, "real", 1)}[tag]
    case = sized_case(n, L, ops, S)
    w = sweep_for(case, seed=550 + n + L, seeds=2)
    u = 0.5 * np.random.default_rng(551).standard_normal((2, case.Nc, case.K))
    items = expand(w, u)
    system = lm.StructuredLindblad(case.h0, gh.lindblad_generators(case) + list(w.perturbations),
                                   case.dissipators, case.operators)
    costs = [getattr(ol, k)(**kw) for k, kw in case.cost_specs]
    model = np.stack([sm.rate_sensitivities(system, items[b], case.initial_densities, case.T, case.N,
                                            costs, factors=w.rate_scales[b])[1] for b in range(2)])
    _SENS[tag] = dict(case=case, w=w, u=u, items=items, model=model)
    return _SENS[tag]


def rate_sensitivities(engine, case, w, u, resident=False):
    set_problem(engine, case, w, case.dissipators)
    engine.set_lindblad_sweep(w.control_scales, w.offsets, w.rate_scales)
    engine.lindblad_sweep_want_rate_sensitivities(True)
    try:
        if resident:
            engine.lindblad_upload_controls(u)
            engine.eval_lindblad_resident(True)
            grads = engine.lindblad_download_results()[1]
        else:
            grads = engine.evaluate_lindblad(u)[1]
        return engine.lindblad_sweep_sensitivities() + (grads,)
    finally:
        engine.lindblad_sweep_want_rate_sensitivities(False)


@pytest.mark.parametrize("tag", ["n4_l1", "n4_l2", "n16_l3_s2_complex_ops", "n20_l2"])
def test_rate_sensitivities_match_the_model(engine, tag):
    r = sensitivity_run(tag)
    case, w, u = r["case"], r["w"], r["u"]
    scales, offsets, rates, _ = rate_sensitivities(engine, case, w, u)
    print(tag, "model", r["model"].ravel(), "device - model", (rates - r["model"]).ravel())
    assert rates.shape == (2, len(case.dissipators))
    # (a signal, not rounding: the gate below is 1e-8 of the largest entry)
    assert np.max(np.abs(r["model"])) > 1e-6
    assert helpers.lindblad_grad_close(rates, r["model"], case)
    # the resident evaluation launches the same kernels on the same values
    assert np.array_equal(rate_sensitivities(engine, case, w, u, resident=True)[2], rates)


@pytest.mark.parametrize("tag", ["n4_l2", "n20_l2"])
def test_rate_sensitivities_in_several_pieces(engine, tag):
    """A stage budget of one seed with pieces of one seed allowed: two launches for the two (distinct)
    seeds, whether they share a sub-division group or not, the stage buffers reused from the first
    to the second - and the result is that of the unforced evaluation, bit for bit."""
    r = sensitivity_run(tag)
    case, twin, pulse = r["case"], r["w"], r["u"]
    whole = rate_sensitivities(engine, case, twin, pulse)
    try:
        engine.debug_lindblad_knobs(1, 1, 0)
        engine.set_timing(True, only="lindblad_combine")
        engine.reset_timing()
        pieces = rate_sensitivities(engine, case, twin, pulse)
        launches = engine.timing()["lindblad_combine"][0]
    finally:
        engine.set_timing(False)
        engine.debug_lindblad_knobs(0, 256, 0)
    assert launches == 2, launches
    for x, y in zip(whole, pieces):
        assert np.array_equal(x, y)
    assert np.all(whole[2] != 0) and np.all(whole[2][0] != whole[2][1])  # two distinct seeds


def test_rate_sensitivities_are_none_where_a_piece_did_not_run_two_sided(engine):
    r = sensitivity_run("n4_l2")
    case, w, u = r["case"], r["w"], r["u"]
    # the recompute path: nothing kept, the classic launch
    try:
        engine.debug_lindblad_knobs(1, 256, 0)
        twin = LindbladSweep(case.hamiltonian(), perturbations=w.perturbations,
                             offsets=w.offsets[[0, 0]], control_scales=w.control_scales[[0, 0]],
                             rate_scales=w.rate_scales)
        set_problem(engine, case, twin, case.dissipators)
        engine.set_lindblad_sweep(twin.control_scales, twin.offsets, np.ones((2, 2)))
        engine.lindblad_sweep_want_rate_sensitivities(True)
        engine.set_timing(True, only="lindblad_combine")
        engine.reset_timing()
        engine.evaluate_lindblad(np.stack([u[0], u[0]]))
        assert engine.timing()["lindblad_combine"][0] == 0
        out = np.empty((2, 2))
        code = engine._lib.qocx_lindblad_sweep_download_sensitivities(
            engine._ctx, None, None, out.ctypes.data_as(_DP))
        assert code == ERR_STATE
        scales, offsets, rates = engine.lindblad_sweep_sensitivities()
        assert rates is None and np.all(np.isfinite(scales)) and np.all(np.isfinite(offsets))
    finally:
        engine.set_timing(False)
        engine.debug_lindblad_knobs(0, 256, 0)
    # not asked for
    engine.lindblad_sweep_want_rate_sensitivities(False)
    engine.evaluate_lindblad(np.stack([u[0], u[0]]))
    assert engine.lindblad_sweep_sensitivities()[2] is None
    # a ForbidDensities step cost (lindblad_n4), five operators (the one-wave kernels): through the evaluator
    for case in (cases_mod.lindblad_case_by_name("lindblad_n4"), sized_case(4, 5)):
        w = sweep_for(case, seed=560, seeds=2)
        ev = device.LindbladEvaluator(
            case.T, case.initial_densities, case.N, hamiltonian=w,
            lindblad_data=case.lindblad_data(), control_count=case.K,
            control_eval_count=case.Nc, costs=product_cost_list(case),
            cost_eval_step=case.cost_eval_step, backend=engine)
        ev.want_rate_sensitivities(True)
        ev.evaluate_batch(0.3 * np.random.default_rng(561).standard_normal((2, case.Nc, case.K)))
        sens = ev.sweep_sensitivities()
        ev.want_rate_sensitivities(False)
        assert sens["rate_scales"] is None
        assert sens["control_scales"].shape == (2, case.K) and np.all(np.isfinite(sens["offsets"]))


def test_channel_sensitivities_in_the_summation_order_of_the_sweep_kernels(engine):
    for tag in ("n4_l2", "n20_l2"):
        r = sensitivity_run(tag)
        case, w, u = r["case"], r["w"], r["u"]
        scales, offsets, _, _ = rate_sensitivities(engine, case, w, u)
        plain = plain_seeds(engine, case, w, u)  # the items' gradients, bit for bit (1)
        g = plain[1]
        for b in range(2):
            assert np.array_equal(scales[b], ordered_sum(u[b] * g[b][:, :case.K]))
            assert np.array_equal(offsets[b], ordered_sum(g[b][:, case.K:]))


# ---- 4. T1 decay per seed --------------------------------------------------------------------------------

def test_t1_decay_per_seed_and_its_time_gradient(engine):
    """One excited level decaying with gamma, four durations: the population is exp(-gamma T_b) to the
    forward tolerance of DESIGN.md section 9 for a known answer (1e-10, the gate of the T1 tests), and
    with the cost 1 - population / n (TargetDensityInfidelity on |1><1|, n = 2: 1 - p / 2)
    dE_b/dT_b = gamma exp(-gamma T_b) / 2 at the gradient gate of 3 (1e-8 of the largest entry)."""
    gamma, ref = 0.7, 1.0
    times = np.array([0.5, 1.0, 1.7, 2.6])
    sm_op = np.array([[0, 1], [0, 0]], dtype=np.complex128)  # |0><1|
    sz = np.diag([0.0, 1.0]).astype(np.complex128)
    rho0 = np.zeros((1, 2, 2), dtype=np.complex128)
    rho0[0, 1, 1] = 1
    w = LindbladSweep.durations(lambda u, t: 0.3 * sz + u[0] * sz, times, ref)
    ev = device.LindbladEvaluator(
        ref, rho0, 7, hamiltonian=w, lindblad_data=lambda t: (np.array([gamma]), sm_op[None]),
        control_count=1, control_eval_count=4, costs=[TargetDensityInfidelity(rho0)], backend=engine)
    ev.want_rate_sensitivities(True)
    errors, _, finals, _ = ev.evaluate_batch(np.zeros((4, 4, 1)))
    sens = ev.sweep_sensitivities()
    ev.want_rate_sensitivities(False)
    population = np.exp(-gamma * times)
    print("population error", np.real(finals[:, 0, 1, 1]) - population)
    assert np.max(np.abs(np.real(finals[:, 0, 1, 1]) - population)) < 1e-10
    assert np.max(np.abs(errors - (1 - population / 2))) < 1e-10
    want = gamma * population / 2
    got = sens["evolution_time_gradients"]
    print("dE/dT", got, "analytic", want, "difference", got - want)
    assert np.all(got > 0)
    assert np.max(np.abs(got - want)) < 1e-8 * np.max(np.abs(want))
    # (c_b = tau_b: E_b = 1 - exp(-gamma c_b reference_time) / 2)
    assert np.max(np.abs(sens["rate_scales"][:, 0] - ref * want)) < 1e-8 * np.max(ref * want)
    # ... and the exact sensitivities (tests/lindblad_exact.py: Frechet derivatives of the superoperator
    # exponentials of seed b, tau_b times the whole Lindbladian) at their gate, far below 1e-8
    from tests import lindblad_exact as ex
    exact = []
    for tau in times / ref:
        r = ex.piecewise_constant(tau * 0.3 * sz, [tau * sz], sm_op[None], [tau * gamma],
                                  np.zeros((4, 1)), ref, 7, rho0, [ol.TargetDensityInfidelity(rho0)])
        exact.append((r.error, r.tau_sens / tau / ref, r.rate_sens[0] / tau))
    exact = np.array(exact)
    print("over the gates: cost", np.max(np.abs(errors - exact[:, 0])) / ex.GATE_COST, "dE/dT",
          np.max(np.abs(got - exact[:, 1])) / np.max(exact[:, 1]) / ex.GATE_SENSITIVITIES)
    assert np.max(np.abs(errors - exact[:, 0])) <= ex.GATE_COST
    assert np.max(np.abs(got - exact[:, 1])) <= ex.GATE_SENSITIVITIES * np.max(np.abs(exact[:, 1]))
    assert (np.max(np.abs(sens["rate_scales"][:, 0] - exact[:, 2]))
            <= ex.GATE_SENSITIVITIES * np.max(np.abs(exact[:, 2])))


# ---- 5. the resident route against the host loop --------------------------------------------------------

class HostAdam(Adam):  # not type(...) is Adam: takes the host loop
    pass


class HostLBFGS(LBFGS):
    pass


OPTIMIZERS = {"adam": (lambda: Adam(learning_rate=5e-2), lambda: HostAdam(learning_rate=5e-2)),
              "lbfgs": (LBFGS, HostLBFGS)}


def route_problem(complex_controls=False):
    n, K, N, Nc, T = 4, 2, 7, 4, 1.8
    rng = np.random.default_rng(1200 + int(complex_controls))
    a = cases_mod.annihilation(n)
    ad = a.conj().T
    h0 = 0.4 * (ad @ a) - 0.15 * (ad @ ad @ a @ a)
    g_re = [0.4 * (a + ad), 0.4 * cases_mod.gue(rng, n)]
    g_im = [0.4j * (a - ad), 0.4 * cases_mod.gue(rng, n)]

    def linear(u, t):
        out = h0
        for k in range(K):
            out = out + (u[k].real * g_re[k] + u[k].imag * g_im[k] if complex_controls
                         else u[k] * g_re[k])
        return out
    gammas, ops = np.array([0.3, 0.2]), np.stack([a / np.sqrt(n - 1), ad @ a / (n - 1)])
    w = LindbladSweep.durations(
        linear, T * np.array([0.6, 1.0, 1.4]), T,
        control_scales=1 + 0.05 * rng.standard_normal((B, K)),
        perturbations=0.3 * cases_mod.gue(rng, n)[None], offsets=0.5 * rng.standard_normal((B, 1)),
        rate_scales=np.array([[1.0, 0.5], [2.0, 1.0], [0.5, 2.0]]))
    init = np.zeros((1, n, n), dtype=np.complex128)
    init[0, 0, 0] = 1
    targ = np.zeros((1, n, n), dtype=np.complex128)
    targ[0, 1, 1] = 1
    head = (K, Nc, [TargetDensityInfidelity(targ)], T, init, N)
    return w, (lambda t: (gammas, ops)), head, rng


def run_routes(routes, optimizer, w, data, head, start, **kw):
    """The resident route, the host loop and B single-seed runs on member(b)."""
    resident, host = OPTIMIZERS[optimizer]
    kw = dict(dict(iteration_count=4, log_iteration_step=0, lindblad_data=data), **kw)
    a = qoc_amd.grape_lindblad_discrete_batch(*head, start.copy(), hamiltonian=w,
                                              optimizer=resident(), **kw)
    assert routes == {"resident": 1, "host": 0}
    b = qoc_amd.grape_lindblad_discrete_batch(*head, start.copy(), hamiltonian=w, optimizer=host(),
                                              **kw)
    assert routes == {"resident": 1, "host": 1}
    single = dict(kw, lindblad_data=None)
    for s in range(start.shape[0]):
        single["lindblad_data"] = w.member_lindblad_data(s, data)
        one = qoc_amd.grape_lindblad_discrete(*head, hamiltonian=w.member(s),
                                              initial_controls=start[s].copy(),
                                              optimizer=resident(), **single)
        assert one.best_iteration == a.best_iteration[s]
        assert abs(one.best_error - a.best_error[s]) < 1e-12
        assert helpers.rel_err(a.best_controls[s], one.best_controls) < 1e-10
        assert abs(one.best_error - b.best_error[s]) < 1e-12
        assert helpers.rel_err(b.best_controls[s], one.best_controls) < 1e-10
    return a, b


def assert_bit_identical(a, b):
    for s in range(len(a.best_error)):
        print("seed", s, "best_error", abs(a.best_error[s] - b.best_error[s]), "best_controls",
              np.max(np.abs(a.best_controls[s] - b.best_controls[s])))
    assert np.array_equal(a.best_error, b.best_error)
    assert np.array_equal(a.best_iteration, b.best_iteration)
    assert np.array_equal(a.iterations_run, b.iterations_run)
    for s in range(len(a.best_error)):
        assert np.array_equal(a.best_controls[s], b.best_controls[s])
        assert np.array_equal(a.best_final_densities[s], b.best_final_densities[s])
    for key in ("control_scales", "offsets", "rate_scales", "evolution_time_gradients"):
        assert np.array_equal(a.sweep_sensitivities[key], b.sweep_sensitivities[key])


@pytest.mark.parametrize("optimizer", ["adam", "lbfgs"])
def test_resident_route_equals_host_loop_and_single_seed_runs(routes, optimizer):
    w, data, head, rng = route_problem()
    K, Nc = head[0], head[1]
    u0 = np.clip(0.6 * rng.standard_normal((B, Nc, K)), -1, 1)
    a, b = run_routes(routes, optimizer, w, data, head, u0, max_control_norms=np.full(K, 1.0))
    assert_bit_identical(a, b)
    assert np.any(a.best_iteration > 0) and a.member_errors == [None] * B
    sens = a.sweep_sensitivities
    assert sens["control_scales"].shape == (B, K) and sens["offsets"].shape == (B, 2)
    assert sens["rate_scales"].shape == (B, 2)
    assert np.all(np.isfinite(sens["evolution_time_gradients"]))


@pytest.mark.parametrize("optimizer", ["adam", "lbfgs"])
def test_resident_route_with_a_sine_basis_and_control_variation_on_the_device(routes, optimizer):
    w, data, head, rng = route_problem()
    K, Nc, costs, T, init, N = head
    head = (K, Nc, costs + [ControlVariation(K, Nc, cost_multiplier=0.4, order=1)], T, init, N)
    basis = ControlBasis.sine(Nc, 3)
    c0 = 0.3 * rng.standard_normal((B, 3, K))
    for s in range(B):
        c0[s] *= min(1.0, 0.9 / np.max(np.abs(basis.expand(c0[s]))))
    resident, host = OPTIMIZERS[optimizer]
    kw = dict(iteration_count=4, log_iteration_step=0, lindblad_data=data, hamiltonian=w,
              control_basis=basis, max_control_norms=np.full(K, 1.0))
    a = qoc_amd.grape_lindblad_discrete_batch(*head, c0.copy(), optimizer=resident(), **kw)
    b = qoc_amd.grape_lindblad_discrete_batch(*head, c0.copy(), optimizer=host(), **kw)
    assert routes == {"resident": 1, "host": 1}
    assert_bit_identical(a, b)
    for s in range(B):
        assert np.array_equal(a.best_coefficients[s], b.best_coefficients[s])


@pytest.mark.parametrize("optimizer", ["adam", "lbfgs"])
def test_resident_route_with_complex_controls(routes, optimizer):
    w, data, head, rng = route_problem(complex_controls=True)
    K, Nc = head[0], head[1]
    u0 = 0.3 * (rng.standard_normal((B, Nc, K)) + 1j * rng.standard_normal((B, Nc, K)))
    # (bounds no step reaches: the two routes are bit-identical only while no clip acts on a complex
    # control - the host clips the modulus in NumPy, the device in its own kernel, as on the plain
    # problem; grape_lindblad_discrete_batch says so)
    a, b = run_routes(routes, optimizer, w, data, head, u0, complex_controls=True,
                      max_control_norms=np.full(K, 50.0))
    print("largest modulus", max(np.max(np.abs(c)) for c in a.best_controls))
    assert_bit_identical(a, b)
    assert all(np.iscomplexobj(c) for c in a.best_controls)
    assert a.sweep_sensitivities["control_scales"].shape == (B, K)


# ---- 6. the engine's rejections ---------------------------------------------------------------------------

def code_of(call, *args):
    with pytest.raises(QocxError) as err:
        call(*args)
    return err.value.code


def test_engine_rejections_and_what_clears_the_sweep(engine):
    case = sized_case(4, 2)
    w = sweep_for(case, seed=600)
    u = 0.3 * np.random.default_rng(601).standard_normal((B, case.Nc, case.K))
    set_problem(engine, case, w, case.dissipators)
    good = (w.control_scales, w.offsets, w.rate_scales)
    bad = lambda i, value: tuple(value if j == i else x for j, x in enumerate(good))  # noqa: E731
    # arguments
    lib, ctx = engine._lib, engine._ctx
    dp = lambda a: a.ctypes.data_as(_DP)  # noqa: E731
    ones = np.ones((2000, 2))
    assert lib.qocx_lindblad_set_sweep(ctx, 0, 0, dp(ones), None, None) == ERR_ARG
    assert lib.qocx_lindblad_set_sweep(ctx, 1025, 0, dp(ones), None, dp(ones)) == ERR_ARG
    assert lib.qocx_lindblad_set_sweep(ctx, 2, 3, None, dp(ones), None) == ERR_ARG   # fixed >= K
    assert lib.qocx_lindblad_set_sweep(ctx, 2, 1, None, None, None) == ERR_ARG       # offsets missing
    assert lib.qocx_lindblad_set_sweep(ctx, 2, 0, None, dp(ones), None) == ERR_ARG   # offsets without J
    for i, value in ((0, w.control_scales * np.nan), (1, w.offsets * np.inf),
                     (2, w.rate_scales * np.nan), (2, -w.rate_scales)):
        assert code_of(engine.set_lindblad_sweep, *bad(i, value)) == ERR_ARG
    # no sweep yet: the sweep's own calls are a state error
    assert code_of(engine.lindblad_sweep_want_rate_sensitivities, True) == ERR_STATE
    assert lib.qocx_lindblad_sweep_download_sensitivities(ctx, None, None, None) == ERR_STATE
    # state: an ensemble and a sweep exclude each other; rates need a static problem
    engine.set_lindblad_ensemble(w.control_scales, w.offsets, np.full(B, 1.0 / B))
    assert code_of(engine.set_lindblad_sweep, *good) == ERR_STATE
    set_problem(engine, case, w, case.dissipators)  # a new problem clears the ensemble
    engine.set_lindblad_sweep(*good)
    engine.set_lindblad_sweep(*good)                # (a sweep may be set again)
    assert code_of(engine.set_lindblad_ensemble, w.control_scales, w.offsets,
                   np.full(B, 1.0 / B)) == ERR_STATE
    assert code_of(engine.set_lindblad_ensemble_rates, w.rate_scales) == ERR_STATE
    assert code_of(engine.lindblad_ensemble_member_costs) == ERR_STATE
    bars = np.zeros((B, 1, 1, case.n, case.n), dtype=np.complex128)
    assert code_of(engine.set_density_cotangents, [case.N - 1], bars) == ERR_STATE
    # any other batch size
    assert code_of(engine.evaluate_lindblad, u[:2]) == ERR_ARG
    assert code_of(engine.lindblad_upload_controls, u[:2]) == ERR_ARG
    # sensitivities need an evaluation with gradients whose controls stand
    assert code_of(engine.lindblad_sweep_sensitivities) == ERR_STATE
    engine.evaluate_lindblad(u, want_grad=False)
    assert code_of(engine.lindblad_sweep_sensitivities) == ERR_STATE
    engine.lindblad_upload_controls(u)
    engine.eval_lindblad_resident(True)
    engine.lindblad_sweep_sensitivities()
    engine.lindblad_opt_begin()
    engine.lindblad_opt_step(0, np.ones(B, bool), np.ones(B, bool), 0.1)  # the controls moved
    assert code_of(engine.lindblad_sweep_sensitivities) == ERR_STATE
    # a new problem clears the sweep: the batch is free again, the K channels are the problem's
    set_problem(engine, case, w, case.dissipators)
    cost, grads, _ = engine.evaluate_lindblad(expand(w, u)[:2])
    assert cost.shape == (2,) and grads.shape == (2, case.Nc, case.K + 1)
    assert code_of(engine.lindblad_sweep_want_rate_sensitivities, True) == ERR_STATE
    # rates on a problem with stage tables
    td = cases_mod.lindblad_case_by_name("lindblad_timedep")
    tw = sweep_for(td, seed=602)
    rec = RecordingEngine(0)
    try:
        device.LindbladEvaluator(
            td.T, td.initial_densities, td.N, hamiltonian=sweep_for(td, seed=602, rates=None),
            lindblad_data=td.lindblad_data(), control_count=td.K, control_eval_count=td.Nc,
            costs=product_cost_list(td), backend=rec, control_bounds=np.ones(td.K))
        assert rec.last_problem[1]["fixed_subdivision"] > 0
        assert code_of(rec.set_lindblad_sweep, tw.control_scales, tw.offsets, tw.rate_scales) == ERR_STATE
        rec.set_lindblad_sweep(tw.control_scales, tw.offsets, None)
    finally:
        rec.close()
