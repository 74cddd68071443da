"""
GPU tests (-m gpu) of per-member dissipation rates on the Lindblad path
(HamiltonianEnsemble(..., rate_scales=c), qocx_lindblad_set_ensemble_rates): member m decays with
gamma_mi = c_mi * gamma_i.

a. every member is, bit for bit, the plain (K_r + J)-channel problem set with dissipators =
   c_m * gamma on host-expanded controls - through qocx_eval_lindblad and the resident calls -, and
   the seeds' costs and gradients are the exact fma fold of the members'; on every kernel that
   reads a control-free generator or a rate (the knobs select them); a table handed to the wrong
   member is seen (swapped rows swap the members);
b. members against the CPU references at the gates of tests/test_gpu_lindblad_ensemble.py: the
   NumPy model of the device algorithm (cost, densities 1e-12, gradients 1e-10 of max |g| with the
   1e-3 floor) and the reference integrator (cost 1e-9, densities 1e-8);
c. the known answer: T1 decay, excited population exp(-c_m gamma T) (1e-10, the gate of the T1 test
   of tests/test_gpu_lindblad.py);
d. members of one seed take different sub-division counts, each the plain problem's, and no result
   depends on the batch neighbours;
e. rates of 1 are the ensemble without rates, and M = 1, c = 1, J = 0 is the plain problem, bit for
   bit;
f. multi-start GRAPE: the resident route against the host loop;
g. the ABI's rejections and what clears the rates.

B = 2 seeds, M = 3 members, at most 11 system evaluation points; rate factors in [0.25, 4].
"""

import numpy as np
import pytest

import qoc_amd
from oracle import qoc_lindblad_numpy as ol
from qoc_amd.engine import Engine, QocxError
from qoc_amd.models import InterpolationPolicy
from qoc_amd.standard import ControlBasis, HamiltonianEnsemble, TargetDensityInfidelity
from qoc_amd.standard.costs import ControlVariation
from tests import cases as cases_mod
from tests import gpu_helpers as gh
from tests import helpers
from tests import lindblad_model as lm
from tests.test_gpu_lindblad_ensemble import (expand, folded, make_evaluator, multistart, rel_err,
                                              routes)  # noqa: F401 (fixture)

pytestmark = pytest.mark.gpu

B, M = 2, 3


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
    """The engine, remembering the arguments of the last set_lindblad_problem (with the interpolation
    keyword in its signature, where the evaluator looks for it)."""

    def set_lindblad_problem(self, *a, interpolation="linear", **kw):
        self.last_problem = (a, dict(kw, interpolation=interpolation))
        Engine.set_lindblad_problem(self, *a, interpolation=interpolation, **kw)


def rate_factors(rng, members, L):
    """(0.25, 1, 4)-like rows: log-uniform factors in [0.25, 4]."""
    return 4.0 ** rng.uniform(-1, 1, (members, L))


def shape_case(n, L, ops="real", N=7, Nc=4):
    """An anharmonic oscillator with two drives and one final TargetDensityInfidelity (the shape of
    the two-sided evaluation), L Lindblad operators: real ladder ones, or random complex ones."""
    c = cases_mod.lindblad_wellconditioned_case(
        "rates_n{}_l{}".format(n, L), n=n, N=N, Nc=Nc, T=0.3 * (N - 1), sigma=0.5, drive=0.4,
        operators=min(max(L, 2), 4))
    a = cases_mod.annihilation(n)
    ad = a.conj().T
    pool = [a / np.sqrt(n - 1), ad @ a / (n - 1), a @ a / (n - 1), (a + 1j * ad @ a) / (n - 1),
            ad / np.sqrt(n - 1)]
    gam = np.array([0.6, 0.3, 0.4, 0.25, 0.15])  # (strong enough for the rates to show in every digit)
    if ops == "random":
        rng = np.random.default_rng(1000 + 10 * n + L)
        pool = [0.5 * (cases_mod.gue(rng, n) + 0.5j * cases_mod.gue(rng, n)) for _ in range(L)]
    c.operators = np.stack(pool[:L])
    c.dissipators = gam[:L].copy()
    return c


def ensemble_for(case, seed, J=1, members=M, twins=False, rates=None):
    """control_scales, J perturbation channels, weights and rate_scales. twins: members 0 and 1 share
    scales and offsets, so they differ by their rates alone."""
    rng = np.random.default_rng(seed)
    L = len(case.dissipators)
    d = np.stack([0.5 * cases_mod.gue(rng, case.n) for _ in range(J)]) if J else None
    offsets = 0.3 * rng.standard_normal((members, J)) if J else None
    scales = 1 + 0.05 * rng.standard_normal((members, case.K))
    if twins:
        scales[1] = scales[0]
        if J:
            offsets[1] = offsets[0]
    return HamiltonianEnsemble(
        case.hamiltonian(), perturbations=d, offsets=offsets, control_scales=scales,
        weights=rng.uniform(0.2, 1.0, members),
        rate_scales=rate_factors(rng, members, L) if rates is None else rates)


def set_problem(engine, case, e, dissipators):
    """The (K_r + J)-channel problem of `case` with the D_j of `e` behind its drives."""
    g = gh.lindblad_generators(case) + ([] if e.perturbations is None else list(e.perturbations))
    engine.set_lindblad_problem(
        case.n, case.initial_densities.shape[0], len(g), case.Nc, case.N, case.T, case.h0, g,
        dissipators, case.operators, case.initial_densities,
        costs=gh.lindblad_device_costs(case), cost_eval_step=case.cost_eval_step)


def ensemble_results(engine, u, rates):
    """(cost, grads, final, members) of the ensemble set on `engine`, with `rates` (None: none are
    set), through qocx_eval_lindblad and through the resident calls."""
    if rates is not None:
        engine.set_lindblad_ensemble_rates(rates)
    host = engine.evaluate_lindblad(u) + (engine.lindblad_ensemble_member_costs(),)
    engine.lindblad_upload_controls(u)
    engine.eval_lindblad_resident(True)
    resident = engine.lindblad_download_results() + (engine.lindblad_ensemble_member_costs(),)
    return host, resident


def plain_members(engine, case, e, u):
    """Every member as the plain problem with dissipators = c_m * gamma on host-expanded controls:
    (cost (B, M), grads (B, M, Nc, K), final (B, M, S, n, n))."""
    items = expand(e, u)
    outs = []
    for m in range(e.member_count):
        set_problem(engine, case, e, e.rate_scales[m] * case.dissipators)
        outs.append(engine.evaluate_lindblad(items[:, m]))
    return tuple(np.stack([o[i] for o in outs], axis=1) for i in range(3))


def assert_members_are_plain(e, results, plain):
    p_cost, p_grads, p_final = plain
    want_cost, want_grads = folded(e, p_cost, p_grads)
    for cost, grads, final, members in results:
        assert np.array_equal(members, p_cost)
        assert np.array_equal(final, p_final)
        assert np.array_equal(cost, want_cost)
        assert np.array_equal(grads, want_grads)


def combine_launches(engine):
    return engine.timing()["lindblad_combine"][0]


# ---- a. members are the plain problem with their own rates, on every kernel ---------------------------

DEFAULT_KNOBS = dict(lindblad_pad_operator=1, lindblad_chain=1, lindblad_q2=1, lindblad_two_sided=1,
                     lindblad_hermitian=1, lindblad_real_ops=1, lindblad_4t=1)
# tag: (n, L, operators, knobs, debug_lindblad_knobs, two-sided evaluation expected)
VARIANTS = {
    # one operator: padded with a zero operator onto the four-wave launches, or the three-wave form
    "n2_l1_pad": (2, 1, "real", dict(lindblad_pad_operator=1), None, True),
    "n2_l1_nopad": (2, 1, "real", dict(lindblad_pad_operator=0), None, True),
    # the one-wave kernel (more than four operators), and one wave per seed forced at L = 2
    "n4_l5": (4, 5, "real", {}, None, False),
    "n4_l2_one_wave": (4, 2, "real", {}, (0, 256, 1), False),
    # stage values recomputed by the adjoint (classic launch, nothing kept)
    "n4_l2_recompute": (4, 2, "real", {}, (1, 256, 0), False),
    "n20_l2_recompute": (20, 2, "real", {}, (1, 256, 0), False),
    "n4_l2_complex_ops": (4, 2, "random", {}, None, True),
    "n4_l3_complex_ops": (4, 3, "random", {}, None, True),
}
for _L in (2, 3, 4):
    VARIANTS["n4_l%d" % _L] = (4, _L, "real", {}, None, True)
    VARIANTS["n4_l%d_nochain" % _L] = (4, _L, "real", dict(lindblad_chain=0), None, True)
    VARIANTS["n4_l%d_noq2" % _L] = (4, _L, "real", dict(lindblad_q2=0), None, True)
    VARIANTS["n4_l%d_classic" % _L] = (4, _L, "real", dict(lindblad_two_sided=0), None, False)
    VARIANTS["n4_l%d_nonherm" % _L] = (4, _L, "real", dict(lindblad_hermitian=0), None, True)
    VARIANTS["n4_l%d_complex_arith" % _L] = (4, _L, "real", dict(lindblad_real_ops=0), None, True)
for _n in (17, 20):
    for _t4 in (1, 0):
        for _herm in (1, 0):
            VARIANTS["n%d_l2_4t%d_herm%d" % (_n, _t4, _herm)] = (
                _n, 2, "real", dict(lindblad_4t=_t4, lindblad_hermitian=_herm), None, _t4 == 1)


@pytest.mark.parametrize("tag", sorted(VARIANTS))
def test_members_are_the_plain_problem_with_their_rates(engine, tag):
    n, L, ops, knobs, debug, two_sided = VARIANTS[tag]
    case = shape_case(n, L, ops, N=4 if n > 16 else 7, Nc=3 if n > 16 else 4)
    e = ensemble_for(case, seed=400 + len(tag))
    rng = np.random.default_rng(401)
    u = 0.5 * rng.standard_normal((B, case.Nc, case.K))
    if debug is not None and debug[0] == 1:
        # (recompute is forced for groups of two items or more: both seeds reach the same maxima,
        # so the items (0, m) and (1, m) share a sub-division count, here and in the plain runs)
        u[1] = -u[0]
    try:
        for name, value in dict(DEFAULT_KNOBS, **knobs).items():
            engine.set_knob(name, value)
        if debug is not None:
            engine.debug_lindblad_knobs(*debug)
        set_problem(engine, case, e, case.dissipators)
        engine.set_lindblad_ensemble(e.control_scales, e.offsets, e.weights)
        engine.set_timing(True, only="lindblad_combine")
        engine.reset_timing()
        results = ensemble_results(engine, u, e.rate_scales)
        combined = combine_launches(engine)
        engine.set_timing(False)
        plain = plain_members(engine, case, e, u)
    finally:
        engine.set_timing(False)
        for name, value in DEFAULT_KNOBS.items():
            engine.set_knob(name, value)
        engine.debug_lindblad_knobs(0, 256, 0)
    S = case.initial_densities.shape[0]
    assert results[0][2].shape == (B, M, S, n, n) and results[0][1].shape == (B, case.Nc, case.K)
    assert_members_are_plain(e, results, plain)
    assert (combined > 0) == two_sided, combined  # the launches this variant is about
    # the rates reach every member: far above any gate
    assert np.min(np.abs(np.diff(plain[0], axis=1))) > 1e-6


def test_the_shape_of_the_benchmark_and_a_problem_with_step_costs(engine):
    """n = 16, L = 2 (lindblad_c4_short, the benchmark's system) and n = 4 with ForbidDensities step
    costs on two densities (the classic launch on several waves)."""
    for name in ("lindblad_c4_short", "lindblad_n4"):
        case = cases_mod.lindblad_case_by_name(name)
        case.dissipators = np.array([0.5, 0.2])
        e = ensemble_for(case, seed=410)
        u = 0.3 * np.random.default_rng(411).standard_normal((B, case.Nc, case.K))
        set_problem(engine, case, e, case.dissipators)
        engine.set_lindblad_ensemble(e.control_scales, e.offsets, e.weights)
        results = ensemble_results(engine, u, e.rate_scales)
        assert_members_are_plain(e, results, plain_members(engine, case, e, u))


def test_swapped_rows_swap_the_members(engine):
    """Members 0 and 1 differ by their rates alone: with the two rows of rate_scales swapped their
    results swap, bit for bit, and they differ by many orders above every gate - a member index that
    was silently 0 (or any other) would show."""
    for n, L in ((4, 2), (20, 2)):
        case = shape_case(n, L, N=4 if n > 16 else 7, Nc=3 if n > 16 else 4)
        e = ensemble_for(case, seed=420, twins=True)
        e.rate_scales[0], e.rate_scales[1], e.rate_scales[2] = (0.25, 0.3), (4.0, 3.5), (1.0, 1.2)
        u = 0.5 * np.random.default_rng(421).standard_normal((B, case.Nc, case.K))
        set_problem(engine, case, e, case.dissipators)
        engine.set_lindblad_ensemble(e.control_scales, e.offsets, np.array([0.5, 0.5, 0.0]))
        first = ensemble_results(engine, u, e.rate_scales)
        swapped = ensemble_results(engine, u, e.rate_scales[[1, 0, 2]])
        for a, b in zip(first, swapped):
            assert np.array_equal(a[3][:, [1, 0, 2]], b[3])         # member costs
            assert np.array_equal(a[2][:, [1, 0, 2]], b[2])         # final densities
            # (1e-6: six orders above the gate members are held to against the device model, 1e-12,
            # and two above the loosest one of this file, 1e-8 against the reference integrator)
            assert np.min(np.abs(a[3][:, 0] - a[3][:, 1])) > 1e-6
            assert np.max(np.abs(a[2][:, 0] - a[2][:, 1])) > 1e-6
            # equal weights on the twins: the fold adds the same two numbers to 0 in either order
            assert np.array_equal(a[0], b[0])


# ---- through the evaluator: b. the CPU references; piecewise-constant and complex controls ------------

_RUNS = {}


def evaluator_run(name, **kw):
    """One ensemble evaluation through LindbladEvaluator and the plain problem of every member set
    from the very arrays the evaluator set, with dissipators = c_m * gamma. Shared, left unchanged."""
    key = (name,) + tuple(sorted(kw))
    if key in _RUNS:
        return _RUNS[key]
    case = cases_mod.lindblad_case_by_name(name)
    e = ensemble_for(case, seed=430 + len(name), members=M)
    rng = np.random.default_rng(431)
    u = 0.4 * rng.standard_normal((B, case.Nc, case.K))
    if case.complex_controls:
        u = u + 0.4j * rng.standard_normal((B, case.Nc, case.K))
    engine = RecordingEngine(0)
    try:
        ev = make_evaluator(case, e, engine, **kw)
        errors, grads, finals, _ = ev.evaluate_batch(u)
        members = ev.member_errors()
        a, pkw = engine.last_problem
        items = expand(e, gh.real_controls(case, u))
        outs = []
        for m in range(M):
            args = list(a)
            args[8] = e.rate_scales[m] * np.asarray(a[8])
            Engine.set_lindblad_problem(engine, *args, **pkw)
            outs.append(engine.evaluate_lindblad(items[:, m]))
    finally:
        engine.close()
    plain = tuple(np.stack([o[i] for o in outs], axis=1) for i in range(3))
    _RUNS[key] = dict(case=case, e=e, u=u, items=items, errors=errors, grads=grads, finals=finals,
                      members=members, plain=plain, problem=(a, pkw))
    return _RUNS[key]


@pytest.mark.parametrize("name,kw", [
    ("lindblad_n4", {}), ("lindblad_wc_n16", {}), ("lindblad_n4_complex", {}),
    ("lindblad_n4", dict(interpolation_policy=InterpolationPolicy.PIECEWISE_CONSTANT))])
def test_the_evaluator_returns_the_members_of_the_engine(name, kw):
    r = evaluator_run(name, **kw)
    case, e = r["case"], r["e"]
    assert r["problem"][1].get("fixed_subdivision", 0) == 0
    assert r["problem"][1]["interpolation"] == ("piecewise_constant" if kw else "linear")
    p_cost, p_grads, p_final = r["plain"]
    assert np.array_equal(r["members"], p_cost) and np.array_equal(r["finals"], p_final)
    kr = p_grads.shape[-1] - e.perturbation_count
    scales = e.real_channel_scales(case.K, case.complex_controls)
    want_cost, want_grads = folded(
        HamiltonianEnsemble(e.hamiltonian, control_scales=scales, weights=e.weights), p_cost, p_grads)
    assert want_grads.shape[-1] == kr
    assert np.array_equal(r["errors"], want_cost)
    assert np.array_equal(r["grads"], gh.complex_grads(case, want_grads))


@pytest.mark.parametrize("name", ["lindblad_n4", "lindblad_wc_n16"])
def test_members_match_the_device_model_and_the_reference_integrator(name):
    """(b) Every member against the reference integrator at both sizes. Against tests/lindblad_model.py:
    every member at n = 4; at n = 16 the last member only - the NumPy model takes seconds per member
    there, and the other two are held bit for bit to the plain problem with their rates
    (test_the_evaluator_returns_the_members_of_the_engine), the device code this member runs too."""
    r = evaluator_run(name)
    case, e, u, items = r["case"], r["e"], r["u"], r["items"]
    final, members, p_grads = r["finals"], r["members"], r["plain"][1]
    costs = [getattr(ol, k)(**kw) for k, kw in case.cost_specs]
    b = 1
    # (the model takes seconds per member at n = 16: there the last member, every member at n = 4;
    # the reference integrator on every member of both)
    for m in range(M):
        if case.n < 16 or m == M - 1:
            system = lm.StructuredLindblad(
                case.h0, gh.lindblad_generators(case) + list(e.perturbations),
                e.rate_scales[m] * case.dissipators, case.operators)
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
            lindblad_data=e.member_lindblad_data(m, case.lindblad_data()),
            control_eval_count=case.Nc, costs=costs, cost_eval_step=case.cost_eval_step,
            control_count=case.K)
        o_err, o_final = ol.evaluate(problem, u[b])
        print(name, m, "reference:", abs(members[b, m] - o_err), np.max(np.abs(final[b, m] - o_final)))
        assert abs(members[b, m] - o_err) < 1e-9
        assert np.max(np.abs(final[b, m] - o_final)) < 1e-8


# ---- c. the known answer ------------------------------------------------------------------------------

def test_t1_decay_of_every_member():
    """One qubit, no Hamiltonian but a sigma_z drive (it does not move populations), L = sigma_-,
    initial |1><1|: member m's excited population at T is exp(-c_m gamma T)."""
    gamma, T = 2.0, 1.0
    sz = np.diag([1.0, -1.0]).astype(np.complex128)
    sm = np.array([[0, 1], [0, 0]], dtype=np.complex128)
    rho0 = np.zeros((1, 2, 2), dtype=np.complex128)
    rho0[0, 1, 1] = 1
    ground = np.zeros((1, 2, 2), dtype=np.complex128)
    ground[0, 0, 0] = 1
    c = np.array([[0.25], [1.0], [4.0]])
    e = HamiltonianEnsemble(lambda u, t: u[0] * sz, control_scales=np.array([[1.0], [0.9], [1.1]]),
                            weights=np.array([0.2, 0.5, 0.3]), rate_scales=c)
    u = 0.7 * np.random.default_rng(440).standard_normal((4, 1))
    r = qoc_amd.evolve_lindblad_discrete(T, rho0, 5, controls=u, hamiltonian=e,
                                         lindblad_data=lambda t: (np.array([gamma]), np.stack([sm])),
                                         costs=[TargetDensityInfidelity(ground)])
    assert r.final_densities.shape == (3, 1, 2, 2)
    for m in range(3):
        excited = np.exp(-c[m, 0] * gamma * T)
        expected = np.array([[1 - excited, 0], [0, excited]])
        print("T1 member", m, np.max(np.abs(r.final_densities[m, 0] - expected)))
        assert np.max(np.abs(r.final_densities[m, 0] - expected)) < 1e-10
    # the faster a member decays, the closer it is to the ground state
    assert r.member_errors[0] > r.member_errors[1] > r.member_errors[2]
    assert abs(r.error - np.dot(e.weights, r.member_errors)) < 1e-14


# ---- d. sub-division groups ---------------------------------------------------------------------------

def test_members_take_the_subdivision_counts_of_their_own_rates(engine):
    case = cases_mod.lindblad_case_by_name("lindblad_n4")
    case.dissipators = np.array([60.0, 24.0])  # stiff decay: the rates decide the sub-division
    rates = np.array([[0.25, 0.3], [1.0, 1.1], [4.0, 3.6]])
    e = ensemble_for(case, seed=450, J=1, rates=rates)
    u = 0.3 * np.random.default_rng(451).standard_normal((B, case.Nc, case.K))
    items = expand(e, u)
    # the precondition, from the model of the device's rule (lm.StructuredLindblad.norm_bound and
    # lm.substep_grid): the members of each seed take three different sub-division counts
    dt = case.T / (case.N - 1)
    gens = gh.lindblad_generators(case) + list(e.perturbations)
    systems = [lm.StructuredLindblad(case.h0, gens, rates[m] * case.dissipators, case.operators)
               for m in range(M)]
    bounds = np.array([[systems[m].norm_bound(np.max(np.abs(items[b, m]), axis=0))
                        for m in range(M)] for b in range(B)])
    counts = np.ceil(bounds * dt / 0.4).astype(int)
    grids = np.array([[len(lm.substep_grid(case.T, case.N, case.Nc, bounds[b, m])[0])
                       for m in range(M)] for b in range(B)])
    print("sub-division counts", counts.tolist(), "sub-intervals", grids.tolist())
    assert all(len(set(counts[b])) == M for b in range(B)), counts
    assert all(len(set(grids[b])) == M for b in range(B)) and np.all(grids >= counts)
    # (the counts are far apart: a 2 % difference between the model's norm and the engine's power
    # iteration cannot merge two of them)
    assert np.all(counts[:, 1] >= 2 * counts[:, 0]) and np.all(counts[:, 2] >= 2 * counts[:, 1])
    set_problem(engine, case, e, case.dissipators)
    engine.set_lindblad_ensemble(e.control_scales, e.offsets, e.weights)
    engine.set_lindblad_ensemble_rates(rates)
    full = engine.evaluate_lindblad(u) + (engine.lindblad_ensemble_member_costs(),)
    subintervals = engine.lindblad_last_subintervals()
    alone, alone_sub = [], 0
    for b in range(B):
        alone.append(engine.evaluate_lindblad(u[b:b + 1]) + (engine.lindblad_ensemble_member_costs(),))
        alone_sub += engine.lindblad_last_subintervals()
    engine.lindblad_upload_controls(u[::-1])
    engine.eval_lindblad_resident(True)
    resident = engine.lindblad_download_results() + (engine.lindblad_ensemble_member_costs(),)
    engine.set_lindblad_ensemble_rates(None)
    engine.evaluate_lindblad(u)
    shared_sub = engine.lindblad_last_subintervals()
    # every member ran on the grid the plain problem with ITS rates runs on ...
    plain_sub = []
    for m in range(M):
        set_problem(engine, case, e, rates[m] * case.dissipators)
        engine.evaluate_lindblad(items[:, m])
        plain_sub.append(engine.lindblad_last_subintervals())
    assert subintervals == sum(plain_sub) == alone_sub
    assert len(set(plain_sub)) == M and plain_sub[0] < plain_sub[1] < plain_sub[2]
    assert shared_sub != subintervals  # ... not on that of the shared rates
    # ... and no result depends on the batch neighbours
    for b in range(B):
        for x, y in zip(full, alone[b]):
            assert np.array_equal(x[b], y[0])
        for x, y in zip(full, resident):
            assert np.array_equal(x[b], y[B - 1 - b])


# ---- e. degenerate cases ------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [4, 20])
def test_rates_of_one_are_the_ensemble_without_rates(engine, n):
    case = shape_case(n, 2, N=4 if n > 16 else 7, Nc=3 if n > 16 else 4)
    e = ensemble_for(case, seed=460)
    u = 0.5 * np.random.default_rng(461).standard_normal((B, case.Nc, case.K))
    set_problem(engine, case, e, case.dissipators)
    engine.set_lindblad_ensemble(e.control_scales, e.offsets, e.weights)
    without = ensemble_results(engine, u, None)
    ones = ensemble_results(engine, u, np.ones((M, 2)))
    engine.set_lindblad_ensemble_rates(None)   # cleared: the shared tables again
    cleared = ensemble_results(engine, u, None)
    for a, b, c in zip(without, ones, cleared):
        for x, y, z in zip(a, b, c):
            assert np.array_equal(x, y) and np.array_equal(x, z)


@pytest.mark.parametrize("name", ["lindblad_n4", "lindblad_wc_n16"])
def test_one_member_with_unit_rates_is_the_plain_problem(engine, name):
    case = cases_mod.lindblad_case_by_name(name)
    u = np.stack(case.controls)
    gh.setup_lindblad_engine(engine, case)
    plain = engine.evaluate_lindblad(u)
    engine.set_lindblad_ensemble(np.ones((1, case.K)), None, np.ones(1))
    host, resident = ensemble_results(engine, u, np.ones((1, len(case.dissipators))))
    for out in (host, resident):
        assert np.array_equal(out[0], plain[0]) and np.array_equal(out[1], plain[1])
        assert np.array_equal(out[2][:, 0], plain[2]) and out[2].shape[1] == 1
        assert np.array_equal(out[3][:, 0], plain[0])


# ---- f. multi-start GRAPE -----------------------------------------------------------------------------

@pytest.mark.parametrize("optimizer", ["adam", "lbfgs"])
def test_resident_route_equals_the_host_loop(routes, optimizer):  # noqa: F811
    case = cases_mod.lindblad_case_by_name("lindblad_n4")
    case.dissipators = np.array([0.5, 0.2])
    e = ensemble_for(case, seed=470, J=2)
    u0 = np.clip(0.5 * np.random.default_rng(471).standard_normal((B, case.Nc, case.K)), -0.8, 0.8)
    a, _ = multistart(routes, optimizer, case, e, u0, iterations=3, single=False,
                      max_control_norms=np.full(case.K, 0.8))
    assert np.any(a.best_iteration > 0)
    # member_errors are those of the members' own rates: far from the shared-rates ensemble's
    shared = HamiltonianEnsemble(e.hamiltonian, perturbations=e.perturbations, offsets=e.offsets,
                                 control_scales=e.control_scales, weights=e.weights)
    ev = make_evaluator(case, shared, Engine(0))
    try:
        ev.evaluate_batch(np.stack(a.best_controls), want_grad=False)
        assert np.max(np.abs(ev.member_errors() - np.stack(a.member_errors))) > 1e-5
    finally:
        ev.backend.close()


def test_resident_route_with_a_sine_basis_and_a_control_cost_on_the_device(routes):  # noqa: F811
    case = cases_mod.lindblad_case_by_name("lindblad_n4")
    case.dissipators = np.array([0.5, 0.2])
    e = ensemble_for(case, seed=472, J=2)
    basis = ControlBasis.sine(case.Nc, 4)
    c0 = 0.2 * np.random.default_rng(473).standard_normal((B, 4, case.K))
    for b in range(B):
        c0[b] *= min(1.0, 0.75 / np.max(np.abs(basis.expand(c0[b]))))
    variation = ControlVariation(case.K, case.Nc, cost_multiplier=0.4, order=1)
    a, b = multistart(routes, "adam", case, e, c0, iterations=3, single=False, control_basis=basis,
                      max_control_norms=np.full(case.K, 0.8), more_costs=[variation])
    for s in range(B):
        assert rel_err(a.best_coefficients[s], b.best_coefficients[s]) < 1e-10
        once = variation.cost(a.best_controls[s], None, case.N - 1)
        assert once > 0
        assert abs(a.best_error[s] - once - np.dot(e.weights, a.member_errors[s])) < 1e-12


# ---- g. the ABI's rejections --------------------------------------------------------------------------

def test_engine_rejections_and_what_clears_the_rates(engine):
    case = cases_mod.lindblad_case_by_name("lindblad_n4")
    case.dissipators = np.array([0.5, 0.2])
    e = ensemble_for(case, seed=480)
    rates = e.rate_scales
    u = 0.3 * np.random.default_rng(481).standard_normal((B, case.Nc, case.K))

    def refused(code, match, value):
        with pytest.raises(QocxError, match=match) as err:
            engine.set_lindblad_ensemble_rates(value)
        assert err.value.code == code

    set_problem(engine, case, e, case.dissipators)
    refused(-3, "no Lindblad ensemble set", rates)           # QOCX_ERR_STATE: no ensemble
    engine.set_lindblad_ensemble(e.control_scales, e.offsets, e.weights)
    shared = ensemble_results(engine, u, None)
    refused(-1, "members differs", np.ones((M + 1, 2)))      # QOCX_ERR_ARG from here on
    refused(-1, "members differs", np.ones((M - 1, 2)))
    refused(-1, "operators differs", np.ones((M, 1)))
    refused(-1, "operators differs", np.ones((M, 3)))
    for value in (-0.5, np.nan, np.inf):
        bad = rates.copy()
        bad[2, 1] = value
        refused(-1, "finite and >= 0", bad)
    # nothing was set by the refused calls
    for a, b in zip(shared, ensemble_results(engine, u, None)):
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
    # setting rates invalidates resident controls and results
    engine.lindblad_upload_controls(u)
    engine.eval_lindblad_resident(True)
    engine.set_lindblad_ensemble_rates(rates)
    with pytest.raises(QocxError, match="no resident Lindblad controls") as err:
        engine.eval_lindblad_resident(True)
    assert err.value.code == -3
    with pytest.raises(QocxError, match="no evaluation results"):
        engine.lindblad_ensemble_member_costs()
    with_rates = ensemble_results(engine, u, None)
    assert np.max(np.abs(with_rates[0][3] - shared[0][3])) > 1e-6
    engine.set_lindblad_ensemble_rates(rates)                # the second setter may be called again
    for a, b in zip(with_rates, ensemble_results(engine, u, None)):
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
    # a new ensemble clears the rates ...
    engine.set_lindblad_ensemble(e.control_scales, e.offsets, e.weights)
    for a, b in zip(shared, ensemble_results(engine, u, None)):
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
    # ... and so does a new problem (with the ensemble: rates need one again)
    engine.set_lindblad_ensemble_rates(rates)
    set_problem(engine, case, e, case.dissipators)
    refused(-3, "no Lindblad ensemble set", rates)
    engine.set_lindblad_ensemble(e.control_scales, e.offsets, e.weights)
    for a, b in zip(shared, ensemble_results(engine, u, None)):
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
    # a problem with stage tables: QOCX_ERR_STATE
    g = gh.lindblad_generators(case) + list(e.perturbations)
    times = engine.lindblad_stage_times(case.T, case.N, case.Nc, len(g), 4)
    engine.set_lindblad_problem(
        case.n, case.initial_densities.shape[0], len(g), case.Nc, case.N, case.T, case.h0, g,
        case.dissipators, case.operators, case.initial_densities,
        costs=gh.lindblad_device_costs(case), cost_eval_step=case.cost_eval_step,
        fixed_subdivision=4, h0_stages=np.stack([case.h0] * len(times)))
    engine.set_lindblad_ensemble(e.control_scales, e.offsets, e.weights)
    refused(-3, "stage tables", rates)
    cost, _, _ = engine.evaluate_lindblad(u)                 # the ensemble itself still runs
    assert np.all(np.isfinite(cost))
