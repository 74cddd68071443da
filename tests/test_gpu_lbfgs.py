"""
GPU tests (-m gpu) of LBFGS in the device-resident multi-start drivers (qocx_opt_lbfgs_* /
qocx_lindblad_opt_lbfgs_*, qoc_amd/csrc/qocx_lbfgs.hip): the resident route walks the host loop's
trajectory bit for bit - the host loop being qoc_amd/standard/optimizers/lbfgs.py, one state
machine per seed, forced by a trivial subclass of LBFGS - and a seed does not depend on the batch
it is part of. Small problems (n <= 16, <= 50 system steps, <= 8 seeds); the parameter counts cover
P < 256 (threads of the workgroup without an element), P = 771 (no multiple of 256, several
elements per thread) and a history ring that wraps.

The two routes are compared under clip bounds that the start controls reach (max_control_norms at
the scale of the controls, as in tests/test_gpu_api.py and its kin): the resident route derives the
evaluation's norm bound - and from it the kernel variants - from max_control_norms alone, the host
loop from the controls it uploads, so under a wide clip the two routes' EVALUATIONS differ in
rounding (tests/test_gpu_mixed_steps.py::test_resident_route_after_clip), whatever the optimizer.
test_step_kernel_equals_update_in_lock_step takes the evaluation out of the comparison: one
resident run, every (parameters, error, gradients) triple read back and fed to LBFGS.update on the
host, every trial point compared.
"""

import numpy as np
import pytest

import qoc_amd
import qoc_amd.standard.costs as product_costs
from qoc_amd.core import batch as batch_mod
from qoc_amd.standard import LBFGS, QuadraticHamiltonian
from qoc_amd.standard.costs import ControlNorm, ControlVariation
from tests import cases as cases_mod
from tests import helpers
from tests.test_gpu_ensemble import transmon_ensemble
from tests.test_gpu_quadratic_hamiltonian import shaped_problem
from tests.test_lindblad_host_api import product_cost_list as lindblad_cost_list

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


class HostLBFGS(LBFGS):  # not type(...) is LBFGS: one clone per seed on the host loop
    pass


def both_routes(run, args, u0, routes, options=None, **kw):
    options = options or {}
    kw = dict(dict(iteration_count=6, log_iteration_step=0), **kw)
    before = dict(routes)
    a = run(*args, u0.copy(), optimizer=LBFGS(**options), **kw)
    assert routes == {"resident": before["resident"] + 1, "host": before["host"]}
    b = run(*args, u0.copy(), optimizer=HostLBFGS(**options), **kw)
    assert routes == {"resident": before["resident"] + 1, "host": before["host"] + 1}
    return a, b


def assert_same_runs(a, b, finals="best_final_states"):
    seeds = len(a.best_error)
    for s in range(seeds):
        print("seed {}: best_error {!r} / {!r}, iteration {} / {}, run {} / {}".format(
            s, a.best_error[s], b.best_error[s], a.best_iteration[s], b.best_iteration[s],
            a.iterations_run[s], b.iterations_run[s]))
    assert np.array_equal(a.best_error, b.best_error)
    assert np.array_equal(a.best_iteration, b.best_iteration)
    assert np.array_equal(a.iterations_run, b.iterations_run)
    for s in range(seeds):
        assert np.array_equal(a.best_controls[s], b.best_controls[s])
        assert np.array_equal(getattr(a, finals)[s], getattr(b, finals)[s])


def schroedinger_problem(n=8, N=21, Nc=10, K=2, h_seed=41):
    case = cases_mod.case_random("lbfgs", n, N, 1, h_seed, S=2, K=K, Nc=Nc, dt=0.3,
                                 full_unitary=True)
    costs = [getattr(product_costs, kind)(**kw) for kind, kw in case.cost_specs]
    return (case.K, case.Nc, costs, case.T, case.hamiltonian(), case.initial_states, case.N)


def starts(args, seeds, sigma, seed, bound=None):
    u = sigma * np.random.default_rng(seed).standard_normal((seeds, args[1], args[0]))
    return u if bound is None else np.clip(u, -bound, bound)


def test_real_controls_below_one_workgroup_with_the_clip_engaged(routes):
    """P = 20 < 256; the unit first step takes entries beyond max_control_norms = 0.5, so the
    accepted steps are the clipped ones."""
    args = schroedinger_problem()
    u0 = starts(args, 6, 0.4, 11, bound=0.5)
    a, b = both_routes(qoc_amd.grape_schroedinger_discrete_batch, args, u0, routes,
                       max_control_norms=np.full(args[0], 0.5), iteration_count=8)
    assert_same_runs(a, b)
    assert np.any(a.best_iteration > 0)
    at_bound = sum(int(np.sum(np.abs(c) == 0.5)) for c, it in zip(a.best_controls, a.best_iteration)
                   if it > 0)
    assert at_bound > 0  # the clip acted on best controls that came out of an update
    assert all(np.max(np.abs(c)) <= 0.5 for c in a.best_controls)


def test_parameter_count_above_and_no_multiple_of_the_workgroup(routes):
    """Nc = 257, K = 3: P = 771 = 3 * 256 + 3."""
    args = schroedinger_problem(n=6, N=41, Nc=257, K=3, h_seed=42)
    u0 = starts(args, 4, 0.3, 12, bound=0.6)
    a, b = both_routes(qoc_amd.grape_schroedinger_discrete_batch, args, u0, routes,
                       max_control_norms=np.full(3, 0.6), iteration_count=7)
    assert_same_runs(a, b)
    assert np.all(a.best_iteration > 0)


def test_history_ring_wraps(routes):
    args = schroedinger_problem(h_seed=43)
    u0 = starts(args, 4, 0.3, 13, bound=0.6)
    a, b = both_routes(qoc_amd.grape_schroedinger_discrete_batch, args, u0, routes,
                       options=dict(history=3), max_control_norms=np.full(args[0], 0.6),
                       iteration_count=14)
    assert_same_runs(a, b)
    # improvements well past the fourth pair (the lock-step test below counts the accepted steps)
    assert np.all(a.best_iteration >= 5)


def test_complex_controls(routes):
    n, K, N, Nc, B = 12, 2, 31, 10, 4
    rng = np.random.default_rng(704)
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
    args = (K, Nc, [product_costs.TargetStateInfidelity(target)], 0.3 * (N - 1), hamiltonian,
            psi0, N)
    u0 = 0.3 * (rng.standard_normal((B, Nc, K)) + 1j * rng.standard_normal((B, Nc, K)))
    a, b = both_routes(qoc_amd.grape_schroedinger_discrete_batch, args, u0, routes,
                       complex_controls=True, max_control_norms=np.full(K, 10.0),
                       iteration_count=8)
    assert_same_runs(a, b)
    assert np.all(a.best_iteration > 0)
    assert all(np.iscomplexobj(c) and c.shape == (Nc, K) for c in a.best_controls)


def test_built_in_control_costs(routes):
    """ControlNorm and ControlVariation on the device (resident) and through their Python classes
    (host loop)."""
    args = schroedinger_problem(h_seed=44)
    K, Nc = args[0], args[1]
    mx = np.full(K, 0.6)
    costs = args[2] + [ControlNorm(K, Nc, cost_multiplier=0.5, max_control_norms=mx),
                       ControlVariation(K, Nc, cost_multiplier=0.4, order=1)]
    args = args[:2] + (costs,) + args[3:]
    u0 = starts(args, 4, 0.3, 14, bound=0.6)
    a, b = both_routes(qoc_amd.grape_schroedinger_discrete_batch, args, u0, routes,
                       max_control_norms=mx, iteration_count=6)
    assert_same_runs(a, b)


def test_quadratic_hamiltonian(routes):
    p = shaped_problem(12, False, seed=5, N=31, Nc=10)
    args = (p["K"], 10, p["costs"], p["T"], QuadraticHamiltonian(p["linear"], p["terms"]),
            p["psi0"], 31)
    u0 = starts(args, 4, 0.6, 15, bound=1.0)
    a, b = both_routes(qoc_amd.grape_schroedinger_discrete_batch, args, u0, routes,
                       max_control_norms=np.full(p["K"], 1.0))
    assert_same_runs(a, b)


def test_hamiltonian_ensemble_of_three(routes):
    K, N, Nc, S, T, n = 3, 31, 10, 2, 1.5, 12
    e, rng = transmon_ensemble(n, K, M=3, J=1, seed=5, complex_controls=False)
    psi0 = cases_mod.column_states(np.eye(n)[:, :S])
    target = cases_mod.column_states(cases_mod.random_unitary(rng, n)[:, :S])
    args = (K, Nc, [product_costs.TargetStateInfidelity(target)], T, e, psi0, N)
    u0 = starts(args, 4, 0.6, 93, bound=1.0)
    a, b = both_routes(qoc_amd.grape_schroedinger_discrete_batch, args, u0, routes,
                       max_control_norms=np.full(K, 1.0))
    assert_same_runs(a, b)
    for s in range(4):
        assert a.best_final_states[s].shape == (3, S, n, 1)
        assert np.array_equal(a.member_errors[s], b.member_errors[s])


def lindblad_problem():
    case = cases_mod.lindblad_case_by_name("lindblad_wc_n16")
    args = (case.K, case.Nc, lindblad_cost_list(case), case.T, case.initial_densities, case.N)
    kw = dict(cost_eval_step=case.cost_eval_step, hamiltonian=case.hamiltonian(),
              lindblad_data=case.lindblad_data(), max_control_norms=np.full(case.K, 2.0))
    return args, kw


def test_lindblad(routes):
    args, kw = lindblad_problem()
    u0 = starts(args, 6, 0.8, 91, bound=2.0)
    a, b = both_routes(qoc_amd.grape_lindblad_discrete_batch, args, u0, routes, **kw)
    assert_same_runs(a, b, finals="best_final_densities")
    assert np.any(a.best_iteration > 0)


def test_two_seeds_stopped_by_min_error(routes):
    args = schroedinger_problem(h_seed=45)
    u0 = starts(args, 6, 0.3, 16, bound=0.6)
    kw = dict(max_control_norms=np.full(args[0], 0.6), log_iteration_step=0)
    probe = qoc_amd.grape_schroedinger_discrete_batch(*args, u0.copy(), optimizer=LBFGS(),
                                                      iteration_count=4, **kw)
    threshold = float(np.sort(probe.best_error)[1])  # two seeds are there after <= 4 iterations
    a, b = both_routes(qoc_amd.grape_schroedinger_discrete_batch, args, u0, routes,
                       min_error=threshold, iteration_count=8, **kw)
    assert_same_runs(a, b)
    assert np.sum(a.iterations_run < 8) >= 2 and np.sum(a.iterations_run == 8) >= 1


def test_seeds_finish(routes):
    """first_step = 1e3 with one backtrack: the first trials sit at the bounds of the clip; a seed
    that finds no decrease there is finished, is back at its accepted point and stops counting."""
    args = schroedinger_problem(h_seed=46)
    u0 = starts(args, 8, 0.3, 17, bound=0.6)
    a, b = both_routes(qoc_amd.grape_schroedinger_discrete_batch, args, u0, routes,
                       options=dict(first_step=1e3, max_backtracks=1),
                       max_control_norms=np.full(args[0], 0.6), iteration_count=8)
    assert_same_runs(a, b)
    assert np.any(a.iterations_run < 8)  # a seed finished
    for s in np.nonzero(a.iterations_run < 8)[0]:
        assert a.iterations_run[s] >= 3  # the first evaluation and two rejected trials


def test_a_seed_does_not_depend_on_its_batch(routes):
    args = schroedinger_problem(n=6, N=41, Nc=257, K=3, h_seed=42)
    u0 = starts(args, 8, 0.3, 18, bound=0.6)
    kw = dict(max_control_norms=np.full(3, 0.6), iteration_count=6, log_iteration_step=0)
    full = qoc_amd.grape_schroedinger_discrete_batch(*args, u0.copy(), optimizer=LBFGS(), **kw)
    for s in (0, 3, 7):
        one = qoc_amd.grape_schroedinger_discrete_batch(*args, u0[s:s + 1].copy(),
                                                        optimizer=LBFGS(), **kw)
        assert one.best_error[0] == full.best_error[s]
        assert one.best_iteration[0] == full.best_iteration[s]
        assert one.iterations_run[0] == full.iterations_run[s]
        assert np.array_equal(one.best_controls[0], full.best_controls[s])
        assert np.array_equal(one.best_final_states[0], full.best_final_states[s])
    assert routes == {"resident": 4, "host": 0}
    args, kw = lindblad_problem()
    u0 = starts(args, 8, 0.8, 91, bound=2.0)
    kw.update(iteration_count=5, log_iteration_step=0)
    full = qoc_amd.grape_lindblad_discrete_batch(*args, u0.copy(), optimizer=LBFGS(), **kw)
    one = qoc_amd.grape_lindblad_discrete_batch(*args, u0[5:6].copy(), optimizer=LBFGS(), **kw)
    assert one.best_error[0] == full.best_error[5]
    assert np.array_equal(one.best_controls[0], full.best_controls[5])
    assert np.array_equal(one.best_final_densities[0], full.best_final_densities[5])


@pytest.mark.parametrize("which", ["real_771_history_3", "complex", "finish"])
def test_step_kernel_equals_update_in_lock_step(which):
    """One resident run under a wide clip; after every evaluation its costs, gradients
    and evaluated parameters come back and go through LBFGS.update on the host: the kernel's next
    trial point - what the next evaluation ran on - and its finished flags equal the host's, bit
    for bit. The evaluation is the same on both sides by construction."""
    from qoc_amd.engine import Engine
    from tests import gpu_helpers as gh
    options = dict(history=3) if which == "real_771_history_3" else {}
    if which == "finish":
        options = dict(first_step=1e3, max_backtracks=1)
    bound = 4.0
    if which == "complex":
        case, B, iterations = cases_mod.case_by_name("small_complex_M2"), 3, 9
    elif which == "finish":  # the problem, starts and clip of test_seeds_finish
        case = cases_mod.case_random("lbfgs", 8, 21, 1, 46, S=2, K=2, Nc=10, dt=0.3,
                                     full_unitary=True)
        B, iterations, bound = 8, 5, 0.6
    else:
        case = cases_mod.case_random("lbfgs", 6, 41, 1, 42, S=2, K=3, Nc=257, dt=0.3,
                                     full_unitary=True)
        B, iterations = 4, 12
    rng = np.random.default_rng(17 if which == "finish" else 19)
    u0 = np.clip(0.3 * rng.standard_normal((B, case.Nc, case.K)), -bound, bound)
    if case.complex_controls:
        u0 = u0 + 0.3j * rng.standard_normal((B, case.Nc, case.K))

    def flat(device_array):  # [Nc, channels] of the device -> the optimizer's parameter vector
        host = gh.complex_grads(case, device_array).reshape(-1)
        return np.hstack((host.real, host.imag)) if case.complex_controls else host

    engine = Engine(0)
    try:
        gh.setup_engine(engine, case)
        engine.upload_controls(gh.real_controls(case, u0))
        (engine.opt_begin_complex if case.complex_controls else engine.opt_begin)()
        engine.opt_lbfgs_begin(LBFGS(**options).history)
        seeds = [LBFGS(**options) for _ in range(B)]
        ones, expect = np.ones(B, dtype=bool), None
        for _ in range(iterations):
            engine.opt_clip(np.full(case.K, bound))
            engine.eval_resident(True)
            cost, grads, _ = engine.download_results(True, False)
            o = seeds[0]
            finished = engine.opt_lbfgs_step(ones, ones, o.first_step, o.armijo, o.shrink,
                                             o.max_backtracks)
            evaluated, _ = engine.opt_download_best()  # (every seed `improved`: what was evaluated)
            got = np.stack([flat(evaluated[b]) for b in range(B)])
            if expect is not None and case.complex_controls:
                assert np.max(np.abs(gh.complex_grads(case, evaluated))) < bound  # no clip acted
                assert np.array_equal(got, expect)
            elif expect is not None:  # (real controls are clipped in place: +-bound exactly)
                assert np.array_equal(got, np.clip(expect, -bound, bound))
            expect = np.stack([seeds[b].update(flat(grads[b]), got[b], cost[b]) for b in range(B)])
            assert np.array_equal(finished, [s.finished for s in seeds])
        accepted = [s.accepted for s in seeds]
        if which == "finish":  # finished seeds kept their first point; the others went on
            assert any(s.finished for s in seeds) and not all(s.finished for s in seeds)
            assert all(s.accepted == 1 for s in seeds if s.finished)
        else:
            assert min(accepted) > (2 * 3 if which == "real_771_history_3" else 3)
            assert not any(s.finished for s in seeds)
    finally:
        engine.close()


def test_engine_rejects_bad_history_and_missing_begin():
    from qoc_amd.engine import Engine, QocxError
    from tests import gpu_helpers as gh
    case = cases_mod.lindblad_case_by_name("lindblad_n4")
    engine = Engine(0)
    try:
        gh.setup_lindblad_engine(engine, case)
        engine.lindblad_upload_controls(0.1 * np.ones((2, case.Nc, case.K)))
        engine.lindblad_opt_begin()
        for history in (0, 65):
            with pytest.raises(QocxError):
                engine.lindblad_opt_lbfgs_begin(history)
        engine.eval_lindblad_resident(True)
        flags = np.ones(2, dtype=bool)
        with pytest.raises(QocxError):  # no lbfgs_begin for this batch
            engine.lindblad_opt_lbfgs_step(flags, flags, 1.0, 1e-4, 0.5, 20)
        engine.lindblad_opt_lbfgs_begin(64)
        finished = engine.lindblad_opt_lbfgs_step(flags, flags, 1.0, 1e-4, 0.5, 20)
        assert finished.shape == (2,) and not finished.any()
    finally:
        engine.close()
