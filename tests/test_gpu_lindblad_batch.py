"""
GPU tests (-m gpu) of multi-start Lindblad GRAPE (grape_lindblad_discrete_batch) and its
device-resident route (qocx_lindblad_upload_controls / qocx_eval_lindblad_resident /
qocx_lindblad_opt_*): a seed's trajectory does not depend on its batch neighbours, the resident
route equals the host loop bit for bit, and a resident evaluation equals qocx_eval_lindblad on the
same controls bit for bit, whatever sub-division groups the seeds fall into.
"""

import numpy as np
import pytest

import qoc_amd
from qoc_amd.core import batch as batch_mod
from qoc_amd.engine import Engine
from qoc_amd.standard import SGD, Adam
from tests import cases as cases_mod
from tests import gpu_helpers as gh
from tests import helpers
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


def rel_err(a, b):
    return np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(np.max(np.abs(np.asarray(b))), 1e-300)


def problem(case):
    args = (case.K, case.Nc, product_cost_list(case), case.T, case.initial_densities, case.N)
    kw = dict(cost_eval_step=case.cost_eval_step, hamiltonian=case.hamiltonian(),
              lindblad_data=case.lindblad_data(), log_iteration_step=0)
    return args, kw


def starts(case, seeds, sigma, seed, bound=None):
    u = sigma * np.random.default_rng(seed).standard_normal((seeds, case.Nc, case.K))
    return u if bound is None else np.clip(u, -bound, bound)


def assert_same_runs(a, b, seeds):
    assert np.array_equal(a.best_error, b.best_error)
    assert np.array_equal(a.best_iteration, b.best_iteration)
    assert np.array_equal(a.iterations_run, b.iterations_run)
    for s in range(seeds):
        assert np.array_equal(a.best_controls[s], b.best_controls[s])
        assert np.array_equal(a.best_final_densities[s], b.best_final_densities[s])
    assert a.global_best_error == b.global_best_error


def test_resident_batch_equals_single_seed_runs(routes):
    case = cases_mod.lindblad_case_by_name("lindblad_wc_n16")
    u0 = starts(case, 8, 0.8, 91, bound=2.0)
    args, kw = problem(case)
    kw.update(iteration_count=6, max_control_norms=np.full(case.K, 2.0))
    full = qoc_amd.grape_lindblad_discrete_batch(*args, u0.copy(),
                                                 optimizer=Adam(learning_rate=2e-2), **kw)
    assert routes == {"resident": 1, "host": 0}
    for b in range(8):
        one = qoc_amd.grape_lindblad_discrete_batch(*args, u0[b:b + 1].copy(),
                                                    optimizer=Adam(learning_rate=2e-2), **kw)
        assert one.best_error[0] == full.best_error[b]
        assert one.best_iteration[0] == full.best_iteration[b]
        assert np.array_equal(one.best_controls[0], full.best_controls[b])
        assert np.array_equal(one.best_final_densities[0], full.best_final_densities[b])
        ref = qoc_amd.grape_lindblad_discrete(*args, initial_controls=u0[b].copy(),
                                              optimizer=Adam(learning_rate=2e-2), **kw)
        assert ref.best_iteration == full.best_iteration[b]
        assert abs(ref.best_error - full.best_error[b]) < 1e-12
        assert rel_err(full.best_controls[b], ref.best_controls) < 1e-10
    assert routes == {"resident": 9, "host": 0}
    assert np.all(full.iterations_run == 6)
    assert full.best_final_densities[0].shape == case.initial_densities.shape


class PluginAdam(Adam):  # not type(...) is Adam: takes the host loop
    pass


class PluginSGD(SGD):
    pass


@pytest.mark.parametrize("which", ["adam_clip_decay", "sgd"])
def test_resident_route_equals_host_loop(which, routes):
    """Clipping of controls and gradients, learning-rate decay and two seeds stopping early at
    min_error: the resident route and the host loop walk the same trajectories bit for bit."""
    case = cases_mod.lindblad_case_by_name("lindblad_wc_n16")
    u0 = starts(case, 6, 0.9, 92, bound=1.0)
    args, kw = problem(case)
    kw.update(iteration_count=5, max_control_norms=np.full(case.K, 1.0))
    if which == "sgd":
        make = lambda cls: cls(learning_rate=0.7)  # noqa: E731
        resident_opt, host_opt = make(SGD), make(PluginSGD)
    else:
        make = lambda cls: cls(learning_rate=8e-2, clip_grads=0.05, learning_rate_decay=2.5)  # noqa: E731
        resident_opt, host_opt = make(Adam), make(PluginAdam)
    probe = qoc_amd.grape_lindblad_discrete_batch(*args, u0.copy(), optimizer=resident_opt,
                                                  **dict(kw, iteration_count=2))
    threshold = float(np.sort(probe.best_error)[1])  # two seeds stop early
    a = qoc_amd.grape_lindblad_discrete_batch(*args, u0.copy(), optimizer=resident_opt,
                                              min_error=threshold, **kw)
    b = qoc_amd.grape_lindblad_discrete_batch(*args, u0.copy(), optimizer=host_opt,
                                              min_error=threshold, **kw)
    assert routes == {"resident": 2, "host": 1}
    assert_same_runs(a, b, 6)
    assert len(set(a.iterations_run.tolist())) >= 2
    assert np.sum(a.iterations_run < 5) >= 2


@pytest.mark.parametrize("name", ["lindblad_n4", "lindblad_wc_n16"])
def test_resident_evaluation_equals_host_controls_across_subdivision_groups(name):
    case = cases_mod.lindblad_case_by_name(name)
    engine = Engine(0)
    try:
        gh.setup_lindblad_engine(engine, case)
        u = starts(case, 2, 0.4, 93)
        mixed = np.concatenate([u, 4.0 * u, 9.0 * u[:1], u[1:] * 0.0])
        counts = set()
        for s in range(mixed.shape[0]):  # sub-intervals of each seed alone: several groups
            engine.evaluate_lindblad(mixed[s:s + 1])
            counts.add(engine.lindblad_last_subintervals())
        assert len(counts) >= 3
        ref = engine.evaluate_lindblad(mixed)
        engine.lindblad_upload_controls(mixed)
        engine.eval_lindblad_resident(True)
        out = engine.lindblad_download_results()
        for x, y in zip(out, ref):
            assert np.array_equal(x, y)
        assert np.array_equal(engine.lindblad_download_costs(), ref[0])
        # a clip moves the 9x seed to a coarser group: the maxima that come back with it decide
        engine.lindblad_opt_begin()
        norms = np.full(case.K, 1.5 * np.max(np.abs(u)))
        engine.lindblad_opt_clip(norms)
        clipped = mixed.copy()
        qoc_amd.engine.host_clip_controls(clipped, norms)
        engine.eval_lindblad_resident(True)
        out = engine.lindblad_download_results()
        ref = engine.evaluate_lindblad(clipped)
        for x, y in zip(out, ref):
            assert np.array_equal(x, y)
        # a step that updates no seed leaves the controls; the next evaluation, with no clip
        # before it, takes the control maxima on the device
        flags = np.ones(mixed.shape[0], dtype=bool)
        engine.lindblad_opt_step(0, flags, ~flags, 0.5)
        engine.eval_lindblad_resident(True)
        for x, y in zip(engine.lindblad_download_results(), ref):
            assert np.array_equal(x, y)
        best_controls, best_finals = engine.lindblad_opt_download_best()
        assert np.array_equal(best_controls, clipped) and np.array_equal(best_finals, ref[2])
        # without gradients, and controls uploaded again
        engine.lindblad_upload_controls(clipped[::-1])
        engine.eval_lindblad_resident(False)
        cost, _, final = engine.lindblad_download_results(want_grad=False)
        ref = engine.evaluate_lindblad(clipped[::-1], want_grad=False)
        assert np.array_equal(cost, ref[0]) and np.array_equal(final, ref[2])
    finally:
        engine.close()


def test_batch_beyond_the_cu_count(routes):
    """B = 300 runs in pieces of one seed per CU; each seed is the one of a B = 8 run."""
    case = cases_mod.lindblad_case_by_name("lindblad_wc_n16")
    u0 = starts(case, 300, 0.8, 94, bound=2.0)
    args, kw = problem(case)
    kw.update(iteration_count=3, max_control_norms=np.full(case.K, 2.0))
    big = qoc_amd.grape_lindblad_discrete_batch(*args, u0.copy(),
                                                optimizer=Adam(learning_rate=2e-2), **kw)
    for lo in (0, 292):
        small = qoc_amd.grape_lindblad_discrete_batch(*args, u0[lo:lo + 8].copy(),
                                                      optimizer=Adam(learning_rate=2e-2), **kw)
        assert np.array_equal(small.best_error, big.best_error[lo:lo + 8])
        assert np.array_equal(small.best_iteration, big.best_iteration[lo:lo + 8])
        for s in range(8):
            assert np.array_equal(small.best_controls[s], big.best_controls[lo + s])
            assert np.array_equal(small.best_final_densities[s], big.best_final_densities[lo + s])
    assert routes == {"resident": 3, "host": 0}


def test_bench_shape_64_seeds(routes, monkeypatch):
    """BASELINE.json configs[3] (n = 16, 501 evaluation points, two operators, K = 2) with the
    benchmark's 64 seeds: resident, and at a small learning rate no seed's error increases."""
    case = cases_mod.lindblad_case_by_name("lindblad_bench_c4")
    u0 = np.stack([0.1 * np.random.default_rng(1000 + b).standard_normal((case.Nc, case.K))
                   for b in range(64)])
    seen = []
    download = Engine.lindblad_download_costs

    def record(self):
        costs = download(self)
        seen.append(costs.copy())
        return costs
    monkeypatch.setattr(Engine, "lindblad_download_costs", record)
    args, kw = problem(case)
    result = qoc_amd.grape_lindblad_discrete_batch(*args, u0, optimizer=Adam(learning_rate=1e-6),
                                                   iteration_count=3,
                                                   max_control_norms=np.full(case.K, 1.0), **kw)
    assert routes == {"resident": 1, "host": 0}
    assert len(seen) == 3 and np.all(result.iterations_run == 3)
    assert np.all(np.isfinite(seen[0])) and np.all(seen[0] > 0)
    assert np.all(seen[1] <= seen[0]) and np.all(seen[2] <= seen[1])
    assert np.array_equal(result.best_error, seen[2])


def test_time_dependent_resident_equals_host_loop(routes):
    """Fixed sub-division (tables of the time-dependent Hamiltonian): no maxima come back, and the
    resident route equals the host loop."""
    case = cases_mod.lindblad_case_by_name("lindblad_timedep")
    u0 = starts(case, 4, 0.6, 95, bound=1.2)
    args, kw = problem(case)
    kw.update(iteration_count=4, max_control_norms=np.full(case.K, 1.2))
    a = qoc_amd.grape_lindblad_discrete_batch(*args, u0.copy(), optimizer=Adam(learning_rate=5e-2),
                                              **kw)
    b = qoc_amd.grape_lindblad_discrete_batch(*args, u0.copy(),
                                              optimizer=PluginAdam(learning_rate=5e-2), **kw)
    assert routes == {"resident": 1, "host": 1}
    assert_same_runs(a, b, 4)
