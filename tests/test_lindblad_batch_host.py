"""
CPU tests of multi-start Lindblad GRAPE (grape_lindblad_discrete_batch) on its host-loop route:
the GPU engine is replaced by the NumPy model of the device algorithm (tests/oracle_backend.py),
which evaluates a batch seed by seed, so every seed must equal grape_lindblad_discrete from the
same start exactly. The device-resident route runs in tests/test_gpu_lindblad_batch.py.
"""

import os
import socket
import sys

import numpy as np
import pytest

import qoc_amd
from qoc_amd import parallel
from qoc_amd.core.lindbladdiscrete import GrapeLindbladBatchResult
from qoc_amd.models import GrapeLindbladResult
from qoc_amd.standard import SGD, Adam, LBFGSB
from tests import cases as cases_mod
from tests import helpers
from tests.oracle_backend import OracleBackend
from tests.test_lindblad_host_api import product_cost_list

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def oracle_engine():
    helpers.set_backend_factory(OracleBackend)
    yield
    helpers.set_backend_factory(None)


def starts(case, seeds, sigma=0.3, seed=321):
    rng = np.random.default_rng(seed)
    shape = (seeds, case.Nc, case.K)
    u = sigma * rng.standard_normal(shape)
    if case.complex_controls:
        u = u + 1j * sigma * rng.standard_normal(shape)
    return u


def problem_args(case):
    return (case.K, case.Nc, product_cost_list(case), case.T, case.initial_densities, case.N)


def problem_kw(case, **kw):
    out = dict(complex_controls=case.complex_controls, cost_eval_step=case.cost_eval_step,
               hamiltonian=case.hamiltonian(), lindblad_data=case.lindblad_data())
    out.update(kw)
    return out


def assert_seeds_equal_single_runs(case, u0, batch, make_optimizer, **kw):
    for b in range(u0.shape[0]):
        single = qoc_amd.grape_lindblad_discrete(
            *problem_args(case), initial_controls=u0[b].copy(), optimizer=make_optimizer(),
            **problem_kw(case, log_iteration_step=0, **kw))
        assert batch.best_error[b] == single.best_error
        assert batch.best_iteration[b] == single.best_iteration
        assert np.array_equal(batch.best_controls[b], single.best_controls)
        assert np.array_equal(batch.best_final_densities[b], single.best_final_densities)


@pytest.mark.parametrize("name", ["lindblad_n4", "lindblad_n4_complex"])
def test_batch_equals_independent_single_runs(name, capsys):
    case = cases_mod.lindblad_case_by_name(name)
    u0 = starts(case, 3)
    kw = dict(iteration_count=5, max_control_norms=np.full(case.K, 2.0))
    batch = qoc_amd.grape_lindblad_discrete_batch(
        *problem_args(case), u0.copy(), optimizer=Adam(learning_rate=3e-2),
        **problem_kw(case, log_iteration_step=2, **kw))
    out = capsys.readouterr().out.splitlines()
    assert out[0].startswith("iter   |  summed error")
    assert [line.split("|")[0].strip() for line in out[2:]] == ["0", "2", "4"]
    assert isinstance(batch, GrapeLindbladBatchResult)
    assert_seeds_equal_single_runs(case, u0, batch, lambda: Adam(learning_rate=3e-2), **kw)
    assert np.all(batch.iterations_run == 5)
    assert batch.best_final_densities[0].shape == case.initial_densities.shape
    assert np.iscomplexobj(batch.best_controls[0]) == case.complex_controls
    best = batch.best
    assert isinstance(best, GrapeLindbladResult)
    assert best.best_error == np.min(batch.best_error)
    assert batch.global_best_error == best.best_error


def test_batch_per_seed_termination_clipping_conditions_and_errors():
    case = cases_mod.lindblad_case_by_name("lindblad_n4")
    u0 = starts(case, 4, sigma=0.2)

    def conditions(controls):
        controls[0, :] = 0
        return controls

    base = problem_kw(case, max_control_norms=np.full(case.K, 1.0), log_iteration_step=0,
                      impose_control_conditions=conditions)
    args = problem_args(case)
    ref = qoc_amd.grape_lindblad_discrete_batch(*args, u0.copy(), iteration_count=3,
                                                optimizer=SGD(learning_rate=50.0), **base)
    # a seed whose first error is below min_error stops at once, the others carry on
    threshold = float(np.sort(ref.best_error)[1]) + 1.0  # generous: at least two seeds stop early
    early = qoc_amd.grape_lindblad_discrete_batch(*args, u0.copy(), iteration_count=3,
                                                  optimizer=SGD(learning_rate=50.0),
                                                  min_error=threshold, **base)
    assert np.all(early.iterations_run >= 1) and np.any(early.iterations_run == 1)
    for b in range(4):
        assert np.all(early.best_controls[b][0] == 0)
        assert np.max(np.abs(early.best_controls[b])) <= 1.0 + 1e-12
        assert np.all(ref.best_controls[b][0] == 0)
        assert np.max(np.abs(ref.best_controls[b])) <= 1.0
    for b in np.nonzero(early.iterations_run == 1)[0]:
        assert early.best_iteration[b] == 0
    assert_seeds_equal_single_runs(case, u0, early, lambda: SGD(learning_rate=50.0),
                                   iteration_count=3, min_error=threshold,
                                   max_control_norms=np.full(case.K, 1.0),
                                   impose_control_conditions=conditions)
    with pytest.raises(ValueError):
        qoc_amd.grape_lindblad_discrete_batch(*args, u0[0], **base)
    with pytest.raises(NotImplementedError):
        qoc_amd.grape_lindblad_discrete_batch(*args, u0.copy(), optimizer=LBFGSB(), **base)
    with pytest.raises(ValueError):  # initial controls beyond max_control_norms
        qoc_amd.grape_lindblad_discrete_batch(*args, 10 * u0, **base)


@pytest.mark.parametrize("name", ["lindblad_timedep", "lindblad_opaque_wc"])
def test_host_loop_route_time_dependent_and_nonlinear(name):
    """A time-dependent Hamiltonian (sampled tables, fixed sub-division) and a Hamiltonian that is
    not linear in the controls (its tangent per control array) run through the host loop."""
    case = cases_mod.lindblad_case_by_name(name)
    u0 = np.clip(starts(case, 3, sigma=0.4, seed=9), -1.0, 1.0)
    kw = dict(iteration_count=4, max_control_norms=np.full(case.K, 1.5))
    batch = qoc_amd.grape_lindblad_discrete_batch(
        *problem_args(case), u0.copy(), optimizer=Adam(learning_rate=5e-2),
        **problem_kw(case, log_iteration_step=0, **kw))
    assert_seeds_equal_single_runs(case, u0, batch, lambda: Adam(learning_rate=5e-2), **kw)
    assert np.all(batch.iterations_run == 4)


def test_oracle_backend_takes_the_host_loop():
    """The resident route needs the engine's lindblad_opt_* entry points; the NumPy model has none."""
    from qoc_amd.core import device
    case = cases_mod.lindblad_case_by_name("lindblad_wc_n4")
    ev = device.LindbladEvaluator(case.T, case.initial_densities, case.N,
                                  hamiltonian=case.hamiltonian(), lindblad_data=case.lindblad_data(),
                                  control_count=case.K, control_eval_count=case.Nc,
                                  costs=product_cost_list(case))
    assert not ev.resident_capable()

    class FakeResident(OracleBackend):
        def lindblad_opt_step(self, *args, **kwargs):
            raise AssertionError("not called here")
    ev = device.LindbladEvaluator(case.T, case.initial_densities, case.N,
                                  hamiltonian=case.hamiltonian(), lindblad_data=case.lindblad_data(),
                                  control_count=case.K, control_eval_count=case.Nc,
                                  costs=product_cost_list(case), backend=FakeResident())
    assert ev.resident_capable()


# ---- the seed axis sharded over two ranks (gloo stands in for the RCCL communicator) -------------

def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _shard_inputs():
    case = cases_mod.lindblad_case_by_name("lindblad_n4")
    return case, starts(case, 5, sigma=0.3, seed=44)


def _run_sharded(case, u0, comm):
    return qoc_amd.grape_lindblad_discrete_batch(
        *problem_args(case), u0.copy(), optimizer=Adam(learning_rate=3e-2), comm=comm,
        **problem_kw(case, log_iteration_step=0, iteration_count=3,
                     max_control_norms=np.full(case.K, 2.0)))


def _rank_main(rank, world, port, out_dir):
    sys.path.insert(0, ROOT)
    import torch
    import torch.distributed as dist
    from tests import helpers as rank_helpers
    from tests.oracle_backend import OracleBackend as RankBackend

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank),
                      WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)

    class GlooComm(object):
        def __init__(self):
            self.rank, self.world = rank, world

        def _reduce(self, array, op):
            t = torch.from_numpy(np.array(array, dtype=np.float64))
            dist.all_reduce(t, op=op)
            return t.numpy()

        def allreduce_sum(self, array):
            return self._reduce(array, dist.ReduceOp.SUM)

        def allreduce_max(self, array):
            return self._reduce(array, dist.ReduceOp.MAX)

        def barrier(self):
            dist.barrier()

    rank_helpers.set_backend_factory(RankBackend)
    case, u0 = _shard_inputs()
    res = _run_sharded(case, u0, GlooComm())
    np.savez(os.path.join(out_dir, "rank%d.npz" % rank), best_error=res.best_error,
             best_iteration=res.best_iteration, controls=np.stack(res.best_controls),
             finals=np.stack(res.best_final_densities), iterations=res.iterations_run,
             global_best=res.global_best_error)
    dist.destroy_process_group()


def test_sharded_over_two_ranks_equals_one_rank(tmp_path):
    import torch.multiprocessing as mp
    world, port = 2, _free_port()
    mp.spawn(_rank_main, args=(world, port, str(tmp_path)), nprocs=world, join=True)
    case, u0 = _shard_inputs()
    one = _run_sharded(case, u0, None)
    for r in range(world):
        lo, hi = parallel.shard_bounds(u0.shape[0], r, world)
        out = np.load(os.path.join(str(tmp_path), "rank%d.npz" % r))
        assert np.array_equal(out["best_error"], one.best_error[lo:hi])
        assert np.array_equal(out["best_iteration"], one.best_iteration[lo:hi])
        assert np.array_equal(out["iterations"], one.iterations_run[lo:hi])
        assert np.array_equal(out["controls"], np.stack(one.best_controls[lo:hi]))
        assert np.array_equal(out["finals"], np.stack(one.best_final_densities[lo:hi]))
        assert float(out["global_best"]) == one.global_best_error
