"""
CPU tests of LBFGS (qoc_amd/standard/optimizers/lbfgs.py): the per-seed state machine on known
functions and against a plain list-based restatement of the algorithm, and its way through the
multi-start drivers' host loop with the oracle backend (tests/oracle_backend.py). The
device-resident route runs in tests/test_gpu_lbfgs.py.
"""

import os
import re

import numpy as np
import pytest

import qoc_amd
from qoc_amd import engine
from qoc_amd.core import batch as batch_mod
from qoc_amd.models import MagnusPolicy
from qoc_amd.standard import LBFGS, Adam
from qoc_amd.standard.optimizers import lbfgs as lbfgs_mod
from tests import cases as cases_mod
from tests import helpers
from tests.oracle_backend import OracleBackend
from tests.test_host_api import product_cost_list
from tests.test_lindblad_host_api import product_cost_list as lindblad_cost_list

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def oracle_engine():
    helpers.set_backend_factory(OracleBackend)
    yield
    helpers.set_backend_factory(None)


# ---- the state machine on known functions --------------------------------------------------------

def quadratic():
    """P = 12, eigenvalues logspace(0, 2, 12) in a random orthogonal basis, and a start."""
    rng = np.random.default_rng(0)
    basis, _ = np.linalg.qr(rng.standard_normal((12, 12)))
    matrix = basis @ np.diag(np.logspace(0, 2, 12)) @ basis.T
    matrix = 0.5 * (matrix + matrix.T)
    start = rng.standard_normal(12)
    return (lambda x: 0.5 * x @ matrix @ x), (lambda x: matrix @ x), start


def rosenbrock(x):
    return float(np.sum(100.0 * (x[1:] - x[:-1] ** 2) ** 2 + (1 - x[:-1]) ** 2))


def rosenbrock_grad(x):
    g = np.zeros_like(x)
    g[:-1] = -400.0 * x[:-1] * (x[1:] - x[:-1] ** 2) - 2 * (1 - x[:-1])
    g[1:] += 200.0 * (x[1:] - x[:-1] ** 2)
    return g


def drive(opt, f, grad, start, evaluations):
    """Feeds `evaluations` evaluations to opt.update; the record of every one:
    (params, error, grads, accepted, x, f, g, d, t of the state BEFORE the update)."""
    p = start.copy()
    record = []
    for _ in range(evaluations):
        fp, gp = f(p), grad(p)
        before = (None if opt.x is None else opt.x.copy(), opt.f,
                  None if opt.g is None else opt.g.copy())
        accepted_before = opt.accepted
        nxt = opt.update(gp, p, fp)
        record.append(dict(p=p.copy(), fp=fp, gp=gp, before=before,
                           accepted=opt.accepted > accepted_before,
                           x=opt.x.copy(), f=opt.f, g=opt.g.copy(), d=opt.d.copy(), t=opt.t))
        p = nxt
        if opt.finished:
            break
    return record


def test_dot_runs_in_the_defined_order():
    rng = np.random.default_rng(5)
    for count in (1, 7, 256, 257, 771, 4000):
        a, b = rng.standard_normal(count), rng.standard_normal(count)
        partial = [0.0] * 256
        for i in range(count):  # lane l: elements l, l + 256, ... in increasing index
            partial[i % 256] = partial[i % 256] + float(a[i]) * float(b[i])
        stride = 128
        while stride:
            for lane in range(stride):
                partial[lane] = partial[lane] + partial[lane + stride]
            stride //= 2
        assert lbfgs_mod.dot(a, b) == partial[0]
        assert abs(lbfgs_mod.dot(a, b) - a @ b) <= 1e-13 * np.sum(np.abs(a * b))


def test_convex_quadratic():
    f, grad, start = quadratic()
    opt = LBFGS()
    record = drive(opt, f, grad, start, 60)
    g0 = np.linalg.norm(grad(start))
    assert np.linalg.norm(opt.g) <= 1e-6 * g0
    accepted = [r for r in record if r["accepted"]]
    errors = [r["fp"] for r in accepted]
    assert len(accepted) > 8
    assert all(later <= earlier for earlier, later in zip(errors, errors[1:]))
    for r in accepted[1:]:  # the Armijo inequality of every accepted step, in the state before it
        x, fx, gx = r["before"]
        assert r["fp"] <= fx + opt.armijo * lbfgs_mod.dot(gx, r["p"] - x)
    assert not opt.finished


def test_rosenbrock():
    opt = LBFGS()
    record = drive(opt, rosenbrock, rosenbrock_grad, np.full(10, -1.2), 400)
    print("rosenbrock: error", record[99]["f"], "after 100 evaluations,", opt.f, "after",
          len(record), "; skipped pairs", opt.skipped_pairs, "restarts", opt.restarts)
    assert opt.skipped_pairs >= 1 or opt.restarts >= 2  # (the first call is restart number one)
    for r in record:  # every direction used is a descent direction
        assert r["g"] @ r["d"] < 0
    assert opt.f < 1e-10
    assert min(r["fp"] for r in record) == opt.f


class ListLBFGS(object):
    """The algorithm of the issue, section 1, restated with plain lists of pairs and no ring."""

    def __init__(self, history, first_step=1.0, armijo=1e-4, shrink=0.5, max_backtracks=20):
        self.m, self.first_step, self.c1 = history, first_step, armijo
        self.shrink, self.max_bt = shrink, max_backtracks
        self.x = None
        self.S, self.Y, self.R = [], [], []
        self.finished = False

    def restart(self):
        self.S, self.Y, self.R = [], [], []
        self.d = -self.g
        self.steepest, self.bt = True, 0
        gg = lbfgs_mod.dot(self.g, self.g)
        self.t = self.first_step / np.sqrt(gg) if gg != 0 else 0.0

    def update(self, gp, p, fp):
        dot = lbfgs_mod.dot
        if self.finished:
            return self.x.copy()
        if self.x is None:
            self.x, self.f, self.g = p.copy(), fp, gp.copy()
            self.restart()
            return self.x + self.t * self.d
        step = p - self.x
        if fp <= self.f + self.c1 * dot(self.g, step):
            y = gp - self.g
            sy, ss, yy = dot(step, y), dot(step, step), dot(y, y)
            if sy > 0 and sy * sy > 1e-20 * ss * yy:
                self.S.append(step)
                self.Y.append(y)
                self.R.append(1 / sy)
                self.scale = sy / yy
                self.S, self.Y, self.R = self.S[-self.m:], self.Y[-self.m:], self.R[-self.m:]
            self.x, self.f, self.g = p.copy(), fp, gp.copy()
            if not self.S:
                self.restart()
            else:
                q = self.g.copy()
                count = len(self.S)
                alpha = [None] * count
                for i in range(count - 1, -1, -1):
                    alpha[i] = self.R[i] * dot(self.S[i], q)
                    q = q - alpha[i] * self.Y[i]
                q = q * self.scale
                for i in range(count):
                    beta = self.R[i] * dot(self.Y[i], q)
                    q = q + (alpha[i] - beta) * self.S[i]
                self.d, self.t, self.bt, self.steepest = -q, 1.0, 0, False
                if not dot(self.g, self.d) < 0:
                    self.restart()
        else:
            self.bt += 1
            self.t = self.t * self.shrink
            if self.bt > self.max_bt:
                if self.steepest:
                    self.finished = True
                    return self.x.copy()
                self.restart()
        return self.x + self.t * self.d


@pytest.mark.parametrize("which", ["quadratic", "rosenbrock"])
def test_history_of_three_equals_the_list_reference(which):
    if which == "quadratic":
        f, grad, start = quadratic()
        evaluations = 40
    else:
        f, grad, start, evaluations = rosenbrock, rosenbrock_grad, np.full(10, -1.2), 120
    opt, ref = LBFGS(history=3), ListLBFGS(3)
    p = start.copy()
    for _ in range(evaluations):
        fp, gp = f(p), grad(p)
        nxt = opt.update(gp, p, fp)
        expect = ref.update(gp, p, fp)
        assert np.array_equal(nxt, expect)
        assert len(opt.pairs) <= 3 and len(opt.pairs) == len(ref.S)
        p = nxt
    assert opt.accepted > 8
    assert np.array_equal(opt.x, ref.x) and opt.f == ref.f


def test_finishing():
    f, grad, start = quadratic()
    opt = LBFGS(first_step=1e3, max_backtracks=1)
    record = drive(opt, f, grad, start, 10)
    assert opt.finished and len(record) < 10
    last = record[-1]
    assert np.array_equal(opt.x, start)  # nothing after the first call was accepted
    nxt = opt.update(last["gp"], last["p"], last["fp"])
    assert np.array_equal(nxt, opt.x)
    state = (opt.x.copy(), opt.f, opt.g.copy(), opt.t, opt.bt)
    for _ in range(3):  # further updates leave it alone
        assert np.array_equal(opt.update(grad(nxt) * 0 + 1.0, nxt + 1.0, -1.0), state[0])
    assert np.array_equal(opt.x, state[0]) and opt.f == state[1] and opt.t == state[3]
    assert np.array_equal(opt.g, state[2]) and opt.bt == state[4] and opt.finished


def test_nan_error_rejects():
    f, grad, start = quadratic()
    opt = LBFGS()
    p = opt.update(grad(start), start, f(start))
    t = opt.t
    opt.update(grad(p), p, float("nan"))
    assert opt.accepted == 1 and opt.bt == 1 and opt.t == t * opt.shrink


# ---- through the host API (oracle backend) -------------------------------------------------------

def transmon():
    case = cases_mod.case_by_name("c2_transmon")
    args = (case.K, case.Nc, product_cost_list(case), case.T, case.hamiltonian(),
            case.initial_states, case.N)
    kw = dict(max_control_norms=np.full(case.K, 5.0), log_iteration_step=0,
              magnus_policy=getattr(MagnusPolicy, case.magnus))
    u0 = 0.3 * np.random.default_rng(321).standard_normal((1, case.Nc, case.K))
    return case, args, kw, u0


def test_lbfgs_beats_adam_on_the_transmon():
    case, args, kw, u0 = transmon()
    quasi = qoc_amd.grape_schroedinger_discrete_batch(*args, u0.copy(), optimizer=LBFGS(),
                                                      iteration_count=20, **kw)
    adam = qoc_amd.grape_schroedinger_discrete_batch(*args, u0.copy(),
                                                     optimizer=Adam(learning_rate=3e-2),
                                                     iteration_count=20, **kw)
    print("c2_transmon, 20 iterations: LBFGS", quasi.best_error[0], "Adam(3e-2)", adam.best_error[0])
    assert quasi.best_error[0] * 10 <= adam.best_error[0]
    assert quasi.iterations_run[0] == 20


def small_problem():
    case = cases_mod.case_by_name("ctrlcosts_r")
    args = (case.K, case.Nc, product_cost_list(case), case.T, case.hamiltonian(),
            case.initial_states, case.N)
    kw = dict(cost_eval_step=case.cost_eval_step, log_iteration_step=0,
              max_control_norms=np.full(case.K, 2.0),
              magnus_policy=getattr(MagnusPolicy, case.magnus))
    u0 = 0.3 * np.random.default_rng(321).standard_normal((5, case.Nc, case.K))
    return args, kw, u0


def assert_seed_equals_single(full, one, b):
    assert one.best_error[0] == full.best_error[b]
    assert one.best_iteration[0] == full.best_iteration[b]
    assert one.iterations_run[0] == full.iterations_run[b]
    assert np.array_equal(one.best_controls[0], full.best_controls[b])
    assert np.array_equal(one.best_final_states[0], full.best_final_states[b])


def test_batch_of_five_equals_single_seed_runs_with_early_stop():
    args, kw, u0 = small_problem()
    probe = qoc_amd.grape_schroedinger_discrete_batch(*args, u0.copy(), optimizer=LBFGS(),
                                                      iteration_count=4, **kw)
    threshold = float(np.min(probe.best_error))  # the best seed stops at iteration <= 3
    full = qoc_amd.grape_schroedinger_discrete_batch(*args, u0.copy(), optimizer=LBFGS(),
                                                     iteration_count=8, min_error=threshold, **kw)
    assert np.sum(full.iterations_run < 8) >= 1 and np.sum(full.iterations_run == 8) >= 1
    for b in range(5):
        one = qoc_amd.grape_schroedinger_discrete_batch(
            *args, u0[b:b + 1].copy(), optimizer=LBFGS(), iteration_count=8,
            min_error=threshold, **kw)
        assert_seed_equals_single(full, one, b)


def test_batch_of_five_equals_single_seed_runs_with_finished_seeds():
    """first_step = 1e3 with one backtrack: the clip holds the first trial at the bounds, where
    the error is worse; the seeds that find no decrease there finish and stop counting."""
    args, kw, u0 = small_problem()
    make = lambda: LBFGS(first_step=1e3, max_backtracks=1)  # noqa: E731
    full = qoc_amd.grape_schroedinger_discrete_batch(*args, u0.copy(), optimizer=make(),
                                                     iteration_count=8, **kw)
    assert np.any(full.iterations_run < 8)  # a seed finished
    for b in range(5):
        one = qoc_amd.grape_schroedinger_discrete_batch(
            *args, u0[b:b + 1].copy(), optimizer=make(), iteration_count=8, **kw)
        assert_seed_equals_single(full, one, b)


def test_plugin_subclass_takes_the_per_seed_clone_route_with_fresh_state():
    class PluginLBFGS(LBFGS):
        pass

    args, kw, u0 = small_problem()
    used = PluginLBFGS()
    used.update(np.ones(3), np.zeros(3), 1.0)  # state of an earlier use must not leak into a seed
    assert batch_mod.batched_stepper(used, u0.reshape(5, -1)) is None
    assert batch_mod.batched_stepper(LBFGS(), u0.reshape(5, -1)) is not None
    a = qoc_amd.grape_schroedinger_discrete_batch(*args, u0.copy(), optimizer=used,
                                                  iteration_count=6, **kw)
    b = qoc_amd.grape_schroedinger_discrete_batch(*args, u0.copy(), optimizer=LBFGS(),
                                                  iteration_count=6, **kw)
    assert np.array_equal(a.best_error, b.best_error)
    assert np.array_equal(a.best_iteration, b.best_iteration)
    for s in range(5):
        assert np.array_equal(a.best_controls[s], b.best_controls[s])


def test_complex_controls_reduce_the_error():
    case = cases_mod.case_by_name("small_complex_M2")
    rng = np.random.default_rng(321)
    shape = (3, case.Nc, case.K)
    u0 = 0.3 * (rng.standard_normal(shape) + 1j * rng.standard_normal(shape))
    out = qoc_amd.grape_schroedinger_discrete_batch(
        case.K, case.Nc, product_cost_list(case), case.T, case.hamiltonian(),
        case.initial_states, case.N, u0.copy(), optimizer=LBFGS(), complex_controls=True,
        cost_eval_step=case.cost_eval_step, iteration_count=8, log_iteration_step=0,
        max_control_norms=np.full(case.K, 2.0), magnus_policy=getattr(MagnusPolicy, case.magnus))
    first = qoc_amd.grape_schroedinger_discrete_batch(
        case.K, case.Nc, product_cost_list(case), case.T, case.hamiltonian(),
        case.initial_states, case.N, u0.copy(), optimizer=LBFGS(), complex_controls=True,
        cost_eval_step=case.cost_eval_step, iteration_count=1, log_iteration_step=0,
        max_control_norms=np.full(case.K, 2.0), magnus_policy=getattr(MagnusPolicy, case.magnus))
    assert np.all(out.best_error < first.best_error)
    assert np.iscomplexobj(out.best_controls[0])


def test_lindblad_batch_reduces_the_error():
    case = cases_mod.lindblad_case_by_name("lindblad_n4")
    u0 = 0.3 * np.random.default_rng(321).standard_normal((3, case.Nc, case.K))
    args = (case.K, case.Nc, lindblad_cost_list(case), case.T, case.initial_densities, case.N)
    kw = dict(cost_eval_step=case.cost_eval_step, hamiltonian=case.hamiltonian(),
              lindblad_data=case.lindblad_data(), log_iteration_step=0,
              max_control_norms=np.full(case.K, 2.0))
    first = qoc_amd.grape_lindblad_discrete_batch(*args, u0.copy(), optimizer=LBFGS(),
                                                  iteration_count=1, **kw)
    out = qoc_amd.grape_lindblad_discrete_batch(*args, u0.copy(), optimizer=LBFGS(),
                                                iteration_count=8, **kw)
    assert np.all(out.best_error < first.best_error)


def test_single_seed_entry_point_runs():
    args, kw, u0 = small_problem()
    first = qoc_amd.grape_schroedinger_discrete(*args, initial_controls=u0[0].copy(),
                                                optimizer=LBFGS(), iteration_count=1, **kw)
    out = qoc_amd.grape_schroedinger_discrete(*args, initial_controls=u0[0].copy(),
                                              optimizer=LBFGS(), iteration_count=8, **kw)
    assert out.best_error < first.best_error
    assert out.best_iteration > 0


def test_new_exports_are_declared_and_bound():
    names = ("qocx_opt_lbfgs_begin", "qocx_opt_lbfgs_step", "qocx_lindblad_opt_lbfgs_begin",
             "qocx_lindblad_opt_lbfgs_step")
    header = open(os.path.join(ROOT, "include", "qocx.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in names:
        assert re.search(r"\bint %s\s*\(" % name, header), name
        assert name in engine.SIGNATURES
        assert "`%s`" % name in integration
    for method in ("opt_lbfgs_begin", "opt_lbfgs_step", "lindblad_opt_lbfgs_begin",
                   "lindblad_opt_lbfgs_step"):
        assert callable(getattr(engine.Engine, method))
    assert qoc_amd.standard.LBFGS is LBFGS and LBFGS.needs_error
