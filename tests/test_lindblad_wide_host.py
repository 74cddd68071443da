"""
CPU tests of what surrounds the Lindblad kernel of 33 <= n <= 64 (wide=True, knob lindblad_wide): the
model's cheap norm bound, the case table's distance from a change of grid, the model against the exact
reference on the cases the engine is held to, and the Python refusals and the knob against a stand-in
backend.
"""

import numpy as np
import pytest

import qoc_amd
from qoc_amd.core.device import LindbladEvaluator
from qoc_amd.standard import HamiltonianEnsemble, LindbladSweep, TargetDensityInfidelity
from tests import helpers
from tests import lindblad_exact as ex
from tests import lindblad_model as lm
from tests import lindblad_wide_cases as wc
from tests.oracle_backend import OracleBackend


@pytest.mark.parametrize("n", [33, 40])
def test_the_cheap_norm_bound_against_the_svd(n):
    """The power iteration of the engine against the n^2 x n^2 SVD of the parent class: within the
    engine's 2 % margin (it comes from below and adds 2 %), and the same sub-division count."""
    rng = np.random.default_rng(n)
    gue = wc.cases_mod.gue
    h0, g = 1.5 * gue(rng, n), [gue(rng, n), gue(rng, n)]
    ops = np.stack([gue(rng, n) + 0.5j * gue(rng, n) for _ in range(2)])
    gammas = np.array([0.1, 0.25])
    cheap = wc.WideLindblad(h0, g, gammas, ops)
    svd = lm.StructuredLindblad(h0, g, gammas, ops)
    for umax in ([0.0, 0.0], [0.7, 0.3]):
        a, b = cheap.norm_bound(umax), svd.norm_bound(umax)
        print(n, umax, a, b)
        assert abs(a - b) <= 0.02 * b
        assert np.ceil(a * 0.3 / 0.4) == np.ceil(b * 0.3 / 0.4)


@pytest.mark.parametrize("name", wc.NAMES + wc.EXACT_NAMES)
def test_every_case_stays_5_percent_away_from_a_change_of_grid(name):
    """norm_bound * dt / 0.4 at least 5 % away from an integer for every seed: the engine's bound and
    the model's differ in the last per cent, and ceil() of them must not."""
    for x in wc.grid_margins(wc.build(name)):
        assert abs(x - round(x)) >= 0.05 * x, (name, x)


def test_the_subdivision_case_cuts_two_grids():
    case = wc.build("n40_subdivisions")
    counts = wc.grid_counts(case)
    assert counts[0] == case.N - 1 and counts[1] >= 2 * (case.N - 1)


@pytest.mark.parametrize("name", wc.EXACT_NAMES)
def test_the_model_against_the_exact_reference(name):
    """What the gates of tests/test_gpu_lindblad_wide.py rest on: ten times the model's error against
    the exact reference stays below the constants of tests/lindblad_exact.py
    (profiles/lindblad_wide_exact.jsonl holds the numbers)."""
    errors = wc.compare(wc.model_results(name), wc.exact_results(name))
    print(name, errors)
    assert 10 * errors["cost"] <= ex.GATE_COST
    assert 10 * errors["densities"] <= ex.GATE_DENSITIES
    assert 10 * errors["gradient"] <= ex.GATE_GRADIENT


class StandIn(OracleBackend):
    """The NumPy backend with a knob log; counts the problems it is given."""

    def __init__(self):
        OracleBackend.__init__(self)
        self.knobs, self.problems, self.ensembles = [], 0, 0

    def set_lindblad_ensemble(self, scales, offsets, weights):
        self.ensembles += 1

    def set_knob(self, name, value):
        self.knobs.append((name, value))

    def set_lindblad_problem(self, *args, **kw):
        self.problems += 1
        return OracleBackend.set_lindblad_problem(self, *args, **kw)


N_WIDE = 34
EYE = np.eye(N_WIDE, dtype=np.complex128)
DRIVE = np.diag(np.arange(N_WIDE) / N_WIDE).astype(np.complex128)
OPS = np.stack([np.diag(np.sqrt(np.arange(1, N_WIDE)), k=1).astype(np.complex128)])
RHO0 = (EYE / N_WIDE)[None]


def linear_h(u, t):
    return 0.3 * DRIVE + u[0] * (DRIVE @ DRIVE)


def static_data(t):
    return np.array([0.05]), OPS


def evaluator(backend, hamiltonian=linear_h, lindblad_data=static_data, n=N_WIDE, **kw):
    rho0 = (np.eye(n, dtype=np.complex128) / n)[None]
    args = dict(hamiltonian=hamiltonian, lindblad_data=lindblad_data, control_count=1, control_eval_count=4,
                costs=[TargetDensityInfidelity(rho0)], backend=backend)
    args.update(kw)
    return LindbladEvaluator(1.0, rho0, 4, **args)


def test_wide_false_still_refuses_n33():
    backend = StandIn()
    with pytest.raises(NotImplementedError, match="hilbert_size <= 32"):
        evaluator(backend, hamiltonian=lambda u, t: np.eye(33), lindblad_data=None, n=33)
    with pytest.raises(NotImplementedError, match="hilbert_size <= 32"):
        evaluator(backend, hamiltonian=lambda u, t: np.eye(33), lindblad_data=None, n=33, wide=False)
    with pytest.raises(NotImplementedError, match=r"hilbert_size <= 64 \(got 65\)"):
        evaluator(backend, hamiltonian=lambda u, t: np.eye(65), lindblad_data=None, n=65, wide=True)
    assert backend.problems == 0 and backend.knobs == []
    with pytest.raises(NotImplementedError, match="hilbert_size <= 32"):
        qoc_amd.evolve_lindblad_discrete(1.0, np.eye(33)[None] / 33, 2, hamiltonian=lambda u, t: np.eye(33))


def test_the_knob_follows_the_keyword():
    """wide=True sets lindblad_wide = 1 before the problem, wide=False sets it to 0: one shared backend
    never leaks the opt-in. A backend without set_knob cannot opt in."""
    backend = StandIn()
    e = evaluator(backend, wide=True)
    assert e.wide and backend.knobs == [("lindblad_wide", 1)] and backend.problems == 1
    evaluator(backend, hamiltonian=lambda u, t: 0.3 * DRIVE[:8, :8] + u[0] * EYE[:8, :8],
              lindblad_data=lambda t: (np.array([0.05]), OPS[:, :8, :8]), n=8)
    assert backend.knobs == [("lindblad_wide", 1), ("lindblad_wide", 0)] and backend.problems == 2
    with pytest.raises(NotImplementedError, match="set_knob"):
        evaluator(OracleBackend(), wide=True)
    # the public entry points hand the keyword on
    helpers.set_backend_factory(lambda: backend)
    try:
        result = qoc_amd.evolve_lindblad_discrete(
            1.0, RHO0, 3, controls=np.zeros((3, 1)), costs=[TargetDensityInfidelity(RHO0)],
            hamiltonian=linear_h, lindblad_data=static_data, wide=True)
        assert np.isfinite(result.error)
    finally:
        helpers.set_backend_factory(None)
    assert backend.knobs[-1] == ("lindblad_wide", 1) and backend.problems == 3


def test_refusals_above_32_by_name():
    """What has kernels of its own at hilbert_size <= 32 only is refused by name, in the wording of the
    other refusals, before the backend sees a problem."""
    backend = StandIn()
    above = "hilbert_size > 32"

    def refused(what, **kw):
        with pytest.raises(NotImplementedError, match=what) as info:
            evaluator(backend, wide=True, **kw)
        assert above in str(info.value), str(info.value)
    refused("time-dependent hamiltonian or lindblad_data",
            hamiltonian=lambda u, t: (0.3 + 0.1 * np.cos(t)) * DRIVE + u[0] * EYE)
    refused("time-dependent hamiltonian or lindblad_data",
            lindblad_data=lambda t: (np.array([0.05 * (1 + t)]), OPS))
    refused("not linear in the controls", hamiltonian=lambda u, t: 0.3 * DRIVE + u[0] ** 2 * EYE)
    refused("not linear in the controls", hamiltonian=lambda u, t: 0.3 * DRIVE + u[0] ** 2 * EYE,
            frozen_controls=np.zeros((4, 1)), need_gradients=False)
    refused("rate_scales of a HamiltonianEnsemble", hamiltonian=HamiltonianEnsemble(
        linear_h, perturbations=[DRIVE], offsets=[[0.1], [-0.1]], rate_scales=[[1.0], [2.0]]))
    refused("rate_scales of a LindbladSweep", hamiltonian=LindbladSweep(
        linear_h, perturbations=[DRIVE], offsets=[[0.1], [-0.1]], rate_scales=[[1.0], [2.0]]))
    refused("durations of a LindbladSweep",
            hamiltonian=LindbladSweep.durations(linear_h, [0.8, 1.2], 1.0))
    refused("duration_search of a LindbladSweep",
            hamiltonian=LindbladSweep.duration_search(linear_h, [0.8, 1.2], 1.0, (0.5, 1.5)))
    assert backend.problems == 0
    # the same ensemble and sweep without rates are taken
    evaluator(backend, wide=True, hamiltonian=HamiltonianEnsemble(
        linear_h, perturbations=[DRIVE], offsets=[[0.1], [-0.1]]))
    assert backend.problems == 1 and backend.ensembles == 1
