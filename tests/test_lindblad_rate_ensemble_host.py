"""CPU tests of per-member dissipation rates (HamiltonianEnsemble(..., rate_scales=c)) on the
Lindblad path (no GPU): the constructor and member_lindblad_data, a stand-in backend with
set_lindblad_ensemble_rates (the evaluator must hand the rates over after the ensemble and reduce
nothing itself), the three entry points, every refusal, and the ABI.

Member references: the plain Lindblad problem of ensemble.member(m) under
ensemble.member_lindblad_data(m, lindblad_data), through the same NumPy model of the device
algorithm (tests/lindblad_model.py). Without perturbations (J = 0) the member and the ensemble's item
see the same control maxima (|s u| = |s| |u|) and the same rates, hence the same sub-interval grid:
they agree to rounding, 1e-12. With perturbations the item carries the D_j as control channels, the
two integrate on different grids and agree as two converged integrations do: 1e-9 (the gate of
tests/test_lindblad_ensemble_host.py). What the stand-in and the evaluator add on top (weighted
sums) is held to 1e-13.
"""

import os

import numpy as np
import pytest

import qoc_amd
from qoc_amd import engine
from qoc_amd.core import device
from qoc_amd.standard import Adam, HamiltonianEnsemble, TargetStateInfidelity
from tests import cases as cases_mod
from tests import helpers
from tests import lindblad_model as lm
from tests.oracle_backend import OracleBackend
from tests.test_lindblad_ensemble_host import LindbladEnsembleStandIn
from tests.test_lindblad_host_api import product_cost_list

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class RateEnsembleStandIn(LindbladEnsembleStandIn):
    """An OracleBackend with set_lindblad_ensemble (LindbladEnsembleStandIn) and
    set_lindblad_ensemble_rates: member m's items are evaluated through the oracle on the system
    with the rates c_m * dissipators, then reduced as the engine reduces them."""

    def __init__(self):
        super().__init__()
        self.rates = None
        self.rate_calls = []   # every (M, L) array received, in order

    def set_lindblad_problem(self, *a, **kw):
        super().set_lindblad_problem(*a, **kw)
        self.rates = None       # a new problem clears the rates ...

    def set_lindblad_ensemble(self, scales, offsets, weights):
        super().set_lindblad_ensemble(scales, offsets, weights)
        self.rates = None       # ... and so does a new ensemble

    def set_lindblad_ensemble_rates(self, rate_scales):
        assert self.ens is not None, "rates come after the ensemble"
        a, kw = self.problems[-1]
        assert not kw.get("fixed_subdivision"), "rates on a problem with stage tables"
        dissipators = np.asarray(a[8], dtype=np.float64)
        rates = np.asarray(rate_scales, dtype=np.float64)
        assert rates.shape == (len(self.ens[2]), len(dissipators))
        assert np.all(np.isfinite(rates)) and np.all(rates >= 0)
        self.rates = rates.copy()
        self.rate_calls.append(rates.copy())

    def evaluate_lindblad(self, controls, want_grad=True, want_final=True):
        if self.rates is None:
            return super().evaluate_lindblad(controls, want_grad, want_final)
        assert not self.keep
        p = self.lb
        a, _ = self.problems[-1]
        n, K, Nc = p["n"], p["K"], p["Nc"]
        h0, g, dissipators, operators = a[6], a[7], np.asarray(a[8], dtype=np.float64), a[9]
        scales, offsets, weights = self.ens
        kr, M = scales.shape[1], len(weights)
        u = np.asarray(controls, dtype=np.float64).reshape(-1, Nc, kr)
        B = u.shape[0]
        items = np.empty((B, M, Nc, K))
        items[..., :kr] = scales[None, :, None, :] * u[:, None]
        items[..., kr:] = offsets[None, :, None, :]
        shared = self.lb_system
        cost, grads, final = [], [], []
        try:
            for m in range(M):  # one system per member: gamma_mi = c_mi * gamma_i
                self.lb_system = lm.StructuredLindblad(
                    np.asarray(h0).reshape(n, n), list(np.asarray(g).reshape(K, n, n)),
                    self.rates[m] * dissipators, operators)
                c, gr, fin = OracleBackend.evaluate_lindblad(self, items[:, m], want_grad, want_final)
                cost.append(c)
                grads.append(gr)
                final.append(fin)
        finally:
            self.lb_system = shared
        self.members = np.stack(cost, axis=1)
        self.item_grads = None if not want_grad else np.stack(grads, axis=1)
        seed_cost = np.zeros(B)
        for m in range(M):
            seed_cost += weights[m] * self.members[:, m]
        seed_grads = None
        if want_grad:
            seed_grads = np.zeros((B, Nc, kr))
            for m in range(M):
                seed_grads += (weights[m] * scales[m]) * self.item_grads[:, m, :, :kr]
        return seed_cost, seed_grads, np.stack(final, axis=1)


def _rates(rng, M, L):
    """Factors in [0.25, 4], log-uniform."""
    return 4.0 ** rng.uniform(-1, 1, (M, L))


def _ensemble(case, rng, M=3, J=0, rates=True):
    d = np.stack([0.5 * cases_mod.gue(rng, case.n) for _ in range(J)]) if J else None
    return HamiltonianEnsemble(
        case.hamiltonian(), perturbations=d,
        offsets=0.3 * rng.standard_normal((M, J)) if J else None,
        control_scales=1 + 0.05 * rng.standard_normal((M, case.K)),
        weights=rng.uniform(0.2, 1.0, M),
        rate_scales=_rates(rng, M, len(case.dissipators)) if rates else None)


def _evaluator(case, hamiltonian, backend, lindblad_data=None, **kw):
    return device.LindbladEvaluator(
        case.T, case.initial_densities, case.N, hamiltonian=hamiltonian,
        lindblad_data=case.lindblad_data() if lindblad_data is None else lindblad_data,
        control_count=case.K, control_eval_count=case.Nc,
        complex_controls=case.complex_controls, costs=product_cost_list(case),
        cost_eval_step=case.cost_eval_step, backend=backend, **kw)


def _seeds(case, rng, B, sigma=0.4):
    u = sigma * rng.standard_normal((B, case.Nc, case.K))
    if case.complex_controls:
        u = u + 1j * sigma * rng.standard_normal((B, case.Nc, case.K))
    return u


# ---- the constructor and member_lindblad_data ---------------------------------------------------------

def test_constructor_validates_rate_scales():
    """(This is the test that fails without the feature: the argument does not exist.)"""
    ham = lambda u, t: np.zeros((2, 2))  # noqa: E731
    c = np.array([[0.25, 1.0], [1.0, 1.0], [4.0, 0.0]])
    e = HamiltonianEnsemble(ham, rate_scales=c)   # M is read from rate_scales alone
    assert e.member_count == 3 and np.array_equal(e.rate_scales, c)
    assert e.rate_scales.dtype == np.float64 and e.rate_scales is not c
    assert np.array_equal(e.weights, np.full(3, 1.0 / 3))
    assert repr(e).endswith("3 members, 0 perturbations, rate_scales 3x2)")
    assert HamiltonianEnsemble(ham, weights=np.ones(2)).rate_scales is None
    assert repr(HamiltonianEnsemble(ham, weights=np.ones(2))).endswith("2 members, 0 perturbations)")
    with pytest.raises(ValueError, match="rate_scales must have 2 dimensions"):
        HamiltonianEnsemble(ham, rate_scales=np.ones(3))
    with pytest.raises(ValueError, match="rate_scales must have 2 dimensions"):
        HamiltonianEnsemble(ham, rate_scales=np.ones((3, 2, 1)))
    with pytest.raises(ValueError, match="disagree on the member count: weights 2, rate_scales 3"):
        HamiltonianEnsemble(ham, weights=np.ones(2), rate_scales=c)
    with pytest.raises(ValueError, match="disagree on the member count"):
        HamiltonianEnsemble(ham, control_scales=np.ones((4, 1)), rate_scales=c)
    bad = c.copy()
    bad[1, 0] = -1e-3
    with pytest.raises(ValueError, match="rate_scales must be >= 0"):
        HamiltonianEnsemble(ham, rate_scales=bad)
    for value in (np.nan, np.inf):
        bad = c.copy()
        bad[2, 1] = value
        with pytest.raises(ValueError, match="rate_scales is not finite"):
            HamiltonianEnsemble(ham, rate_scales=bad)
    with pytest.raises(ValueError, match="rate_scales must be real"):
        HamiltonianEnsemble(ham, rate_scales=c.astype(np.complex128))
    with pytest.raises(ValueError, match="at least one member"):
        HamiltonianEnsemble(ham, rate_scales=np.ones((0, 2)))


def test_member_lindblad_data_scales_the_rates_and_keeps_the_operators():
    rng = np.random.default_rng(81)
    gam = np.array([0.3, 0.02, 1.5])
    ops = rng.standard_normal((3, 4, 4)) + 1j * rng.standard_normal((3, 4, 4))
    data = lambda t: (gam * (1 + t), ops)  # noqa: E731
    c = _rates(rng, 2, 3)
    e = HamiltonianEnsemble(lambda u, t: np.zeros((4, 4)), rate_scales=c)
    for m in range(2):
        member = e.member_lindblad_data(m, data)
        for t in (0.0, 0.7):
            g_m, ops_m = member(t)
            assert np.array_equal(g_m, c[m] * (gam * (1 + t)))  # one product
            assert ops_m is ops
    with pytest.raises(IndexError):
        e.member_lindblad_data(2, data)
    with pytest.raises(ValueError, match="callable"):
        e.member_lindblad_data(0, (gam, ops))
    with pytest.raises(ValueError, match=r"\(M, L\) with L = 2"):
        e.member_lindblad_data(0, lambda t: (gam[:2], ops[:2]))(0.0)
    # without rate_scales every member has the problem's own lindblad_data
    plain = HamiltonianEnsemble(lambda u, t: np.zeros((4, 4)), weights=np.ones(2))
    assert plain.member_lindblad_data(1, data) is data


# ---- the evaluator and the entry points through the stand-in -------------------------------------------

@pytest.mark.parametrize("name", ["lindblad_n4", "lindblad_n4_complex"])
def test_evaluator_hands_the_rates_over_and_reduces_the_member_evaluations(name):
    case = cases_mod.lindblad_case_by_name(name)
    rng = np.random.default_rng(82)
    M, B = 3, 2
    e = _ensemble(case, rng, M)
    backend = RateEnsembleStandIn()
    ev = _evaluator(case, e, backend)
    assert len(backend.problems) == 1 and len(backend.received) == 1
    assert len(backend.rate_calls) == 1 and np.array_equal(backend.rate_calls[0], e.rate_scales)
    # the problem itself carries the rates as given: the members' are the engine's business
    assert np.array_equal(backend.problems[-1][0][8], case.dissipators)
    u = _seeds(case, rng, B)
    errors, grads, finals, _ = ev.evaluate_batch(u)
    members = ev.member_errors()
    S, n = case.initial_densities.shape[0], case.n
    assert finals.shape == (B, M, S, n, n) and members.shape == (B, M)
    member_evs = [_evaluator(case, e.member(m), OracleBackend(),
                             lindblad_data=e.member_lindblad_data(m, case.lindblad_data()))
                  for m in range(M)]
    spread = 0.0
    for b in range(B):
        want_err, want_grad = 0.0, 0.0
        for m in range(M):
            err, gr, fin, _ = member_evs[m].evaluate(u[b])
            assert abs(members[b, m] - err) < 1e-12
            assert np.max(np.abs(finals[b, m] - fin)) < 1e-12
            want_err += e.weights[m] * err
            want_grad = want_grad + e.weights[m] * gr
        assert abs(errors[b] - want_err) < 1e-12
        assert abs(errors[b] - np.dot(e.weights, members[b])) < 1e-13
        assert np.max(np.abs(grads[b] - want_grad)) < 1e-11
        spread = max(spread, np.ptp(members[b]))
    # the rates reach the members: with the shared lindblad_data the member costs differ from these
    shared = _evaluator(case, HamiltonianEnsemble(
        e.hamiltonian, control_scales=e.control_scales, weights=e.weights), RateEnsembleStandIn())
    shared.evaluate_batch(u)
    assert np.max(np.abs(shared.member_errors() - members)) > 1e-5
    assert spread > 1e-5


def test_members_with_perturbations_match_the_member_problems():
    """J = 2: items and member problems integrate on different grids (module docstring): 1e-9."""
    case = cases_mod.lindblad_case_by_name("lindblad_n4")
    rng = np.random.default_rng(83)
    M = 3
    e = _ensemble(case, rng, M, J=2)
    ev = _evaluator(case, e, RateEnsembleStandIn())
    u = _seeds(case, rng, 1)
    errors, grads, finals, _ = ev.evaluate_batch(u)
    want_err, want_grad = 0.0, 0.0
    for m in range(M):
        member = _evaluator(case, e.member(m), OracleBackend(),
                            lindblad_data=e.member_lindblad_data(m, case.lindblad_data()))
        err, gr, fin, _ = member.evaluate(u[0])
        assert abs(ev.member_errors()[0, m] - err) < 1e-9
        assert np.max(np.abs(finals[0, m] - fin)) < 1e-9
        want_err += e.weights[m] * err
        want_grad = want_grad + e.weights[m] * gr
    assert abs(errors[0] - want_err) < 1e-9
    assert np.max(np.abs(grads[0] - want_grad)) < 1e-8


def test_entry_points_with_rates():
    case = cases_mod.lindblad_case_by_name("lindblad_n4")
    rng = np.random.default_rng(85)
    M = 3
    e = _ensemble(case, rng, M)
    S, n = case.initial_densities.shape[0], case.n
    costs = product_cost_list(case)
    data = case.lindblad_data()
    u = 0.5 * _seeds(case, rng, 1)[0]
    kw = dict(cost_eval_step=case.cost_eval_step, hamiltonian=e, lindblad_data=data)
    helpers.set_backend_factory(RateEnsembleStandIn)
    try:
        r = qoc_amd.evolve_lindblad_discrete(case.T, case.initial_densities, case.N, controls=u,
                                             costs=costs, **kw)
        assert r.final_densities.shape == (M, S, n, n) and r.member_errors.shape == (M,)
        want = 0.0
        for m in range(M):
            helpers.set_backend_factory(OracleBackend)
            member = qoc_amd.evolve_lindblad_discrete(
                case.T, case.initial_densities, case.N, controls=u, costs=costs,
                **dict(kw, hamiltonian=e.member(m), lindblad_data=e.member_lindblad_data(m, data)))
            helpers.set_backend_factory(RateEnsembleStandIn)
            assert abs(member.error - r.member_errors[m]) < 1e-12
            assert np.max(np.abs(member.final_densities - r.final_densities[m])) < 1e-12
            want += e.weights[m] * member.error
        assert abs(r.error - want) < 1e-12
        gkw = dict(kw, complex_controls=case.complex_controls, iteration_count=3,
                   log_iteration_step=0, optimizer=Adam(learning_rate=1e-2))
        g = qoc_amd.grape_lindblad_discrete(case.K, case.Nc, costs, case.T,
                                            case.initial_densities, case.N, initial_controls=u,
                                            **gkw)
        assert g.best_final_densities.shape == (M, S, n, n)
        assert abs(g.best_error - np.dot(e.weights, g.member_errors)) < 1e-13
        u0 = 0.5 * _seeds(case, rng, 2)
        gb = qoc_amd.grape_lindblad_discrete_batch(case.K, case.Nc, costs, case.T,
                                                   case.initial_densities, case.N, u0, **gkw)
        for b in range(2):
            assert gb.best_final_densities[b].shape == (M, S, n, n)
            assert abs(gb.best_error[b] - np.dot(e.weights, gb.member_errors[b])) < 1e-13
        # every seed of the batch walks its single-seed trajectory
        for b in range(2):
            one = qoc_amd.grape_lindblad_discrete(case.K, case.Nc, costs, case.T,
                                                  case.initial_densities, case.N,
                                                  initial_controls=u0[b], **gkw)
            assert one.best_iteration == gb.best_iteration[b]
            assert abs(one.best_error - gb.best_error[b]) < 1e-13
            assert np.max(np.abs(one.best_controls - gb.best_controls[b])) < 1e-13
            assert np.max(np.abs(one.member_errors - gb.member_errors[b])) < 1e-13
    finally:
        helpers.set_backend_factory(None)


# ---- refusals -------------------------------------------------------------------------------------------

class _NoProblemBackend(RateEnsembleStandIn):
    """Fails the test if a problem reaches it."""

    def set_lindblad_problem(self, *a, **kw):
        raise AssertionError("the backend saw a problem")


def test_refusals_on_the_lindblad_path():
    case = cases_mod.lindblad_case_by_name("lindblad_n4")
    rng = np.random.default_rng(86)
    L = len(case.dissipators)
    base = case.hamiltonian()
    weights = np.ones(2) / 2
    # the second dimension is not L: known once lindblad_data has been probed
    for wrong in (L - 1, L + 1):
        e = HamiltonianEnsemble(base, weights=weights, rate_scales=np.ones((2, wrong)))
        with pytest.raises(ValueError, match=r"rate_scales must be \(M, L\) with L = {}".format(L)):
            _evaluator(case, e, _NoProblemBackend())
    with pytest.raises(ValueError, match=r"with L = 0"):   # no lindblad_data at all
        device.LindbladEvaluator(
            case.T, case.initial_densities, case.N, control_count=case.K,
            control_eval_count=case.Nc, costs=product_cost_list(case),
            hamiltonian=HamiltonianEnsemble(base, weights=weights, rate_scales=np.ones((2, L))),
            backend=_NoProblemBackend())
    e = HamiltonianEnsemble(base, weights=weights, rate_scales=_rates(rng, 2, L))
    # stage tables: a time-dependent lindblad_data, base Hamiltonian or drive - each refused by name,
    # before the backend sees a problem, with and without control bounds
    moving_data = lambda t: (case.dissipators * (1 + 0.5 * np.sin(2.0 * t)), case.operators)  # noqa: E731
    for kw in (dict(), dict(control_bounds=np.full(case.K, 0.9))):
        with pytest.raises(NotImplementedError, match="time-independent system: lindblad_data"):
            _evaluator(case, e, _NoProblemBackend(), lindblad_data=moving_data, **kw)
        timedep = cases_mod.lindblad_case_by_name("lindblad_timedep")
        e_t = HamiltonianEnsemble(timedep.hamiltonian(), weights=weights,
                                  rate_scales=_rates(rng, 2, len(timedep.dissipators)))
        with pytest.raises(NotImplementedError, match="time-independent system: the hamiltonian"):
            _evaluator(timedep, e_t, _NoProblemBackend(), **kw)
        zero = np.zeros(case.K)
        unit = np.array([1.0] + [0.0] * (case.K - 1))

        def driven(u, t):  # the first drive operator breathes
            return base(u, t) + 0.2 * np.cos(2.3 * t) * u[0] * (base(unit, t) - base(zero, t))
        e_d = HamiltonianEnsemble(driven, weights=weights, rate_scales=e.rate_scales)
        with pytest.raises(NotImplementedError, match="fixed_subdivision > 0"):
            _evaluator(case, e_d, _NoProblemBackend(), **kw)
    # the same time-dependent problems are taken without rates (nothing else was refused)
    plain = HamiltonianEnsemble(base, weights=weights)
    assert _evaluator(case, plain, RateEnsembleStandIn(), lindblad_data=moving_data,
                      control_bounds=np.full(case.K, 0.9)).time_dependent
    # a backend with ensembles but without the rates setter
    backend = LindbladEnsembleStandIn()
    with pytest.raises(NotImplementedError, match="set_lindblad_ensemble_rates"):
        _evaluator(case, e, backend)
    assert backend.problems == []
    assert _evaluator(case, plain, LindbladEnsembleStandIn()).ensemble is plain
    # ... and through the entry points
    u = case.controls[0]
    costs = product_cost_list(case)
    helpers.set_backend_factory(_NoProblemBackend)
    try:
        with pytest.raises(NotImplementedError, match="time-independent system"):
            qoc_amd.evolve_lindblad_discrete(case.T, case.initial_densities, case.N, controls=u,
                                             costs=costs, hamiltonian=e, lindblad_data=moving_data,
                                             cost_eval_step=case.cost_eval_step)
        with pytest.raises(NotImplementedError, match="time-independent system"):
            qoc_amd.grape_lindblad_discrete(case.K, case.Nc, costs, case.T, case.initial_densities,
                                            case.N, hamiltonian=e, lindblad_data=moving_data,
                                            initial_controls=u, cost_eval_step=case.cost_eval_step)
        with pytest.raises(NotImplementedError, match="time-independent system"):
            qoc_amd.grape_lindblad_discrete_batch(
                case.K, case.Nc, costs, case.T, case.initial_densities, case.N, u[None],
                hamiltonian=e, lindblad_data=moving_data, cost_eval_step=case.cost_eval_step)
    finally:
        helpers.set_backend_factory(None)


def test_the_schroedinger_entry_points_refuse_rate_scales():
    rng = np.random.default_rng(87)
    n, K, Nc, N = 4, 2, 5, 9
    h0, g = cases_mod.gue(rng, n), [cases_mod.gue(rng, n) for _ in range(K)]
    ham = lambda u, t: h0 + u[0] * g[0] + u[1] * g[1]  # noqa: E731
    e = HamiltonianEnsemble(ham, weights=np.ones(2) / 2, rate_scales=np.ones((2, 1)))
    psi0 = cases_mod.column_states(np.eye(n)[:, :1])
    costs = [TargetStateInfidelity(cases_mod.column_states(np.eye(n)[:, 1:2]))]
    u = 0.3 * rng.standard_normal((Nc, K))

    class NoBackend(object):
        def __init__(self):
            raise AssertionError("a backend was made")
    helpers.set_backend_factory(NoBackend)
    try:
        with pytest.raises(ValueError, match="nothing to scale"):
            qoc_amd.evolve_schroedinger_discrete(0.6, e, psi0, N, controls=u, costs=costs)
        with pytest.raises(ValueError, match="nothing to scale"):
            qoc_amd.grape_schroedinger_discrete(K, Nc, costs, 0.6, e, psi0, N, initial_controls=u,
                                                iteration_count=2, log_iteration_step=0)
        with pytest.raises(ValueError, match="nothing to scale"):
            qoc_amd.grape_schroedinger_discrete_batch(K, Nc, costs, 0.6, e, psi0, N, u[None],
                                                      iteration_count=2, log_iteration_step=0)
        with pytest.raises(ValueError, match="nothing to scale"):
            device.SchroedingerEvaluator(0.6, e, psi0, N, costs=costs, control_count=K,
                                         control_eval_count=Nc)
    finally:
        helpers.set_backend_factory(None)


# ---- the ABI ---------------------------------------------------------------------------------------------

def test_the_abi_declares_the_entry_point():
    name = "qocx_lindblad_set_ensemble_rates"
    lib = engine.load_library()
    assert name in engine.SIGNATURES and hasattr(lib, name)
    vp, i32, dp = engine._VP, engine._I32, engine._c_double_p
    assert engine.SIGNATURES[name] == (engine.ctypes.c_int, [vp, i32, i32, dp])
    assert hasattr(engine.Engine, "set_lindblad_ensemble_rates")
    header = open(os.path.join(ROOT, "include", "qocx.h")).read()
    assert ("int qocx_lindblad_set_ensemble_rates(qocx_ctx* ctx, int32_t members, int32_t operators,"
            in header)
    assert "Not built: per-member dissipation rates" not in header
    assert "`{}`".format(name) in open(os.path.join(ROOT, "INTEGRATION.md")).read()
