"""CPU tests of a HamiltonianEnsemble over a QuadraticHamiltonian base (no GPU): the constructor's
checks of quadratic_scales, member(m) against the formula

    H_m(u, t) = H_lin(s_m u, t) + sum_j delta_mj D_j + sum_q c_mq (s_m,kq r_kq)(s_m,lq r_lq) Q_q

written out in NumPy, a stand-in backend that takes ensembles, quadratic terms and the members'
term scales (where the evaluator must hand over the structured problem and call no callable during
an evaluation), the rejections, and the ABI.

The gradients. The oracle's evaluate_with_grad takes dH/du from H(e_k) - H(0), which is the
derivative of a LINEAR callable only. For a member that is quadratic in the controls the oracle
is therefore run on the member's tangent at the controls under test,

    H_tan(w, t) = H_m(u(t), t) + sum_k (w_k - u_k(t)) dH_m/du_k (u(t), t),

a callable linear in w with the member's value and derivative at w = u: the same cost, the same
final states, and the member's own gradient. The bound on the gradient stays 1e-12.
"""

import numpy as np
import pytest

from oracle import qoc_numpy as onp
from qoc_amd import engine
from qoc_amd.core import device
from qoc_amd.models import MagnusPolicy
from qoc_amd.standard import (ControlNorm, HamiltonianEnsemble, QuadraticHamiltonian,
                              TargetStateInfidelity)
from tests import cases as cases_mod
from tests.oracle_backend import OracleBackend


class Counted(object):
    def __init__(self, fn):
        self.fn, self.calls = fn, 0

    def __call__(self, *a):
        self.calls += 1
        return self.fn(*a)


def _system(n, K, seed, complex_controls=False, time_dependent=True):
    rng = np.random.default_rng(seed)
    h0 = cases_mod.gue(rng, n)
    g_re = [cases_mod.gue(rng, n) for _ in range(K)]
    g_im = [cases_mod.gue(rng, n) for _ in range(K)]

    def linear(u, t):
        out = h0 * (1 + 0.3 * np.cos(1.7 * t)) if time_dependent else h0
        for k in range(K):
            out = out + (u[k].real * g_re[k] + u[k].imag * g_im[k] if complex_controls
                         else u[k] * g_re[k])
        return out
    return linear, rng


def _terms(rng, n, kr):
    """One square and one cross pair of the real channels."""
    return [(0, 0, 0.6 * cases_mod.gue(rng, n)), (0, kr - 1, 0.5 * cases_mod.gue(rng, n))]


def _ensemble(base, rng, n, K, M=3, J=2, term_scales=True):
    d = np.stack([cases_mod.gue(rng, n) for _ in range(J)]) if J else None
    return HamiltonianEnsemble(
        base, perturbations=d, offsets=0.3 * rng.standard_normal((M, J)) if J else None,
        control_scales=1 + 0.05 * rng.standard_normal((M, K)), weights=rng.uniform(0.2, 1.0, M),
        quadratic_scales=(1 + 0.2 * rng.standard_normal((M, len(base.pairs)))
                          if term_scales else None))


def tangent(h, controls, evolution_time, complex_controls):
    """(w, t) -> the tangent of the callable h at the knot controls `controls` (central
    differences of h: exact for a quadratic up to rounding)."""
    controls = np.asarray(controls)
    times = np.linspace(0, evolution_time, controls.shape[0])
    K = controls.shape[1]

    def h_tan(w, t):
        u = onp.interpolate_linear_set(t, times, controls)
        out = np.asarray(h(u, t), dtype=np.complex128)
        for k in range(K):
            for unit in ((1.0, 1.0j) if complex_controls else (1.0,)):
                e = np.zeros(K, dtype=controls.dtype)
                e[k] = unit
                slope = (np.asarray(h(u + e, t)) - np.asarray(h(u - e, t))) / 2
                delta = w[k] - u[k]
                out = out + (np.imag(delta) if unit == 1.0j else np.real(delta)) * slope
        return out
    return h_tan


# ---- the constructor ------------------------------------------------------------------------------

def _quadratic_base(n=3):
    return QuadraticHamiltonian(lambda u, t: np.eye(n) * u[0], [(0, 0, np.eye(n)), (0, 1, np.eye(n)),
                                                                (0, 0, np.eye(n))])


@pytest.mark.parametrize("kw, fragment", [
    (dict(quadratic_scales=np.ones((2, 3))), "Q = 2 quadratic terms"),           # merged terms: 2
    (dict(quadratic_scales=np.ones(2)), "quadratic_scales must have 2 dimensions"),
    (dict(quadratic_scales=np.array([[1.0, np.nan]])), "quadratic_scales is not finite"),
    (dict(quadratic_scales=np.array([[1.0, 1.0j]])), "quadratic_scales must be real"),
    (dict(quadratic_scales=np.ones((2, 2)), weights=np.ones(3)), "disagree"),
    (dict(quadratic_scales=np.ones((2, 2)), control_scales=np.ones((4, 2))), "disagree"),
    (dict(quadratic_scales=np.ones((0, 2))), "at least one member"),
])
def test_constructor_checks_quadratic_scales(kw, fragment):
    with pytest.raises(ValueError, match=fragment):
        HamiltonianEnsemble(_quadratic_base(), **kw)


def test_constructor_needs_a_quadratic_base_and_reads_m():
    with pytest.raises(ValueError, match="QuadraticHamiltonian base"):
        HamiltonianEnsemble(lambda u, t: np.eye(3), quadratic_scales=np.ones((2, 2)))
    e = HamiltonianEnsemble(_quadratic_base(), quadratic_scales=np.ones((4, 2)))
    assert e.member_count == 4 and np.array_equal(e.weights, np.full(4, 0.25))
    assert e.quadratic_scales.shape == (4, 2)
    e = HamiltonianEnsemble(_quadratic_base(), weights=np.ones(2))
    assert e.quadratic_scales is None


# ---- member(m) ------------------------------------------------------------------------------------

@pytest.mark.parametrize("complex_controls", [False, True])
@pytest.mark.parametrize("term_scales", [False, True])
def test_member_is_the_formula(complex_controls, term_scales):
    n, K, M, J = 4, 3, 3, 2
    kr = 2 * K if complex_controls else K
    linear, rng = _system(n, K, 7, complex_controls)
    terms = _terms(rng, n, kr)
    e = _ensemble(QuadraticHamiltonian(linear, terms), rng, n, K, M, J, term_scales)
    for m in range(M):
        h = e.member(m)
        for _ in range(3):
            u = rng.standard_normal(K)
            if complex_controls:
                u = u + 1j * rng.standard_normal(K)
            t = rng.uniform(0, 2)
            su = e.control_scales[m] * u
            r = np.stack([su.real, su.imag], axis=1).reshape(-1) if complex_controls else su
            want = linear(su, t) + sum(e.offsets[m, j] * e.perturbations[j] for j in range(J))
            for q, (k, l, mat) in enumerate(terms):
                c = e.quadratic_scales[m, q] if term_scales else 1.0
                want = want + c * r[k] * r[l] * mat
            assert np.allclose(h(u, t), want, rtol=0, atol=1e-13)


# ---- a stand-in backend with the three entry points ----------------------------------------------

class EnsembleQuadraticStandIn(OracleBackend):
    """The oracle backend plus set_ensemble, set_quadratic_terms and
    set_ensemble_quadratic_scales. It expands the seeds into their members on the host, evaluates
    every item on the (K_r + J)-channel problem it was given plus c_mq v_k v_l Q_q (the oracle on
    the item's tangent, slopes written out), and reduces as the engine does."""

    def __init__(self):
        super().__init__()
        self.order = []
        self.ens = self.pairs = self.term_scales = None

    def set_schroedinger_problem(self, *a, **kw):
        super().set_schroedinger_problem(*a, **kw)
        self.order.append("problem")
        self.linear = self.problem.hamiltonian
        self.ens = self.pairs = self.term_scales = None

    def set_quadratic_terms(self, pairs, matrices):
        self.order.append("quadratic")
        self.pairs = np.asarray(pairs, dtype=np.int32).reshape(-1, 2)
        self.matrices = np.asarray(matrices, dtype=np.complex128)
        self.term_scales = None

    def set_ensemble(self, scales, offsets, weights):
        self.order.append("ensemble")
        n, S, K, Nc, N = self.dims
        weights = np.asarray(weights, dtype=np.float64)
        M = weights.shape[0]
        J = 0 if offsets is None else np.asarray(offsets).shape[1]
        scales = np.ones((M, K - J)) if scales is None else np.asarray(scales, dtype=np.float64)
        offsets = np.zeros((M, 0)) if offsets is None else np.asarray(offsets, dtype=np.float64)
        assert scales.shape == (M, K - J) and offsets.shape == (M, J)
        self.ens = (scales, offsets, weights)
        self.term_scales = None

    def set_ensemble_quadratic_scales(self, scales):
        self.order.append("term scales")
        assert self.ens is not None and self.pairs is not None
        scales = np.asarray(scales, dtype=np.float64)
        assert scales.shape == (len(self.ens[2]), len(self.pairs))
        self.term_scales = scales

    def upload_generators(self, generators):
        raise AssertionError("the structured route must not sample generators")

    def upload_controls(self, controls):
        n, S, K, Nc, N = self.dims
        scales, offsets, weights = self.ens
        kr, M = scales.shape[1], len(weights)
        assert self.pairs.max() < kr
        u = np.asarray(controls, dtype=np.float64).reshape(-1, Nc, kr)
        items = np.empty((u.shape[0], M, Nc, K))
        items[..., :kr] = scales[None, :, None, :] * u[:, None]
        items[..., kr:] = offsets[None, :, None, :]
        self.seeds = u.shape[0]
        super().upload_controls(items.reshape(-1, Nc, K))

    def _item_tangent(self, item, v_knots):
        n, S, K, Nc, N = self.dims
        M = len(self.ens[2])
        c = np.ones(len(self.pairs)) if self.term_scales is None else self.term_scales[item % M]
        times = self.problem.control_eval_times
        linear, pairs, mats = self.linear, self.pairs, self.matrices
        zero = np.zeros(K)

        def h_tan(w, t):
            v = onp.interpolate_linear_set(t, times, v_knots)
            h0 = linear(zero, t)
            slopes = [linear(np.eye(K)[k], t) - h0 for k in range(K)]
            out = linear(v, t)
            for q, (k, l) in enumerate(pairs):
                out = out + c[q] * v[k] * v[l] * mats[q]
                slopes[k] = slopes[k] + c[q] * v[l] * mats[q]
                slopes[l] = slopes[l] + c[q] * v[k] * mats[q]
            for k in range(K):
                out = out + (w[k] - v[k]) * slopes[k]
            return out
        return h_tan

    def eval_resident(self, want_grad=True):
        self.calls += 1
        self.cost, self.grads, self.final = [], [], []
        for item, v in enumerate(self.controls):
            self.problem.hamiltonian = self._item_tangent(item, v)
            err, gr, fin = onp.evaluate_with_grad(self.problem, v)
            self.cost.append(err)
            self.grads.append(gr)
            self.final.append(np.asarray(fin)[:, :, 0])
        self.problem.hamiltonian = self.linear

    def download_results(self, want_grad=True, want_final=True):
        n, S, K, Nc, N = self.dims
        scales, offsets, weights = self.ens
        kr, M, B = scales.shape[1], len(weights), self.seeds
        cost, grads, final = super().download_results(want_grad, want_final)
        self.members = cost.reshape(B, M)
        seed_cost = np.zeros(B)
        for m in range(M):
            seed_cost += weights[m] * self.members[:, m]
        seed_grads = None
        if grads is not None:
            g = grads.reshape(B, M, Nc, K)[..., :kr]
            seed_grads = np.zeros((B, Nc, kr))
            for m in range(M):
                seed_grads += (weights[m] * scales[m]) * g[:, m]
        return seed_cost, seed_grads, None if final is None else final.reshape(B, M, S, n)

    def ensemble_member_costs(self):
        return self.members


@pytest.mark.parametrize("complex_controls", [False, True])
@pytest.mark.parametrize("term_scales", [False, True])
def test_stand_in_takes_the_structured_route_and_reduces_the_members(complex_controls, term_scales):
    n, K, N, Nc, S, M, J, B, T = 4, 3, 9, 5, 2, 3, 2, 2, 0.8
    kr = 2 * K if complex_controls else K
    linear, rng = _system(n, K, 31, complex_controls)
    counted = Counted(linear)
    terms = _terms(rng, n, kr)
    base = QuadraticHamiltonian(counted, terms)
    e = _ensemble(base, rng, n, K, M, J, term_scales)
    psi0 = cases_mod.column_states(np.eye(n)[:, :S])
    target = cases_mod.column_states(cases_mod.random_unitary(rng, n)[:, :S])
    norm = ControlNorm(K, Nc, cost_multiplier=0.3)
    backend = EnsembleQuadraticStandIn()
    ev = device.SchroedingerEvaluator(
        T, e, psi0, N, control_count=K, control_eval_count=Nc, complex_controls=complex_controls,
        costs=[TargetStateInfidelity(target), norm], backend=backend)
    assert ev.ensemble is e and ev.quadratic_terms is not None
    assert ev.opaque_hamiltonian is None and ev.linearized_hamiltonian is None
    assert backend.order == ["problem", "quadratic", "ensemble"] + ["term scales"] * term_scales
    assert backend.dims[2] == kr + J
    assert backend.pairs.tolist() == [[0, 0], [0, kr - 1]]
    assert np.array_equal(backend.ens[0], e.real_channel_scales(K, complex_controls))
    if term_scales:
        assert np.array_equal(backend.term_scales, e.quadratic_scales)
    u = 0.5 * rng.standard_normal((B, Nc, K))
    if complex_controls:
        u = u + 0.5j * rng.standard_normal((B, Nc, K))
    counted.calls = 0
    errors, grads, finals, _ = ev.evaluate_batch(u)
    assert counted.calls == 0  # no call of the user's callable during an evaluation
    assert finals.shape == (B, M, S, n, 1)
    members = ev.member_errors()
    assert members.shape == (B, M)
    for b in range(B):
        want_err, want_grad = 0.0, 0.0
        for m in range(M):
            p = onp.SchroedingerProblem(
                T, tangent(e.member(m), u[b], T, complex_controls), psi0, N,
                control_eval_count=Nc, costs=[onp.TargetStateInfidelity(target)],
                complex_controls=complex_controls, control_count=K)
            err, gr, fin = onp.evaluate_with_grad(p, u[b])
            p.hamiltonian = e.member(m)  # the member itself: the same forward evaluation
            err_m, fin_m = onp.evaluate(p, u[b])
            assert abs(err - err_m) < 1e-13 and np.max(np.abs(fin - fin_m)) < 1e-13
            assert abs(members[b, m] - err_m) < 1e-12
            assert np.max(np.abs(finals[b, m] - fin_m)) < 1e-12
            want_err += e.weights[m] * err_m
            want_grad = want_grad + e.weights[m] * gr
        # the costs of the controls: once per seed, on the seed's own controls
        want_err += norm.cost(u[b], None, N - 1)
        want_grad = want_grad + norm.controls_bar(u[b], None, N - 1)
        assert abs(errors[b] - want_err) < 1e-12
        if not complex_controls:
            want_grad = np.real(want_grad)
        assert np.max(np.abs(grads[b] - want_grad)) < 1e-12


def test_the_quadratic_index_check_runs_against_the_seed_channels():
    n, K, N, Nc, J = 4, 3, 7, 4, 2
    linear, rng = _system(n, K, 5)
    psi0 = cases_mod.column_states(np.eye(n)[:, :1])
    target = cases_mod.column_states(np.roll(np.eye(n), 1, axis=0)[:, :1])
    # index 3 is a channel of the (K_r + J)-channel problem, not one of the K_r = 3 seed channels
    base = QuadraticHamiltonian(linear, [(0, K, cases_mod.gue(rng, n))])
    e = _ensemble(base, rng, n, K, 2, J, term_scales=False)
    with pytest.raises(ValueError, match="out of range for 3 real controls"):
        device.SchroedingerEvaluator(0.6, e, psi0, N, control_count=K, control_eval_count=Nc,
                                     costs=[TargetStateInfidelity(target)],
                                     backend=EnsembleQuadraticStandIn())


# ---- rejections -----------------------------------------------------------------------------------

class _NoQuadraticTerms(EnsembleQuadraticStandIn):
    set_quadratic_terms = property()  # hasattr(...) is False


class _NoTermScales(EnsembleQuadraticStandIn):
    set_ensemble_quadratic_scales = property()


def test_rejections():
    n, K, N, Nc = 4, 2, 7, 4
    linear, rng = _system(n, K, 13)
    base = QuadraticHamiltonian(linear, _terms(rng, n, K))
    plain = _ensemble(base, rng, n, K, 2, 1, term_scales=False)
    scaled = _ensemble(base, rng, n, K, 2, 1, term_scales=True)
    psi0 = cases_mod.column_states(np.eye(n)[:, :1])
    target = cases_mod.column_states(np.roll(np.eye(n), 1, axis=0)[:, :1])
    kw = dict(control_count=K, control_eval_count=Nc, costs=[TargetStateInfidelity(target)])
    assert not hasattr(_NoQuadraticTerms(), "set_quadratic_terms")
    assert not hasattr(_NoTermScales(), "set_ensemble_quadratic_scales")
    for magnus in (MagnusPolicy.M4, MagnusPolicy.M6):
        with pytest.raises(NotImplementedError, match="linear in the controls"):
            device.SchroedingerEvaluator(0.6, plain, psi0, N, magnus_policy=magnus,
                                         backend=EnsembleQuadraticStandIn(), **kw)
    with pytest.raises(NotImplementedError, match="linear in the controls"):
        device.SchroedingerEvaluator(0.6, plain, psi0, N, backend=_NoQuadraticTerms(), **kw)
    with pytest.raises(NotImplementedError, match="linear in the controls"):
        device.SchroedingerEvaluator(0.6, scaled, psi0, N, backend=_NoTermScales(), **kw)
    # ... which takes the ensemble without term scales
    ev = device.SchroedingerEvaluator(0.6, plain, psi0, N, backend=_NoTermScales(), **kw)
    assert ev.quadratic_terms is not None and ev.ensemble is plain


def test_the_abi_declares_the_entry_point():
    lib = engine.load_library()
    assert "qocx_set_ensemble_quadratic_scales" in engine.SIGNATURES
    assert hasattr(lib, "qocx_set_ensemble_quadratic_scales")
    assert hasattr(engine.Engine, "set_ensemble_quadratic_scales")
