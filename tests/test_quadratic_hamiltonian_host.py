"""CPU tests of qoc_amd.standard.QuadraticHamiltonian and its host routing (no GPU): the
constructor's checks, the callable contract, the oracle backend (where it is just a callable) and
a stand-in backend that takes quadratic terms (where the callable must not be called per
evaluation)."""

import numpy as np
import pytest

from oracle import qoc_numpy as onp
from qoc_amd import engine
from qoc_amd.core import device
from qoc_amd.models import MagnusPolicy
from qoc_amd.standard import QuadraticHamiltonian, TargetStateInfidelity
from tests import cases as cases_mod
from tests.oracle_backend import OracleBackend


def _system(n=5, K=2, seed=3, complex_controls=False, time_dependent=False):
    rng = np.random.default_rng(seed)
    h0 = cases_mod.gue(rng, n)
    g_re = [cases_mod.gue(rng, n) for _ in range(K)]
    g_im = [cases_mod.gue(rng, n) for _ in range(K)]

    def linear(u, t):
        out = h0 * (1 + 0.3 * np.cos(1.7 * t)) if time_dependent else h0
        if u is None:
            return out
        for k in range(K):
            out = out + (u[k].real * g_re[k] + u[k].imag * g_im[k] if complex_controls
                         else u[k] * g_re[k])
        return out
    return linear, rng


class Counted(object):
    """Counts the calls of a callable."""

    def __init__(self, fn):
        self.fn, self.calls = fn, 0

    def __call__(self, *a):
        self.calls += 1
        return self.fn(*a)


# ---- the constructor ------------------------------------------------------------------------------

@pytest.mark.parametrize("terms, fragment", [
    ([(1, 0, np.eye(3))], "0 <= k <= l"),
    ([(-1, 0, np.eye(3))], "0 <= k <= l"),
    ([(0.5, 1, np.eye(3))], "integers"),
    ([(0, 1, np.ones((3, 2)))], "square"),
    ([(0, 1, np.eye(3)), (1, 1, np.eye(4))], "shape"),
    ([(0, 0, np.full((3, 3), np.nan))], "finite"),
    ([(0, 0)], "(k, l, Q)"),
])
def test_constructor_rejects_bad_terms(terms, fragment):
    with pytest.raises(ValueError, match=fragment.replace("(", r"\(").replace(")", r"\)")):
        QuadraticHamiltonian(lambda u, t: np.eye(3), terms)


def test_constructor_rejects_a_non_callable_and_merges_repeated_pairs():
    with pytest.raises(ValueError):
        QuadraticHamiltonian(np.eye(3), [])
    q1, q2 = np.diag([1.0, 2.0, 3.0]), np.eye(3) * 1j
    h = QuadraticHamiltonian(lambda u, t: np.zeros((3, 3)), [(0, 1, q1), (2, 2, q2), (0, 1, q2)])
    assert h.pairs.tolist() == [[0, 1], [2, 2]]
    assert np.array_equal(h.matrices[0], q1 + q2) and np.array_equal(h.matrices[1], q2)
    with pytest.raises(ValueError, match="out of range"):
        h(np.zeros(2), 0.0)


# ---- the callable contract ----------------------------------------------------------------------

@pytest.mark.parametrize("complex_controls", [False, True])
def test_call_equals_the_explicit_sum(complex_controls):
    n, K = 4, 2
    linear, rng = _system(n, K, complex_controls=complex_controls, time_dependent=True)
    kr = 2 * K if complex_controls else K
    terms = [(0, 0, cases_mod.gue(rng, n)), (0, kr - 1, rng.standard_normal((n, n)) + 0j),
             (1, kr - 1, cases_mod.gue(rng, n))]
    h = QuadraticHamiltonian(linear, terms)
    for _ in range(5):
        u = rng.standard_normal(K)
        if complex_controls:
            u = u + 1j * rng.standard_normal(K)
        t = rng.uniform(0, 3)
        r = np.empty(kr)
        if complex_controls:
            r[0::2], r[1::2] = u.real, u.imag
        else:
            r[:] = u
        want = linear(u, t) + sum(r[k] * r[l] * q for k, l, q in terms)
        assert np.allclose(h(u, t), want, rtol=0, atol=1e-14)


# ---- the oracle backend: a QuadraticHamiltonian is just a callable there -------------------------

def _evaluator(hamiltonian, backend, magnus=MagnusPolicy.M2, n=5, K=2, N=9, Nc=5, S=1,
               complex_controls=False):
    psi0 = cases_mod.column_states(np.eye(n)[:, :S])
    target = cases_mod.column_states(np.roll(np.eye(n), 1, axis=0)[:, :S])
    return device.SchroedingerEvaluator(
        0.8, hamiltonian, psi0, N, control_count=K, control_eval_count=Nc,
        complex_controls=complex_controls, costs=[TargetStateInfidelity(target)],
        magnus_policy=magnus, backend=backend), psi0, target


def _quadratic_and_plain(n=5, K=2, seed=11):
    linear, rng = _system(n, K, seed=seed, time_dependent=True)
    terms = [(0, 0, 0.7 * cases_mod.gue(rng, n)), (0, 1, 0.4 * cases_mod.gue(rng, n))]
    quad = QuadraticHamiltonian(linear, terms)
    plain = lambda u, t: quad(u, t)  # noqa: E731 - the same function, no type to recognise
    return quad, plain, rng


def test_oracle_backend_takes_the_callable_route_with_the_same_results():
    quad, plain, rng = _quadratic_and_plain()
    controls = 0.6 * rng.standard_normal((2, 5, 2))
    ev_q, _, _ = _evaluator(quad, OracleBackend(), magnus=MagnusPolicy.M4)
    ev_p, _, _ = _evaluator(plain, OracleBackend(), magnus=MagnusPolicy.M4)
    assert ev_q.quadratic_terms is None and ev_q.linearized_hamiltonian is quad
    out_q = ev_q.evaluate_batch(controls)
    out_p = ev_p.evaluate_batch(controls)
    for a, b in zip(out_q[:3], out_p[:3]):
        assert np.array_equal(a, b)
    # M2 on a backend without qocx_set_quadratic_terms: today's opaque route
    ev_m2, _, _ = _evaluator(quad, OracleBackend())
    assert ev_m2.quadratic_terms is None and ev_m2.opaque_hamiltonian is quad


def test_plain_callables_keep_their_routes():
    _, plain, _ = _quadratic_and_plain()
    ev, _, _ = _evaluator(plain, QuadraticStandIn())
    assert ev.opaque_hamiltonian is plain and ev.quadratic_terms is None


# ---- a stand-in backend WITH the entry point ------------------------------------------------------

class QuadraticStandIn(OracleBackend):
    """The oracle backend plus qocx_set_quadratic_terms: it adds sum r_k r_l Q_kl to the linear
    problem it was given (forward only; the oracle's gradient assumes a linear Hamiltonian)."""

    def __init__(self):
        super().__init__()
        self.received = []

    def set_schroedinger_problem(self, *a, **kw):
        super().set_schroedinger_problem(*a, **kw)
        self.linear = self.problem.hamiltonian
        self.terms = None

    def set_quadratic_terms(self, pairs, matrices):
        pairs = np.asarray(pairs, dtype=np.int32).reshape(-1, 2)
        matrices = np.asarray(matrices, dtype=np.complex128)
        self.received.append((pairs.copy(), matrices.copy()))
        linear = self.linear

        def hamiltonian(u, t):
            out = linear(u, t)
            for (k, l), q in zip(pairs, matrices):
                out = out + u[k] * u[l] * q
            return out
        self.problem.hamiltonian = hamiltonian

    def upload_generators(self, generators):
        raise AssertionError("the quadratic route must not sample generators")


@pytest.mark.parametrize("complex_controls", [False, True])
def test_stand_in_receives_the_terms_and_no_callable_call_during_evaluation(complex_controls):
    n, K, N, Nc = 5, 2, 9, 5
    linear, rng = _system(n, K, seed=21, complex_controls=complex_controls, time_dependent=True)
    kr = 2 * K if complex_controls else K
    q0, q1, q2 = (cases_mod.gue(rng, n) for _ in range(3))
    terms = [(0, 0, q0), (1, kr - 1, q1), (0, 0, q2)]
    counted = Counted(linear)
    h = QuadraticHamiltonian(counted, terms)
    backend = QuadraticStandIn()
    ev, psi0, target = _evaluator(h, backend, complex_controls=complex_controls)
    assert ev.opaque_hamiltonian is None and ev.linearized_hamiltonian is None
    assert len(backend.received) == 1
    pairs, mats = backend.received[0]
    assert pairs.tolist() == [[0, 0], [1, kr - 1]]
    assert np.array_equal(mats[0], q0 + q2) and np.array_equal(mats[1], q1)
    controls = 0.5 * rng.standard_normal((3, Nc, K))
    if complex_controls:
        controls = controls + 0.5j * rng.standard_normal((3, Nc, K))
    counted.calls = 0
    errors, _, finals, _ = ev.evaluate_batch(controls, want_grad=False)
    assert counted.calls == 0
    problem = onp.SchroedingerProblem(
        0.8, h, psi0, N, control_eval_count=Nc,
        costs=[onp.TargetStateInfidelity(target)], complex_controls=complex_controls,
        control_count=K)
    for b in range(3):
        err, fin = onp.evaluate(problem, controls[b])
        assert abs(err - errors[b]) < 1e-12
        assert np.max(np.abs(fin - finals[b])) < 1e-12


def test_stand_in_rejects_out_of_range_indices_and_other_policies_take_the_callable():
    linear, rng = _system(5, 2, seed=5)
    with pytest.raises(ValueError, match="out of range"):
        _evaluator(QuadraticHamiltonian(linear, [(0, 2, np.eye(5))]), QuadraticStandIn())
    h = QuadraticHamiltonian(linear, [(0, 1, cases_mod.gue(rng, 5))])
    backend = QuadraticStandIn()
    ev, _, _ = _evaluator(h, backend, magnus=MagnusPolicy.M4)
    assert ev.quadratic_terms is None and ev.linearized_hamiltonian is h
    assert backend.received == []


def test_the_abi_declares_the_entry_point():
    assert "qocx_set_quadratic_terms" in engine.SIGNATURES
    assert hasattr(engine.load_library(), "qocx_set_quadratic_terms")
    assert hasattr(engine.Engine, "set_quadratic_terms")


def test_route_follows_the_backend_the_factory_makes():
    """backend=None: the route is decided on the backend make_backend() returns (here the oracle
    backend, which has no quadratic entry point: the callable route)."""
    from tests import helpers
    quad, _, _ = _quadratic_and_plain()
    helpers.set_backend_factory(OracleBackend)
    try:
        ev, _, _ = _evaluator(quad, None, magnus=MagnusPolicy.M4)
        assert ev.quadratic_terms is None and ev.linearized_hamiltonian is quad
        helpers.set_backend_factory(QuadraticStandIn)
        ev, _, _ = _evaluator(quad, None)
        assert ev.quadratic_terms is not None and isinstance(ev.backend, QuadraticStandIn)
    finally:
        helpers.set_backend_factory(None)
