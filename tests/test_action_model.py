"""
CPU tests of the matrix-free route's mathematics (tests/action_model.py, the NumPy restatement of
qoc_amd/csrc/qocx_action.hip): the truncated Taylor series applied to the state and to the
back-propagated target, with the exact reverse rule of the polynomial, equals the oracle
(onp.evaluate_with_grad: [13/13] Pade with squaring and its adjoint) at the project's gates -
1e-10 for cost and final state, 1e-8 of the largest entry for the gradient.
"""

import numpy as np
import pytest

from oracle import qoc_numpy as onp
from tests import action_model as am
from tests.helpers import rel_err


def hermitian(rng, n):
    m = rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))
    m = (m + m.conj().T) / 2
    return m / onp.one_norm(m)


def problem(n, seed, amplitude=1.0, N=13, K=2, dt=0.05):
    rng = np.random.default_rng(seed)
    h0, g = hermitian(rng, n), [hermitian(rng, n) for _ in range(K)]
    psi0 = np.eye(n, dtype=np.complex128)[0]
    target = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    target /= np.linalg.norm(target)
    controls = amplitude * rng.uniform(-1, 1, (N, K))
    T = dt * (N - 1)
    oracle = onp.SchroedingerProblem(
        T, lambda u, t: h0 + sum(u[k] * g[k] for k in range(K)), psi0[None, :, None], N,
        control_eval_count=N, costs=[onp.TargetStateInfidelity(target[None, :, None])],
        control_count=K)
    return dict(h0=h0, g=g, psi0=psi0, target=target, N=N, T=T, controls=controls, oracle=oracle)


@pytest.mark.parametrize("n", [5, 17])
@pytest.mark.parametrize("degree", [None, "+2", 18])
def test_model_equals_oracle(n, degree):
    """12 steps; the degree of every step from the bound (None), two above it, and the largest."""
    p = problem(n, 100 + n)
    _, _, _, natural = am.evaluate_with_grad(p["h0"], p["g"], p["psi0"], p["target"], p["N"], p["T"],
                                             p["controls"])
    assert len(natural) == 12 and 8 <= min(natural) <= max(natural) <= 11, natural
    if degree == "+2":
        degree = max(natural) + 2
    cost, grads, final, used = am.evaluate_with_grad(p["h0"], p["g"], p["psi0"], p["target"], p["N"],
                                                     p["T"], p["controls"], degree=degree)
    ref_cost, ref_grads, ref_final = onp.evaluate_with_grad(p["oracle"], p["controls"])
    print("n={} degrees {}: cost {:.1e} final {:.1e} grad {:.1e}".format(
        n, sorted(set(used)), abs(cost - ref_cost), np.abs(final - ref_final[0, :, 0]).max(),
        rel_err(grads, ref_grads)))
    assert abs(cost - ref_cost) < 1e-10
    assert np.abs(final - ref_final[0, :, 0]).max() < 1e-10
    assert rel_err(grads, ref_grads) < 1e-8


@pytest.mark.parametrize("n", [5, 17])
@pytest.mark.parametrize("m", [1, 2, 7, 12, 18])
def test_generator_cotangent_is_the_reverse_rule_of_the_polynomial(n, m):
    rng = np.random.default_rng(7 * n + m)
    a = -1j * 0.2 * hermitian(rng, n)
    psi = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    lam = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    psi /= np.linalg.norm(psi)
    lam /= np.linalg.norm(lam)
    _, v = am.forward_step(a, psi, m)
    _, w = am.adjoint_step(a, lam, m)
    abar = am.generator_cotangent(v, w, m)
    dense = am.dense_reverse_rule(a, psi, lam, m)
    assert np.abs(abar - dense).max() < 1e-13 * max(1.0, np.abs(dense).max())
    # and it IS the derivative: <abar, E> = d/de Re <lam, T_m(a + e E) psi> for a direction E
    e = rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))
    h = 1e-6
    up, _ = am.forward_step(a + h * e, psi, m)
    dn, _ = am.forward_step(a - h * e, psi, m)
    numeric = np.real(np.vdot(lam, up - dn)) / (2 * h)
    assert abs(np.real(np.sum(np.conj(abar) * e)) - numeric) < 1e-8 * max(1.0, abs(numeric))


def test_degree_follows_the_theta_table():
    assert sorted(am.THETA) == list(range(1, am.MAX_DEGREE + 1))
    for m in range(1, am.MAX_DEGREE + 1):
        assert am.degree_for(am.THETA[m]) == m
        assert am.degree_for(am.THETA[m] * 0.98) == m
        assert am.degree_for(am.THETA[m] * 1.02) == m + 1
    assert am.degree_for(0.0) == 1
    assert am.degree_for(float("nan")) == am.MAX_DEGREE + 1


def test_device_header_carries_the_same_table():
    import os
    import re
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "qoc_amd", "csrc",
                        "qocx_action.h")
    found = {int(m): float(v) for m, v in re.findall(r"case (\d+): return ([0-9.e-]+);", open(path).read())}
    assert found == am.THETA
