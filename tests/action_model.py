"""
action_model.py - TEST INFRASTRUCTURE: a NumPy model of the matrix-free route
(qoc_amd/csrc/qocx_action.hip), in the style of tests/device_model.py, so that its mathematics is
checked against the oracle on the CPU before, and independently of, the device code.

Per step, with a = -i dt H(u_mid) skew-Hermitian and Taylor degree m (Al-Mohy & Higham 2011):

  forward   v_0 = psi,     v_p = a v_(p-1) / p,    psi'   = sum_{p=0..m} v_p
  adjoint   w_0 = lambda', w_p = -a w_(p-1) / p,   lambda = sum_{p=0..m} w_p         (a^H = -a)
  abar      = sum_{i<m} w_i rho_i^H,  rho_i = sum_{l<m-i} c_il v_l,  c_il = i! l! / (i + l + 1)!
  gamma_k   = sum conj(abar) (.) (-i dt G_k)   per step, under the unit adjoint: lambda_N is the
              target, and the gradient is Re(conj(c) gamma_k) with the cost's scalar c

Nothing here is imported by the product.
"""

from math import factorial

import numpy as np

from oracle import qoc_numpy as onp

MAX_DEGREE = 18
# theta_m, m = 1 .. 18: scipy.sparse.linalg._expm_multiply._theta (Al-Mohy & Higham 2011, Table 3.1)
THETA = {1: 2.29e-16, 2: 2.58e-8, 3: 1.39e-5, 4: 3.40e-4, 5: 2.40e-3, 6: 9.07e-3, 7: 2.38e-2,
         8: 5.00e-2, 9: 8.96e-2, 10: 1.44e-1, 11: 2.14e-1, 12: 3.00e-1, 13: 4.00e-1, 14: 5.14e-1,
         15: 6.41e-1, 16: 7.81e-1, 17: 9.31e-1, 18: 1.09}


def degree_for(bound):
    """The least m with bound <= theta_m; MAX_DEGREE + 1 above theta_18."""
    for m in range(1, MAX_DEGREE + 1):
        if bound <= THETA[m]:
            return m
    return MAX_DEGREE + 1


def coefficient(i, l):
    return factorial(i) * factorial(l) / factorial(i + l + 1)


def taylor_terms(a, x, m):
    """[x, a x, a^2 x / 2, ..., a^m x / m!]"""
    terms = [np.asarray(x, dtype=np.complex128)]
    for p in range(1, m + 1):
        terms.append(a @ terms[-1] / p)
    return terms


def forward_step(a, psi, m):
    v = taylor_terms(a, psi, m)
    return sum(v), v[:m]


def adjoint_step(a, lam, m):
    w = taylor_terms(-a, lam, m)
    return sum(w), w[:m]


def generator_cotangent(v, w, m):
    abar = np.zeros((len(v[0]), len(v[0])), dtype=np.complex128)
    for i in range(m):
        rho = sum(coefficient(i, l) * v[l] for l in range(m - i))
        abar += np.outer(w[i], rho.conj())
    return abar


def dense_reverse_rule(a, psi, lam, m):
    """Cotangent of a in psi' = T_m(a) psi, T_m(a) = sum_{p<=m} a^p / p!, written out with matrix
    powers: abar = sum_p 1/p! sum_{i+l=p-1} (a^H)^i lam psi^H (a^H)^l."""
    n = a.shape[0]
    ah = a.conj().T
    powers = [np.eye(n, dtype=np.complex128)]
    for _ in range(m):
        powers.append(powers[-1] @ ah)
    ubar = np.outer(lam, psi.conj())
    abar = np.zeros((n, n), dtype=np.complex128)
    for p in range(1, m + 1):
        for i in range(p):
            abar += powers[i] @ ubar @ powers[p - 1 - i] / factorial(p)
    return abar


def evaluate_with_grad(h0, g, psi0, target, N, T, controls, degree=None, scale=1.0):
    """One state, one final TargetStateInfidelity (cost multiplier `scale`), M2, linear interpolation
    of controls [Nc, K]. degree: forced for every step, or None - from the step table's bound
    dt (||H0||_1 + sum |u_k| ||G_k||_1). Returns (cost, grads [Nc, K], final state, degrees)."""
    controls = np.asarray(controls, dtype=np.float64)
    nc, K = controls.shape
    nsteps = N - 1
    dt = T / nsteps
    times = np.linspace(0, T, nc)
    h0n = onp.one_norm(h0)
    gn = [onp.one_norm(m) for m in g]
    gens, degrees = [], []
    for j in range(nsteps):
        u = onp.interpolate_linear_set(j * dt + 0.5 * dt, times, controls)
        bound = abs(dt) * (h0n + sum(abs(u[k]) * gn[k] for k in range(K)))
        degrees.append(degree if degree is not None else degree_for(bound))
        gens.append(-1j * dt * (h0 + sum(u[k] * g[k] for k in range(K))))
    psi = np.asarray(psi0, dtype=np.complex128)
    vs = []
    for j in range(nsteps):
        psi, v = forward_step(gens[j], psi, degrees[j])
        vs.append(v)
    ip = np.vdot(target, psi)
    cost = scale * (1.0 - abs(ip) ** 2)
    c = -2.0 * scale * ip  # the cotangent of the final state is c * target
    lam = np.asarray(target, dtype=np.complex128)
    grads = np.zeros((nc, K))
    for j in range(nsteps - 1, -1, -1):
        lam, w = adjoint_step(gens[j], lam, degrees[j])
        abar = generator_cotangent(vs[j], w, degrees[j])
        i1, w1, i2, w2 = onp.interpolation_weights(j * dt + 0.5 * dt, times)
        for k in range(K):
            gamma = np.sum(np.conj(abar) * (-1j * dt * g[k]))
            gk = np.real(np.conj(c) * gamma)
            grads[i1, k] += w1 * gk
            grads[i2, k] += w2 * gk
    return cost, grads, psi, degrees
