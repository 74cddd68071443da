"""
action_degree_model.py - TEST INFRASTRUCTURE: a NumPy twin of the degree rule of the matrix-free route
(qoc_amd/csrc/qocx_action.h: action_degree_normal, action_degree_rule; knob "action_degree").

A step's generator a = -i dt H is normal when H is Hermitian: its eigenvalues i lambda lie on the
imaginary axis, |lambda| <= beta = ||a||_2, and in the eigenbasis T_m(a) psi - exp(a) psi is the
Lagrange remainder of e^(i lambda) entry by entry - at most beta^(m+1) / (m+1)! ||psi||. Asking that to
be <= 2^-53 gives theta'_m = ((m+1)! 2^-53)^(1/(m+1)); the table below holds each rounded DOWN to a
double (the inequality holds at the table's value in exact arithmetic). The degree of a step is the
lesser of the Al-Mohy-Higham degree of its 1-norm bound (tests/action_model.py: degree_for) and the
degree of its spectral-norm bound by this table.

Nothing here is imported by the product.
"""

from fractions import Fraction
from math import factorial

import numpy as np

from oracle import qoc_numpy as onp
from tests import action_model as am

MAX_DEGREE = am.MAX_DEGREE
THETA_NORMAL = {
    1: 1.4901161193847656e-08, 2: 8.733476581980375e-06, 3: 0.00022719845192922352,
    4: 0.0016784882105346471, 5: 0.006563323151782549, 6: 0.01777016817886154,
    7: 0.038138740273514826, 8: 0.06998730192918919, 9: 0.11495221029281477,
    10: 0.17401909444156718, 11: 0.24763513660365769, 12: 0.3358381601514265,
    13: 0.43837339055193697, 14: 0.5547883372015275, 15: 0.6845053769594961,
    16: 0.8268751230769177, 17: 0.9812145020859808, 18: 1.1468331956329982}


def remainder_holds(beta, m):
    """beta^(m+1) / (m+1)! <= 2^-53, in exact rational arithmetic."""
    return Fraction(beta) ** (m + 1) <= Fraction(factorial(m + 1), 2 ** 53)


def degree_normal(beta):
    """The least m with beta <= theta'_m; MAX_DEGREE + 1 above theta'_18 and for NaN."""
    for m in range(1, MAX_DEGREE + 1):
        if beta <= THETA_NORMAL[m]:
            return m
    return MAX_DEGREE + 1


def degree_rule(bound1, bound2, rule=1):
    m1 = am.degree_for(bound1)
    return m1 if rule == 0 else min(m1, degree_normal(bound2))


def step_bounds(h0, g, N, T, controls, norms2=None):
    """Per step of one seed (controls [Nc, K], linear interpolation at the midpoints, M2):
    (|dt| (||H0||_1 + sum |u_k| ||G_k||_1), |dt| (rho(H0) + sum |u_k| rho(G_k))) as the step table forms
    them. norms2: [rho(H0), rho(G_1), ...] - None: the exact spectral radii; a test that compares degrees
    with the engine passes the engine's own upper bounds (qocx_debug_spectral_bound, at most 1 % above)."""
    controls = np.asarray(controls, dtype=np.float64)
    nc, K = controls.shape
    nsteps = N - 1
    dt = T / nsteps
    times = np.linspace(0, T, nc)
    n1 = [onp.one_norm(h0)] + [onp.one_norm(m) for m in g]
    n2 = list(norms2) if norms2 is not None else [spectral_radius(h0)] + [spectral_radius(m) for m in g]
    out = []
    for j in range(nsteps):
        u = onp.interpolate_linear_set(j * dt + 0.5 * dt, times, controls)
        out.append((abs(dt) * (n1[0] + sum(abs(u[k]) * n1[k + 1] for k in range(K))),
                    abs(dt) * (n2[0] + sum(abs(u[k]) * n2[k + 1] for k in range(K)))))
    return out


def spectral_radius(m):
    return float(np.abs(np.linalg.eigvalsh(m)).max())


def margin_to_thresholds(bounds, rule=1):
    """The least relative distance of any step's bound to a threshold of its table (both tables under
    rule 1): a device bound that differs from the model's in the last digits must not change a degree."""
    worst = np.inf
    for b1, b2 in bounds:
        for th in am.THETA.values():
            worst = min(worst, abs(b1 - th) / th)
        if rule:
            for th in THETA_NORMAL.values():
                worst = min(worst, abs(b2 - th) / th)
    return worst


def evaluate_with_grad(h0, g, psi0, target, N, T, controls, rule=1):
    """tests/action_model.py's evaluation with the per-step degrees of the rule. Returns (cost, grads,
    final state, degrees)."""
    degrees = [degree_rule(b1, b2, rule) for b1, b2 in step_bounds(h0, g, N, T, controls)]
    return evaluate_with_degrees(h0, g, psi0, target, N, T, controls, degrees)


def evaluate_with_degrees(h0, g, psi0, target, N, T, controls, degrees):
    controls = np.asarray(controls, dtype=np.float64)
    nc, K = controls.shape
    nsteps = N - 1
    dt = T / nsteps
    times = np.linspace(0, T, nc)
    gens = []
    for j in range(nsteps):
        u = onp.interpolate_linear_set(j * dt + 0.5 * dt, times, controls)
        gens.append(-1j * dt * (h0 + sum(u[k] * g[k] for k in range(K))))
    psi = np.asarray(psi0, dtype=np.complex128)
    vs = []
    for j in range(nsteps):
        psi, v = am.forward_step(gens[j], psi, degrees[j])
        vs.append(v)
    ip = np.vdot(target, psi)
    cost = 1.0 - abs(ip) ** 2
    c = -2.0 * ip
    lam = np.asarray(target, dtype=np.complex128)
    grads = np.zeros((nc, K))
    for j in range(nsteps - 1, -1, -1):
        lam, w = am.adjoint_step(gens[j], lam, degrees[j])
        abar = am.generator_cotangent(vs[j], w, degrees[j])
        i1, w1, i2, w2 = onp.interpolation_weights(j * dt + 0.5 * dt, times)
        for k in range(K):
            gamma = np.sum(np.conj(abar) * (-1j * dt * g[k]))
            gk = np.real(np.conj(c) * gamma)
            grads[i1, k] += w1 * gk
            grads[i2, k] += w2 * gk
    return cost, grads, psi, degrees
