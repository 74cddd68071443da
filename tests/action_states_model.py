"""
action_states_model.py - TEST INFRASTRUCTURE: the NumPy model of tests/action_model.py for S states per
seed under one coherent final TargetStateInfidelity (qoc_amd/csrc/qocx_action_states.hip).

The S forward chains and the S back-propagated targets are independent and each is the arithmetic of
the one-state model. The states meet in two places:

  cost      1 - |sum_s <t_s|psi_s>|^2 / S^2, and the cotangent of final state s is c t_s with ONE scalar
            c = -2 scale sum_s <t_s|psi_s> / S^2
  abar      = sum_s sum_{i<m} w_(s,i) rho_(s,i)^H per step (the states in the order s = 0 .. S - 1), ONE
            contraction gamma_k = sum conj(abar) (.) (-i dt G_k), gradient Re(conj(c) gamma_k)

Nothing here is imported by the product.
"""

import numpy as np

from oracle import qoc_numpy as onp
from tests.action_model import adjoint_step, degree_for, forward_step, generator_cotangent


def evaluate_with_grad(h0, g, psi0, target, N, T, controls, degree=None, scale=1.0):
    """psi0, target [S, n]; controls [Nc, K]; otherwise as action_model.evaluate_with_grad, whose
    operations these are at S = 1. Returns (cost, grads [Nc, K], final states [S, n], degrees)."""
    controls = np.asarray(controls, dtype=np.float64)
    psi0 = np.asarray(psi0, dtype=np.complex128)
    target = np.asarray(target, dtype=np.complex128)
    S = psi0.shape[0]
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
    psi = [psi0[s] for s in range(S)]
    vs = [[] for _ in range(S)]
    for j in range(nsteps):
        for s in range(S):
            psi[s], v = forward_step(gens[j], psi[s], degrees[j])
            vs[s].append(v)
    ip = np.vdot(target[0], psi[0])
    for s in range(1, S):
        ip = ip + np.vdot(target[s], psi[s])
    cost = scale * (1.0 - abs(ip) ** 2 / (S * S))
    c = -2.0 * scale * ip / (S * S)  # the cotangent of final state s is c * target[s]
    lam = [target[s] for s in range(S)]
    grads = np.zeros((nc, K))
    for j in range(nsteps - 1, -1, -1):
        abar = None
        for s in range(S):
            lam[s], w = adjoint_step(gens[j], lam[s], degrees[j])
            part = generator_cotangent(vs[s][j], w, degrees[j])
            abar = part if abar is None else abar + part
        i1, w1, i2, w2 = onp.interpolation_weights(j * dt + 0.5 * dt, times)
        for k in range(K):
            gamma = np.sum(np.conj(abar) * (-1j * dt * g[k]))
            gk = np.real(np.conj(c) * gamma)
            grads[i1, k] += w1 * gk
            grads[i2, k] += w2 * gk
    return cost, grads, np.stack(psi), degrees
