"""
action_costs_model.py - TEST INFRASTRUCTURE: the NumPy model of tests/action_model.py under any set of
state-cost descriptors (qoc_amd/csrc/qocx_action_costs.hip): one state, the truncated Taylor series per
step, and the GENERAL adjoint - the sweep carries the true cotangent instead of the target.

  forward   psi_(j+1) = T_m(a_j) psi_j, v_0 .. v_(m-1) kept. Step costs are evaluated on psi_j at the
            system steps j != 0 with j % cost_eval_step == 0 (before the step leaves psi_j), and at the
            end first the step costs, if (N - 1) % cost_eval_step == 0, then the final costs.
  adjoint   lambda_(N-1) = the cotangent of the costs evaluated on the final state; for j = N - 2 .. 0:
            lambda <- T_m(a_j)^H lambda (w_0 .. w_(m-1) kept), then, if j is a cost step, lambda += the
            cotangent of the step costs at psi_j = v_0 of step j.
  gradient  abar_j = sum_i w_i rho_i^H (action_model.generator_cotangent), and the step gradient is the
            real number Re sum conj(abar_j) (.) (-i dt G_k): no scalar is applied afterwards.

The costs are tests/state_costs.py::DescriptorCost (cost and states_bar in the convention dC/dRe + i
dC/dIm of the device's eval_costs). Nothing here is imported by the product.
"""

import numpy as np

from oracle import qoc_numpy as onp
from tests import action_model as am


def _cost_and_bar(costs, psi, step, step_pass, final_pass, want_bar):
    """The costs selected as the device selects them (a step descriptor on a step pass, a final one on
    the final pass) on the state psi (n,): (sum, cotangent (n,) or None)."""
    total, bar = 0.0, np.zeros(len(psi), dtype=np.complex128) if want_bar else None
    states = psi[None, :, None]
    for c in costs:
        if not (step_pass if c.requires_step_evaluation else final_pass):
            continue
        total += c.cost(None, states, step)
        if want_bar:
            bar += c.states_bar(None, states, step)[0, :, 0]
    return total, bar


def evaluate_with_grad(h0, g, psi0, costs, cost_eval_step, N, T, controls, degree=None, want_grad=True):
    """One state, M2, linear interpolation of controls [Nc, K], `costs` DescriptorCosts. degree: forced
    for every step, or None - from the step table's bound. Returns (cost, grads [Nc, K] or None, final
    state, degrees)."""
    controls = np.asarray(controls, dtype=np.float64)
    nc, K = controls.shape
    nsteps = N - 1
    dt = T / nsteps
    times = np.linspace(0, T, nc)
    h0n = onp.one_norm(h0)
    gn = [onp.one_norm(m) for m in g]
    ces = cost_eval_step
    has_step = any(c.requires_step_evaluation for c in costs)

    def cost_step(j):
        return j != 0 and has_step and j % ces == 0

    gens, degrees = [], []
    for j in range(nsteps):
        u = onp.interpolate_linear_set(j * dt + 0.5 * dt, times, controls)
        bound = abs(dt) * (h0n + sum(abs(u[k]) * gn[k] for k in range(K)))
        degrees.append(degree if degree is not None else am.degree_for(bound))
        gens.append(-1j * dt * (h0 + sum(u[k] * g[k] for k in range(K))))
    psi = np.asarray(psi0, dtype=np.complex128)
    vs, cost = [], 0.0
    for j in range(nsteps):
        if cost_step(j):
            cost += _cost_and_bar(costs, psi, j, True, False, False)[0]
        psi, v = am.forward_step(gens[j], psi, degrees[j])
        vs.append(v)
    if cost_step(nsteps):
        cost += _cost_and_bar(costs, psi, nsteps, True, False, False)[0]
    cost += _cost_and_bar(costs, psi, nsteps, False, True, False)[0]
    if not want_grad:
        return cost, None, psi, degrees
    lam = _cost_and_bar(costs, psi, nsteps, cost_step(nsteps), True, True)[1]
    grads = np.zeros((nc, K))
    for j in range(nsteps - 1, -1, -1):
        lam, w = am.adjoint_step(gens[j], lam, degrees[j])
        abar = am.generator_cotangent(vs[j], w, degrees[j])
        i1, w1, i2, w2 = onp.interpolation_weights(j * dt + 0.5 * dt, times)
        for k in range(K):
            gk = np.real(np.sum(np.conj(abar) * (-1j * dt * g[k])))
            grads[i1, k] += w1 * gk
            grads[i2, k] += w2 * gk
        if cost_step(j):
            lam = lam + _cost_and_bar(costs, vs[j][0], j, True, False, True)[1]
    return cost, grads, psi, degrees
