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

evaluate_with_grad is the route as it was first built (one state, one final target, linear controls);
evaluate_features the same mathematics at any control count and knot count, under piecewise-constant
controls, several states and any oracle costs, with the ways a kernel could get those wrong (MUTANTS).

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


# ---- any K, any Nc, piecewise-constant controls, several states, any oracle costs -------------------

MUTANTS = ("generator without k >= 2", "gradient without k >= 2", "wrong step for k >= 2",
           "second image at K = 1", "slice off by one", "transposed knot weights")


def step_controls(controls, N, T, interpolation="linear", mutant=None):
    """What a step reads and where its cotangent goes: (u [N - 1, K], [[(knot, weight), ...]] per step).
    Linear: the oracle's interpolation at the step's midpoint and its transpose. Piecewise constant: the
    slice of the midpoint by tests/piecewise_constant.py::slice_of, weight 1."""
    from tests import piecewise_constant as pc
    controls = np.asarray(controls, dtype=np.float64)
    nc = controls.shape[0]
    nsteps = N - 1
    dt = T / nsteps
    times = np.linspace(0, T, nc)
    u, weights = [], []
    for j in range(nsteps):
        t = j * dt + 0.5 * dt
        if interpolation == "piecewise_constant":
            s = pc.slice_of(t, nc, T)
            if mutant == "slice off by one":
                s = min(s + 1, nc - 1)
            u.append(controls[s])
            weights.append([(s, 1.0)])
        else:
            u.append(onp.interpolate_linear_set(t, times, controls))
            i1, w1, i2, w2 = onp.interpolation_weights(t, times)
            weights.append([(i1, w2), (i2, w1)] if mutant == "transposed knot weights" else [(i1, w1), (i2, w2)])
    return np.array(u), weights


def evaluate_features(h0, g, psi0, costs, N, T, controls, interpolation="linear", cost_eval_step=1,
                      mutant=None, ghost=None, scalar=None, first=2):
    """The route's mathematics at any control count K, any knot count Nc, either interpolation, psi0
    (S, n) and any oracle costs (oracle/qoc_numpy.py: cost and states_bar on states (S, n, 1)): the
    general adjoint of tests/action_costs_model.py - the sweep carries the true cotangent, the step
    gradient is Re sum conj(abar) (.) (-i dt G_k) summed over the states - which for one final coherent
    target is the unit adjoint times its scalar. Degrees from the step table's 1-norm bound.

    scalar: the final cotangent is scalar * target instead of the cost's own (the unit adjoint with a
    scalar from elsewhere; one final coherent TargetStateInfidelity only). mutant: one of MUTANTS - a
    plausibly wrong kernel; ghost: the matrix a kernel that keeps two images would read at K = 1; first: the
    control at which the "k >= 2" mutants begin - the boundary between two ways a kernel holds its images
    (2: the register images of qocx_action.hip; 1 and 4: registers / LDS / streamed in qocx_action16.hip).
    Returns dict(cost, grads [Nc, K], final (S, n), degrees, scalar - that of the unit adjoint or None)."""
    controls = np.asarray(controls, dtype=np.float64)
    nc, K = controls.shape
    nsteps = N - 1
    dt = T / nsteps
    psi = np.asarray(psi0, dtype=np.complex128)
    S = psi.shape[0]
    ustep, weights = step_controls(controls, N, T, interpolation, mutant)
    h0n = onp.one_norm(h0)
    gn = [onp.one_norm(m) for m in g]
    has_step = any(c.requires_step_evaluation for c in costs)

    def cost_step(j):
        return j != 0 and has_step and j % cost_eval_step == 0

    def total(states, step, step_pass, final_pass, want_bar):
        value, bar = 0.0, np.zeros((S, psi.shape[1]), dtype=np.complex128)
        for c in costs:
            if step_pass if c.requires_step_evaluation else final_pass:
                value += c.cost(None, states[:, :, None], step)
                if want_bar:
                    bar += c.states_bar(None, states[:, :, None], step)[:, :, 0]
        return value, bar

    gens, degrees = [], []
    for j in range(nsteps):
        u = ustep[j]
        bound = abs(dt) * (h0n + sum(abs(u[k]) * gn[k] for k in range(K)))
        degrees.append(degree_for(bound))
        h = h0 + sum(u[k] * g[k] for k in range(min(K, first)))
        for k in range(first, K):
            if mutant == "generator without k >= 2":
                continue
            uk = ustep[(j + 1) % nsteps][k] if mutant == "wrong step for k >= 2" else u[k]
            h = h + uk * g[k]
        if mutant == "second image at K = 1" and K == 1:
            h = h + u[0] * ghost
        gens.append(-1j * dt * h)
    vs, cost = [], 0.0
    for j in range(nsteps):
        if cost_step(j):
            cost += total(psi, j, True, False, False)[0]
        out = [forward_step(gens[j], psi[s], degrees[j]) for s in range(S)]
        psi = np.array([o[0] for o in out])
        vs.append([o[1] for o in out])
    if cost_step(nsteps):
        cost += total(psi, nsteps, True, False, False)[0]
    cost += total(psi, nsteps, False, True, False)[0]
    lam = total(psi, nsteps, cost_step(nsteps), True, True)[1]
    unit = None
    if len(costs) == 1 and not has_step and not getattr(costs[0], "neglect_relative_pahse", True):
        target = costs[0].target_states[:, :, 0]
        unit = -2.0 * costs[0].cost_multiplier * np.sum(np.conj(target) * psi) / S ** 2
        if scalar is not None:
            lam = scalar * target
    grads = np.zeros((nc, K))
    for j in range(nsteps - 1, -1, -1):
        abar = 0
        new = []
        for s in range(S):
            ls, w = adjoint_step(gens[j], lam[s], degrees[j])
            new.append(ls)
            abar = abar + generator_cotangent(vs[j][s], w, degrees[j])
        lam = np.array(new)
        for k in range(K):
            if mutant == "gradient without k >= 2" and k >= first:
                continue
            gk = np.real(np.sum(np.conj(abar) * (-1j * dt * g[k])))
            for knot, weight in weights[j]:
                grads[knot, k] += weight * gk
        if cost_step(j):
            lam = lam + total(np.array([v[0] for v in vs[j]]), j, True, False, True)[1]
    return dict(cost=cost, grads=grads, final=psi, degrees=degrees, scalar=unit)
