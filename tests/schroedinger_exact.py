"""
schroedinger_exact.py - TEST INFRASTRUCTURE: a reference of the Schroedinger path that shares nothing
with the device scheme. No Pade table, no Taylor table, no scaling and squaring and no LU lives here:
only numpy.linalg.eigh / eig, the oracle's interpolation, its cost objects (cost and states_bar) and,
for the two LINEAR M4 / M6 cases, its magnus_combine / magnus_combine_vjp.

The exact statement of the scheme. Under MagnusPolicy.M2 a step IS exp(-i dt H(u(t_mid), t_mid)), for
LINEAR and for PIECEWISE_CONSTANT controls, any Nc, any nt: the reference takes the per-step midpoint
controls from the interpolation and nothing else. Under M4 / M6 the same statement is exact when the
system is constant in time and the slice edges of PIECEWISE_CONSTANT lie on system steps (every node of
a step reads the same slice, the commutators vanish). Under M4 / M6 on LINEAR controls the reference
exponentiates the step's Magnus generator Omega exactly and takes Omega and its reverse rule from the
oracle: that holds the exponential and its derivative on the magnus4w and general::magnus_kernel routes,
it does NOT hold the Magnus coefficients (the oracle's golden files and convergence tests do).

exp and its derivative. a = -i dt H (or Omega). Hermitian H: a is normal, i a = V diag(l) V^H by eigh,
x = -i l. Otherwise a = V diag(x) V^-1 by eig - accepted per case only as far as it agrees with mpmath
(mpmath_check below). exp(a) = V diag(e^x) V^-1, and along any direction E

    L_exp(a; E) = V (Phi o (V^-1 E V)) V^-1,    Phi_ab = (e^x_a - e^x_b) / (x_a - x_b)
                                                       = e^((x_a + x_b) / 2) sinh(d / 2) / (d / 2),  d = x_a - x_b

(Daleckii-Krein). The second form has no cancellation; near-degenerate pairs (|d| < 2e-4) take the
series e^((x_a + x_b) / 2) (1 + d^2 / 24). With lam the cotangent at the end of a step and psi the
states at its start, Re <lam, L_exp(a; E) psi> = Re sum_ij E_ij Z_ij with

    Z = V^-T (Phi o (sum_s conj(V^H lam_s) (V^-1 psi_s)^T)) V^T

so ONE pass per step serves every direction E: the oracle's cotangent of a is abar = conj(Z)
(dC = Re tr(abar^H da)), and dC / dr_k = Re sum conj(abar) (-i dt G_k).

evaluate(...) works on REAL channels r_k, as the device does: H = H0(t) + sum_k r_k G_k(t) (+ sum_q
r_k r_l Q_q). Complex controls are the channels (Re u_k, Im u_k) on the slopes (G_k, G'_k) that
SchroedingerProblem.hamiltonian_slopes gives; ensembles, sweeps and durations are chain rules on the
per-step cotangents (tests/schroedinger_exact_cases.py).

GATES (section 3 of the pull request that added this file). Per quantity and per family - the LU-based
Pade routes, the inverse-image routes (sweepi, latency mode, the general path) and the matrix-free
routes round differently - the gate is 10 x the worst model-versus-exact number of its family in
profiles/schroedinger_exact.jsonl (tools/measure_schroedinger_exact.py: the NumPy models of the routes
against this file, on the CPU, over the table of tests/schroedinger_exact_cases.py), and never below 10 x
the recorded mpmath disagreement of this reference. The factor 10 covers a different summation order
and fused multiply-adds at the same magnitude. The numbers are measured by the models, never by the
engine.

Nothing here is imported by the product.
"""

from types import SimpleNamespace

import numpy as np

from oracle import qoc_numpy as onp
from tests.lindblad_exact import _step_hits
from tests.piecewise_constant import slice_of

LINEAR, PWC = "linear", "piecewise_constant"
FAMILIES = ("lu", "inverse", "matrix_free")

# The reference against mpmath at 40 digits on the smallest case of each kind
# (tests/schroedinger_exact_cases.py: MPMATH_CASES; profiles/schroedinger_exact.jsonl, the lines "mpmath"
# and "mpmath_worst" of the last line): the largest disagreement, rounded up. No gate is below 10 x these.
MPMATH_COST = 7.3e-16     # 7.22e-16 (mp_linear_m4_n6)
MPMATH_STATES = 4.4e-15   # 4.4e-15 (mp_gue_n8_level20)
MPMATH_DERIVATIVE = 2.4e-14  # 2.38e-14 of the derivative along a random direction (mp_gue_n8_level20)

# family: {quantity: gate}: 10 x the worst model-against-exact number of the family, rounded up to two
# digits - the number and its case beside it, from "worst" in the last line of
# profiles/schroedinger_exact.jsonl - or 10 x the mpmath disagreement where that is larger. Costs and
# states are absolute (costs of order 1, unit states); gradients are relative to the largest entry of a
# seed's gradient, the sensitivity tables and dE/dtau to the largest entry of the table.
GATES = {
    "lu": dict(
        cost=2.2e-14,  # 2.11e-15 (k1a_n20_ladder_4theta13)
        states=1.6e-13,  # 1.6e-14 (k1a_n20_ladder_4theta13)
        gradient=2.5e-12,  # 2.5e-13 (k1a_n20_ladder_4theta13)
        sensitivities=2.4e-13,  # 6.33e-15 (duration_n20): 10 x MPMATH_DERIVATIVE is the larger
        tau_gradient=2.4e-13),  # 6.49e-15 (duration_n20): 10 x MPMATH_DERIVATIVE is the larger
    "inverse": dict(
        cost=1.2e-14,  # 1.12e-15 (sweepi_n16_s1)
        states=9.2e-14,  # 9.18e-15 (general_n72_level20)
        gradient=8.5e-13,  # 8.43e-14 (general_n72_level20)
        sensitivities=2.4e-13,  # 8.34e-15 (duration_n8): 10 x MPMATH_DERIVATIVE is the larger
        tau_gradient=2.4e-13),  # 6.16e-15 (duration_n8): 10 x MPMATH_DERIVATIVE is the larger
    "matrix_free": dict(  # (no sweep runs on these routes in the table: no sensitivity gates)
        cost=7.3e-15,  # 4.45e-16 (action_n17_degree6): 10 x MPMATH_COST is the larger
        states=4.4e-14,  # 3.07e-15 (action_ensemble_n20): 10 x MPMATH_STATES is the larger
        gradient=6.1e-13),  # 6.08e-14 (action_wide_n64)
}
QUANTITY_GATE = dict(cost="cost", member_cost="cost", states="states", gradient="gradient",
                     scale_sens="sensitivities", offset_sens="sensitivities", tau_grad="tau_gradient")


def gates_of(family):
    """{quantity of schroedinger_exact_cases.compare: gate}."""
    return {q: GATES[family][g] for q, g in QUANTITY_GATE.items() if g in GATES[family]}


def dagger(x):
    return np.conjugate(np.swapaxes(x, -1, -2))


# ---- what a step reads, and where its cotangent goes --------------------------------------------------

def step_controls(controls, N, T, interpolation=LINEAR, nodes=(0.5,)):
    """(r [N - 1, nodes, K], weights [step][node] = [(knot, weight), ...]): the channel values at the
    nodes t_j + c dt of every step - the oracle's linear interpolation on the knots linspace(0, T, Nc),
    or the slice of PIECEWISE_CONSTANT that holds the node - and the transpose of that map."""
    controls = np.asarray(controls, dtype=np.float64)
    Nc = controls.shape[0]
    dt = T / (N - 1)
    knots = np.linspace(0, T, Nc)
    r = np.empty((N - 1, len(nodes), controls.shape[1]))
    weights = []
    for j in range(N - 1):
        row = []
        for i, c in enumerate(nodes):
            t = j * dt + c * dt
            if interpolation == PWC:
                s = slice_of(t, Nc, T)
                r[j, i] = controls[s]
                row.append([(s, 1.0)])
            else:
                r[j, i] = onp.interpolate_linear_set(t, knots, controls)
                i1, w1, i2, w2 = onp.interpolation_weights(t, knots)
                row.append([(i1, w1), (i2, w2)])
        weights.append(row)
    return r, weights


def step_hamiltonians(h0, g, controls, T, N, interpolation=LINEAR, nodes=(0.5,), quadratic=None):
    """(r, weights, H [step][node], dH/dr_k [step][node][k]) of H = H0(t) + sum_k r_k G_k(t) + sum_q
    r_k r_l Q_q at the nodes of every step: h0 :: (n, n) or (nt, n, n), g :: (K, n, n) or
    (nt, K, n, n), table row `step * nodes + node` as the engine reads it; quadratic :: (pairs, matrices)
    or None (the quadratic terms make the slopes depend on r)."""
    h0 = np.asarray(h0, dtype=np.complex128)
    h0 = h0[None] if h0.ndim == 2 else h0
    n = h0.shape[-1]
    controls = np.asarray(controls, dtype=np.float64)
    K = controls.shape[1]
    g = np.asarray(g, dtype=np.complex128).reshape(-1, K, n, n)
    r, weights = step_controls(controls, N, T, interpolation, nodes)
    pairs, qmats = ((), ()) if quadratic is None else quadratic
    hams, slopes = [], []
    for j in range(N - 1):
        hrow, srow = [], []
        for i in range(len(nodes)):
            row = j * len(nodes) + i
            h = h0[row if h0.shape[0] > 1 else 0]
            slope = [g[row if g.shape[0] > 1 else 0, k] for k in range(K)]
            for k in range(K):
                h = h + r[j, i, k] * slope[k]
            for (k, l), q in zip(pairs, qmats):
                h = h + r[j, i, k] * r[j, i, l] * q
                slope[k] = slope[k] + r[j, i, l] * q
                slope[l] = slope[l] + r[j, i, k] * q
            hrow.append(h)
            srow.append(slope)
        hams.append(hrow)
        slopes.append(srow)
    return r, weights, hams, slopes


# ---- the exponential and its derivative -----------------------------------------------------------------

def spectral(a, normal):
    """(x, V, V^-1) with a = V diag(x) V^-1. normal: a is anti-Hermitian (-i dt H of a Hermitian H, or
    its Magnus generator) - eigh of i a, V unitary; otherwise eig."""
    if normal:
        lam, v = np.linalg.eigh(1j * (a - dagger(a)) / 2)
        return -1j * lam, v, dagger(v)
    x, v = np.linalg.eig(a)
    return x, v, np.linalg.inv(v)


def divided_differences(x):
    """Phi_ab = (e^x_a - e^x_b) / (x_a - x_b) without cancellation; Phi_aa = e^x_a."""
    half = 0.5 * (x[:, None] - x[None, :])
    small = np.abs(half) < 1e-4
    safe = np.where(small, 1.0, half)
    sinhc = np.where(small, 1.0 + half * half / 6.0, np.sinh(safe) / safe)
    return np.exp(0.5 * (x[:, None] + x[None, :])) * sinhc


class StepExponential(object):
    """exp(a) of one step: apply it, apply its adjoint, and the cotangent of a."""

    def __init__(self, a, normal):
        self.x, self.v, self.vinv = spectral(a, normal)
        self.ex = np.exp(self.x)

    def forward(self, psi):
        """exp(a) psi for psi (n, S)."""
        return self.v @ (self.ex[:, None] * (self.vinv @ psi))

    def adjoint(self, lam):
        """exp(a)^H lam."""
        return dagger(self.vinv) @ (np.conj(self.ex)[:, None] * (dagger(self.v) @ lam))

    def cotangent(self, psi, lam):
        """abar with Re <lam, L_exp(a; E) psi> = Re sum conj(abar) E for every E (summed over the
        states)."""
        left = dagger(self.v) @ lam            # (n, S)
        right = self.vinv @ psi                # (n, S)
        m = divided_differences(self.x) * (np.conj(left) @ right.T)
        return np.conj(self.vinv.T @ m @ self.v.T)


# ---- the evaluation ---------------------------------------------------------------------------------------

def evaluate(h0, g, controls, T, N, initial_states, costs, cost_eval_step=1, interpolation=LINEAR,
             magnus="M2", hermitian=True, quadratic=None, want_grad=True, step_generator=None):
    """
    h0 :: (n, n) or (nt, n, n); g :: (K, n, n) or (nt, K, n, n), table row `step * nodes + node` as the
    engine reads it (nt = 1: constant); controls :: (Nc, K) real channel values; initial_states ::
    (S, n); costs :: oracle cost objects; quadratic :: (pairs (count, 2), matrices (count, n, n)) or None
    (M2 only). hermitian: every H met is Hermitian (eigh); False: eig.
    step_generator(step, a) -> a: a hook for the mutation proofs of
    tests/test_schroedinger_exact_host.py (the generator of a step may be replaced), never set otherwise.

    Returns a namespace: error, final (S, n), steps (N, S, n) and with want_grad grad (Nc, K) = dE/dr_jk
    (the step cotangents scattered through the transpose of the interpolation) and step_grad
    (N - 1, nodes, K), the cotangents of the channel values each node of each step read.
    """
    nodes = onp.MAGNUS_NODES[magnus]
    controls = np.asarray(controls, dtype=np.float64)
    Nc, K = controls.shape
    dt = T / (N - 1)
    assert quadratic is None or magnus == "M2"
    _, weights, hams, slope_rows_of = step_hamiltonians(h0, g, controls, T, N, interpolation, nodes, quadratic)
    n = hams[0][0].shape[0]
    hits = _step_hits(costs, N, cost_eval_step)
    psi = np.asarray(initial_states, dtype=np.complex128).T.copy()  # (n, S)
    tape, steps = [], [psi]
    for j in range(N - 1):
        gens = [-1j * h for h in hams[j]]
        a, mcache = onp.magnus_combine(magnus, dt, gens)
        if step_generator is not None:
            a = step_generator(j, a)
        ex = StepExponential(a, hermitian)
        tape.append((gens, mcache, slope_rows_of[j], ex, psi))
        psi = ex.forward(psi)
        steps.append(psi)
    steps = np.stack([s.T for s in steps])  # (N, S, n)
    error = 0.0
    for step in sorted(hits):
        for c in hits[step]:
            error = error + c.cost(controls, steps[step][:, :, None], step)
    out = SimpleNamespace(error=float(np.real(error)), final=steps[-1], steps=steps)
    if not want_grad:
        return out

    def bar(step):
        total = np.zeros((n, steps.shape[1]), dtype=np.complex128)
        for c in hits.get(step, []):
            total = total + c.states_bar(controls, steps[step][:, :, None], step)[:, :, 0].T
        return total

    grad = np.zeros((Nc, K))
    step_grad = np.zeros((N - 1, len(nodes), K))
    lam = bar(N - 1)
    for j in range(N - 2, -1, -1):
        gens, mcache, slope_rows, ex, psi = tape[j]
        abar = ex.cotangent(psi, lam)
        for i, genbar in enumerate(onp.magnus_combine_vjp(magnus, dt, gens, mcache, abar)):
            for k in range(K):
                step_grad[j, i, k] = np.real(np.sum(np.conj(genbar) * (-1j * slope_rows[i][k])))
            for knot, w in weights[j][i]:
                grad[knot] += w * step_grad[j, i]
        lam = ex.adjoint(lam)
        if j > 0:
            lam = lam + bar(j)
    out.grad, out.step_grad = grad, step_grad
    return out


# ---- the self-check of the reference: mpmath at 40 digits ---------------------------------------------------

def mpmath_check(h0, g, controls, direction, T, N, initial_states, costs, cost_eval_step=1,
                 interpolation=LINEAR, magnus="M2", digits=40):
    """
    The final states and the derivative of the error along `direction` (Nc, K) of a constant system
    with mpmath.expm at `digits` digits: the derivative of a step's exponential is the upper right
    block of expm([[a, e], [0, a]]). Under M4 / M6 the Magnus generator and (M4: exactly, the generator
    is quadratic in its node generators) its derivative along the direction come from the oracle's
    magnus_combine; under M6 only the states are checked (derivative None).
    Returns (error, final (S, n), derivative or None).
    """
    import mpmath
    nodes = onp.MAGNUS_NODES[magnus]
    h0 = np.asarray(h0, dtype=np.complex128)
    n = h0.shape[0]
    controls = np.asarray(controls, dtype=np.float64)
    K = controls.shape[1]
    dt = T / (N - 1)
    r, _ = step_controls(controls, N, T, interpolation, nodes)
    d, _ = step_controls(direction, N, T, interpolation, nodes)
    hits = _step_hits(costs, N, cost_eval_step)
    with mpmath.workdps(digits):
        def to_mp(m):
            return mpmath.matrix([[mpmath.mpc(complex(v)) for v in row] for row in np.atleast_2d(m)])

        def to_np(m):
            return np.array([[complex(m[i, j]) for j in range(m.cols)] for i in range(m.rows)])

        psi = to_mp(np.asarray(initial_states, dtype=np.complex128).T)
        dpsi = psi * 0
        states, tangents = [to_np(psi)], [to_np(dpsi)]
        for j in range(N - 1):
            def generators(values):
                return [-1j * (h0 + sum(values[j, i, k] * g[k] for k in range(K)))
                        for i in range(len(nodes))]
            gens = generators(r)
            a = onp.magnus_combine(magnus, dt, gens)[0]
            if magnus == "M2":
                e = -1j * dt * sum(d[j, 0, k] * g[k] for k in range(K))
            elif magnus == "M4":  # quadratic in the node generators: the central difference is exact
                e = 0.5 * (onp.magnus_combine(magnus, dt, generators(r + d))[0]
                           - onp.magnus_combine(magnus, dt, generators(r - d))[0])
            else:
                e = None
            if e is None:
                psi = mpmath.expm(to_mp(a)) * psi
            else:
                block = mpmath.zeros(2 * n)
                am, em = to_mp(a), to_mp(e)
                for p in range(n):
                    for q in range(n):
                        block[p, q] = block[n + p, n + q] = am[p, q]
                        block[p, n + q] = em[p, q]
                big = mpmath.expm(block)
                u, du = big[:n, :n], big[:n, n:]
                psi, dpsi = u * psi, du * psi + u * dpsi
            states.append(to_np(psi))
            tangents.append(to_np(dpsi))
    error, derivative = 0.0, 0.0
    for step in sorted(hits):
        for c in hits[step]:
            as_states = states[step].T[:, :, None]
            error = error + c.cost(controls, as_states, step)
            derivative += np.real(np.sum(np.conj(c.states_bar(controls, as_states, step)[:, :, 0])
                                         * tangents[step].T))
    return float(np.real(error)), states[-1].T, (None if magnus == "M6" else float(derivative))
