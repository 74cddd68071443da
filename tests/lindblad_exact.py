"""
lindblad_exact.py - TEST INFRASTRUCTURE: references of the Lindblad path that share nothing with the
device scheme. No Runge-Kutta tableau and no sub-division rule lives here: only NumPy, SciPy's expm /
expm_frechet / solve_ivp, and the oracle's cost objects (cost and states_bar on densities).

    d rho / dt = -i [H, rho] + sum_l gamma_l (L_l rho L_l^H - 1/2 {L_l^H L_l, rho})

in row-major vec, vec(A rho B) = (A (x) B^T) vec(rho). H need not be Hermitian: it enters as the plain
commutator, as in the reference's get_lindbladian (an effective Hamiltonian with loss does NOT put
H^H on the right of rho; the trace is preserved whatever H is).

piecewise_constant(...): the Liouvillian is constant on every slice of InterpolationPolicy.
PIECEWISE_CONSTANT, so the evolution is a product of exponentials of the n^2 x n^2 superoperator, on
the grid that merges the slice edges j T / Nc with the system steps. Every derivative is a Frechet
derivative of those exponentials. With lam the cotangent at the end of an interval of length h and rho
the densities at its start,

    Re <lam, L_exp(h Lv; h E) rho> = Re <L_exp(h Lv^H; sum_s lam_s rho_s^H), h E>_F

(the adjoint of L_exp(A; .) in the Frobenius product is L_exp(A^H; .)), so ONE expm_frechet per
interval serves every direction E: the drives -i [G_k, .] (control gradient), the dissipators
gamma_l D_l (rate sensitivities dE/dc_l at c = 1) and the whole Liouvillian (dE/dtau at tau = 1 of
rho' = tau Lv rho: the duration of a duration sweep).

linear(...): InterpolationPolicy.LINEAR and time-dependent H0(t) have no closed form; the vectorised
master equation and its forward sensitivity along a direction d in control space go through
scipy.integrate.solve_ivp at rtol 1e-13 / atol 1e-15, restarted at every control knot and system step,
once with DOP853 (complex) and once with LSODA (real and imaginary parts split). The reference is the
DOP853 run; `disagreement` says how far LSODA is from it, and a gate may never be below ten times that.

GATES (section "How the gates are set" of the pull request that added this file): per quantity the
largest of 10 x the worst model-versus-exact number of profiles/lindblad_exact.jsonl
(tools/measure_lindblad_exact.py: tests/lindblad_model.py against this file, on the CPU, over the case
table of tests/lindblad_exact_cases.py), 10 x the two-method disagreement of the linear(...) cases and
the device-versus-model gate of tests/test_gpu_lindblad.py (1e-12 absolute, 1e-10 relative for
gradients). The numbers are measured by the model, never by the engine.

Nothing here is imported by the product.
"""

from types import SimpleNamespace

import numpy as np
from scipy.integrate import solve_ivp
from scipy.linalg import expm, expm_frechet

# quantity: gate            # worst model-against-exact number of profiles/lindblad_exact.jsonl, its case
GATE_COST = 1e-12           # 1.4e-14 (sweep_n4_l2): the device-versus-model gate is the larger
GATE_DENSITIES = 4.7e-12    # 4.65e-13 (n2_s8), times ten
GATE_GRADIENT = 1.2e-10     # 1.195e-11 of the largest entry (n4_l0), times ten
GATE_SENSITIVITIES = 1e-10  # 7.4e-12 of a table's largest entry (sweep_n4_l2): device-versus-model
# LINEAR controls and h0(t); the two solve_ivp methods disagree by 2.3e-16 / 5.0e-15 / 4.2e-13
GATE_LINEAR_COST = 1e-12          # 1.2e-14 (linear_n4_l2_nc5): device-versus-model
GATE_LINEAR_DENSITIES = 1.4e-12   # 1.36e-13 (linear_n4_l2_nc5), times ten
GATE_LINEAR_DERIVATIVE = 1e-10    # 3.2e-12 of the largest direction (linear_n4_l2_nc5): device-versus-model


def dagger(x):
    return np.conjugate(np.swapaxes(x, -1, -2))


def hamiltonian_superoperator(h):
    """rho -> -i [H, rho]."""
    h = np.asarray(h, dtype=np.complex128)
    eye = np.eye(h.shape[0])
    return -1j * (np.kron(h, eye) - np.kron(eye, h.T))


def dissipator_superoperator(op):
    """rho -> L rho L^H - 1/2 (L^H L rho + rho L^H L)."""
    op = np.asarray(op, dtype=np.complex128)
    eye = np.eye(op.shape[0])
    ldl = dagger(op) @ op
    return np.kron(op, op.conj()) - 0.5 * np.kron(ldl, eye) - 0.5 * np.kron(eye, ldl.T)


def liouvillian(h, operators=None, gammas=None):
    """The n^2 x n^2 generator in row-major vec."""
    out = hamiltonian_superoperator(h)
    if operators is not None:
        for gm, op in zip(gammas, operators):
            out = out + gm * dissipator_superoperator(op)
    return out


def to_vec(densities):
    """(S, n, n) -> (n^2, S)."""
    d = np.asarray(densities, dtype=np.complex128)
    return d.reshape(d.shape[0], -1).T.copy()


def from_vec(vec, n):
    return vec.T.reshape(-1, n, n).copy()


def merged_grid(N, Nc):
    """System steps i T / (N - 1) and slice edges j T / Nc in units of T / ((N - 1) Nc): integers, so
    that a coincidence of an edge with a step is exact. Returns (points, unit denominator)."""
    steps, nc = N - 1, max(Nc, 1)
    return sorted(set(i * nc for i in range(N)) | set(j * steps for j in range(nc + 1))), steps * nc


def _step_hits(costs, N, cost_eval_step):
    """{system step: costs evaluated there}, as the oracle's evolve loop places them."""
    hits = {}
    for step in range(1, N):
        if step % cost_eval_step == 0:
            for c in costs:
                if c.requires_step_evaluation:
                    hits.setdefault(step, []).append(c)
    for c in costs:
        if not c.requires_step_evaluation:
            hits.setdefault(N - 1, []).append(c)
    return hits


def piecewise_constant(h0, g, operators, gammas, controls, T, N, initial_densities, costs,
                       cost_eval_step=1, want_grad=True, step_liouvillian=None):
    """
    h0 :: (n, n); g :: K matrices; operators :: (L, n, n) or None; gammas :: (L,); controls ::
    (Nc, K) real, controls[j] the value on slice j of Nc equal slices; costs :: oracle cost objects.
    step_liouvillian(q, slice, lv) -> lv: a hook for the mutation proofs of
    tests/test_lindblad_exact_host.py (the generator of interval q may be replaced), never set
    otherwise.

    Returns a namespace: error, final (S, n, n), steps (N, S, n, n), and with want_grad
    grad (Nc, K) = dE/du_jk, rate_sens (L,) = dE/dc_l at c = 1 (rates c_l gamma_l), tau_sens =
    dE/dtau at tau = 1 of the whole Liouvillian scaled by tau.
    """
    h0 = np.asarray(h0, dtype=np.complex128)
    n = h0.shape[0]
    g = [np.asarray(x, dtype=np.complex128) for x in (g if g is not None else [])]
    K = len(g)
    L = 0 if operators is None else len(operators)
    controls = np.zeros((1, 0)) if K == 0 else np.asarray(controls, dtype=np.float64).reshape(-1, K)
    Nc = controls.shape[0]
    base = liouvillian(h0, operators, gammas)
    drives = [hamiltonian_superoperator(x) for x in g]
    points, denominator = merged_grid(N, Nc)
    unit = T / denominator
    hits = _step_hits(costs, N, cost_eval_step)

    rho = to_vec(initial_densities)
    step_vecs = {0: rho}
    intervals = []
    for q in range(len(points) - 1):
        a, b = points[q], points[q + 1]
        j = min(a // (N - 1), Nc - 1)
        lv = base + sum((controls[j, k] * drives[k] for k in range(K)), np.zeros_like(base))
        if step_liouvillian is not None:
            lv = step_liouvillian(q, j, lv)
        hh = (b - a) * unit
        prop = expm(hh * lv)
        intervals.append((a, j, hh, lv, prop, rho))
        rho = prop @ rho
        if b % Nc == 0 or K == 0:
            step_vecs[b // max(Nc, 1)] = rho
    steps = np.stack([from_vec(step_vecs[i], n) for i in range(N)])
    error = 0.0
    for step in sorted(hits):
        for c in hits[step]:
            error = error + c.cost(controls, steps[step], step)
    out = SimpleNamespace(error=float(np.real(error)), final=steps[-1], steps=steps)
    if not want_grad:
        return out

    def bar(step):
        return sum((to_vec(c.states_bar(controls, steps[step], step)) for c in hits.get(step, [])),
                   np.zeros_like(rho))

    diss = [gammas[l] * dissipator_superoperator(operators[l]) for l in range(L)]
    grad = np.zeros((Nc, K))
    rate_sens = np.zeros(L)
    tau_sens = 0.0
    lam = bar(N - 1)
    for a, j, hh, lv, prop, rho_start in reversed(intervals):
        m = np.conj(expm_frechet(hh * dagger(lv), lam @ dagger(rho_start), compute_expm=False))
        for k in range(K):
            grad[j, k] += hh * np.real(np.sum(m * drives[k]))
        for l in range(L):
            rate_sens[l] += hh * np.real(np.sum(m * diss[l]))
        tau_sens += hh * np.real(np.sum(m * lv))
        lam = dagger(prop) @ lam
        if a % max(Nc, 1) == 0 and 0 < a // max(Nc, 1) < N - 1:
            lam = lam + bar(a // max(Nc, 1))
    out.grad, out.rate_sens, out.tau_sens = grad, rate_sens, float(tau_sens)
    return out


def sweep_member(h0, g, operators, gammas, seed_controls, scales, offsets, rate_scales, T, N,
                 initial_densities, costs, cost_eval_step=1, want_grad=True):
    """
    One seed of a sweep, or one member of an ensemble: the K = K_r + J channel problem on the
    controls [scales * u, offsets] with the rates rate_scales * gammas. Returns the namespace of
    piecewise_constant with, in addition, seed_grad (Nc, K_r) = dE/du, scale_sens (K_r,) = dE/ds_k,
    offset_sens (J,) = dE/ddelta_j, rate_sens (L,) = dE/dc_l (at the given c) and tau_sens (dE/dtau
    at tau = 1 of the whole scaled Liouvillian).
    """
    u = np.asarray(seed_controls, dtype=np.float64)
    Nc, kr = u.shape
    J = 0 if offsets is None else len(offsets)
    L = 0 if operators is None else len(operators)
    scales = np.ones(kr) if scales is None else np.asarray(scales, dtype=np.float64)
    c = np.ones(L) if rate_scales is None else np.asarray(rate_scales, dtype=np.float64)
    items = np.empty((Nc, kr + J))
    items[:, :kr] = scales[None, :] * u
    if J:
        items[:, kr:] = np.asarray(offsets, dtype=np.float64)[None, :]
    out = piecewise_constant(h0, g, operators, None if L == 0 else c * np.asarray(gammas), items, T,
                             N, initial_densities, costs, cost_eval_step, want_grad)
    if want_grad:
        out.seed_grad = scales[None, :] * out.grad[:, :kr]
        out.scale_sens = np.sum(u * out.grad[:, :kr], axis=0)
        out.offset_sens = np.sum(out.grad[:, kr:], axis=0)
        # piecewise_constant differentiates with respect to a factor on (c gamma) at 1: dE/dc = that / c
        out.rate_sens = np.where(c > 0, out.rate_sens / np.where(c > 0, c, 1.0), 0.0)
    return out


# ---- LINEAR controls, time-dependent H0(t) -----------------------------------------------------------

def hat_weights(t, knots):
    """w_j(t) of the hat functions on `knots`, (Nc,)."""
    w = np.zeros(len(knots))
    if t <= knots[0]:
        w[0] = 1.0
    elif t >= knots[-1]:
        w[-1] = 1.0
    else:
        i = int(np.searchsorted(knots, t, side="right")) - 1
        theta = (t - knots[i]) / (knots[i + 1] - knots[i])
        w[i], w[i + 1] = 1.0 - theta, theta
    return w


def _integrate(method, base_of_t, drives, controls, directions, T, N, rho0_vec, breaks,
               rtol, atol):
    """[rho, d_1 rho, ..., d_D rho] at every system step: (N, 1 + D, n^2) for ONE density."""
    Nc, K = controls.shape
    knots = np.linspace(0.0, T, Nc)
    D = len(directions)
    size = rho0_vec.shape[0]

    def rhs_complex(t, y):
        y = y.reshape(1 + D, size)
        w = hat_weights(t, knots)
        lv = base_of_t(t) + sum(((w @ controls[:, k]) * drives[k] for k in range(K)), 0.0)
        out = y @ lv.T
        for i, d in enumerate(directions):
            if d is None:  # the factor tau on the whole Lindbladian, at tau = 1
                out[1 + i] += lv @ y[0]
                continue
            dv = sum(((w @ d[:, k]) * drives[k] for k in range(K)), 0.0)
            out[1 + i] += dv @ y[0]
        return out.ravel()

    if method == "LSODA":  # real arithmetic only: real and imaginary parts split
        def rhs(t, y):
            z = rhs_complex(t, y[:y.size // 2] + 1j * y[y.size // 2:])
            return np.concatenate([z.real, z.imag])

        def pack(z):
            return np.concatenate([z.real, z.imag])

        def unpack(y):
            return y[:y.size // 2] + 1j * y[y.size // 2:]
    else:
        rhs, pack, unpack = rhs_complex, (lambda z: z), (lambda y: y)

    y = np.zeros((1 + D) * size, dtype=np.complex128)
    y[:size] = rho0_vec
    dt = T / (N - 1)
    out = {0: y.reshape(1 + D, size).copy()}
    for a, b in zip(breaks[:-1], breaks[1:]):
        sol = solve_ivp(rhs, (a, b), pack(y), method=method, rtol=rtol, atol=atol)
        assert sol.success, sol.message
        y = unpack(sol.y[:, -1])
        step = int(round(b / dt))
        if abs(step * dt - b) < 1e-12 * T:
            out[step] = y.reshape(1 + D, size).copy()
    return np.stack([out[i] for i in range(N)])


def linear(h0, g, operators, gammas, controls, T, N, initial_densities, costs, cost_eval_step=1,
           directions=(), h0_of_t=None, methods=("DOP853", "LSODA"), rtol=1e-13, atol=1e-15):
    """
    The truth for LINEAR controls (controls :: (Nc, K) on the knots linspace(0, T, Nc)) and for a
    time-dependent h0_of_t(t): error, final densities, densities at the steps, and the derivative of
    the error along every direction d (Nc, K) of `directions`, by the forward sensitivity equation
    d/dt drho = Lv(t) drho + sum_k (sum_j d_jk w_j(t)) G_k rho. Integrated with both `methods`; the
    namespace returned holds the first one's results and `disagreement` = dict(cost, densities,
    derivative (relative to the largest of the directions)) between the two.
    """
    h0 = np.asarray(h0, dtype=np.complex128)
    n = h0.shape[0]
    controls = np.asarray(controls, dtype=np.float64)
    Nc, K = controls.shape
    drives = [hamiltonian_superoperator(x) for x in g]
    diss = np.zeros((n * n, n * n), dtype=np.complex128)
    if operators is not None:
        for gm, op in zip(gammas, operators):
            diss = diss + gm * dissipator_superoperator(op)
    static = hamiltonian_superoperator(h0) + diss

    def base_of_t(t):
        return static if h0_of_t is None else hamiltonian_superoperator(h0_of_t(t)) + diss

    # (a direction None stands for the factor tau on the whole Lindbladian: dE/dtau at tau = 1)
    directions = [None if d is None else np.asarray(d, dtype=np.float64) for d in directions]
    dt = T / (N - 1)
    marks = sorted(set([i * dt for i in range(N)]) | set(np.linspace(0.0, T, Nc).tolist()))
    breaks = [marks[0]]
    for m in marks[1:]:  # (a knot that is a step to rounding is one break)
        if m - breaks[-1] > 1e-12 * T:
            breaks.append(m)
    hits = _step_hits(costs, N, cost_eval_step)
    rho0 = to_vec(initial_densities)
    runs = []
    for method in methods:
        per_density = [_integrate(method, base_of_t, drives, controls, directions, T, N, rho0[:, s],
                                  breaks, rtol, atol) for s in range(rho0.shape[1])]
        y = np.stack(per_density, axis=2)  # (N, 1 + D, S, n^2)
        steps = y[:, 0].reshape(N, -1, n, n)
        error, derivative = 0.0, np.zeros(len(directions))
        for step in sorted(hits):
            for c in hits[step]:
                error = error + c.cost(controls, steps[step], step)
                bar = c.states_bar(controls, steps[step], step)
                for i in range(len(directions)):
                    moved = y[step, 1 + i].reshape(-1, n, n)
                    derivative[i] += np.real(np.sum(np.conj(bar) * moved))
        runs.append(SimpleNamespace(error=float(np.real(error)), final=steps[-1], steps=steps,
                                    derivative=derivative))
    out = runs[0]
    out.disagreement = dict(cost=0.0, densities=0.0, derivative=0.0)
    for other in runs[1:]:
        out.disagreement["cost"] = max(out.disagreement["cost"], abs(out.error - other.error))
        out.disagreement["densities"] = max(out.disagreement["densities"],
                                            float(np.max(np.abs(out.steps - other.steps))))
        if len(directions):
            out.disagreement["derivative"] = max(
                out.disagreement["derivative"],
                float(np.max(np.abs(out.derivative - other.derivative))
                      / np.max(np.abs(out.derivative))))
    return out
