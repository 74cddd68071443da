"""
piecewise_constant.py - TEST INFRASTRUCTURE shared by tests/test_piecewise_constant_host.py and
tests/test_gpu_piecewise_constant.py: small random systems and the two references of
InterpolationPolicy.PIECEWISE_CONSTANT.

Reference A: the oracle cannot interpolate this way, so a pulse c (Nc x K) is folded into a
control-free oracle problem whose callable is t -> H(c[min(floor(t Nc / T), Nc - 1)], t); its
gradient is central differences (h = 1e-5) of that forward pass.
Reference B (M2, N - 1 = Nc): the LINEAR problem on the twin knots u_0 = c_0, u_{j+1} = 2 c_j - u_j
has the slice values at its step midpoints, hence the same generators; u = J c, and a gradient
with respect to u maps back by J^T.
"""

import numpy as np

from oracle import qoc_lindblad_numpy as ol
from oracle import qoc_numpy as onp

FD_STEP = 1e-5


def hermitian(rng, n, norm=1.0):
    a = rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))
    a = (a + a.conj().T) / 2
    return norm * a / np.linalg.norm(a, 2)


def system(n, K, seed, drive_frequency=None, drive_norm=1.0):
    """hamiltonian(u, t) = H0 + sum_k u_k G_k [cos(w_k t)], real-linear in real or complex u
    (complex: Re(u_k) G_k + Im(u_k) G'_k). drive_frequency: time-dependent G_k(t) and H0(t)."""
    rng = np.random.default_rng(seed)
    h0 = hermitian(rng, n)
    g = [hermitian(rng, n, drive_norm) for _ in range(K)]
    gi = [hermitian(rng, n, drive_norm) for _ in range(K)]

    def hamiltonian(u, t):
        f = 1.0 if drive_frequency is None else np.cos(drive_frequency * t)
        h = h0 * (1.0 if drive_frequency is None else 1.0 + 0.3 * np.sin(drive_frequency * t))
        if u is None:
            return h
        for k in range(K):
            h = h + np.real(u[k]) * f * g[k] + np.imag(u[k]) * f * gi[k]
        return h
    return hamiltonian


def states(n, S, seed):
    """(initial (S, n, 1), targets (S, n, 1)): orthonormal columns of two random unitaries."""
    rng = np.random.default_rng(seed)
    q0 = np.linalg.qr(rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n)))[0]
    q1 = np.linalg.qr(rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n)))[0]
    return q0.T[:S, :, None].copy(), q1.T[:S, :, None].copy()


def slice_of(t, Nc, T):
    t = float(np.real(t))  # (the Lindblad oracle's integrator carries its abscissa as complex)
    return min(max(int(np.floor(t * Nc / T)), 0), Nc - 1)


def closure(hamiltonian, c, T):
    """The control-free callable of Reference A."""
    c = np.asarray(c)
    Nc = c.shape[0]
    return lambda _, t: hamiltonian(c[slice_of(t, Nc, T)], t)


def reference_a(hamiltonian, c, T, initial_states, N, costs, magnus="M2", cost_eval_step=1,
                intermediate=None):
    """(error, final states (S, n, 1)) of the pulse c on the oracle; costs :: oracle costs."""
    problem = onp.SchroedingerProblem(T, closure(hamiltonian, c, T), initial_states, N,
                                      control_eval_count=0, costs=costs,
                                      cost_eval_step=cost_eval_step, magnus_policy=magnus,
                                      control_count=0)
    return onp.evaluate(problem, None, intermediate=intermediate)


def central_differences(cost_of, c, h=FD_STEP):
    """d cost / d Re(c) (+ i d cost / d Im(c) for complex c), entry by entry."""
    c = np.array(c)
    out = np.zeros(c.shape, dtype=c.dtype)
    for index in np.ndindex(*c.shape):
        for direction in ((1.0, 1.0j) if np.iscomplexobj(c) else (1.0,)):
            up, down = c.copy(), c.copy()
            up[index] += h * direction
            down[index] -= h * direction
            out[index] += direction * (cost_of(up) - cost_of(down)) / (2 * h)
    return out


def richardson_differences(cost_of, c, indices, h):
    """d cost / d c.flat[i] for i in indices by twice Richardson-extrapolated central differences,
    R2(h) = (16 R1(h / 2) - R1(h)) / 15 with R1(h) = (4 D(h / 2) - D(h)) / 3: error O(h^6), so that
    the step can be LARGE. The reference's adaptive Lindblad forward pass reproduces itself only
    to ~1.2e-11, which a quotient divides by its step (tools/gen_golden_lindblad.py extrapolates
    once, at h = 2e-2, for the same reason)."""
    c = np.asarray(c, dtype=np.float64)

    def central(i, step):
        up, down = c.copy(), c.copy()
        up.flat[i] += step
        down.flat[i] -= step
        return (cost_of(up) - cost_of(down)) / (2 * step)

    def once(i, step):
        return (4 * central(i, step / 2) - central(i, step)) / 3
    return np.array([(16 * once(i, h / 2) - once(i, h)) / 15 for i in indices])


def reference_a_gradient(hamiltonian, c, T, initial_states, N, costs, magnus="M2",
                         cost_eval_step=1):
    return central_differences(
        lambda x: reference_a(hamiltonian, x, T, initial_states, N, costs, magnus,
                              cost_eval_step)[0], c)


def lindblad_reference_a(hamiltonian, c, T, initial_densities, N, costs, lindblad_data,
                         cost_eval_step=1):
    """(error, final densities (S, n, n)) on the reference's adaptive integrator."""
    problem = ol.LindbladProblem(T, initial_densities, N, hamiltonian=closure(hamiltonian, c, T),
                                 lindblad_data=lindblad_data, control_eval_count=0, costs=costs,
                                 cost_eval_step=cost_eval_step, control_count=0)
    return ol.evaluate(problem, None)


def linear_twin(c):
    """(u (Nc + 1, K), J (Nc + 1, Nc)) with u = J c: u_0 = c_0, u_{j+1} = 2 c_j - u_j."""
    c = np.asarray(c)
    Nc = c.shape[0]
    J = np.zeros((Nc + 1, Nc))
    J[0, 0] = 1.0
    for j in range(Nc):
        J[j + 1] = -J[j]
        J[j + 1, j] += 2.0
    return np.tensordot(J, c, axes=(1, 0)), J


def lowering(n):
    return np.diag(np.sqrt(np.arange(1, n)), 1).astype(np.complex128)


def lindblad_system(n, L, seed):
    """(lindblad_data(t), initial densities (1, n, n), target (1, n, n))."""
    a = lowering(n)
    ops = np.stack([a, a.conj().T @ a][:L])
    gam = np.array([0.08, 0.05][:L])
    # a target the initial density overlaps with: a well-conditioned gradient (max |g| >= 1e-2 with
    # cost_multiplier = n, which undoes the cost's division by the Hilbert size)
    rng = np.random.default_rng(seed)
    psi = 0.2 * (rng.standard_normal(n) + 1j * rng.standard_normal(n)) / np.sqrt(n)
    psi[0] += 1.0
    psi[1] += 1.0
    psi /= np.linalg.norm(psi)
    rho0 = np.zeros((1, n, n), dtype=np.complex128)
    rho0[0, 0, 0] = 1.0
    target = np.outer(psi, psi.conj())[None]
    return (lambda t: (gam, ops)), rho0, target
