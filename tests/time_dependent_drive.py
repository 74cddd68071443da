"""
time_dependent_drive.py - TEST INFRASTRUCTURE (NumPy only): problems whose drive operators depend on
time,

    H(u, t) = H0(t) + sum_k u_k G_k(t),   G_k(t) = e(t) (cos(w_k t + k) A_k + sin(w_k t) B_k),

every w_k different and w_k dt in 0.5 .. 1.0, so that the samples of G_k at neighbouring quadrature
times differ by O(1); H0(t) = H0 (1 + 0.3 cos(w_0 t)) with a frequency of its own, so that the h0 and
the g tables cannot be mistaken for each other. Every other fixture of the suite repeats one set of
G_k over the time axis of the ABI's g[nt][K][n][n]: a kernel that read G_k at the wrong time would
pass them all. drive_problem() returns the callable, its samples at the quadrature times of the
Magnus policy, the oracle problem and the device's cost descriptors; mutants() returns oracle
problems that read G_k at a wrong time in the ways a kernel could (tests/
test_time_dependent_drive_host.py proves that each moves the results by many orders of magnitude
more than the parity gates). lindblad_drive_problem() is the twin for the Lindblad path.

Nothing here is imported by the product.
"""

import numpy as np

from oracle import qoc_numpy as onp
from tests import device_model as dm
from tests.cases import gue

NODES = {"M2": (0.5,), "M4": (0.5 - 3 ** 0.5 / 6, 0.5 + 3 ** 0.5 / 6),
         "M6": (0.5 - 15 ** 0.5 / 10, 0.5, 0.5 + 15 ** 0.5 / 10)}  # = tests/fuzz_parity.py: NODES
COST_TARGET_COHERENT, COST_TARGET_INCOHERENT, COST_FORBID = 0, 1, 2  # include/qocx.h
THETA5 = dm.PADE_THETA[5]
GATES = dict(cost=1e-10, states=1e-10, grad=1e-8)
ENVELOPE_GROWTH = 20.0


def quadrature_times(N, dt, policy):
    return [j * dt + c * dt for j in range(N - 1) for c in NODES[policy]]


class Drive(object):
    """The operators of one problem and the callables made of them."""

    def __init__(self, h0, a, b, omega0, omegas, T, envelope, complex_controls=False):
        self.h0, self.a, self.b = h0, a, b
        self.omega0, self.omegas, self.T, self.envelope = omega0, omegas, T, envelope
        self.K = len(a)
        self.complex_controls = complex_controls

    def h0_at(self, t):
        return self.h0 * (1 + 0.3 * np.cos(self.omega0 * t))

    def g_at(self, t):
        """[G_0(t) .. G_K-1(t)]"""
        e = ENVELOPE_GROWTH ** (t / self.T - 1.0) if self.envelope else 1.0
        return [e * (np.cos(w * t + k) * self.a[k] + np.sin(w * t) * self.b[k])
                for k, w in enumerate(self.omegas)]

    def hamiltonian(self, u, t, g_time=None):
        """H(u, t), the G_k read at g_time (default: t). Complex controls: channel 2 k carries
        Re(u_k), channel 2 k + 1 Im(u_k), as the device orders them."""
        g = self.g_at(t if g_time is None else g_time)
        if self.complex_controls:
            return self.h0_at(t) + sum(np.real(u[k]) * g[2 * k] + np.imag(u[k]) * g[2 * k + 1]
                                       for k in range(len(u)))
        return self.h0_at(t) + sum(u[k] * g[k] for k in range(self.K))


def state_costs(rng, n, S, N, ces, costs):
    """(device descriptors, oracle costs). costs = "final": one final coherent target (the unit
    adjoint, factorising from both ends); "general": final + step incoherent + forbid."""
    targ = rng.standard_normal((S, n)) + 1j * rng.standard_normal((S, n))
    targ /= np.linalg.norm(targ, axis=1, keepdims=True)
    forb = rng.standard_normal((S, 2, n)) + 1j * rng.standard_normal((S, 2, n))
    forb /= np.linalg.norm(forb, axis=2, keepdims=True)
    descs = [dict(kind=COST_TARGET_COHERENT, step_cost=0, scale=0.7, vectors=targ)]
    ocosts = [onp.TargetStateInfidelity(targ[:, :, None], cost_multiplier=0.7)]
    if costs == "general":
        count = (N - 1) // ces
        assert count > 0
        descs += [dict(kind=COST_TARGET_INCOHERENT, step_cost=1, scale=1.3 / count, vectors=targ),
                  dict(kind=COST_FORBID, step_cost=1, scale=0.9 / (count * S),
                       vectors=forb.reshape(-1, n), counts=[2] * S)]
        ocosts += [onp.TargetStateInfidelityTime(N, targ[:, :, None], neglect_relative_pahse=True,
                                                 cost_eval_step=ces, cost_multiplier=1.3),
                   onp.ForbidStates(forb[:, :, :, None], N, cost_eval_step=ces,
                                    cost_multiplier=0.9)]
    else:
        assert costs == "final"
    return descs, ocosts


def drive_problem(n, N, Nc, K, S, policy="M2", hermitian=True, dt=0.2, costs="general", seed=0,
                  envelope=False, ces=2, complex_controls=False):
    """
    A problem with G_k(t) as above, K real control channels (complex_controls: K even, the channels
    are the (Re, Im) pairs of K / 2 complex controls). The operators are scaled by their 1-norms:
    dt ||H0||_1 = 0.04 and ||A_k||_1 = ||B_k||_1 = 1, so that controls() can place a seed below
    theta_5 and another above it. hermitian=False adds 0.3j gue to B_0. envelope=True multiplies
    every G_k by 20^(t / T - 1): the drive grows 20-fold over the pulse.
    """
    rng = np.random.default_rng(1000 * n + 10 * N + seed)
    T = dt * (N - 1)

    def unit(m):
        return m / onp.one_norm(m)

    h0 = unit(gue(rng, n)) * 0.04 / dt
    a = [unit(gue(rng, n)) for _ in range(K)]
    b = [unit(gue(rng, n)) for _ in range(K)]
    if not hermitian:
        b[0] = unit(b[0] + 0.3j * gue(rng, n))
    # w_k dt evenly spread over 0.5 .. 1.0, all different; H0 beats at 0.37 / dt
    omegas = [(0.5 + 0.5 * (k + 0.5) / K) / dt for k in range(K)]
    drive = Drive(h0, a, b, 0.37 / dt, omegas, T, envelope, complex_controls)
    times = quadrature_times(N, dt, policy)
    h0s = np.stack([drive.h0_at(t) for t in times])
    gs = np.stack([np.stack(drive.g_at(t)) for t in times])
    assert not np.allclose(gs[0], gs[1]) and not np.allclose(h0s[0], h0s[1])
    for ti in range(len(times) - 1):  # every sample differs from its neighbour, channel by channel
        for k in range(K):
            assert np.max(np.abs(gs[ti, k] - gs[ti + 1, k])) > 1e-3 * np.max(np.abs(gs[:, k]))
    init = rng.standard_normal((S, n)) + 1j * rng.standard_normal((S, n))
    init /= np.linalg.norm(init, axis=1, keepdims=True)
    descs, ocosts = state_costs(rng, n, S, N, ces, costs)
    p = dict(n=n, N=N, Nc=Nc, K=K, S=S, T=T, dt=dt, policy=policy, hermitian=hermitian, ces=ces,
             nodes=len(NODES[policy]), drive=drive, hamiltonian=drive.hamiltonian, times=times,
             h0=h0s, g=gs, init=init, descs=descs, ocosts=ocosts, seed=seed, envelope=envelope,
             complex_controls=complex_controls)
    p["oracle"] = oracle_problem(p, drive.hamiltonian)
    return p


def oracle_problem(p, hamiltonian, cls=onp.SchroedingerProblem):
    return cls(p["T"], hamiltonian, p["init"][:, :, None], p["N"], control_eval_count=p["Nc"],
               costs=p["ocosts"], cost_eval_step=p["ces"], magnus_policy=p["policy"],
               complex_controls=p["complex_controls"],
               control_count=p["K"] // 2 if p["complex_controls"] else p["K"])


def set_engine_problem(engine, p):
    engine.set_schroedinger_problem(p["n"], p["S"], p["K"], p["Nc"], p["N"], p["T"], p["h0"], p["g"],
                                    p["init"], costs=p["descs"], cost_eval_step=p["ces"],
                                    magnus_policy=p["policy"])


def g_norms(p):
    """max over the samples of ||G_k(t)||_1, as the host bounds the step generators."""
    return np.array([max(onp.one_norm(m) for m in p["g"][:, k]) for k in range(p["K"])])


def controls(p, B=2, quiet=0.12, loud=4.0, channels=None):
    """(B, Nc, K) real controls: seed 0 quiet - the host's bound dt (||H0||_1 + sum_k |u_k| ||G_k||_1)
    stays below 0.052 + `quiet` < theta_5 at every knot -, seed 1 loud (`loud` in the same measure,
    every knot at 60 .. 100 % of it), a third seed between them."""
    K = p["K"] if channels is None else channels  # (an ensemble's seeds drive the first K_r channels)
    rng = np.random.default_rng(p["seed"] + 31 * p["n"] + 7)
    gn = g_norms(p)[:K]
    level = np.array([quiet, loud, 0.3 * loud, 0.05 * loud])[:B]
    assert B <= 4 and 0.04 * 1.3 + quiet < THETA5
    mag = rng.uniform(0.6, 1.0, (B, p["Nc"], K)) * rng.choice([-1.0, 1.0], (B, p["Nc"], K))
    return mag * level[:, None, None] / (p["dt"] * gn * K)


def envelope_controls(p):
    """For envelope=True: the quiet seed, and one whose bound reaches 40 (7.4 theta_13) where the
    envelope ends - its first steps, a twentieth of that, need no squaring."""
    return controls(p, 2, loud=40.0)


def config_controls(p, B=2):
    """The controls the GPU tests run a configuration with."""
    return envelope_controls(p) if p["envelope"] else controls(p, B)


def clip_controls(p, level=2.0):
    """(clip norms (K,), controls (3, Nc, K)) for the resident route after a clip. qocx_opt_clip bounds
    the clipped controls by the clip norms alone, an upload by its largest knot sum; they coincide -
    and with them every route decision - when some knot holds every channel AT its norm and no knot
    sum exceeds theirs. Seeds 1 and 2: knot 0 at the norms, at every other knot one channel at 1.5
    times its norm (clipped) and the others at <= 0.5 / (K - 1) of theirs; seed 0 quiet (untouched).
    The clip bound is dt (||H0||_1 + sum_k norms_k ||G_k||_1) = 0.052 + `level`."""
    K, Nc = p["K"], p["Nc"]
    assert K >= 2
    rng = np.random.default_rng(p["seed"] + 13 * p["n"] + 5)
    norms = level / (p["dt"] * g_norms(p) * K)
    u = np.empty((3, Nc, K))
    u[0] = controls(p, 1)[0]
    for b in (1, 2):
        sign = rng.choice([-1.0, 1.0], (Nc, K))
        frac = rng.uniform(0.2, 0.5, (Nc, K)) / (K - 1)
        for j in range(Nc):
            frac[j, (j + b) % K] = 1.5
        frac[0] = 1.0
        u[b] = sign * frac * norms
    return norms, u


def step_norms(p, u):
    """Exact 1-norms of the step generators the oracle exponentiates for one seed's controls."""
    prob = p["oracle"]
    out = []
    for step in range(p["N"] - 1):
        gens = [onp._generator(prob, u, step * p["dt"] + c * p["dt"]) for c in NODES[p["policy"]]]
        out.append(onp.one_norm(onp.magnus_combine(p["policy"], p["dt"], gens)[0]))
    return np.array(out)


# ---- the ways to read G_k at the wrong time -----------------------------------------------------------

class _ShiftedSlopes(onp.SchroedingerProblem):
    """Forward pass exact; the gradient contraction reads G_k one step late."""

    def hamiltonian_slopes(self, time):
        g = [np.asarray(m, dtype=np.complex128) for m in self.drive.g_at(time + self.dt)]
        if self.complex_controls:
            return g[0::2], g[1::2]
        return g, []


def mutants(p):
    """{name: oracle problem}: "frozen" (G_k(0) at every time), "shift one step" (G_k(t + dt)),
    "mirror nodes" (the quadrature nodes of a step in reverse order: the identity for M2) and
    "gradient-only shift" (hamiltonian_slopes alone reads G_k(t + dt)). H0(t) is left alone."""
    d, dt = p["drive"], p["dt"]

    def mirrored(t):
        return (2 * np.floor(t / dt) + 1) * dt - t

    out = {"frozen": oracle_problem(p, lambda u, t: d.hamiltonian(u, t, 0.0)),
           "shift one step": oracle_problem(p, lambda u, t: d.hamiltonian(u, t, t + dt)),
           "mirror nodes": oracle_problem(p, lambda u, t: d.hamiltonian(u, t, mirrored(t)))}
    late = oracle_problem(p, d.hamiltonian, cls=_ShiftedSlopes)
    late.drive = d
    out["gradient-only shift"] = late
    return out


def relative_moves(ref, other):
    """(gradient, final states): max |difference| relative to max |reference| (the gradient's floored
    at 1e-3, as the parity gate's is)."""
    return (np.max(np.abs(ref[1] - other[1])) / max(np.max(np.abs(ref[1])), 1e-3),
            np.max(np.abs(ref[2] - other[2])) / max(np.max(np.abs(ref[2])), 1e-300))


def gate_fractions(ref, out):
    """Errors of out = (cost, grads (Nc, K), final (S, n)) against the oracle's ref = (error, grads,
    final_states (S, n, 1)) as fractions of the parity gates (tests/mixed_pulses.py: gate_fractions)."""
    err, gr, fin = ref
    cost, grads, final = out
    return dict(cost=abs(err - cost) / max(1.0, abs(err)) / GATES["cost"],
                states=np.max(np.abs(fin[:, :, 0] - final)) / max(np.max(np.abs(fin)), 1e-300)
                / GATES["states"],
                grad=np.max(np.abs(gr - grads)) / max(np.max(np.abs(gr)), 1e-3) / GATES["grad"])


# ---- quadratic terms and ensembles on the time-dependent tables ----------------------------------------------

class _SlopesAtControls(onp.SchroedingerProblem):
    """A Hamiltonian that is not linear in the controls: the gradient contraction takes d H / d u_k at
    the controls under evaluation (what autograd's trace of the callable gives the reference)."""

    def hamiltonian_slopes(self, time):
        u = onp.interpolate_linear_set(time, self.control_eval_times, self.at_controls)
        return [np.asarray(m, dtype=np.complex128) for m in self.slopes(u, time)], []


def quadratic_terms(p, scale=0.02):
    """Two constant Q_q on the real channels (0, 0) and (1, 2) - the second not Hermitian -, of 1-norm
    `scale`: with controls() the quadratic share of a loud step generator is comparable to its linear."""
    rng = np.random.default_rng(p["seed"] + 4242)
    n = p["n"]
    q0 = gue(rng, n)
    q1 = rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))
    return np.array([[0, 0], [1, 2]], dtype=np.int32), np.stack(
        [scale * q0 / onp.one_norm(q0), scale * q1 / onp.one_norm(q1)])


def ensemble_of(p, M=3, J=2):
    """scales (M, K - J), offsets (M, J), weights (M,): the last J channels of p are the D_j(t)."""
    rng = np.random.default_rng(p["seed"] + 777)
    return (1 + 0.05 * rng.standard_normal((M, p["K"] - J)), 0.4 * rng.standard_normal((M, J)),
            rng.uniform(0.2, 1.0, M))


def member_oracle(p, u, quadratic=None, scales=None, offsets=None):
    """The oracle problem of one ensemble member (or of the problem itself) with quadratic terms, at
    the seed controls u (Nc, K_r) - include/qocx.h:
        H_m(u, t) = H0(t) + sum_k s_k u_k G_k(t) + sum_j delta_j D_j(t) + sum_q (s_kq u_kq)(s_lq u_lq) Q_q."""
    d = p["drive"]
    J = 0 if offsets is None else len(offsets)
    kr = p["K"] - J
    s = np.ones(kr) if scales is None else np.asarray(scales)
    pairs, mats = quadratic if quadratic is not None else (np.zeros((0, 2), dtype=int), [])

    def hamiltonian(v, t):
        g = d.g_at(t)
        out = d.h0_at(t) + sum(s[k] * v[k] * g[k] for k in range(kr))
        out = out + sum((offsets[j] * g[kr + j] for j in range(J)), np.zeros_like(out))
        for (k, l), q in zip(pairs, mats):
            out = out + (s[k] * v[k]) * (s[l] * v[l]) * q
        return out

    def slopes(v, t):
        g = d.g_at(t)
        out = [s[k] * g[k] for k in range(kr)]
        for (k, l), q in zip(pairs, mats):
            out[k] = out[k] + s[k] * s[l] * v[l] * q
            out[l] = out[l] + s[k] * s[l] * v[k] * q
        return out

    prob = _SlopesAtControls(p["T"], hamiltonian, p["init"][:, :, None], p["N"],
                             control_eval_count=p["Nc"], costs=p["ocosts"], cost_eval_step=p["ces"],
                             magnus_policy=p["policy"], control_count=kr)
    prob.slopes, prob.at_controls = slopes, np.asarray(u)
    return prob


# ---- the configurations the GPU tests run ---------------------------------------------------------------

# name: arguments of drive_problem(). tests/test_time_dependent_drive_host.py proves the discrimination
# condition for every one of them; tests/test_gpu_time_dependent_drive.py runs them.
def _configs():
    out = {}
    for n in (1, 5, 16):  # one wave
        out["wave_n%d" % n] = dict(n=n, N=7, Nc=5, K=2, S=2)
    for n, N in ((8, 6), (8, 7), (3, 6), (3, 7)):  # pack8: two steps to a tile, odd and even step counts
        out["pack8_n%d_N%d" % (n, N)] = dict(n=n, N=N, Nc=N, K=2, S=1)
    for n in (17, 20, 32):  # two tiles
        out["two_n%d" % n] = dict(n=n, N=7, Nc=7, K=2, S=2)
    for n in (33, 40, 64):  # sixteen tiles
        out["four_n%d" % n] = dict(n=n, N=6, Nc=4, K=2, S=2)
    for n in (66, 72):  # general path
        out["general_n%d" % n] = dict(n=n, N=5, Nc=4, K=2, S=2)
    out["general_n40_S20"] = dict(n=40, N=5, Nc=4, K=2, S=20)
    out["sweep_n24"] = dict(n=24, N=8, Nc=8, K=2, S=2)
    out["dense_n24_S8"] = dict(n=24, N=6, Nc=5, K=2, S=8)
    out["edge_K1"] = dict(n=12, N=6, Nc=4, K=1, S=1)
    out["edge_K8"] = dict(n=20, N=6, Nc=4, K=8, S=3)
    out["edge_Nc2"] = dict(n=9, N=7, Nc=2, K=2, S=3)
    out["edge_Nc_above_N"] = dict(n=24, N=5, Nc=9, K=2, S=1)
    for n in (6, 20, 40, 70):  # Magnus
        for policy in ("M4", "M6"):
            out["%s_n%d" % (policy, n)] = dict(n=n, N=6, Nc=4, K=3 if n != 40 else 1, S=2,
                                               policy=policy)
    for n in (8, 24, 40, 72):  # pipeline and batching
        out["pipe_n%d" % n] = dict(n=n, N=14, Nc=9, K=2, S=2)
    for n in (24, 72):  # quadratic terms (K = 3) and ensembles (K_r = 3, J = 2)
        out["quadratic_n%d" % n] = dict(n=n, N=7, Nc=5, K=3, S=2, seed=3)
        out["ensemble_n%d" % n] = dict(n=n, N=7, Nc=5, K=5, S=2, seed=3)
    for n in (20, 40):  # norms that vary with time
        out["envelope_n%d" % n] = dict(n=n, N=12, Nc=12, K=2, S=1, envelope=True)
    return out


CONFIGS = _configs()
VARIANTS = [(h, c) for h in (True, False) for c in ("final", "general")]


def configured(name, hermitian=True, costs="general"):
    return drive_problem(hermitian=hermitian, costs=costs, **CONFIGS[name])


# ---- Lindblad twin -----------------------------------------------------------------------------------------

def lindblad_drive_problem(n, N, Nc, K, S, L, subdivision, stage_times, complex_ops=True,
                           costs="general", seed=0, data_stages=False, B=3):
    """
    The Lindblad twin: h0 constant in time (the ABI wants an h0_stages table whenever g_stages is
    given: the constant repeated), g_stages = G_k at the integrator's stage times - `stage_times` is
    Engine.lindblad_stage_times, passed in so that this file needs no library -, and the model system
    (tests/lindblad_model.py: StructuredLindblad with g_of_t). w_k dt in 2 .. 4: G_k turns by that
    many radians per system step, over the twelve distinct stage times of each of its pieces.
    B seeds of amplitudes 0.2, 0.7, 1.2 (over K, every knot clipped at two sigma). The time step
    follows from the engine's rule for the sub-division it is handed: (2 ||H0||_2 + 2 sum gamma
    ||L||_2^2 + 2 sum_k max|u_k| ||G_k||_2) dt <= 0.4 pieces, kept to 0.3 here.
    data_stages=True adds time-dependent lindblad_data (diss_stages / op_stages).
    Returns a dict with the engine arguments (args, kwargs), the controls, the model system's
    arguments and the model's costs.
    """
    from oracle import qoc_lindblad_numpy as ol
    from tests.cases import random_density
    COST_TARGET_DENSITY, COST_FORBID_DENSITY = 3, 4
    rng = np.random.default_rng(5000 * n + 100 * L + 10 * K + seed)
    h0 = gue(rng, n) * 1.5
    a = [gue(rng, n) for _ in range(K)]
    b = [gue(rng, n) for _ in range(K)]
    u = np.clip(rng.standard_normal((B, Nc, K)), -2.0, 2.0)
    u *= np.array([0.2, 0.7, 1.2, 0.5])[:B, None, None] / max(K, 1)

    def g_of_t(t):
        return [np.cos(w * t + k) * a[k] + np.sin(w * t) * b[k] for k, w in enumerate(omegas)]

    def op():
        return gue(rng, n) + (0.5j * gue(rng, n) if complex_ops else 0.0)

    ops = np.stack([op() for _ in range(L)]) if L else None
    ops_b = np.stack([0.2 * op() for _ in range(L)]) if L else None
    if L and not complex_ops:
        ops, ops_b = ops.real.astype(np.complex128), ops_b.real.astype(np.complex128)
    gam = rng.uniform(0.05, 0.3, L) if L else None
    diss = sum(1.3 * g_ * (np.linalg.norm(o, 2) + np.linalg.norm(ob, 2)) ** 2
               for g_, o, ob in zip(gam, ops, ops_b)) if L else 0.0
    bound = 2 * 1.5 + 2 * diss + 2 * 2.4 * 2.0  # ||G_k(t)||_2 <= ||A_k|| + ||B_k|| = 2
    dt = 0.3 * subdivision / bound
    T = dt * (N - 1)
    omegas = [(2.0 + 2.0 * (k + 0.5) / max(K, 1)) / dt for k in range(K)]

    def data_of_t(t):
        return gam * (1.0 + 0.3 * np.cos(9.0 * t)), ops + np.sin(7.0 * t) * ops_b

    rho0 = np.stack([random_density(rng, n) for _ in range(S)])
    targ = np.stack([random_density(rng, n) for _ in range(S)])
    forb = np.stack([random_density(rng, n) for _ in range(2 * S)])
    times = stage_times(T, N, Nc, K, subdivision)
    g_st = np.stack([np.stack(g_of_t(t)) for t in times])
    assert not np.allclose(g_st[0], g_st[1])
    descs = [dict(kind=COST_TARGET_DENSITY, step_cost=0, scale=0.8, vectors=targ)]
    mcosts = [ol.TargetDensityInfidelity(targ, cost_multiplier=0.8)]
    if costs == "general":
        descs.append(dict(kind=COST_FORBID_DENSITY, step_cost=1, scale=1.5 / ((N - 1) * S),
                          vectors=forb, counts=[2] * S))
        mcosts.append(ol.ForbidDensities(forb.reshape(S, 2, n, n), N, cost_multiplier=1.5))
    kwargs = dict(costs=descs, fixed_subdivision=subdivision,
                  h0_stages=np.repeat(h0[None], len(times), axis=0), g_stages=g_st)
    data = None
    if data_stages and L:
        data = data_of_t
        kwargs["diss_stages"] = np.stack([data_of_t(t)[0] for t in times])
        kwargs["op_stages"] = np.stack([data_of_t(t)[1] for t in times])
    system_args = (h0, g_of_t(0.0), gam, ops)
    return dict(n=n, N=N, Nc=Nc, K=K, S=S, L=L, T=T, subdivision=subdivision, times=times,
                args=(n, S, K, Nc, N, T, h0, g_of_t(0.0), gam, ops, rho0), kwargs=kwargs,
                system_args=system_args, g_of_t=g_of_t, data_of_t=data, rho0=rho0, mcosts=mcosts,
                seed=seed, controls=u, dt=dt)


def lindblad_model_system(q, g_of_t=None):
    from tests import lindblad_model as lm
    return lm.StructuredLindblad(*q["system_args"], g_of_t=q["g_of_t"] if g_of_t is None else g_of_t,
                                 data_of_t=q["data_of_t"])
