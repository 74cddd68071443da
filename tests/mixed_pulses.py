"""
mixed_pulses.py - TEST INFRASTRUCTURE (NumPy only): control pulses whose steps differ in generator
norm by four orders of magnitude inside one seed and one upload, and a model of the decisions the
product takes from them.

Every other fixture of the suite draws its controls as sigma * standard_normal with one sigma per
problem: one Pade order, one squaring count and one pivoting regime per launch. The product decides
per step (step_table_kernel, qocx_kernels.hip; the K1a kernels from the matrix they built) and per
upload (qocx_upload_controls, qocx_api.hip / qocx_opt_clip, qocx_api_multistart.hip: norm_bound,
norm_bound_mid, sbound, and from them prefer_low, the three-wave K1a with order_max 5, all_dominant, pack8, the slot layout).
The pulses here make those decisions differ between neighbouring steps and between the seeds of a
batch; tests/test_mixed_pulses_host.py proves on the CPU that they do, tests/test_gpu_mixed_steps.py
runs them on the device.

Nothing here is imported by the product.
"""

import numpy as np

from oracle import qoc_numpy as onp
from tests import device_model as dm
from tests.cases import gue

THETA = dm.PADE_THETA
ORDERS = (3, 5, 7, 9, 13)
FAMILIES = ("quiet", "bell", "spike", "square", "ramp", "loud")
DOMINANCE_MARGIN = 0.40  # qocx_lu5.h: pade_denominator_dominant
POLICY = {1: "M2", 2: "M4", 3: "M6"}


# ---- pulse families --------------------------------------------------------------------------------

def families(N, K, amp_hi, rng, quiet_sigma=0.02):
    """Named (N, K) control arrays (N knots, K channels); amp_hi is the peak amplitude, carried by
    the last channel. (The claims of the names need K >= 2 and a few dozen knots; the fuzzer also
    draws fewer.)"""
    t = np.arange(N)
    out = {}
    out["quiet"] = quiet_sigma * rng.standard_normal((N, K))
    # Gaussian envelope times a carrier, exactly zero at the two outermost knots of either end, peak
    # amp_hi on the last channel
    env = np.exp(-0.5 * ((t - 0.5 * (N - 1)) / (0.15 * (N - 1))) ** 2)
    floor = env[1] if N >= 5 else env[0]
    env = np.maximum(env - floor, 0.0) / (1.0 - floor)
    bell = np.empty((N, K))
    for k in range(K):
        bell[:, k] = env * np.cos(0.9 * t + 1.3 * k) * (amp_hi if k == K - 1 else amp_hi / 8)
    if np.max(np.abs(bell[:, K - 1])) > 0:
        bell[:, K - 1] *= amp_hi / np.max(np.abs(bell[:, K - 1]))
    out["bell"] = bell
    spike = np.zeros((N, K))
    spike[N // 4, 0] = amp_hi / 8
    spike[(2 * N) // 3, K - 1] = -amp_hi
    out["spike"] = spike
    square = np.zeros((N, K))
    a, b, c = N // 6, N // 2, (5 * N) // 6
    square[a:b, :] = amp_hi / 3
    square[b:c, :] = 0.0
    square[b:c, K - 1] = -amp_hi
    out["square"] = square
    # geometric from 1e-3 to amp_hi, the sign alternating every third knot (from knot to knot the
    # midpoints of a grid with a knot per step would cancel); the other channels an eighth
    ramp = np.empty((N, K))
    mag = 1e-3 * (amp_hi / 1e-3) ** (t / (N - 1.0))
    for k in range(K):
        ramp[:, k] = mag * (-1.0) ** (t // 3 + k) * (1.0 if k == K - 1 else 0.125)
    out["ramp"] = ramp
    out["loud"] = 0.5 * amp_hi * rng.standard_normal((N, K))
    return out


# ---- the product's decisions, restated ---------------------------------------------------------------

def magnus_norm_bound(nodes, bound):
    """qocx_api.hip: 1-norm bound of the step generator from the bound of its node generators."""
    if nodes == 2:
        return bound + (np.sqrt(3.0) / 12) * 2 * bound * bound
    if nodes == 3:
        b1, b2, b3 = bound, (np.sqrt(15.0) / 3) * 2 * bound, (10.0 / 3) * 4 * bound
        c12 = 2 * b1 * b2
        x, w = 20 * b1 + b3 + c12, 2 * b3 + c12
        y = b2 + (1.0 / 60) * 2 * b1 * w
        return b1 + 0.5 * b3 + (1.0 / 240) * 2 * x * y
    return bound


def squarings(bound):
    """Doubling from theta_13, as step_table_kernel and pade_scale_count (qocx_api.hip) count."""
    s, th = 0, onp.THETA_13
    while bound > th:
        th *= 2.0
        s += 1
    return s


def dominance_eps(order, theta):
    """eps_m(theta) = sum_{j>=1} (b_j / b_0) theta^j of qocx_lu5.h::pade_denominator_dominant."""
    b = dm.PADE_COEFFS[order]
    eps, tp = 0.0, 1.0
    for j in range(1, order + 1):
        tp *= theta
        eps += b[j] / b[0] * tp
    return eps


def pade_eps_max(theta):
    """qocx_api.hip: the largest eps_m(theta) over the orders - all_dominant asks for <= 0.40 at norm_bound."""
    return max(dominance_eps(m, theta) for m in ORDERS)


def decide(values):
    """Per-step (order, squarings, dominant, eps) from an array of norms or bounds."""
    order = np.array([dm.pade_order(v) for v in values])
    sq = np.array([squarings(v) if o == 13 else 0 for v, o in zip(values, order)])
    eps = np.array([dominance_eps(int(o), v * 2.0 ** -int(s)) for v, o, s in zip(values, order, sq)])
    return order, sq, eps <= DOMINANCE_MARGIN, eps


def step_table(h0, g, controls, dt, N, Nc, nodes=1):
    """
    NumPy model of step_table_kernel for one seed: controls (Nc, K) interpolated as the reference
    does (onp.interpolate_linear_set) at the quadrature nodes of each of the N - 1 steps, the bound
    dt (||H0||_1 + sum_k |u_k| ||G_k||_1) of the node generators (through magnus_norm_bound for
    nodes > 1, as the host does), and the exact 1-norm of the step generator the oracle exponentiates.
    Returns per-step arrays:
      bound / exact / sqfree     the triangle bound, ||m||_1, and max column sum of |re| + |im| (the
                                 square-root-free norm the two-wave K1a forms when it has no table)
      order_*, sq_*, dominant_*  the decisions from each (order by dm.pade_order)
    """
    policy = POLICY[nodes]
    cs = onp.MAGNUS_NODES[policy]
    T = dt * (N - 1)
    xs = np.linspace(0, T, Nc)
    h0n = onp.one_norm(h0)
    gn = np.array([onp.one_norm(m) for m in g])
    bound, exact, sqfree = np.empty(N - 1), np.empty(N - 1), np.empty(N - 1)
    for step in range(N - 1):
        gens, nb = [], 0.0
        for c in cs:
            u = onp.interpolate_linear_set(step * dt + c * dt, xs, controls)
            gens.append(-1j * (h0 + sum(u[k] * g[k] for k in range(len(g)))))
            nb = max(nb, abs(dt) * (h0n + float(np.sum(np.abs(u) * gn))))
        m = onp.magnus_combine(policy, dt, gens)[0]
        bound[step] = magnus_norm_bound(nodes, nb)
        exact[step] = onp.one_norm(m)
        sqfree[step] = np.max(np.sum(np.abs(m.real) + np.abs(m.imag), axis=0))
    out = dict(bound=bound, exact=exact, sqfree=sqfree)
    for key in ("bound", "exact", "sqfree"):
        order, sq, dom, eps = decide(out[key])
        out["order_" + key], out["sq_" + key] = order, sq
        out["dominant_" + key], out["eps_" + key] = dom, eps
    return out


def host_bounds(h0, g, controls, dt, N, Nc, nodes=1):
    """
    norm_bound, norm_bound_mid and sbound of qocx_upload_controls for a batch controls (B, Nc, K)
    of a problem without quadratic terms: the largest knot sum bounds every step; the midpoint bound
    (|u_mid| <= (|u_j| + |u_j+1|) / 2) holds only for M2 with a control knot per system step.
    """
    controls = np.asarray(controls, dtype=np.float64).reshape(-1, Nc, len(g))
    h0n = onp.one_norm(h0)
    gn = np.array([onp.one_norm(m) for m in g])
    rows = np.sum(np.abs(controls) * gn, axis=2)  # (B, Nc)
    smax = float(np.max(rows))
    smid = float(np.max(0.5 * (rows[:, 1:] + rows[:, :-1])))
    if nodes == 1 and Nc == N:
        mid = (h0n + smid) * abs(dt) * (1.0 + 1e-12)
    else:
        mid = 1e300
    bound = magnus_norm_bound(nodes, (h0n + smax) * abs(dt))
    return dict(norm_bound=bound, norm_bound_mid=mid, sbound=squarings(bound))


def near_threshold(values, orders=None, sqs=None, rel=1e-9):
    """True if a value lies within `rel` relative of a decision threshold: theta_3 .. theta_13 2^s, or
    the dominance margin (in eps, at the order and squaring count the value itself selects)."""
    values = np.asarray(values)
    ths = [THETA[m] for m in (3, 5, 7, 9)] + [onp.THETA_13 * 2.0 ** s for s in range(0, 12)]
    for th in ths:
        if np.any(np.abs(values - th) <= rel * th):
            return True
    _, _, _, eps = decide(values)
    return bool(np.any(np.abs(eps - DOMINANCE_MARGIN) <= rel * DOMINANCE_MARGIN))


# ---- problems ---------------------------------------------------------------------------------------

COST_TARGET_COHERENT, COST_TARGET_INCOHERENT, COST_FORBID = 0, 1, 2  # include/qocx.h


def problem(n, hermitian, magnus, S, N, Nc, seed, K=2, dt=0.05, ces=4, peak=11.5, g_scale=None):
    """
    GUE-like H0 and G_k, random states / targets / forbidden states and all three state-cost kinds,
    as test_gpu_engine.py::test_edge_shapes_against_oracle builds them. H0 is scaled so that
    dt ||H0||_1 < theta_3; `peak` is the step bound dt amp_hi ||G_K-1||_1 the loudest knot of a
    family reaches on the last channel alone. Returns a dict with the engine arguments, the
    onp.SchroedingerProblem, and the calibration (amp_hi, quiet_sigma).
    """
    rng = np.random.default_rng(seed)
    h0 = gue(rng, n) * 0.05
    g = [gue(rng, n) * (1.0 if g_scale is None else g_scale[k]) for k in range(K)]
    if not hermitian:
        # (small anti-Hermitian parts: the loud pulses must not blow the state norm up)
        h0 = h0 + 0.3j * 0.05 * gue(rng, n)
        g[0] = g[0] + 0.002j * gue(rng, n)
    init = rng.standard_normal((S, n)) + 1j * rng.standard_normal((S, n))
    init /= np.linalg.norm(init, axis=1, keepdims=True)
    targ = rng.standard_normal((S, n)) + 1j * rng.standard_normal((S, n))
    targ /= np.linalg.norm(targ, axis=1, keepdims=True)
    forb = rng.standard_normal((S, 2, n)) + 1j * rng.standard_normal((S, 2, n))
    forb /= np.linalg.norm(forb, axis=2, keepdims=True)
    T = dt * (N - 1)
    count = max((N - 1) // ces, 1)
    descs = [dict(kind=COST_TARGET_COHERENT, step_cost=0, scale=0.7, vectors=targ),
             dict(kind=COST_TARGET_INCOHERENT, step_cost=1, scale=1.3 / count, vectors=targ),
             dict(kind=COST_FORBID, step_cost=1, scale=0.9 / (count * S),
                  vectors=forb.reshape(-1, n), counts=[2] * S)]
    ocosts = [onp.TargetStateInfidelity(targ[:, :, None], cost_multiplier=0.7),
              onp.TargetStateInfidelityTime(N, targ[:, :, None], neglect_relative_pahse=True,
                                            cost_eval_step=ces, cost_multiplier=1.3),
              onp.ForbidStates(forb[:, :, :, None], N, cost_eval_step=ces, cost_multiplier=0.9)]
    oracle_problem = onp.SchroedingerProblem(
        T, lambda u, t: h0 + sum(u[k] * g[k] for k in range(K)), init[:, :, None], N,
        control_eval_count=Nc, costs=ocosts, cost_eval_step=ces, magnus_policy=magnus,
        control_count=K)
    gn = [onp.one_norm(m) for m in g]
    h0n = onp.one_norm(h0)
    assert dt * h0n < THETA[3]
    amp_hi = peak / (dt * gn[-1])
    # quiet: the typical step bound sits a quarter above theta_3, so that orders 3 and 5 both occur
    # by the bound and by the norm itself (E|N(0, 1)| = 0.798 per channel)
    quiet_sigma = (1.25 * THETA[3] / dt - h0n) / (0.798 * sum(gn))
    nodes = {"M2": 1, "M4": 2, "M6": 3}[magnus]
    return dict(n=n, S=S, K=K, N=N, Nc=Nc, T=T, dt=dt, ces=ces, magnus=magnus, nodes=nodes,
                hermitian=hermitian, h0=h0, g=g, init=init, descs=descs, oracle=oracle_problem,
                amp_hi=amp_hi, quiet_sigma=quiet_sigma, seed=seed)


def mixed_controls(p):
    """The six families of a problem as one (6, Nc, K) batch, in the order of FAMILIES."""
    rng = np.random.default_rng(p["seed"] + 77)
    fam = families(p["Nc"], p["K"], p["amp_hi"], rng, quiet_sigma=p["quiet_sigma"])
    return np.stack([fam[name] for name in FAMILIES])


def set_engine_problem(engine, p):
    engine.set_schroedinger_problem(p["n"], p["S"], p["K"], p["Nc"], p["N"], p["T"], p["h0"][None],
                                    np.stack(p["g"])[None], p["init"], costs=p["descs"],
                                    cost_eval_step=p["ces"], magnus_policy=p["magnus"])


def tables(p, controls):
    return [step_table(p["h0"], p["g"], u, p["dt"], p["N"], p["Nc"], p["nodes"]) for u in controls]


# ---- the device algorithm with the order by norm, any Magnus policy -----------------------------------

def model_evaluate_with_grad(problem, controls):
    """
    tests/device_model.py::evaluate_with_grad (Pade order by norm, LU with partial pivoting, 2^s
    solves per step, Krylov adjoint) extended to M4 / M6: the step generator is the oracle's
    magnus_combine, its cotangent goes back through magnus_combine_vjp. Returns (error, grads, final).
    """
    if problem.magnus_policy == "M2":
        return dm.evaluate_with_grad(problem, controls)
    controls = np.asarray(controls)
    policy, dt, xs = problem.magnus_policy, problem.dt, problem.control_eval_times
    n_steps = problem.system_eval_count - 1
    psi = problem.initial_states[:, :, 0].T.copy()
    n, S = psi.shape
    tape, hits, error = [], {}, 0.0
    for step in range(problem.system_eval_count):
        if step % problem.cost_eval_step == 0 and step != 0:
            for c in problem.step_costs:
                error = error + c.cost(controls, psi.T[:, :, None], step)
                hits.setdefault(step, []).append(c)
        if step == n_steps:
            break
        times = [step * dt + dt * c for c in onp.MAGNUS_NODES[policy]]
        gens = [-1j * problem.hamiltonian(onp.interpolate_linear_set(t, xs, controls), t)
                for t in times]
        m, mcache = onp.magnus_combine(policy, dt, gens)
        f = dm.pade_factor(m)
        subs = [psi]
        for _ in range(2 ** f["s"]):
            subs.append(dm.solve_lu(f["lu"], f["perm"], f["q"] @ subs[-1]))
        tape.append((times, gens, mcache, f, subs))
        psi = subs[-1]
    final_states = psi.T[:, :, None]
    grads = np.zeros(controls.shape, dtype=np.complex128)
    for c in problem.costs:
        if not c.requires_step_evaluation:
            error = error + c.cost(controls, final_states, n_steps)
            hits.setdefault(n_steps, []).append(c)
    lam = np.zeros((n, S), dtype=np.complex128)
    for c in hits.get(n_steps, []):
        sb = c.states_bar(controls, final_states, n_steps)
        if sb is not None:
            lam = lam + sb[:, :, 0].T
    for step in range(n_steps - 1, -1, -1):
        times, gens, mcache, f, subs = tape[step]
        triples = []
        for sub in range(2 ** f["s"] - 1, -1, -1):
            x = dm.solve_lu_adjoint(f["lu"], f["perm"], lam)
            lam = f["q"].conj().T @ x
            triples.append((x, subs[sub], subs[sub + 1]))
        mbar = dm.krylov_abar_horner(f["a"], triples, f["order"]) * (2 ** -f["s"])
        for t, abar in zip(times, onp.magnus_combine_vjp(policy, dt, gens, mcache, mbar)):
            hbar = 1j * abar
            g_re, _ = problem.hamiltonian_slopes(t)
            ubar = np.array([np.real(np.sum(np.conj(hbar) * g_re[k]))
                             for k in range(problem.control_count)])
            i1, w1, i2, w2 = onp.interpolation_weights(t, xs)
            grads[i1] += w1 * ubar
            grads[i2] += w2 * ubar
        for c in hits.get(step, []):
            sb = c.states_bar(controls, subs[0].T[:, :, None], step)
            if sb is not None:
                lam = lam + sb[:, :, 0].T
    return error, np.real(grads), final_states


# ---- comparison at the parity gates ------------------------------------------------------

GATES = dict(cost=1e-10, states=1e-10, grad=1e-8)


def gate_fractions(ref, out):
    """
    Errors of out = (cost, grads (Nc, K), final (S, n)) against the oracle's ref = (error, grads,
    final_states (S, n, 1)) as fractions of the parity gates: cost and states 1e-10 relative,
    gradient max|dg| / max(max|g|, 1e-3) against 1e-8 - per seed, and per control channel.
    """
    err, gr, fin = ref
    cost, grads, final = out
    fr = dict(cost=abs(err - cost) / max(1.0, abs(err)) / GATES["cost"],
              states=np.max(np.abs(fin[:, :, 0] - final)) / max(np.max(np.abs(fin)), 1e-300)
              / GATES["states"],
              grad=np.max(np.abs(gr - grads)) / max(np.max(np.abs(gr)), 1e-3) / GATES["grad"])
    fr["grad_channel"] = max(
        np.max(np.abs(gr[:, k] - grads[:, k])) / max(np.max(np.abs(gr[:, k])), 1e-3) / GATES["grad"]
        for k in range(gr.shape[1]))
    return fr


# ---- the shared parameter list ------------------------------------------------------------------------

# name: arguments of problem(). Hermitian and not, S = 1 and 3, Nc == N and Nc < N, M2 / M4 / M6;
# n = 8 (two steps to a tile, pack8), 16, 20, 32 (three-wave K1a, one-state sweep), 48 (four-wave
# K1a, lu4m, lu_redo), 72 (general path). At most 129 steps each.
# (M6: the host's bound of the Magnus series grows with the cube of the node bound, and a node bound
# above ~12.8 needs more than the 2^10 squarings the slot layout allows: the upload is rejected. A
# step with two squarings needs a norm above 10.7. Both hold only where norm and bound nearly coincide:
# the first generator is a tenth of the second, so the loud seeds are carried by one generator.)
PROBLEMS = {
    "n8_M2_S1": dict(n=8, hermitian=True, magnus="M2", S=1, N=98, Nc=98, seed=961),
    "n8_M2_S3_nonherm": dict(n=8, hermitian=False, magnus="M2", S=3, N=97, Nc=33, seed=852),
    "n16_M6_S1": dict(n=16, hermitian=True, magnus="M6", S=1, N=65, Nc=65, seed=1621, peak=11.0,
                      g_scale=(0.1, 1.0)),
    "n16_M2_S3": dict(n=16, hermitian=True, magnus="M2", S=3, N=97, Nc=25, seed=1672),
    "n20_M4_S3_nonherm": dict(n=20, hermitian=False, magnus="M4", S=3, N=97, Nc=41, seed=2001),
    "n20_M2_S1_nonherm": dict(n=20, hermitian=False, magnus="M2", S=1, N=97, Nc=97, seed=2002),
    "n32_M2_S1": dict(n=32, hermitian=True, magnus="M2", S=1, N=129, Nc=129, seed=3201),
    "n32_M2_S3": dict(n=32, hermitian=True, magnus="M2", S=3, N=97, Nc=33, seed=3212),
    "n48_M2_S1": dict(n=48, hermitian=True, magnus="M2", S=1, N=65, Nc=65, seed=4801),
    "n48_M2_S3_nonherm": dict(n=48, hermitian=False, magnus="M2", S=3, N=49, Nc=17, seed=4802),
    "n72_M2_S1": dict(n=72, hermitian=True, magnus="M2", S=1, N=41, Nc=21, seed=7211),
}
PROBLEM_NAMES = tuple(PROBLEMS)


def named_problem(name):
    return problem(**PROBLEMS[name])


# ---- item 3c: the bound at the step midpoints ------------------------------------------------------------

def spike_controls(p, Nc, knots, level=0.40, width=1):
    """Seeds of zeros with `width` consecutive knots at a level whose knot bound dt (||H0|| + |u|
    ||G_k||) is `level` + dt ||H0||_1: above theta_5, and below it when halved."""
    gn = [onp.one_norm(m) for m in p["g"]]
    u = np.zeros((len(knots), Nc, p["K"]))
    for b, (knot, k) in enumerate(knots):
        u[b, knot:knot + width, k] = (-1.0) ** b * level / (p["dt"] * gn[k])
    return u


def midpoint_problems():
    """
    (midpoint, counter, plateau): Hermitian, M2, n = 24.
      midpoint  Nc == N, single-knot spikes: the knot bound exceeds theta_5, every midpoint stays below
                it - the three-wave K1a with order_max = 5 is taken on the strength of norm_bound_mid.
      counter   the same spikes on a grid of 1.5 steps per knot: every odd knot is a step midpoint, the
                step there needs order 7 (and no midpoint bound applies).
      plateau   Nc == N, the spike two knots wide: the midpoint between them carries the full level,
                norm_bound_mid itself exceeds theta_5.
    Each a dict with the problem (p) and its controls (u).
    """
    base = dict(n=24, hermitian=True, magnus="M2", S=1, seed=2401)
    mid = problem(N=49, Nc=49, **base)
    knots = [(7, 0), (21, 1), (29, 1)]  # odd knots: step midpoints of the counter-problem
    counter = problem(N=49, Nc=33, **base)
    return (dict(p=mid, u=spike_controls(mid, 49, knots)),
            dict(p=counter, u=spike_controls(counter, 33, knots)),
            dict(p=mid, u=spike_controls(mid, 49, knots, width=2)))


# ---- item 3g: deep squaring inside a quiet pulse ----------------------------------------------------------

DEEP_S = 6


def deep_problem():
    """n = 8, 16 steps, one seed: order-3 steps and a single knot whose step needs DEEP_S squarings."""
    p = problem(n=8, hermitian=True, magnus="M2", S=3, N=17, Nc=17, seed=899)
    gn = onp.one_norm(p["g"][1])
    u = np.zeros((1, 17, 2))
    u[0, :, 0] = 0.25 * p["quiet_sigma"] * np.cos(np.arange(17.0))
    # the two steps that touch knot 8 see half its level: theta_13 2^(s-1) < bound <= theta_13 2^s
    u[0, 8, 1] = 2 * 0.75 * onp.THETA_13 * 2.0 ** DEEP_S / (p["dt"] * gn)
    return dict(p=p, u=u)
