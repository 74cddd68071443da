"""
action_effective.py - TEST INFRASTRUCTURE (NumPy only): the problems that hold the matrix-free route on
EFFECTIVE controls (qoc_amd/csrc/qocx_action_eff.hip, knob "action_eff" = 1) to the oracle, and a NumPy
model of that route on top of tests/action_model.py. Imported by tests/test_action_effective_host.py (CPU)
and tests/test_gpu_action_effective.py (GPU).

The route: M4 on a time-independent system and a Hamiltonian quadratic in the controls have a step generator

    a_j = -i dt (H0 + sum_e v_e(j) G^_e)

linear in Ke effective controls over an augmented operator set, so the Taylor sweeps of the plain route run
on one row of Ke controls per step and a chain rule folds the Ke step cotangents back:

  M4         u1, u2 the controls at the nodes t_j + (1/2 -+ sqrt(3)/6) dt;  v_k = (u1_k + u2_k) / 2 on G_k,
             w_k = F0 dt (u2_k - u1_k) on A_k = -i [G_k, H0],  z_kl = F0 dt (u2_k u1_l - u2_l u1_k) on
             B_kl = -i [G_k, G_l] (k < l), F0 = sqrt(3) / 12:  Ke = 2 K + K (K - 1) / 2
  quadratic  u the controls at the midpoint;  u_k on G_k,  c_q u_kq u_lq on Q_q:  Ke = K + count

The degree of a step is action_degree_rule of qoc_amd/csrc/qocx_action.h (tests/action_degree_model.py) on
b1 = |dt| (||H0||_1 + sum_e |v_e| ||G^_e||_1) and b2, the same sum over the spectral bounds.

The fixture is that of tests/action_features.py: N = 14, DT = 0.05, Hermitian operators of 1-norm 1, three
seeds at the amplitudes 1e-3, 1 and 5 (2 / K for K > 2), one final coherent target. Q_q is a Hermitian matrix
of 1-norm 1. QUADRATIC problems take the amplitudes 1e-3, 1 and 2.5 instead: the host's bound of a quadratic
problem carries sum_q ||Q_q||_1 max|r_k| max|r_l| over the whole upload, which at an amplitude of 5 is
DT (1 + 10 + 50) = 3.05 - above theta_18 = 1.09, where the route must yield (and does: the yield test). At 2.5
it is at most DT (1 + 5 + 12.5) = 0.925 <= 0.9 theta_18, and the three seeds still span nine degrees.

Nothing here is imported by the product.
"""

import contextlib
import ctypes

import numpy as np

from oracle import qoc_numpy as onp
from tests import action_degree_model as dm
from tests import action_features as af
from tests import action_model as am
from tests import piecewise_constant as pc

N, DT, T = af.N, af.DT, af.T
STEPS = N - 1
LINEAR, PWC = af.LINEAR, af.PWC
F0 = np.sqrt(3.0) / 12
M4_NODES = (onp.M4_C1, onp.M4_C2)
THETA_18 = am.THETA[18]
QUADRATIC_AMPLITUDES = (1e-3, 1.0, 2.5)
SQUARE_AND_CROSS = ((0, 0), (0, 1))

# (kind, n, K, interpolation, Nc, terms): "m4" MagnusPolicy M4, "quad" M2 with the terms (k, l) on Q_q
M4_COUNTS = [("m4", n, K, LINEAR, N, ()) for n in (17, 32) for K in (1, 2, 3)]  # Ke = 2, 5, 9
M4_KNOTS = [("m4", 20, 2, interpolation, Nc, ())
            for interpolation, Nc in ((LINEAR, 5), (LINEAR, 27), (PWC, 3), (PWC, 13))]
QUADRATIC = [("quad", 17, 2, LINEAR, N, SQUARE_AND_CROSS), ("quad", 24, 2, LINEAR, N, SQUARE_AND_CROSS),
             ("quad", 20, 1, LINEAR, N, ((0, 0),)), ("quad", 20, 2, PWC, 3, SQUARE_AND_CROSS)]
SMALL = [("m4", 5, 2, LINEAR, N, ()), ("m4", 16, 2, LINEAR, N, ()), ("quad", 9, 2, LINEAR, N, ((0, 1),))]
WIDE = [("m4", 33, 2, LINEAR, N, ()), ("m4", 64, 2, LINEAR, N, ())]
CASES = M4_COUNTS + M4_KNOTS + QUADRATIC + SMALL + WIDE
BITS_CASE = ("m4", 17, 2, LINEAR, N, ())
OPTIMISER_CASE = ("m4", 20, 2, LINEAR, 5, ())
PYTHON_CASES = [("m4", 20, 2, LINEAR, 5, ()), ("quad", 20, 2, LINEAR, 5, SQUARE_AND_CROSS)]

MUTANTS = ("generator without e >= K", "gradient without e >= K", "nodes swapped", "chain without pair terms",
           "c_q = 1 for a square", "term scale of member 0")


def case_id(case):
    kind, n, K, interpolation, Nc, terms = case
    return "{}-n{}-K{}-{}-Nc{}{}".format(kind, n, K, interpolation, Nc,
                                         "".join("-%d%d" % t for t in terms))


def knobs(case):
    """What the route needs beside "action_eff" = 1 at the case's size."""
    n = case[1]
    return dict(action_small=1) if n <= 16 else dict(action=2) if n > 32 else {}


def effective_count(case):
    kind, _, K, _, _, terms = case
    return 2 * K + K * (K - 1) // 2 if kind == "m4" else K + len(terms)


_problems = {}


def build(case):
    """The problem of a case as a dict, on the operators, target and controls of action_features.build (kernel
    tag "effective"); "q" (count, n, n) the term matrices, "controls" (3, Nc, K)."""
    if case in _problems:
        return _problems[case]
    kind, n, K, interpolation, Nc, terms = case
    p = dict(af.build("effective", n, K, 1, interpolation, Nc))
    p.pop("refs", None)
    p.update(kind=kind, terms=tuple(terms), case=case, term_scale=None)
    rng = np.random.default_rng([n, K, Nc, len(terms), 0x65666663])
    p["q"] = np.stack([af.hermitian(rng, n) for _ in terms]) if terms else np.zeros((0, n, n), dtype=np.complex128)
    if kind == "quad":  # (the module docstring: the loud seed at 2.5)
        p["controls"] = p["controls"] / af.amplitudes(K)[:, None, None] * np.array(QUADRATIC_AMPLITUDES)[:, None, None]
    _problems[case] = p
    return p


# ---- the operators and their norms ----------------------------------------------------------------------

def hermitian_part(m):
    return (m + m.conj().T) / 2


def operators(p):
    """The augmented set G^_e, in the order of the effective controls."""
    h0, g = p["h0"], list(p["g"])
    if p["kind"] == "quad":
        return g + list(p["q"])
    K = len(g)
    ops = g + [hermitian_part(-1j * (m @ h0 - h0 @ m)) for m in g]
    ops += [hermitian_part(-1j * (g[k] @ g[l] - g[l] @ g[k])) for k in range(K) for l in range(k + 1, K)]
    return ops


def library_spectral_bound(m):
    """The host function behind the engine's spectral bounds (qocx_debug_spectral_bound: no GPU call) - never
    below the spectral radius of a Hermitian matrix and at most 1 % above it."""
    from qoc_amd import engine
    lib = engine.load_library()
    m = np.ascontiguousarray(m, dtype=np.complex128)
    out = ctypes.c_double(-1.0)
    rc = lib.qocx_debug_spectral_bound(m.view(np.float64).ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                       m.shape[0], ctypes.byref(out))
    assert rc == 0
    return out.value


def norms(p, spectral=library_spectral_bound):
    """([||H0||_1, ||G^_e||_1 ...], [the spectral bounds of the same, never above the 1-norms]); computed once
    per problem for the default `spectral`."""
    key = "norms" if spectral is library_spectral_bound else None
    if key and key in p:
        return p[key]
    mats = [p["h0"]] + operators(p)
    n1 = [onp.one_norm(m) for m in mats]
    n2 = [min(spectral(m), a) if a > 0 else 0.0 for m, a in zip(mats, n1)]
    if key:
        p[key] = (n1, n2)
    return n1, n2


# ---- the effective controls and their chain rule ---------------------------------------------------------

def node_controls(controls, interpolation, c):
    """(u [STEPS, K] at t_j + c DT, [[(knot, weight), ...]] per step): the oracle's linear interpolation and
    its transpose, or the slice the time lies in (tests/piecewise_constant.py: slice_of), weight 1."""
    controls = np.asarray(controls, dtype=np.float64)
    nc = controls.shape[0]
    times = np.linspace(0, T, nc)
    u, weights = [], []
    for j in range(STEPS):
        t = j * DT + c * DT
        if interpolation == PWC:
            s = pc.slice_of(t, nc, T)
            u.append(controls[s])
            weights.append([(s, 1.0)])
        else:
            u.append(onp.interpolate_linear_set(t, times, controls))
            i1, w1, i2, w2 = onp.interpolation_weights(t, times)
            weights.append([(i1, w1), (i2, w2)])
    return np.array(u), weights


def pairs_of(K):
    return [(k, l) for k in range(K) for l in range(k + 1, K)]


def effective_controls(p, controls, mutant=None, term_scale=None):
    """(v [STEPS, Ke], chain): chain(gbar [STEPS, Ke]) -> grads [Nc, K], the chain rule of
    m4lin_chain_kernel / quad_chain_kernel and the scatter behind it."""
    controls = np.asarray(controls, dtype=np.float64)
    nc, K = controls.shape
    if p["kind"] == "m4":
        (u1, w1), (u2, w2) = (node_controls(controls, p["interpolation"], c) for c in M4_NODES)
        if mutant == "nodes swapped":
            u1, u2 = u2, u1
        f = F0 * DT
        pairs = pairs_of(K)
        v = np.concatenate([0.5 * (u1 + u2), f * (u2 - u1)]
                           + [(f * (u2[:, k] * u1[:, l] - u2[:, l] * u1[:, k]))[:, None] for k, l in pairs], axis=1)

        def chain(gbar):
            grads = np.zeros((nc, K))
            for j in range(STEPS):
                g1 = 0.5 * gbar[j, :K] - f * gbar[j, K:2 * K]
                g2 = 0.5 * gbar[j, :K] + f * gbar[j, K:2 * K]
                for e, (k, l) in enumerate(pairs):
                    if mutant == "chain without pair terms":
                        break
                    gz = f * gbar[j, 2 * K + e]
                    g1[l] += gz * u2[j, k]
                    g1[k] -= gz * u2[j, l]
                    g2[k] += gz * u1[j, l]
                    g2[l] -= gz * u1[j, k]
                for knot, weight in w1[j]:
                    grads[knot] += weight * g1
                for knot, weight in w2[j]:
                    grads[knot] += weight * g2
            return grads
        return v, chain
    u, w = node_controls(controls, p["interpolation"], onp.M2_C1)
    terms = p["terms"]
    scale = np.ones(len(terms)) if term_scale is None else np.asarray(term_scale, dtype=np.float64)
    v = np.concatenate([u] + [(scale[q] * u[:, k] * u[:, l])[:, None] for q, (k, l) in enumerate(terms)], axis=1)

    def chain(gbar):
        grads = np.zeros((nc, K))
        for j in range(STEPS):
            acc = gbar[j, :K].copy()
            for q, (k, l) in enumerate(terms):
                ge = scale[q] * gbar[j, K + q]
                if k == l:
                    acc[k] += (1.0 if mutant == "c_q = 1 for a square" else 2.0) * u[j, k] * ge
                else:
                    acc[k] += u[j, l] * ge
                    acc[l] += u[j, k] * ge
            for knot, weight in w[j]:
                grads[knot] += weight * acc
        return grads
    return v, chain


def step_bounds(p, controls, term_scale=None):
    """[(b1, b2)] per step as effective_table_kernel forms them."""
    n1, n2 = norms(p)
    v, _ = effective_controls(p, controls, term_scale=term_scale)
    return [(DT * (n1[0] + np.abs(row) @ np.array(n1[1:])), DT * (n2[0] + np.abs(row) @ np.array(n2[1:])))
            for row in v]


def degrees_of(p, controls, term_scale=None):
    return [dm.degree_rule(b1, b2) for b1, b2 in step_bounds(p, controls, term_scale)]


def histogram(degree_lists):
    out = {}
    for degrees in degree_lists:
        for m in degrees:
            out[m] = out.get(m, 0) + 1
    return out


def evaluate(p, controls, mutant=None, term_scale=None, wrong_scale=None):
    """The route on one seed: dict(cost, grads [Nc, K], final (1, n), degrees). mutant: one of MUTANTS - a
    plausibly wrong kernel; wrong_scale: the term scales the "term scale of member 0" mutant applies."""
    if mutant == "term scale of member 0":
        term_scale = wrong_scale
    v, chain = effective_controls(p, controls, mutant, term_scale)
    ops = operators(p)
    K = np.asarray(controls).shape[1]
    degrees = degrees_of(p, controls, term_scale)
    gens = []
    for j in range(STEPS):
        used = K if mutant == "generator without e >= K" else len(ops)
        gens.append(-1j * DT * (p["h0"] + sum(v[j, e] * ops[e] for e in range(used))))
    psi = np.asarray(p["psi0"][0], dtype=np.complex128)
    vs = []
    for j in range(STEPS):
        psi, terms = am.forward_step(gens[j], psi, degrees[j])
        vs.append(terms)
    target = p["target"][0]
    ip = np.vdot(target, psi)
    cost = 1.0 - abs(ip) ** 2
    c = -2.0 * ip
    lam = np.asarray(target, dtype=np.complex128)
    gbar = np.zeros((STEPS, len(ops)))
    for j in range(STEPS - 1, -1, -1):
        lam, w = am.adjoint_step(gens[j], lam, degrees[j])
        abar = am.generator_cotangent(vs[j], w, degrees[j])
        for e in range(len(ops)):
            if mutant == "gradient without e >= K" and e >= K:
                continue
            gbar[j, e] = np.real(np.conj(c) * np.sum(np.conj(abar) * (-1j * DT * ops[e])))
    return dict(cost=cost, grads=chain(gbar), final=psi[None], degrees=degrees)


# ---- the oracle -------------------------------------------------------------------------------------------

@contextlib.contextmanager
def sliced_oracle():
    """The oracle reads a control at a time through two functions, interpolate_linear_set and its transpose
    interpolation_weights. Inside this context they follow the piecewise-constant rule - the slice the time
    lies in, weight 1 - so that the oracle's own Magnus combination and reverse rules run on piecewise
    constant pulses (tests/test_action_effective_host.py checks the result against
    tests/piecewise_constant.py: reference_a, which has no gradient)."""
    linear, weights = onp.interpolate_linear_set, onp.interpolation_weights

    def sliced(x, xs, ys):
        return np.asarray(ys)[pc.slice_of(x, len(xs), xs[-1])]

    def sliced_weights(x, xs):
        s = pc.slice_of(x, len(xs), xs[-1])
        return s, 1.0, s, 0.0
    onp.interpolate_linear_set, onp.interpolation_weights = sliced, sliced_weights
    try:
        yield
    finally:
        onp.interpolate_linear_set, onp.interpolation_weights = linear, weights


class _SlopesAtControls(onp.SchroedingerProblem):
    """H not linear in the controls: d H / d u_k at the controls under evaluation (tests/state_costs.py)."""

    def hamiltonian_slopes(self, time):
        u = onp.interpolate_linear_set(time, self.control_eval_times, self.at_controls)
        return [np.asarray(m, dtype=np.complex128) for m in self.slopes(u)], []


def hamiltonian(p, term_scale=None):
    h0, g, q, terms = p["h0"], p["g"], p["q"], p["terms"]
    scale = np.ones(len(terms)) if term_scale is None else np.asarray(term_scale, dtype=np.float64)
    return lambda u, t: (h0 + sum(u[k] * g[k] for k in range(len(g)))
                         + sum(scale[i] * u[k] * u[l] * q[i] for i, (k, l) in enumerate(terms)))


def slopes(p, term_scale=None):
    g, q, terms = p["g"], p["q"], p["terms"]
    scale = np.ones(len(terms)) if term_scale is None else np.asarray(term_scale, dtype=np.float64)

    def at(u):
        out = [np.array(m) for m in g]
        for i, (k, l) in enumerate(terms):
            out[k] = out[k] + scale[i] * u[l] * q[i]
            out[l] = out[l] + scale[i] * u[k] * q[i]
        return out
    return at


def oracle_problem(p, controls, term_scale=None, evolution_time=None):
    controls = np.asarray(controls, dtype=np.float64)
    kw = dict(control_eval_count=controls.shape[0], costs=[onp.TargetStateInfidelity(p["target"][:, :, None])],
              control_count=controls.shape[1])
    time = T if evolution_time is None else evolution_time
    if p["kind"] == "m4":
        return onp.SchroedingerProblem(time, hamiltonian(p), p["psi0"][:, :, None], N, magnus_policy="M4", **kw)
    prob = _SlopesAtControls(time, hamiltonian(p, term_scale), p["psi0"][:, :, None], N, **kw)
    prob.slopes = slopes(p, term_scale)
    prob.at_controls = controls
    return prob


def reference(p, controls, term_scale=None):
    """(cost, grads (Nc, K), final (1, n, 1)) of one seed by the oracle: magnus_policy "M4", or the quadratic
    callable under M2; a piecewise-constant pulse inside sliced_oracle()."""
    context = sliced_oracle() if p["interpolation"] == PWC else contextlib.nullcontext()
    with context:
        cost, grads, final = onp.evaluate_with_grad(oracle_problem(p, controls, term_scale), controls)
    return cost, np.real(grads), final


def references(p):
    if "refs" not in p:
        p["refs"] = [reference(p, u) for u in p["controls"]]
    return p["refs"]


# ---- the host's bound -------------------------------------------------------------------------------------

def host_bound(p, items=None, channel_max=None, scale_max=None):
    """ctx->norm_bound as qocx_upload_controls forms it for the upload `items` (B, Nc, K): DT times ||H0||_1
    plus the largest knot sum plus, for quadratic terms, sum_q ||Q_q||_1 max|r_k| max|r_l| over the whole
    upload (an ensemble: channel_max the largest |r_k| of the seeds' channels, scale_max[k] = max_m |s_mk|,
    times the largest term scale); M4: magnus_norm_bound of that, b + (sqrt(3) / 12) 2 b^2."""
    items = p["controls"] if items is None else np.asarray(items)
    K = items.shape[-1]
    n1 = [onp.one_norm(m) for m in [p["h0"]] + list(p["g"])[:K]]
    bound = n1[0] + np.max(np.abs(items) @ np.array(n1[1:]))
    if p["terms"]:
        umax = np.abs(items).reshape(-1, K).max(axis=0) if channel_max is None else np.asarray(channel_max)
        smax = np.ones(K) if scale_max is None else np.asarray(scale_max)
        cmax = np.ones(len(p["terms"])) if p["term_scale"] is None else np.abs(p["term_scale"]).max(axis=0)
        bound += sum(onp.one_norm(p["q"][i]) * cmax[i] * smax[k] * umax[k] * smax[l] * umax[l]
                     for i, (k, l) in enumerate(p["terms"]))
    bound *= DT
    return bound + F0 * 2 * bound * bound if p["kind"] == "m4" else bound


# ---- seed tables at n = 20 --------------------------------------------------------------------------------

def ensemble():
    """M = 3 members, K_r = 2 control channels and J = 1 perturbation over a quadratic base with the terms
    (0, 0) and (0, 1) and term scales c_mq; B = 2 seeds (quiet and loud, at 1.8: the host's bound multiplies
    the largest scales of the members into the terms). "items" (6, 5, 3): the expanded (K_r + J)-channel
    controls, item b M + m; "item_scale" [6]: the term scales of each item's member."""
    if "ensemble" not in _problems:
        p = dict(build(("quad", 20, 3, LINEAR, 5, SQUARE_AND_CROSS)))
        p.pop("refs", None)
        p.pop("norms", None)
        rng = np.random.default_rng([20, 3, 0x656e7365])
        p.update(kr=2, J=1, M=3, B=2, scales=1 + 0.05 * rng.standard_normal((3, 2)),
                 offsets=np.array([[-0.9], [0.1], [0.7]]), weights=rng.uniform(0.1, 1.0, 3),
                 term_scale=1 + 0.2 * rng.standard_normal((3, 2)),
                 u=rng.uniform(-1, 1, (2, 5, 2)) * np.array([1e-3, 1.8])[:, None, None])
        items = np.empty((2, 3, 5, 3))
        items[..., :2] = p["scales"][None, :, None, :] * p["u"][:, None]
        items[..., 2:] = p["offsets"][None, :, None, :]
        p["items"] = items.reshape(6, 5, 3)
        p["item_scale"] = [p["term_scale"][i % 3] for i in range(6)]
        _problems["ensemble"] = p
    return _problems["ensemble"]


def ensemble_host_bound(p):
    return host_bound(p, p["items"], channel_max=np.abs(p["u"]).reshape(-1, p["kr"]).max(axis=0).tolist() + [0.0],
                      scale_max=np.abs(p["scales"]).max(axis=0).tolist() + [0.0])


def durations():
    """Four durations of the K = 2 system under M4 (action_features.durations at n = 20): on the device the
    channels are [G_0, G_1, H0] on the controls [tau u, tau] and H0 is zero - the A_k are zero operators.
    "expanded": that plain three-channel M4 problem, whose items the seeds are."""
    if "durations" not in _problems:
        d = af.durations("one")
        p = dict(d, kind="m4", terms=(), q=np.zeros((0, d["n"], d["n"])), term_scale=None)
        p.pop("refs", None)
        p["expanded"] = dict(d["expanded"], kind="m4", terms=(), q=p["q"], term_scale=None,
                             controls=d["items"])
        p["expanded"].pop("refs", None)
        _problems["durations"] = p
    return _problems["durations"]
