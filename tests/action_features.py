"""
action_features.py - TEST INFRASTRUCTURE (NumPy only): the problems that hold the matrix-free route
(qoc_amd/csrc/qocx_action.hip, qocx_action4.hip, qocx_action16.hip, qocx_action_states.hip,
qocx_action_costs.hip) to a reference away from K = 2, Nc = N, linear interpolation and a plain batch.
Imported by tests/test_action_features_host.py (CPU: the conditions below) and
tests/test_gpu_action_features.py (GPU).

The fixture is that of tests/test_gpu_action.py::problem - 13 steps (N = 14), DT = 0.05, Hermitian H0 and
G_k of 1-norm 1, psi0 = e_0 .. e_(S-1), random unit targets, seeds at amplitudes 1e-3, 1 and 5 - with the
amplitudes scaled by 2 / K for K > 2 (kept at K = 1), so that a step's bound DT (1 + sum |u_k|) spans
several Taylor degrees and the loud seed stays at or below 0.55, half of theta_18. K counts the channels
the device sees: K_r + J under an ensemble or a sweep, K + 1 under a duration sweep.

Conditions (tests/test_action_features_host.py, by the oracle and tests/action_model.py alone): the host's
knot bound of every case, after the expansion of its seed tables, is <= 0.9 theta_18; the degrees of a
case take >= 3 values; the model agrees with the oracle on every case; and every plausibly wrong kernel
(action_model.MUTANTS, the seed-0 scalar of an ensemble) misses a gate by a factor of 100 on some case.

The kernel tag "small" (qocx_action16.hip, n <= 16) has rows in every table below, at the boundaries that are
its own (K = 1, 2, 4, 6, 9: registers, LDS, images streamed per step), seed tables and optimiser starts at
n = 13, and one problem no sibling has: incoherent(), one final incoherent target of scale 0.7.

Nothing here is imported by the product.
"""

import numpy as np

from oracle import qoc_numpy as onp
from tests import piecewise_constant as pc

N, DT, CES = 14, 0.05, 3
T = DT * (N - 1)
AMPLITUDES = (1e-3, 1.0, 5.0)
LINEAR, PWC = "linear", "piecewise_constant"

# (kernel, n, K, S): the control counts. "one" the one-state kernel, "states" knob action_states,
# "costs" knob action_costs under one final target and one step cost, "wide" knob action = 2, "small" knob
# action_small = 1 (n <= 16: control 0 in registers, controls 1 .. 3 in LDS, controls >= 4 streamed per step).
# tests/test_gpu_action_wide.py::test_control_counts already holds K = 1 and 3 at n = 40 and 64 to the
# oracle; n = 33 (one row past two tiles) it does not.
CONTROL_COUNTS = ([("one", n, K, 1) for n in (17, 32) for K in (1, 3, 5)]
                  + [("states", 20, K, S) for S in (2, 4) for K in (1, 3)]
                  + [("costs", 20, K, 1) for K in (1, 3)]
                  + [("wide", 33, K, 1) for K in (1, 3)]
                  # near = min(K - 1, 3) = 0, 1, 3 with nothing streamed (K = 4), then two and five streamed
                  # images (K = 6, 9); n = 3 mostly padding, n = 16 full
                  + [("small", n, K, 1) for n in (3, 16) for K in (1, 2, 4, 6, 9)])
# (interpolation, Nc): the fewest knots, a count that divides nothing, more knots than grid points; slices
# that cut steps (13 steps in 3) and one slice per step
KNOTS = ((LINEAR, 2), (LINEAR, 5), (LINEAR, 27), (PWC, 3), (PWC, 13))
INTERPOLATIONS = [(kernel, n, 3, S, interpolation, Nc)
                  for kernel, n, S in (("one", 17, 1), ("one", 32, 1), ("costs", 20, 1), ("states", 20, 3),
                                       ("wide", 40, 1))
                  for interpolation, Nc in KNOTS]
# the step table launched for the sweeps alone at n <= 16; K = 5: a streamed control under a scatter
INTERPOLATIONS += [("small", n, 3, 1, interpolation, Nc) for n in (5, 9, 16) for interpolation, Nc in KNOTS]
INTERPOLATIONS += [("small", 16, 5, 1, LINEAR, 5), ("small", 16, 5, 1, PWC, 3)]
# (kernel, n): one final INCOHERENT target of scale 0.7 at K = 3, (LINEAR, 5) - incoherent()
INCOHERENT_TARGETS = [("small", 9), ("small", 16)]
INCOHERENT_SCALE = 0.7
# the size of the seed tables and of the optimiser's starts, per kernel
TABLE_SIZE = dict(one=20, small=13)

_problems = {}


def amplitudes(K, base=AMPLITUDES):
    return np.array(base) * (2.0 / K if K > 2 else 1.0)


def hermitian(rng, n):
    m = rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))
    m = (m + m.conj().T) / 2
    return m / onp.one_norm(m)


def build(kernel, n, K, S=1, interpolation=LINEAR, Nc=N):
    """The problem as a dict; "controls" :: (3, Nc, K). "ghost" is a further operator of 1-norm 1: what a
    kernel that keeps two images in registers would read as the second one at K = 1."""
    key = (kernel, n, K, S, interpolation, Nc)
    if key in _problems:
        return _problems[key]
    rng = np.random.default_rng([n, K, S, Nc, int(interpolation == PWC), int(kernel == "costs"), 0x66656174])
    h0 = hermitian(rng, n)
    g = np.stack([hermitian(rng, n) for _ in range(K)])
    ghost = hermitian(rng, n)
    psi0 = np.eye(n, dtype=np.complex128)[:S]
    target = rng.standard_normal((S, n)) + 1j * rng.standard_normal((S, n))
    target /= np.linalg.norm(target, axis=1, keepdims=True)
    controls = rng.uniform(-1, 1, (3, Nc, K)) * amplitudes(K)[:, None, None]
    p = dict(kernel=kernel, n=n, K=K, S=S, N=N, Nc=Nc, T=T, interpolation=interpolation, h0=h0, g=g,
             ghost=ghost, psi0=psi0, target=target, controls=controls, ces=CES if kernel == "costs" else 1)
    _problems[key] = p
    return p


def incoherent(kernel, n):
    """The K = 3, (LINEAR, 5) problem of `kernel` at n under ONE final incoherent target of scale 0.7."""
    key = ("incoherent", kernel, n)
    if key not in _problems:
        p = dict(build(kernel, n, 3, 1, LINEAR, 5), final="incoherent")
        p.pop("refs", None)
        _problems[key] = p
    return _problems[key]


def oracle_costs(p):
    """One final coherent target; the "costs" kernel adds an incoherent step target at every third step.
    incoherent(): one final incoherent target of scale 0.7 instead."""
    target = p["target"][:, :, None]
    if p.get("final") == "incoherent":
        return [onp.TargetStateInfidelity(target, neglect_relative_pahse=True, cost_multiplier=INCOHERENT_SCALE)]
    costs = [onp.TargetStateInfidelity(target)]
    if p["kernel"] == "costs":
        costs.append(onp.TargetStateInfidelityTime(N, target, neglect_relative_pahse=True,
                                                   cost_eval_step=CES, cost_multiplier=1.3))
    return costs


def descriptors(p):
    """What Engine.set_schroedinger_problem takes as costs (kinds 0 coherent, 1 incoherent: qocx.h)."""
    if p.get("final") == "incoherent":
        return [dict(kind=1, step_cost=0, scale=INCOHERENT_SCALE, vectors=p["target"])]
    descs = [dict(kind=0, step_cost=0, scale=1.0, vectors=p["target"])]
    if p["kernel"] == "costs":
        descs.append(dict(kind=1, step_cost=1, scale=1.3 / ((N - 1) // CES), vectors=p["target"]))
    return descs


def hamiltonian(p):
    h0, g = p["h0"], p["g"]
    return lambda u, t: h0 + sum(u[k] * g[k] for k in range(len(g)))


def oracle_problem(p, knots, evolution_time=None, ham=None, control_count=None):
    return onp.SchroedingerProblem(
        p["T"] if evolution_time is None else evolution_time, hamiltonian(p) if ham is None else ham,
        p["psi0"][:, :, None], N, control_eval_count=knots, costs=oracle_costs(p), cost_eval_step=p["ces"],
        control_count=len(p["g"]) if control_count is None else control_count)


def step_slices(Nc):
    """The slice every step reads under PIECEWISE_CONSTANT: that of its midpoint."""
    return [pc.slice_of((j + 0.5) * DT, Nc, T) for j in range(N - 1)]


def reference(p, controls):
    """(cost, grads (Nc, K), final (S, n, 1)) of one seed by the oracle. It interpolates linearly only: a
    piecewise-constant pulse is the linear problem on the twin knots of its step values
    (tests/piecewise_constant.py: linear_twin - the same generators at every step midpoint), and the
    gradient comes back through the transposes of the twin map and of the slice rule."""
    controls = np.asarray(controls, dtype=np.float64)
    if p["interpolation"] == LINEAR:
        cost, grads, final = onp.evaluate_with_grad(oracle_problem(p, controls.shape[0]), controls)
        return cost, np.real(grads), final
    slices = step_slices(controls.shape[0])
    u, J = pc.linear_twin(controls[slices])
    cost, gu, final = onp.evaluate_with_grad(oracle_problem(p, N), u)
    gsteps = J.T @ np.real(gu)
    grads = np.zeros(controls.shape)
    for j, s in enumerate(slices):
        grads[s] += gsteps[j]
    return cost, grads, final


def references(p):
    """The oracle's answers for the three seeds: computed once."""
    if "refs" not in p:
        p["refs"] = [reference(p, u) for u in p["controls"]]
    return p["refs"]


def host_bound(p, items=None):
    """The bound qocx_upload_controls forms from the 1-norms: DT (||H0||_1 + the largest knot sum
    sum_k |r_k| ||G_k||_1 over the items' knots)."""
    items = p["controls"] if items is None else items
    gn = np.array([onp.one_norm(m) for m in p["g"]])
    return DT * (onp.one_norm(p["h0"]) + np.max(np.abs(items) @ gn))


# ---- seed tables: S = 1, Nc = 5, at n = 20 ("one") and n = 13 ("small") -------------------------------

def _table_key(name, kernel):
    return name if kernel == "one" else name + "_" + kernel


def _seed_problem(tag, K, kernel="one", n=None):
    n = TABLE_SIZE[kernel] if n is None else n
    p = dict(build(kernel, n, K, 1, LINEAR, 5))  # (a copy: the tables below are its own)
    p["rng"] = np.random.default_rng([K, tag] if kernel == "one" else [K, tag, n])
    p.pop("refs", None)
    return p


def ensemble(kernel="one"):
    """M = 3 members, K_r = 2 control channels and J = 1 perturbation, B = 2 seeds (quiet and loud)."""
    key = _table_key("ensemble", kernel)
    if key not in _problems:
        p = _seed_problem(1, 3, kernel)
        rng = p.pop("rng")
        p.update(kr=2, J=1, M=3, B=2, scales=1 + 0.05 * rng.standard_normal((3, 2)),
                 offsets=np.array([[-0.9], [0.1], [0.7]]), weights=rng.uniform(0.1, 1.0, 3),
                 u=rng.uniform(-1, 1, (2, 5, 2)) * amplitudes(3, (1e-3, 5.0))[:, None, None])
        items = np.empty((2, 3, 5, 3))
        items[..., :2] = p["scales"][None, :, None, :] * p["u"][:, None]
        items[..., 2:] = p["offsets"][None, :, None, :]
        p["items"] = items.reshape(6, 5, 3)
        _problems[key] = p
    return _problems[key]


def ensemble_streamed():
    """The small kernel at n = 16 with K_r + J = 6: K_r = 4 control channels (registers and LDS) and J = 2
    fixed perturbations - the channels 4 and 5, whose images the sweep streams at every step. M = 3, B = 2."""
    if "ensemble_streamed" not in _problems:
        p = _seed_problem(4, 6, "small", 16)
        rng = p.pop("rng")
        p.update(kr=4, J=2, M=3, B=2, scales=1 + 0.05 * rng.standard_normal((3, 4)),
                 offsets=np.array([[-0.9, 0.3], [0.1, -0.6], [0.7, 0.5]]), weights=rng.uniform(0.1, 1.0, 3),
                 u=rng.uniform(-1, 1, (2, 5, 4)) * amplitudes(6, (1e-3, 5.0))[:, None, None])
        items = np.empty((2, 3, 5, 6))
        items[..., :4] = p["scales"][None, :, None, :] * p["u"][:, None]
        items[..., 4:] = p["offsets"][None, :, None, :]
        p["items"] = items.reshape(6, 5, 6)
        _problems["ensemble_streamed"] = p
    return _problems["ensemble_streamed"]


def sweep(kernel="one"):
    """B = 3 seeds, each a system of its own: K_r = 2 scaled channels and J = 2 fixed ones."""
    key = _table_key("sweep", kernel)
    if key not in _problems:
        p = _seed_problem(2, 4, kernel)
        rng = p.pop("rng")
        p.update(kr=2, J=2, B=3, scales=np.linspace(0.6, 1.3, 3)[:, None] * (1 + 0.05 * rng.standard_normal((3, 2))),
                 offsets=0.4 * rng.standard_normal((3, 2)),
                 u=rng.uniform(-1, 1, (3, 5, 2)) * amplitudes(4)[:, None, None])
        items = np.empty((3, 5, 4))
        items[..., :2] = p["scales"][:, None, :] * p["u"]
        items[..., 2:] = p["offsets"][:, None, :]
        p["items"] = items
        _problems[key] = p
    return _problems[key]


def durations(kernel="one"):
    """Four durations of the K = 2 system: on the device the channels are [G_0, G_1, H0] on the controls
    [tau u, tau] over the reference time, and H0 itself is zero."""
    key = _table_key("durations", kernel)
    if key not in _problems:
        p = _seed_problem(3, 2, kernel)
        rng = p.pop("rng")
        taus = np.array([0.5, 0.8, 1.0, 1.3])
        u = rng.uniform(-1, 1, (4, 5, 2)) * amplitudes(3, (1e-3, 1.0, 5.0, 2.5))[:, None, None]
        items = np.concatenate([taus[:, None, None] * u, np.broadcast_to(taus[:, None, None], (4, 5, 1))], axis=2)
        p.update(B=4, taus=taus, times=taus * T, u=u, items=items)
        # the expanded problem, as the device holds it
        p["expanded"] = dict(p, h0=np.zeros_like(p["h0"]), g=np.concatenate([p["g"], p["h0"][None]]), K=3)
        _problems[key] = p
    return _problems[key]


def item_reference(p, items):
    """The oracle on every item of an expanded seed table: [(cost, grads (Nc, K), final)]."""
    if "item_refs" not in p:
        p["item_refs"] = [reference(p, r) for r in items]
    return p["item_refs"]


# ---- the resident optimiser: S = 1, at n = 20 ("one") and n = 13 ("small") ------------------------------

OPTIMISER_STARTS = ("real", "complex", "basis", "control_cost")
ADAM = dict(learning_rate=1e-2, beta_1=0.9, beta_2=0.999, epsilon=1e-8)
VARIATION_MULTIPLIER = 0.5  # of the ControlVariation (order 1) of the "control_cost" start


def optimiser_start(variant, kernel="one"):
    """The problem, its start and the norms opt_clip holds the controls to - below the loud seed's
    amplitude, so that the clip binds. "controls" :: (3, Nc, channels) as uploaded; "complex": one complex
    control as the channels [Re, Im] and one bound on its modulus; "basis": "coefficients" (3, 4, K) of
    the sine basis "matrix" (9, 4), "controls" their expansion."""
    key = ("optimiser", variant) if kernel == "one" else ("optimiser", variant, kernel)
    if key in _problems:
        return _problems[key]
    n = TABLE_SIZE[kernel]
    if variant == "complex":
        p = dict(build(kernel, n, 2, 1, LINEAR, 5), max_norms=np.array([1.5]))
    elif variant == "basis":
        p = dict(build(kernel, n, 3, 1, LINEAR, 9))
        j = np.arange(9)[:, None]
        p["matrix"] = np.sin(np.pi * (np.arange(4)[None, :] + 1) * (j + 0.5) / 9)
        rng = np.random.default_rng([4, 9, 0x62617369] if kernel == "one" else [4, 9, n, 0x62617369])
        p["coefficients"] = rng.uniform(-1, 1, (3, 4, 3)) * (0.5 * amplitudes(3))[:, None, None]
        p["controls"] = np.einsum("jp,bpk->bjk", p["matrix"], p["coefficients"])
        p["max_norms"] = np.full(3, 1.0)
    else:
        p = dict(build(kernel, n, 3, 1, LINEAR, 5), max_norms=np.full(3, 1.0))
    p.pop("refs", None)
    p["variant"] = variant
    _problems[key] = p
    return p


def optimiser_reference(p, controls):
    """The oracle at the controls the driver evaluated; "control_cost" adds its ControlVariation."""
    cost, grads, final = reference(p, controls)
    if p["variant"] == "control_cost":
        extra = onp.ControlVariation(p["K"], p["Nc"], cost_multiplier=VARIATION_MULTIPLIER)
        cost = cost + extra.cost(controls, None, 0)
        grads = grads + extra.controls_bar(controls, None, 0)
    return cost, grads, final
