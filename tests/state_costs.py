"""
state_costs.py - TEST INFRASTRUCTURE (NumPy only): the state-cost descriptors of include/qocx.h
(qocx_cost_desc) restated in complex128, the problems and descriptor sets that
tests/test_gpu_state_costs.py runs on every sweep route, and the ways a kernel could misread a cost
table.

Every other GPU problem of the suite hands the kernels one cost triple (final COHERENT, step
INCOHERENT, step FORBID with counts [2] * S) or one coherent final target. The cost code - eval_costs,
unit_adjoint_scales and unit_adjoint_seed of qocx_sweep_common.h, eval_costs_g of qocx_general.hip,
effctl_cotangent of qocx_effctl.hip, density_costs of the Lindblad cores - exists in several copies,
and the cotangent it forms seeds every gradient. Here:

  * DescriptorCost / DescriptorDensityCost evaluate ONE descriptor exactly as qocx.h words it; they are
    oracle costs (onp.OracleCost), so onp.evaluate_with_grad and lindblad_model.evaluate_with_grad take
    them unchanged. They are the only way to state ragged forbid counts to the oracle.
  * build(row, N) makes the problem of a route-table row, descriptor_set(name, p) one of the named sets
    on it, and ROWS / SETS / pairs() list what the GPU module runs.
  * TableCost reads a descriptor through the device's cost table (upload_costs of qocx_api.hip: one
    vector pool, one counts array, vec_offset / cnt_offset per descriptor) and can read it WRONGLY;
    mutants() returns the misreadings. tests/test_state_costs_host.py proves that each moves the
    oracle's gradient by >= 1e-3 relative on every (set, row) - 1e5 parity gates.

Nothing here is imported by the product.
"""

import numpy as np

from oracle import qoc_numpy as onp
from tests.cases import gue, random_density

COHERENT, INCOHERENT, FORBID, TARGET_DENSITY, FORBID_DENSITY = 0, 1, 2, 3, 4  # include/qocx.h
GATES = dict(cost=1e-10, states=1e-10, grad=1e-8)
CES = 3            # cost_eval_step of every Schroedinger problem here
STEP_COUNTS = (7, 8)  # N: (N - 1) % CES == 0 - the final step is a cost step - and != 0
SIGMAS = (0.1, 0.8, 2.5)  # control amplitudes of the three seeds: Pade orders and squarings differ
DT = 0.3
K, NC = 2, 4
CYCLE = (1, 3, 2, 5)


def ragged_counts(S, start=0):
    """F_s drawn from 1, 3, 2, 5, ... cyclic over the states, beginning at CYCLE[start]."""
    return [CYCLE[(start + s) % len(CYCLE)] for s in range(S)]


# ---- one descriptor, as include/qocx.h words it ------------------------------------------------------

class DescriptorCost(onp.OracleCost):
    """
    kind 0: scale (1 - |sum_s <t_s|psi_s>|^2 / S^2)       vectors (S, n)
    kind 1: scale (1 - sum_s |<t_s|psi_s>|^2 / S)          vectors (S, n)
    kind 2: scale sum_s (1 / F_s) sum_f |<f_sf|psi_s>|^2   vectors (sum_s F_s, n) state-major, counts (S,)
    step_cost 1: at the system steps j cost_eval_step, j >= 1 (the final step among them when
    (N - 1) % cost_eval_step == 0); 0: on the final states only. states :: (S, n, 1).
    """
    name = "descriptor"

    def __init__(self, kind, step_cost, scale, vectors, counts=None):
        super().__init__(scale)
        self.kind, self.step_cost, self.scale = int(kind), int(bool(step_cost)), float(scale)
        self.vectors = np.asarray(vectors, dtype=np.complex128)
        self.counts = None if counts is None else [int(c) for c in counts]
        self.requires_step_evaluation = bool(step_cost)
        assert self.kind in (COHERENT, INCOHERENT, FORBID) and self.vectors.ndim == 2
        assert (self.counts is not None and sum(self.counts) == len(self.vectors)) or self.kind != FORBID

    def descriptor(self):
        """The dict Engine.set_schroedinger_problem takes."""
        d = dict(kind=self.kind, step_cost=self.step_cost, scale=self.scale, vectors=self.vectors)
        if self.kind == FORBID:
            d["counts"] = list(self.counts)
        return d

    def _overlaps(self, states):
        """kinds 0, 1: <t_s|psi_s> (S,). kind 2: [(s, f_sf, <f_sf|psi_s>)]."""
        psi = np.asarray(states, dtype=np.complex128)[:, :, 0]
        if self.kind != FORBID:
            assert len(psi) == len(self.vectors)
            return np.sum(np.conjugate(self.vectors) * psi, axis=1)
        out, base = [], 0
        assert len(self.counts) == len(psi)
        for s, fs in enumerate(self.counts):
            for f in self.vectors[base:base + fs]:
                out.append((s, f, np.sum(np.conjugate(f) * psi[s])))
            base += fs
        return out

    def cost(self, controls, states, step):
        S = len(states)
        ip = self._overlaps(states)
        if self.kind == COHERENT:
            return self.scale * (1 - abs(np.sum(ip)) ** 2 / S ** 2)
        if self.kind == INCOHERENT:
            return self.scale * (1 - np.sum(np.abs(ip) ** 2) / S)
        return self.scale * sum(abs(z) ** 2 / self.counts[s] for s, _, z in ip)

    def states_bar(self, controls, states, step):
        S = len(states)
        ip = self._overlaps(states)
        if self.kind == COHERENT:
            return (-2 * self.scale / S ** 2 * np.sum(ip) * self.vectors)[:, :, None]
        if self.kind == INCOHERENT:
            return (-2 * self.scale / S * ip[:, None] * self.vectors)[:, :, None]
        out = np.zeros(np.shape(states), dtype=np.complex128)
        for s, f, z in ip:
            out[s, :, 0] += 2 * self.scale / self.counts[s] * z * f
        return out


class DescriptorDensityCost(onp.OracleCost):
    """
    kind 3: scale (1 - sum_s |tr(T_s^H rho_s)| / (S n))                 vectors (S, n, n)
    kind 4: scale sum_s (1 / F_s) sum_f |tr(F_sf^H rho_s) / n|^2        vectors (sum_s F_s, n, n), counts
    for tests/lindblad_model.evaluate_with_grad. densities :: (S, n, n).
    """
    name = "density_descriptor"

    def __init__(self, kind, step_cost, scale, vectors, counts=None):
        super().__init__(scale)
        self.kind, self.step_cost, self.scale = int(kind), int(bool(step_cost)), float(scale)
        self.vectors = np.asarray(vectors, dtype=np.complex128)
        self.counts = None if counts is None else [int(c) for c in counts]
        self.requires_step_evaluation = bool(step_cost)
        assert self.kind in (TARGET_DENSITY, FORBID_DENSITY) and self.vectors.ndim == 3
        assert self.kind == TARGET_DENSITY or sum(self.counts) == len(self.vectors)

    def descriptor(self):
        d = dict(kind=self.kind, step_cost=self.step_cost, scale=self.scale, vectors=self.vectors)
        if self.kind == FORBID_DENSITY:
            d["counts"] = list(self.counts)
        return d

    def _traces(self, densities):
        """[(s, M, tr(M^H rho_s))] over the matrices of the descriptor."""
        counts = [1] * len(densities) if self.kind == TARGET_DENSITY else self.counts
        assert len(counts) == len(densities)
        out, base = [], 0
        for s, fs in enumerate(counts):
            for m in self.vectors[base:base + fs]:
                out.append((s, m, np.sum(np.conjugate(m) * densities[s])))
            base += fs
        return out

    def cost(self, controls, densities, step):
        S, n = len(densities), densities.shape[-1]
        tr = self._traces(densities)
        if self.kind == TARGET_DENSITY:
            return self.scale * (1 - sum(abs(z) for _, _, z in tr) / (S * n))
        return self.scale * sum(abs(z / n) ** 2 / self.counts[s] for s, _, z in tr)

    def states_bar(self, controls, densities, step):
        S, n = len(densities), densities.shape[-1]
        out = np.zeros(np.shape(densities), dtype=np.complex128)
        for s, m, z in self._traces(densities):
            if self.kind == TARGET_DENSITY:
                if abs(z) > 0:
                    out[s] += -self.scale / (S * n) * (z / abs(z)) * m
            else:
                out[s] += 2 * self.scale / (self.counts[s] * n) * (z / n) * m
        return out


# ---- the route table ------------------------------------------------------------------------------------

def _row(route, n, S, knobs=None, kind="plain"):
    name = "{}_n{}_S{}".format(route, n, S)
    return dict(name=name, route=route, n=n, S=S, knobs=dict(knobs or {}), kind=kind)


# One row per (route, n, S): the rule of resident_route (qocx_host_resident.hip) that the knobs and the
# shape select. K = 2, Nc = 4, three seeds. kind: "plain" (M2, H0 + sum u_k G_k), "quadratic" (M2 plus
# u_0^2 Q through qocx_set_quadratic_terms: the quadratic effective controls), "m4" (MagnusPolicy.M4
# on constant H0, G_k: the M4-linear effective controls, knob m4_linear).
ROWS = (
    [_row("sweepi", n, S) for n, S in ((3, 1), (16, 5), (16, 8))]
    # (one state at n <= 32 is sweep1's by default; knob sweep_one 0 leaves it to the one-wave chain)
    + [_row("chain1", n, S, dict(sweep_inverse_small=0)) for n, S in ((8, 1), (16, 3))]
    + [_row("chain_one_wave", 8, 1, dict(sweep_inverse_small=0, sweep_one=0)),
       _row("chain_one_wave", 17, 1, dict(sweep_one=0))]
    + [_row("sweep1", n, 1) for n in (17, 32)]
    + [_row("chain2", n, S) for n, S in ((20, 2), (20, 5), (24, 7))]
    + [_row("sweepd", 24, S) for S in (8, 9)]
    + [_row("chain2_dense_off", 24, S, dict(sweep_dense=0)) for S in (8, 9)]
    # (n <= 16: the inverse-image sweep takes precedence over sweep_impl 3 unless it is switched off)
    + [_row("sweep3", 12, 1, dict(sweep_impl=3, sweep_inverse_small=0)), _row("sweep3", 24, 3, dict(sweep_impl=3))]
    + [_row("latency_umode%d" % um, n, 1, dict(latency=1, sweep_umode=um))
       for um in (1, 0) for n in (8, 24)]
    + [_row("chain4", n, S) for n, S in ((33, 1), (40, 5), (64, 13))]
    + [_row("general", n, S) for n, S in ((66, 1), (66, 3), (40, 14))]
    + [_row("quadratic", 12, S, kind="quadratic") for S in (1, 2)]
    + [_row("m4_linear", 12, S, kind="m4") for S in (1, 2)])
ROW_BY_NAME = dict((r["name"], r) for r in ROWS)
assert len(ROW_BY_NAME) == len(ROWS)

SETS = ("final_incoherent", "final_coherent", "step_coherent", "step_incoherent_alone", "forbid_ragged",
        "two_forbids", "target_after_ragged_forbid", "two_finals", "forbid_final")
MULTI_SETS = ("two_forbids", "target_after_ragged_forbid", "two_finals")

# (set, row name) pairs the engine refuses by design: none. Latency mode (one control set at a time)
# takes every descriptor set; the rows that set it evaluate their seeds one by one.
REFUSED = ()


def pairs():
    """Every (set, row) the GPU module runs and the CPU module proves the conditions for."""
    return [(s, r["name"]) for r in ROWS for s in SETS if (s, r["name"]) not in REFUSED]


def _unit_vectors(rng, count, n):
    v = rng.standard_normal((count, n)) + 1j * rng.standard_normal((count, n))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


class _SlopesAtControls(onp.SchroedingerProblem):
    """H not linear in the controls: d H / d u_k at the controls under evaluation."""

    def hamiltonian_slopes(self, time):
        u = onp.interpolate_linear_set(time, self.control_eval_times, self.at_controls)
        return [np.asarray(m, dtype=np.complex128) for m in self.slopes(u)], []


_problems = {}

# (n, S, kind): which draw of the random inputs a shape uses (default 0). Chance makes an overlap sum_s
# <t_s|psi_s> small now and then, and the descriptor that carries it then holds less than a tenth of
# the gradient at one seed: those shapes take the first draw on which every condition of
# tests/test_state_costs_host.py holds. Inputs are chosen, no condition is loosened.
DRAWS = {(24, 7, "plain"): 1, (24, 9, "plain"): 1, (33, 1, "plain"): 1, (64, 13, "plain"): 1}


def build(row, N):
    """
    The problem of a row at N system steps: H0 = 2 gue, K = 2 gue drives (spectral norm 1 each),
    dt = 0.3, random unit initial states, and the vector pools of the descriptor sets: complex random
    unit targets A and B (so that sum_s <t_s|psi_s> carries a phase, and no target is the orthonormal
    completion of another) and three pools of forbidden vectors. The operators, states and controls of
    a row are the same at both N. Returns a dict; "controls" :: (3, Nc, K).
    """
    row = ROW_BY_NAME[row] if isinstance(row, str) else row
    key = (row["n"], row["S"], row["kind"], N)
    if key in _problems:
        return _problems[key]
    n, S, kind = row["n"], row["S"], row["kind"]
    rng = np.random.default_rng([n, S, ("plain", "quadratic", "m4").index(kind),
                                 DRAWS.get((n, S, kind), 0), 0x636F7374])
    h0 = 2.0 * gue(rng, n)
    g = [gue(rng, n) for _ in range(K)]
    quad = 0.5 * gue(rng, n)
    init = _unit_vectors(rng, S, n)
    vec = dict(A=_unit_vectors(rng, S, n), B=_unit_vectors(rng, S, n))
    for i, start in enumerate((0, 1, 2)):
        vec["F%d" % i] = _unit_vectors(rng, sum(ragged_counts(S, start)), n)
    controls = np.stack([s * rng.standard_normal((NC, K)) for s in SIGMAS])
    p = dict(row=row, n=n, S=S, N=N, Nc=NC, K=K, T=DT * (N - 1), dt=DT, ces=CES, kind=kind,
             policy="M4" if kind == "m4" else "M2", h0=h0, g=np.stack(g), init=init, vec=vec,
             controls=controls, count=(N - 1) // CES,
             quadratic=(np.array([[0, 0]], dtype=np.int32), quad[None]) if kind == "quadratic" else None)
    _problems[key] = p
    return p


def oracle_problem(p, costs, seed=None):
    """The oracle's problem with `costs`; a quadratic row needs the seed whose controls it is evaluated at."""
    h0, g = p["h0"], p["g"]
    args = dict(control_eval_count=p["Nc"], costs=costs, cost_eval_step=p["ces"],
                magnus_policy=p["policy"], control_count=p["K"])
    if p["kind"] != "quadratic":
        return onp.SchroedingerProblem(p["T"], lambda u, t: h0 + u[0] * g[0] + u[1] * g[1],
                                       p["init"][:, :, None], p["N"], **args)
    q = p["quadratic"][1][0]
    prob = _SlopesAtControls(p["T"], lambda u, t: h0 + u[0] * g[0] + u[1] * g[1] + u[0] * u[0] * q,
                             p["init"][:, :, None], p["N"], **args)
    prob.slopes = lambda u: [g[0] + 2 * u[0] * q, g[1]]
    prob.at_controls = p["controls"][seed]
    return prob


def evaluate(p, costs, seed):
    """onp.evaluate_with_grad of seed `seed`: (error, grads (Nc, K), final (S, n, 1))."""
    return onp.evaluate_with_grad(oracle_problem(p, costs, seed), p["controls"][seed])


BALANCED_GRADIENT = 0.1


def descriptor_set(name, p):
    """
    The named set as DescriptorCosts. Step scales carry 1 / count, count = (N - 1) // ces = 2, forbid
    scales 1 / S as well, as the product's classes fold them in. The scales are then balanced: the
    gradient of a random cost is as large as chance makes its overlaps (and falls with n and S), so
    each scale is multiplied by BALANCED_GRADIENT over the geometric mean, over the three seeds, of the
    max-norm of the oracle gradient of that descriptor alone. Every gradient then stands above the
    floor of the gradient gate (1e-3), and no descriptor of a set of several hides behind another
    (tests/test_state_costs_host.py: each holds >= 10 % of the gradient at every seed).
    """
    key = ("set", name)
    if key not in p:
        costs = _nominal_set(name, p)
        for c in costs:
            norms = [np.max(np.abs(evaluate(p, [c], b)[1])) for b in range(len(SIGMAS))]
            c.scale *= BALANCED_GRADIENT / float(np.exp(np.mean(np.log(norms))))
            c.cost_multiplier = c.scale
        p[key] = costs
    return p[key]


def _nominal_set(name, p):
    S, v, count = p["S"], p["vec"], p["count"]
    r0, r1, r2 = ragged_counts(S, 0), ragged_counts(S, 1), ragged_counts(S, 2)
    D = DescriptorCost
    if name == "final_incoherent":
        return [D(INCOHERENT, 0, 0.7, v["A"])]
    if name == "final_coherent":
        return [D(COHERENT, 0, 0.7, v["A"])]
    if name == "step_coherent":
        return [D(COHERENT, 1, 1.3 / count, v["A"])]
    if name == "step_incoherent_alone":
        return [D(INCOHERENT, 1, 1.3 / count, v["A"])]
    if name == "forbid_ragged":
        return [D(FORBID, 1, 0.9 / (count * S), v["F0"], r0)]
    if name == "two_forbids":
        return [D(FORBID, 1, 0.9 / (count * S), v["F0"], r0), D(FORBID, 1, 1.1 / (count * S), v["F1"], r1)]
    # (counts 2, 5, 1, 3, ...: their sum differs from S F_0 at every S >= 2 - "vec_offset uniform" bites)
    if name == "target_after_ragged_forbid":
        return [D(FORBID, 1, 0.9 / (count * S), v["F2"], r2), D(INCOHERENT, 1, 1.3 / count, v["A"]),
                D(COHERENT, 0, 0.7, v["B"])]
    if name == "two_finals":
        return [D(COHERENT, 0, 0.7, v["A"]), D(INCOHERENT, 0, 1.1, v["B"])]
    if name == "forbid_final":
        return [D(FORBID, 0, 0.9 / S, v["F1"], r1)]
    raise KeyError(name)


def unit_adjoint_applies(name, S):
    """upload_costs: unit_ok = one final COHERENT cost, or one final INCOHERENT cost on one state."""
    return name == "final_coherent" or (name == "final_incoherent" and S == 1)


# ---- the device's cost table, and the ways to misread it -----------------------------------------------

def device_table(costs):
    """upload_costs (qocx_api.hip) restated: the vectors of all descriptors in one pool, the forbid
    counts in one array, and per descriptor (vec_offset, cnt_offset)."""
    pool, counts, offsets = [], [], []
    for c in costs:
        offsets.append((len(pool), len(counts)))
        pool.extend(c.vectors)
        if c.kind == FORBID:
            counts.extend(c.counts)
    return np.array(pool), counts, offsets


class TableCost(onp.OracleCost):
    """
    A descriptor read through the device's table as eval_costs reads it - and, by its options, read
    wrongly: `kind` another kind; `vec_offset` / `cnt_offset` other offsets; uniform=True: F_s =
    counts[cnt_offset] for every state; scalar_of_state0=True: the cotangent of an incoherent cost with
    <t_0|psi_0> in place of every <t_s|psi_s> (the value is untouched). Reads past the pool wrap around.
    """

    def __init__(self, table, index, cost, kind=None, vec_offset=None, cnt_offset=None, uniform=False,
                 scalar_of_state0=False):
        super().__init__(cost.scale)
        self.pool, self.counts, offsets = table
        self.kind = cost.kind if kind is None else kind
        self.scale, self.requires_step_evaluation = cost.scale, cost.requires_step_evaluation
        self.vec_offset = offsets[index][0] if vec_offset is None else vec_offset
        self.cnt_offset = offsets[index][1] if cnt_offset is None else cnt_offset
        self.uniform, self.scalar_of_state0 = uniform, scalar_of_state0

    def _read(self, S):
        """kinds 0, 1: the S vectors. kind 2: [(s, F_s, vector)]."""
        def at(i):
            return self.pool[(self.vec_offset + i) % len(self.pool)]
        if self.kind != FORBID:
            return np.array([at(s) for s in range(S)])
        out, base = [], 0
        for s in range(S):
            fs = self.counts[(self.cnt_offset + (0 if self.uniform else s)) % len(self.counts)]
            out.extend((s, fs, at(base + f)) for f in range(fs))
            base += fs
        return out

    def cost(self, controls, states, step):
        psi, S = np.asarray(states)[:, :, 0], len(states)
        if self.kind == FORBID:
            return self.scale * sum(abs(np.vdot(f, psi[s])) ** 2 / fs for s, fs, f in self._read(S))
        ip = np.sum(np.conjugate(self._read(S)) * psi, axis=1)
        if self.kind == COHERENT:
            return self.scale * (1 - abs(np.sum(ip)) ** 2 / S ** 2)
        return self.scale * (1 - np.sum(np.abs(ip) ** 2) / S)

    def states_bar(self, controls, states, step):
        psi, S = np.asarray(states)[:, :, 0], len(states)
        out = np.zeros((S, psi.shape[1]), dtype=np.complex128)
        if self.kind == FORBID:
            for s, fs, f in self._read(S):
                out[s] += 2 * self.scale / fs * np.vdot(f, psi[s]) * f
            return out[:, :, None]
        t = self._read(S)
        ip = np.sum(np.conjugate(t) * psi, axis=1)
        if self.kind == COHERENT:
            return (-2 * self.scale / S ** 2 * np.sum(ip) * t)[:, :, None]
        if self.scalar_of_state0:
            ip = np.full(S, ip[0])
        return (-2 * self.scale / S * ip[:, None] * t)[:, :, None]


class _NotAtStep(onp.OracleCost):
    """A step cost that the final step leaves out."""

    def __init__(self, cost, step):
        super().__init__(cost.scale)
        self.inner, self.step, self.requires_step_evaluation = cost, step, True

    def cost(self, controls, states, step):
        return 0.0 if step == self.step else self.inner.cost(controls, states, step)

    def states_bar(self, controls, states, step):
        if step == self.step:
            return np.zeros(np.shape(states), dtype=np.complex128)
        return self.inner.states_bar(controls, states, step)


def mutants(costs, S, N, ces=CES):
    """
    {name: (costs, touches the forward value)}: the ways a kernel could misread the table of `costs`
    (DescriptorCosts) that apply to it. A mutation that would be the identity on this set - a swap of
    the target kinds or state 0's scalar at S = 1, uniform counts where nothing is ragged - is absent.
      kinds swapped                 every COHERENT read as INCOHERENT and vice versa (S >= 2)
      scalar of state 0             an INCOHERENT cotangent with state 0's <t|psi> for all states (S >= 2)
      counts uniform                every FORBID with F_s = F_0 for all states (S >= 2)
      counts of the first forbid    the second FORBID reads the counts of the first (cnt_offset 0)
      vec_offset uniform            the descriptors behind a FORBID placed as if its counts were
                                    uniform: vec_offset = S F_0 behind it (S >= 2)
      final step cost               step costs left out at the final step when (N - 1) % ces == 0, and
                                    counted there when it is not
    """
    table = device_table(costs)
    kinds = [c.kind for c in costs]
    out = {}

    def read(**per_index):
        return [TableCost(table, i, c, **per_index.get("i%d" % i, {})) for i, c in enumerate(costs)]

    swap = {COHERENT: INCOHERENT, INCOHERENT: COHERENT}
    if S >= 2 and any(k in swap for k in kinds):
        out["kinds swapped"] = (read(**{"i%d" % i: dict(kind=swap[k]) for i, k in enumerate(kinds)
                                        if k in swap}), True)
    if S >= 2 and INCOHERENT in kinds:
        out["scalar of state 0"] = (read(**{"i%d" % i: dict(scalar_of_state0=True)
                                            for i, k in enumerate(kinds) if k == INCOHERENT}), False)
    forbids = [i for i, k in enumerate(kinds) if k == FORBID]
    if S >= 2 and forbids:
        out["counts uniform"] = (read(**{"i%d" % i: dict(uniform=True) for i in forbids}), True)
    if len(forbids) >= 2:
        out["counts of the first forbid"] = (read(**{"i%d" % forbids[1]: dict(cnt_offset=0)}), True)
    if S >= 2 and forbids and forbids[0] + 1 < len(costs):
        wrong, opts = table[2][forbids[0]][0] + S * costs[forbids[0]].counts[0], {}
        for i in range(forbids[0] + 1, len(costs)):
            opts["i%d" % i] = dict(vec_offset=wrong)
            wrong += S * costs[i].counts[0] if costs[i].kind == FORBID else S
        out["vec_offset uniform"] = (read(**opts), True)
    if any(c.step_cost for c in costs):
        if (N - 1) % ces == 0:
            out["final step cost"] = ([_NotAtStep(c, N - 1) if c.step_cost else c for c in costs], True)
        else:
            extra = [DescriptorCost(c.kind, 0, c.scale, c.vectors, c.counts) for c in costs if c.step_cost]
            out["final step cost"] = (list(costs) + extra, True)
    return out


# ---- gates ----------------------------------------------------------------------------------------------

def gate_fractions(ref, out):
    """Errors of out = (cost, grads (Nc, K), final (S, n)) against the oracle's ref = (error, grads,
    final (S, n, 1)) as fractions of the parity gates: cost and states 1e-10 relative, gradient 1e-8 of
    max(|g|, 1e-3) - over the whole gradient and per control channel (tests/mixed_pulses.py)."""
    err, gr, fin = ref
    cost, grads, final = out
    fr = dict(cost=abs(err - cost) / max(1.0, abs(err)) / GATES["cost"],
              states=np.max(np.abs(fin[:, :, 0] - final)) / max(np.max(np.abs(fin)), 1e-300) / GATES["states"],
              grad=np.max(np.abs(gr - grads)) / max(np.max(np.abs(gr)), 1e-3) / GATES["grad"])
    fr["grad_channel"] = max(
        np.max(np.abs(gr[:, k] - grads[:, k])) / max(np.max(np.abs(gr[:, k])), 1e-3) / GATES["grad"]
        for k in range(gr.shape[1]))
    return fr


# ---- Lindblad companion ------------------------------------------------------------------------------------

LINDBLAD_SHAPES = (dict(n=4, L=1, knobs={}), dict(n=16, L=2, knobs={}),
                   dict(n=20, L=2, knobs=dict(lindblad_4t=1)), dict(n=20, L=2, knobs=dict(lindblad_4t=0)))
LINDBLAD_SETS = ("target_final", "two_target_finals", "two_forbids", "target_step")
LINDBLAD_DRAWS = {}  # n: draw of the random inputs, as DRAWS
_lindblad_problems = {}


def lindblad_problem(n, L):
    """S = 2, N = 4, Nc = 3, K = 2, a quiet and a loud seed; T = 0.9."""
    if (n, L) in _lindblad_problems:
        return _lindblad_problems[n, L]
    S, N, Nc = 2, 4, 3
    rng = np.random.default_rng([n, L, LINDBLAD_DRAWS.get(n, 0), 0x6C696E64])
    h0 = 1.5 * gue(rng, n)
    g = [gue(rng, n) for _ in range(K)]
    ops = np.stack([gue(rng, n) + 0.5j * gue(rng, n) for _ in range(L)])
    gam = rng.uniform(0.05, 0.3, L)

    def dyads(count, hermitian=True):
        """|a><b| of random unit vectors: tr(M^H rho) = <a|rho|b> carries a phase (and the engine takes
        the stages of a problem that is not Hermitian); hermitian: |a><b| + |b><a|, a real trace of
        either sign, on the Hermitian stages."""
        a, b = _unit_vectors(rng, count, n), _unit_vectors(rng, count, n)
        m = a[:, :, None] * np.conjugate(b)[:, None, :]
        return m + np.conjugate(np.swapaxes(m, 1, 2)) if hermitian else m

    # (random densities lie near the maximally mixed one, which answers no control: half pure ones, and
    # matrices of rank <= 2 to project on)
    pure = _unit_vectors(rng, S, n)
    rho0 = np.stack([0.5 * np.outer(v, np.conjugate(v)) + 0.5 * random_density(rng, n) for v in pure])
    vec = dict(A=dyads(S), B=dyads(S, hermitian=False), F0=dyads(4), F1=dyads(3))
    q = dict(n=n, S=S, N=N, Nc=Nc, K=K, L=L, T=0.3 * (N - 1), h0=h0, g=g, ops=ops, gam=gam,
             rho0=rho0, vec=vec,
             controls=np.array([0.3, 1.0])[:, None, None] * rng.standard_normal((2, Nc, K)))
    _lindblad_problems[n, L] = q
    return q


def lindblad_model_run(q, costs, ces, seed, want_grad=True):
    from tests import lindblad_model as lm
    system = lm.StructuredLindblad(q["h0"], q["g"], q["gam"], q["ops"])
    return lm.evaluate_with_grad(system, q["controls"][seed], q["rho0"], q["T"], q["N"], costs, ces,
                                 want_grad=want_grad)


def lindblad_set(name, q, ces):
    """
    The gates of the Lindblad tests are absolute (1e-12 on the cost), so the scales keep every cost at
    O(1): a target cost is scale (1 - O(1 / n)) - scale 0.2 n, for a gradient of O(1e-3) -, a forbid
    cost scale O(1 / n^2). The two descriptors of a set of two are balanced against each other as in
    descriptor_set(), their product kept.
    """
    key = ("set", name, ces)
    if key in q:
        return q[key]
    v, S, n = q["vec"], q["S"], q["n"]
    count = (q["N"] - 1) // ces
    D = DescriptorDensityCost
    if name == "target_final":
        costs = [D(TARGET_DENSITY, 0, 0.2 * n, v["A"])]
    elif name == "two_target_finals":
        costs = [D(TARGET_DENSITY, 0, 0.2 * n, v["A"]), D(TARGET_DENSITY, 0, 0.2 * n, v["B"])]
    elif name == "two_forbids":
        costs = [D(FORBID_DENSITY, 1, 10.0 * n * n / (count * S), v["F0"], [1, 3]),
                 D(FORBID_DENSITY, 1, 10.0 * n * n / (count * S), v["F1"], [2, 1])]
    elif name == "target_step":
        costs = [D(TARGET_DENSITY, 1, 0.2 * n / count, v["A"])]
    else:
        raise KeyError(name)
    if len(costs) == 2:
        mean = [np.exp(np.mean([np.log(np.max(np.abs(lindblad_model_run(q, [c], ces, b)[1])))
                                for b in range(len(q["controls"]))])) for c in costs]
        for c, factor in zip(costs, (np.sqrt(mean[1] / mean[0]), np.sqrt(mean[0] / mean[1]))):
            c.scale *= float(factor)
            c.cost_multiplier = c.scale
    q[key] = costs
    return costs
