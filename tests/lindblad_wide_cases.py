"""
lindblad_wide_cases.py - TEST INFRASTRUCTURE: the case table of the Lindblad engine at
33 <= n <= 64 (knob lindblad_wide, qoc_amd/csrc/qocx_lindblad16t.hip), shared by
tests/test_lindblad_wide_host.py (CPU), tools/measure_lindblad_wide_exact.py (the numbers the gates
against exact quote) and tests/test_gpu_lindblad_wide.py (the engine against the model, against exact
and against the oracle).

A table of its own: tests/lindblad_exact_cases.py is parametrised over its NAMES by files that stay as
they are. The cases are built as that table builds them (_spec, cases.gue; densities of low rank, see low_rank_density) and
results / compare are its own, so the two tables measure the same quantities the same way.

WideLindblad is the model's system with the engine's own bound of the control-free Liouvillian: the
matrix-free power iteration of liouvillian_norm (qocx_api_lindblad.hip), not the n^2 x n^2 SVD of
lindblad_model.StructuredLindblad.norm_bound, which takes 23 s at n = 64. Every case keeps
norm_bound * dt / 0.4 at least 5 % away from an integer (tests/test_lindblad_wide_host.py asserts it),
so the engine and the model cut the same grid although their bounds differ in the last per cent.

kinds: plain (PIECEWISE_CONSTANT controls), linear (LINEAR controls; model only). The step lengths dt of
the table are those that keep every seed's grid that far from an integer.

Nothing here is imported by the product.
"""

from types import SimpleNamespace

import numpy as np

from oracle import qoc_lindblad_numpy as ol
from tests import cases as cases_mod
from tests import lindblad_exact as ex
from tests import lindblad_exact_cases as xc
from tests import lindblad_model as lm

compare = xc.compare
oracle_costs = xc.oracle_costs


class WideLindblad(lm.StructuredLindblad):
    """StructuredLindblad with the norm bound the engine computes (static systems only)."""

    def liouvillian_norm(self):
        """liouvillian_norm of qocx_api_lindblad.hip: power iteration on L^H L from the engine's start
        matrix, stopped at 1e-4 relative change (not before the ninth pass), + 2 %."""
        n = self.h0.shape[0]
        al = -1j * self.h0 - 0.5 * self.decay
        ar = 1j * self.h0 - 0.5 * self.decay
        ops, gammas = self.ops, self.gammas

        def apply(x, adjoint):
            if adjoint:
                y = lm.h(al) @ x + x @ lm.h(ar)
                for gm, op in zip(gammas, ops):
                    y = y + gm * (lm.h(op) @ x @ op)
                return y
            y = al @ x + x @ ar
            for gm, op in zip(gammas, ops):
                y = y + gm * (op @ x @ lm.h(op))
            return y
        r, c = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
        x = 1.0 / (1.0 + r + c) + (r == c) + 1j * (0.3 * ((3 * r + c) % 4) - 0.4)
        x = x / np.linalg.norm(x)
        sigma, prev = 0.0, -1.0
        for it in range(400):
            y = apply(x, False)
            sigma = np.linalg.norm(y)
            if not (0 < sigma < 1e300):
                break
            if it >= 8 and abs(sigma - prev) <= 1e-4 * sigma:
                break
            prev = sigma
            x = apply(y, True)
            nx = np.linalg.norm(x)
            if not nx > 0:
                break
            x = x / nx
        return 1.02 * sigma

    def norm_bound(self, umax):
        assert self.h0_of_t is None and self.g_of_t is None and self.data_of_t is None
        ctl = sum(um * 2 * np.linalg.norm(gk, 2) for um, gk in zip(umax, self.g))
        simple = 2 * np.linalg.norm(self.h0, 2) + 2 * sum(
            abs(gm) * np.linalg.norm(op, 2) ** 2 for gm, op in zip(self.gammas, self.ops))
        return min(self.liouvillian_norm(), 1.02 * simple) + 1.02 * ctl


def _spec(name, n, L, **kw):
    return xc._spec(name, n, L, **dict(dict(N=4, ragged=False, bars=False), **kw))


SPECS = [
    # three live tiles per side with 15 pad rows in the last, a fourth of pure padding; two densities
    _spec("n33_s2_k1_l1", 33, 1, dt=0.23, S=2, K=1),
    # the last element before / exactly on a tile edge; seven waves own only padding
    _spec("n47_l2", 47, 2, dt=0.28),
    _spec("n48_l2", 48, 2, dt=0.26),
    # the first size whose fourth tile row is live; no dissipation
    _spec("n49_l0_k2", 49, 0, dt=0.21),
    # no padding at all, the most controls, the second, third and fourth operator pair
    _spec("n64_k8_l4", 64, 4, dt=0.28, S=1, K=8, amp=0.3, ops_scale=0.6, mirror=True),
    _spec("n64_k8_l5", 64, 5, dt=0.23, S=1, K=8, amp=0.3, ops_scale=0.6),
    _spec("n64_k8_l8", 64, 8, dt=0.26, S=1, K=8, amp=0.3, ops_scale=0.6, mirror=True),
    # both cost kinds, a step cost with ragged forbid counts: the sums over sixteen waves' partials
    _spec("n40_costs_ces1", 40, 2, dt=0.24, S=2, N=5, forbid=True, ragged=True, ces=1),
    _spec("n40_costs_ces2", 40, 2, dt=0.29, S=2, N=5, forbid=True, ragged=True, ces=2),
    # the general stage
    _spec("n36_nonhermitian_h0", 36, 2, dt=0.26, nonhermitian=True),
    # 1 and >= 2 sub-intervals per step in one batch
    _spec("n40_subdivisions", 40, 2, dt=0.21, h0_scale=0.3, ops_scale=0.3, amplitudes=(0.05, 2.0)),
    # stage values recomputed from the checkpoints
    _spec("n40_recompute", 40, 2, dt=0.28, debug=(1, 256, 0), mirror=True),
    # host-supplied density cotangents
    _spec("n40_cotangents", 40, 2, dt=0.21, S=2, bars=True),
    # knots and slice edges inside steps
    _spec("n40_linear_nc3_on_4_steps", 40, 2, dt=0.3, kind="linear", N=5, Nc=3),
    _spec("n40_pwc_nc7_on_4_steps", 40, 2, dt=0.25, N=5, Nc=7),
]
NAMES = [s["name"] for s in SPECS]
# against the exact superoperator reference: three cases only (4.5 - 13 s of CPU each)
EXACT_SPECS = [
    _spec("exact_n33_l2", 33, 2, dt=0.28, N=3),
    _spec("exact_n36_l1_s2_k1", 36, 1, dt=0.26, S=2, K=1, N=3),
    _spec("exact_n33_forbid", 33, 2, dt=0.29, N=3, forbid=True),
]
EXACT_NAMES = [s["name"] for s in EXACT_SPECS]
_ALL = SPECS + EXACT_SPECS
_BUILT, _MODEL, _EXACT = {}, {}, {}


def low_rank_density(rng, n, rank=3):
    """A random density of rank 3. cases.random_density is full rank, at these sizes close to the
    maximally mixed state, whose overlaps with a target hardly move with the controls (gradients of
    3e-6 at n = 33): the gradient gate, relative to the largest entry, would then hold next to nothing."""
    a = rng.standard_normal((n, rank)) + 1j * rng.standard_normal((n, rank))
    rho = a @ a.conj().T
    return rho / np.trace(rho)


def build(name):
    """The case `name` with its data (built once), as lindblad_exact_cases.build builds a plain or
    linear case, with densities of low rank."""
    if name in _BUILT:
        return _BUILT[name]
    index = [s["name"] for s in _ALL].index(name)
    c = SimpleNamespace(**_ALL[index])
    rng = np.random.default_rng(5000 + index)
    n, L, S, K, N = c.n, c.L, c.S, c.K, c.N
    c.Nc = N - 1 if c.Nc is None else c.Nc
    c.T = c.dt * (N - 1)
    gue = cases_mod.gue
    c.h0 = c.h0_scale * gue(rng, n)
    if c.nonhermitian:  # an effective Hamiltonian with a loss term: the general stages
        c.h0 = c.h0 - 0.05j * np.diag(np.arange(n) / n)
    c.g = [gue(rng, n) for _ in range(K)]
    if L == 0:
        c.operators, c.gammas = None, None
    else:
        c.operators = np.stack([c.ops_scale * (gue(rng, n) + 0.5j * gue(rng, n)) for _ in range(L)])
        c.gammas = rng.uniform(0.05, 0.3, L)
    c.rho0 = np.stack([low_rank_density(rng, n) for _ in range(S)])
    targ = np.stack([low_rank_density(rng, n) for _ in range(S)])
    c.cost_specs = [("TargetDensityInfidelity", dict(target_densities=targ, cost_multiplier=0.8))]
    if c.forbid:
        counts = [1 + (s % 2) for s in range(S)] if c.ragged else [2] * S
        forb = np.empty(S, dtype=object)
        for s in range(S):
            forb[s] = np.stack([low_rank_density(rng, n) for _ in range(counts[s])])
        if not c.ragged:
            forb = np.stack(list(forb))
        c.cost_specs.append(("ForbidDensities", dict(
            forbidden_densities=forb, system_eval_count=N, cost_eval_step=c.ces,
            cost_multiplier=0.5)))
    c.controls = c.amp * rng.standard_normal((c.seeds, c.Nc, K))
    if c.amplitudes is not None:
        c.controls *= (np.asarray(c.amplitudes)
                       / np.max(np.abs(c.controls), axis=(1, 2)))[:, None, None]
    if c.mirror:  # both seeds reach the same maxima: one sub-division group
        c.controls[1] = -c.controls[0]
    if c.bars:
        c.bar_steps = [2, N - 1]
        shape = (c.seeds, len(c.bar_steps), S, n, n)
        c.bar_values = 0.05 * (rng.standard_normal(shape) + 1j * rng.standard_normal(shape))
    _BUILT[name] = c
    return c


class ForbidDensitiesRagged(ol.ForbidDensities):
    """oracle ForbidDensities for a different number of forbidden matrices per density (the oracle's
    constructor reads the shape of one array)."""

    def __init__(self, forbidden_densities, system_eval_count, cost_eval_step=1, cost_multiplier=1.):
        ol.OracleCost.__init__(self, cost_multiplier)
        count, _ = np.divmod(system_eval_count - 1, cost_eval_step)
        self.cost_normalization_constant = count * len(forbidden_densities)
        self.forbidden = [np.asarray(f, dtype=np.complex128) for f in forbidden_densities]
        self.forbidden_densities_count = np.array([f.shape[0] for f in self.forbidden])
        self.hilbert_size = self.forbidden[0].shape[2]


class HostCotangents(object):
    """The cotangents of qocx_set_density_cotangents as the model sees them: a step cost of value zero
    whose states_bar at step k is the host's array for seed b."""
    requires_step_evaluation = True

    def __init__(self, steps, bars):
        self.steps, self.bars = list(steps), bars

    def cost(self, controls, densities, step):
        return 0.0

    def states_bar(self, controls, densities, step):
        if step in self.steps:
            return self.bars[self.steps.index(step)]
        return np.zeros_like(densities)


def case_costs(case, seed=None):
    costs = []
    for kind, kw in case.cost_specs:
        ragged = kind == "ForbidDensities" and case.ragged
        costs.append(ForbidDensitiesRagged(**kw) if ragged else getattr(ol, kind)(**kw))
    if case.bars and seed is not None:
        costs.append(HostCotangents(case.bar_steps, case.bar_values[seed]))
    return costs


def system_of(case):
    return WideLindblad(case.h0, case.g, case.gammas, case.operators)


def grid_counts(case):
    """Sub-intervals of every seed's evaluation on the model's grid."""
    system = system_of(case)
    pwc = case.kind == "plain"
    out = []
    for u in case.controls:
        umax = np.max(np.abs(u), axis=0)
        grid = lm.substep_grid(case.T, case.N, case.Nc + 1 if pwc else case.Nc, system.norm_bound(umax))
        out.append(sum(len(step) for step in grid))
    return out


def grid_margins(case):
    """norm_bound * dt / 0.4 of every seed: what ceil() turns into the sub-division count."""
    system = system_of(case)
    return [system.norm_bound(np.max(np.abs(u), axis=0)) * case.dt / 0.4 for u in case.controls]


def model_results(name):
    """The NumPy model of the device scheme on the case (computed once, shared, left unchanged)."""
    if name not in _MODEL:
        case = build(name)
        system = system_of(case)
        rows = [lm.evaluate_with_grad(system, case.controls[b], case.rho0, case.T, case.N,
                                      case_costs(case, b), case.ces,
                                      piecewise_constant=case.kind == "plain")
                for b in range(case.controls.shape[0])]
        _MODEL[name] = dict(cost=np.array([r[0] for r in rows]), grad=np.stack([r[1] for r in rows]),
                            final=np.stack([r[2] for r in rows]))
    return _MODEL[name]


def exact_results(name):
    """The exact reference of a plain case (tests/lindblad_exact.py; computed once)."""
    if name not in _EXACT:
        _EXACT[name] = xc.results(build(name), ex.sweep_member)
    return _EXACT[name]
