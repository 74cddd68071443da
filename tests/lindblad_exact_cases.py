"""
lindblad_exact_cases.py - TEST INFRASTRUCTURE: the case table shared by
tests/test_lindblad_exact_host.py (model against exact, on the CPU), tools/measure_lindblad_exact.py
(the numbers the gates of tests/lindblad_exact.py quote) and tests/test_gpu_lindblad_exact.py (the
engine against exact).

A case is random Hermitian h0 and G_k (cases.gue), random densities (cases.random_density), one final
TargetDensityInfidelity unless it names a step cost, and `seeds` pulses. results(case, member) runs
every seed (member, sweep seed) through `member`, a function with the signature of
lindblad_exact.sweep_member: exact_results uses that one, model_results the NumPy model of the device
scheme driven the same way. compare(got, want) gives the error of every quantity as the gates of
tests/lindblad_exact.py measure it.

kinds: plain (PIECEWISE_CONSTANT), linear (LINEAR controls, or h0(t) through stage tables), ensemble
(set_lindblad_ensemble + rates), sweep (set_lindblad_sweep), duration (a sweep whose tables carry
tau_b: h0 is the first fixed channel), search (lindblad_sweep_set_durations on a duration case).

Nothing here is imported by the product.
"""

from types import SimpleNamespace

import numpy as np

from oracle import qoc_lindblad_numpy as ol
from tests import cases as cases_mod
from tests import lindblad_exact as ex

DT = 0.3


def _spec(name, n, L, **kw):
    return dict(dict(name=name, kind="plain", n=n, L=L, S=1, K=2, N=5, Nc=None, seeds=2, ops="complex",
                     knobs={}, debug=None, forbid=False, ces=1, amp=0.7, dt=DT, h0_scale=1.5,
                     ops_scale=1.0, gamma=None, nonhermitian=False, amplitudes=None, mirror=False,
                     h0_frequency=None, subdivision=0, base=None, weight=0.0), **kw)


SPECS = [
    # one tile, n <= 16
    _spec("n4_l0", 4, 0),
    _spec("n4_l1_pad1", 4, 1, knobs=dict(lindblad_pad_operator=1)),
    _spec("n4_l1_pad0", 4, 1, knobs=dict(lindblad_pad_operator=0)),
    _spec("n7_l2", 7, 2, N=6),
    _spec("n16_l3_complex_ops", 16, 3, N=4),
    _spec("n16_l3_real_ops", 16, 3, N=4, ops="real"),
    _spec("n16_l4_complex_ops", 16, 4, N=3),
    _spec("n16_l4_real_ops", 16, 4, N=3, ops="real"),
    _spec("n3_l5_one_wave", 3, 5, ops_scale=0.6),
    _spec("n3_l8_one_wave", 3, 8, ops_scale=0.6),
    _spec("n2_s8", 2, 2, S=8),
    _spec("n3_s12_hbm_scratch", 3, 2, S=12),
    _spec("n5_k8", 5, 2, K=8, N=4, amp=0.3),
    _spec("n6_nonhermitian_h0", 6, 2, nonhermitian=True),
    # tile kernel, 17 <= n <= 32
    _spec("n17_l1_s2", 17, 1, S=2, N=4),
    _spec("n20_l3", 20, 3, N=4),
    _spec("n24_l0", 24, 0, N=3),
    _spec("n32_l1", 32, 1, N=3, K=1),
    _spec("n20_l3_4t0", 20, 3, N=4, knobs=dict(lindblad_4t=0)),
    _spec("n20_l3_hermitian0", 20, 3, N=4, knobs=dict(lindblad_hermitian=0)),
    # classic launch
    _spec("n4_forbid_ces1", 4, 2, N=6, forbid=True, ces=1),
    _spec("n4_forbid_ces2", 4, 2, N=6, forbid=True, ces=2),
    _spec("n20_forbid_ces1", 20, 2, N=4, forbid=True, ces=1),
    _spec("n20_forbid_ces2", 20, 2, N=5, forbid=True, ces=2),
    _spec("n4_two_sided0", 4, 2, knobs=dict(lindblad_two_sided=0)),
    _spec("n20_two_sided0", 20, 2, N=4, knobs=dict(lindblad_two_sided=0)),
    _spec("n4_recompute", 4, 2, debug=(1, 256, 0), mirror=True),
    _spec("n20_recompute", 20, 2, N=4, debug=(1, 256, 0), mirror=True),
    _spec("n4_one_wave", 4, 2, debug=(0, 256, 1)),
    # sub-division counts: 1, 2 and >= 4 sub-intervals per step in one batch; gamma ||L||^2 >> ||H||
    _spec("n4_l2_subdivisions", 4, 2, seeds=3, h0_scale=0.3, ops_scale=0.3,
          amplitudes=(0.05, 0.3, 2.0)),
    _spec("n4_l2_dissipator_dominated", 4, 2, gamma=8.0),
    # slices that do not line up with the steps
    _spec("n5_nc4_on_6_steps", 5, 2, N=7, Nc=4),
    _spec("n5_nc7_on_3_steps", 5, 2, N=4, Nc=7),
    # accumulation
    _spec("n4_l2_n501", 4, 2, N=501, seeds=1, dt=0.05),
    # LINEAR controls and h0(t), against linear(...)
    _spec("linear_n4_l2_nc5", 4, 2, kind="linear", N=5, Nc=5),
    _spec("linear_n20_l2_nc3", 20, 2, kind="linear", N=4, Nc=3),
    _spec("linear_n4_h0_of_t", 4, 2, kind="linear", N=5, Nc=4, h0_frequency=2.0, h0_scale=1.0,
          ops_scale=0.5, amp=0.4, dt=0.2, subdivision=6),
    # rates and sweeps
    _spec("ensemble_n4", 4, 2, kind="ensemble"),
    _spec("ensemble_n20", 20, 2, kind="ensemble", N=3),
    _spec("sweep_n4_l1", 4, 1, kind="sweep", seeds=4),
    _spec("sweep_n4_l2", 4, 2, kind="sweep", seeds=4),
    _spec("sweep_n16_l3_complex_ops", 16, 3, kind="sweep", seeds=4, N=4),
    _spec("sweep_n20_l2", 20, 2, kind="sweep", seeds=4, N=3),
    _spec("duration_n4_l1", 4, 1, kind="duration", seeds=4),
    _spec("duration_n4_l2", 4, 2, kind="duration", seeds=4),
    _spec("duration_n16_l3_complex_ops", 16, 3, kind="duration", seeds=4, N=4),
    _spec("duration_n20_l2", 20, 2, kind="duration", seeds=4, N=3),
    _spec("search_n4_l2_free", 4, 2, kind="search", seeds=4, base="duration_n4_l2", weight=0.0),
    _spec("search_n4_l2_priced", 4, 2, kind="search", seeds=4, base="duration_n4_l2", weight=0.3),
    _spec("search_n20_l2_free", 20, 2, kind="search", seeds=4, N=3, base="duration_n20_l2",
          weight=0.0),
    _spec("search_n20_l2_priced", 20, 2, kind="search", seeds=4, N=3, base="duration_n20_l2",
          weight=0.3),
    # gamma ||L||^2 T = 50 and 20: where rounding residue that a stage loop lets grow at the rate of the
    # dissipators shows (the Hermitian chain form did: 1e-8 on the first of these before it took the
    # anti-Hermitian part of its argument off at every sub-interval)
    _spec("n4_l2_dissipator_dominated_long", 4, 2, N=9, gamma=8.0),
    _spec("n20_l2_dissipator_dominated", 20, 2, N=4, gamma=8.0),
]
NAMES = [s["name"] for s in SPECS]
TAUS = np.array([0.5, 0.8, 1.2, 1.5])
MEMBERS = 3
_BUILT, _EXACT = {}, {}


def build(name):
    """The case `name` with its data (built once)."""
    if name in _BUILT:
        return _BUILT[name]
    spec = next(s for s in SPECS if s["name"] == name)
    if spec["base"] is not None:  # a search runs on the data of its duration sweep
        c = SimpleNamespace(**dict(vars(build(spec["base"])), name=name, kind="search",
                                   weight=spec["weight"], base=spec["base"]))
        _BUILT[name] = c
        return c
    c = SimpleNamespace(**spec)
    rng = np.random.default_rng(1000 + NAMES.index(name))
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
        if c.ops == "real":
            c.operators = np.stack([c.ops_scale * rng.standard_normal((n, n)) / np.sqrt(n)
                                    for _ in range(L)]).astype(np.complex128)
        else:
            c.operators = np.stack([c.ops_scale * (gue(rng, n) + 0.5j * gue(rng, n))
                                    for _ in range(L)])
        c.gammas = rng.uniform(0.05, 0.3, L) if c.gamma is None else np.full(L, c.gamma)
    c.rho0 = np.stack([cases_mod.random_density(rng, n) for _ in range(S)])
    targ = np.stack([cases_mod.random_density(rng, n) for _ in range(S)])
    c.cost_specs = [("TargetDensityInfidelity", dict(target_densities=targ, cost_multiplier=0.8))]
    if c.forbid:
        forb = np.stack([cases_mod.random_density(rng, n) for _ in range(2 * S)]).reshape(S, 2, n, n)
        c.cost_specs.append(("ForbidDensities", dict(
            forbidden_densities=forb, system_eval_count=N, cost_eval_step=c.ces,
            cost_multiplier=0.5)))
    c.controls = c.amp * rng.standard_normal((c.seeds, c.Nc, K))
    if c.amplitudes is not None:
        c.controls *= (np.asarray(c.amplitudes)
                       / np.max(np.abs(c.controls), axis=(1, 2)))[:, None, None]
    if c.mirror:  # both seeds reach the same maxima: one sub-division group
        c.controls[1] = -c.controls[0]
    if c.kind == "linear":
        c.directions = rng.standard_normal((c.seeds, 3, c.Nc, K))
        c.h0_of_t = None
        if c.h0_frequency is not None:
            h0, w = c.h0, c.h0_frequency
            c.h0_of_t = lambda t: h0 * (1 + 0.3 * np.cos(w * t))
    if c.kind in ("ensemble", "sweep", "duration"):
        rows = MEMBERS if c.kind == "ensemble" else c.seeds
        c.perturbations = [0.5 * gue(rng, n)]
        c.scales = 1 + 0.05 * rng.standard_normal((rows, K))
        c.offsets = 0.3 * rng.standard_normal((rows, 1))
        c.rate_scales = np.array([[0.5, 1.0, 2.0][(b + l) % 3] for b in range(rows)
                                  for l in range(L)]).reshape(rows, L)
        c.weights = rng.uniform(0.2, 1.0, rows)
        c.channels = c.g + c.perturbations
        c.problem_h0 = c.h0
    if c.kind == "duration":
        # tau_b times the whole Lindbladian: the drift is the first fixed channel, the problem's own
        # h0 is zero, and the tables carry tau_b
        c.taus = TAUS[:c.seeds].copy()
        c.s0, c.c0 = c.scales, c.rate_scales
        c.d0 = np.concatenate([np.ones((rows, 1)), c.offsets], axis=1)
        c.channels = c.g + [c.h0] + c.perturbations
        c.problem_h0 = np.zeros((n, n), dtype=np.complex128)
        c.scales = c.taus[:, None] * c.s0
        c.offsets = c.taus[:, None] * c.d0
        c.rate_scales = c.taus[:, None] * c.c0
    _BUILT[name] = c
    return c


def oracle_costs(case):
    return [getattr(ol, kind)(**kw) for kind, kw in case.cost_specs]


def results(case, member, linear=None):
    """Every quantity of `case` as arrays, from member(h0, g, operators, gammas, u, scales, offsets,
    rate_scales, T, N, rho0, costs, cost_eval_step) -> the namespace of lindblad_exact.sweep_member
    (linear cases: from linear(case, b) -> (error, final, derivative (3,)))."""
    costs = oracle_costs(case)
    B = case.controls.shape[0]
    if case.kind == "linear":
        rows = [linear(case, b) for b in range(B)]
        return dict(cost=np.array([r[0] for r in rows]), final=np.stack([r[1] for r in rows]),
                    derivative=np.stack([r[2] for r in rows]))
    if case.kind == "plain":
        rows = [member(case.h0, case.g, case.operators, case.gammas, case.controls[b], None, None,
                       None, case.T, case.N, case.rho0, costs, case.ces) for b in range(B)]
        return dict(cost=np.array([r.error for r in rows]), final=np.stack([r.final for r in rows]),
                    grad=np.stack([r.seed_grad for r in rows]))

    def run(b, row):
        return member(case.problem_h0, case.channels, case.operators, case.gammas, case.controls[b],
                      case.scales[row], case.offsets[row], case.rate_scales[row], case.T, case.N,
                      case.rho0, costs, case.ces)
    if case.kind == "ensemble":
        rows = [[run(b, m) for m in range(MEMBERS)] for b in range(B)]
        w = case.weights
        return dict(
            member_cost=np.array([[r.error for r in row] for row in rows]),
            final=np.stack([np.stack([r.final for r in row]) for row in rows]),
            cost=np.array([sum(w[m] * row[m].error for m in range(MEMBERS)) for row in rows]),
            grad=np.stack([sum(w[m] * row[m].seed_grad for m in range(MEMBERS)) for row in rows]))
    rows = [run(b, b) for b in range(B)]
    out = dict(cost=np.array([r.error for r in rows]), final=np.stack([r.final for r in rows]),
               grad=np.stack([r.seed_grad for r in rows]),
               scale_sens=np.stack([r.scale_sens for r in rows]),
               offset_sens=np.stack([r.offset_sens for r in rows]),
               rate_sens=np.stack([r.rate_sens for r in rows]))
    if case.kind in ("duration", "search"):
        out["tau_grad"] = np.array([r.tau_sens for r in rows]) / case.taus
    return out


def exact_results(name):
    """The exact reference of a case (computed once; a search shares its duration sweep's)."""
    case = build(name)
    key = case.base if case.kind == "search" else name
    if key not in _EXACT:
        def linear(c, b):
            r = ex.linear(c.h0, c.g, c.operators, c.gammas, c.controls[b], c.T, c.N, c.rho0,
                          oracle_costs(c), c.ces, directions=c.directions[b], h0_of_t=c.h0_of_t)
            linear.disagreement = {k: max(v, linear.disagreement.get(k, 0.0))
                                   for k, v in r.disagreement.items()}
            return r.error, r.final, r.derivative
        linear.disagreement = {}
        _EXACT[key] = results(build(key), ex.sweep_member, linear)
        if linear.disagreement:
            _EXACT[key]["disagreement"] = linear.disagreement
    return _EXACT[key]


def model_results(name):
    """The NumPy model of the device scheme (tests/lindblad_model.py, tests/lindblad_sweep_model.py)
    on the same case, quantity by quantity."""
    from tests import lindblad_model as lm
    from tests import lindblad_sweep_model as sm
    case = build(name)
    if case.kind == "search":
        case = build(case.base)
    tables = case.kind in ("sweep", "duration")

    def member(h0, g, operators, gammas, u, scales, offsets, rate_scales, T, N, rho0, costs, ces):
        u = np.asarray(u, dtype=np.float64)
        kr = u.shape[1]
        J = 0 if offsets is None else len(offsets)
        L = 0 if operators is None else len(operators)
        s = np.ones(kr) if scales is None else np.asarray(scales)
        c = np.ones(L) if rate_scales is None else np.asarray(rate_scales)
        items = np.empty((u.shape[0], kr + J))
        items[:, :kr] = s[None, :] * u
        if J:
            items[:, kr:] = np.asarray(offsets)[None, :]
        base = lm.StructuredLindblad(h0, g, gammas, operators)
        system = sm.scaled_system(base, c) if L else base
        error, grad, final = lm.evaluate_with_grad(system, items, rho0, T, N, costs, ces,
                                                   piecewise_constant=True)
        out = SimpleNamespace(error=error, final=final, seed_grad=s[None, :] * grad[:, :kr],
                              scale_sens=np.sum(u * grad[:, :kr], axis=0),
                              offset_sens=np.sum(grad[:, kr:], axis=0), rate_sens=np.zeros(L),
                              tau_sens=0.0)
        if tables and L:
            out.rate_sens = sm.rate_sensitivities(base, items, rho0, T, N, costs, ces, factors=c,
                                                  piecewise_constant=True)[1]
        # (h0 = 0 in a duration sweep: the factor on the whole Lindbladian is one on every table)
        out.tau_sens = float(np.sum(items * grad) + np.sum(c * out.rate_sens))
        return out

    def linear(c, b):
        system = lm.StructuredLindblad(c.h0, c.g, c.gammas, c.operators, h0_of_t=c.h0_of_t)
        error, grad, final = lm.evaluate_with_grad(
            system, c.controls[b], c.rho0, c.T, c.N, oracle_costs(c), c.ces,
            subdivision=c.subdivision or None)
        return error, final, np.array([np.sum(grad * d) for d in c.directions[b]])
    return results(case, member, linear)


def compare(got, want):
    """{quantity: error} of two result dicts as the gates measure it: costs and densities absolute,
    gradients relative to the largest entry of each seed's, every other table relative to its
    largest entry."""
    out = {}
    for key in ("cost", "member_cost"):
        if key in want:
            out[key] = float(np.max(np.abs(got[key] - want[key])))
    out["densities"] = float(np.max(np.abs(got["final"] - want["final"])))
    if "grad" in want:
        B = want["grad"].shape[0]
        out["gradient"] = float(max(
            np.max(np.abs(got["grad"][b] - want["grad"][b])) / np.max(np.abs(want["grad"][b]))
            for b in range(B)))
    for key in ("scale_sens", "offset_sens", "rate_sens", "tau_grad", "derivative"):
        if key in want and want[key].size:
            out[key] = float(np.max(np.abs(got[key] - want[key])) / np.max(np.abs(want[key])))
    return out
