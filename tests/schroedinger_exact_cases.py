"""
schroedinger_exact_cases.py - TEST INFRASTRUCTURE: the case table shared by
tests/test_schroedinger_exact_host.py (the models against exact, on the CPU),
tools/measure_schroedinger_exact.py (the numbers the gates of tests/schroedinger_exact.py quote) and
tests/test_gpu_schroedinger_exact.py (the engine against exact).

A case is a system of one operator kind scaled to a stated LEVEL, random unit states and targets, one
final coherent TargetStateInfidelity unless it names a step cost, and `seeds` pulses.

  kinds of operators   "gue": cases.gue (||a||_1 is 2 to 3 times ||a||_2: the operators least able to
                       show a wrong Pade order); "ladder": a random real diagonal and nearest-neighbour
                       coupling 0.02 sqrt(k), real, so that ||.||_1 ~ ||.||_2 and the device's
                       |re| + |im| column bound equals the 1-norm, as in a transmon.
  level                the largest step bound of the batch as the host's step table computes it,
                       dt (||H0||_1 + sum_k |r_k| ||G_k||_1) (tests/mixed_pulses.py: step_table), set
                       through dt. Pade cases: 0.97 theta_m, m = 3, 5, 7, 9, 13, then 1.9 theta_13,
                       0.97 x 4 theta_13 and 20 (0, 1 and 2 squarings; 4 theta_13 itself is the threshold
                       between 2 and 3 squarings, and no step of the table may lie on a threshold).
                       The control amplitudes are 0.08 of the drift, so that the bound and the step
                       generator's own norm nearly coincide. Matrix-free cases (norm "two"): the largest
                       SPECTRAL step bound dt (rho(H0) + sum |r_k| rho(G_k)) at 0.97 theta'_m of
                       qoc_amd/csrc/qocx_action.h (tests/action_degree_model.py: THETA_NORMAL).
                       A case with `data` takes the numbers of another case (the same problem on
                       another route).
  family               which gates apply (tests/schroedinger_exact.py: GATES): "lu", "inverse",
                       "matrix_free".
  kind                 plain, ensemble (set_ensemble), sweep (set_sweep), duration (a sweep whose tables
                       carry tau_b: h0 is the first fixed channel), search (sweep_set_durations on a
                       duration case).

results(case, member) runs every seed (member, sweep seed) through `member(case, h0, g, items)`:
exact_results uses tests/schroedinger_exact.py, model_results the NumPy model of the case's route.
compare(got, want) gives the error of every quantity as the gates measure it.

Nothing here is imported by the product.
"""

import zlib
from types import SimpleNamespace

import numpy as np

from oracle import qoc_numpy as onp
from tests import action_degree_model as adm
from tests import action_model as am
from tests import cases as cases_mod
from tests import device_model as dm
from tests import mixed_pulses as mp
from tests import schroedinger_exact as ex

TH = dm.PADE_THETA
THN = adm.THETA_NORMAL
ORDERS = mp.ORDERS
NEAR = 0.97
NODES = {"M2": 1, "M4": 2, "M6": 3}
# the knobs a case may set, with the values they are restored to
KNOB_DEFAULTS = dict(action=1, action_states=0, action_costs=0, action_degree=1, pade_order=0, latency=0,
                     sweep_umode=1, sweep_impl=1, sweep_inverse_small=1, sweep_dense=1, sweep_one=1,
                     m4_linear=1, k1a_three=1, lu_dpp=1)


def _spec(name, family, n, level, **kw):
    return dict(dict(name=name, family=family, n=n, level=level, kind="plain", ops="ladder", S=1, K=2,
                     N=7, Nc=None, seeds=2, norm="one", hermitian=True, interpolation=ex.LINEAR,
                     magnus="M2", knobs={}, forbid=False, ces=1, complex_controls=False, timedep=False,
                     quadratic=False, model="pade", policy=0, rule=1, order=None, squarings=None,
                     degree=None, mixed=False, one_by_one=False, data=None, base=None, weight=0.0,
                     amp=0.08), **kw)


def _pade_levels(prefix, family, n, ops="ladder", **kw):
    """The eight levels of a Pade family at one size: every order, then 2, 2 and 1 squarings."""
    rows = [_spec("%s_%s_order%d" % (prefix, ops, m), family, n, NEAR * TH[m], ops=ops, order=m,
                  squarings=0, **kw) for m in ORDERS]
    rows.append(_spec("%s_%s_4theta13" % (prefix, ops), family, n, NEAR * 4 * TH[13], ops=ops, order=13,
                      squarings=2, **kw))
    rows.append(_spec("%s_%s_level20" % (prefix, ops), family, n, 20.0, ops=ops, order=13, squarings=2,
                      **kw))
    rows.append(_spec("%s_%s_1p9theta13" % (prefix, ops), family, n, 1.9 * TH[13], ops=ops, order=13,
                      squarings=1, **kw))
    return rows


ACTION_OFF = dict(action=0)
SPECS = (
    # ---- LU-based Pade routes: 17 <= n <= 32 with the matrix-free route off, the three-wave K1a at
    # orders 3 and 5, the two-wave K1a above, lu5 where the pivots are provable (the low levels), lu4
    # where they are not (4 theta_13 and 20)
    _pade_levels("k1a_n20", "lu", 20, knobs=ACTION_OFF)
    + _pade_levels("k1a_n20", "lu", 20, ops="gue", knobs=ACTION_OFF)
    + [
        _spec("k1a_n17_order13_policy", "lu", 17, NEAR * TH[5], knobs=dict(pade_order=13), policy=13,
              order=13, squarings=0),
        # the problems of the default matrix-free route on the Pade route: knob action 0, knob pade_order 13
        _spec("k1a_n20_action_off", "lu", 20, NEAR * THN[11], norm="two", knobs=ACTION_OFF,
              data="action_n20_degree11", order=7, squarings=0),
        _spec("k1a_n20_pade_order13", "lu", 20, NEAR * THN[11], norm="two", knobs=dict(pade_order=13),
              policy=13, data="action_n20_degree11", order=13, squarings=0),
        _spec("k1a_n32_action_off", "lu", 32, NEAR * THN[16], norm="two", knobs=ACTION_OFF,
              data="action_n32_degree16", order=7, squarings=0, N=6),
        _spec("k1a_n32_order7_two_wave_only", "lu", 32, NEAR * TH[7], knobs=dict(action=0, k1a_three=0),
              order=7, squarings=0, N=6),
        _spec("k1a_n24_mixed_batch", "lu", 24, NEAR * 4 * TH[13], knobs=ACTION_OFF, mixed=True, order=13,
              squarings=2),
        _spec("chain2_n24_s3", "lu", 24, NEAR * TH[9], S=3, order=9, squarings=0),
        _spec("sweep3_n24_s3", "lu", 24, NEAR * TH[7], S=3, knobs=dict(sweep_impl=3), order=7,
              squarings=0),
        _spec("nonhermitian_n24", "lu", 24, NEAR * TH[9], hermitian=False, order=9, squarings=0),
        _spec("forbid_n20_ces2", "lu", 20, NEAR * TH[7], forbid=True, ces=2, order=7, squarings=0),
        # four-wave K1a / qocx_big.hip
        _spec("big_n33", "lu", 33, NEAR * TH[13], order=13, squarings=0, N=6),
        _spec("big_n48_order7", "lu", 48, NEAR * TH[7], order=7, squarings=0, N=6),
        _spec("big_n64_level20", "lu", 64, 20.0, order=13, squarings=2, N=6),
        _spec("big_n40_nonhermitian", "lu", 40, NEAR * TH[9], hermitian=False, order=9, squarings=0,
              N=6),
        _spec("big_n48_gue_order5", "lu", 48, NEAR * TH[5], ops="gue", order=5, squarings=0, N=6),
        # aligned PIECEWISE_CONSTANT under M4 / M6, two LINEAR M4 / M6 cases
        _spec("pwc_m4_n20", "lu", 20, NEAR * TH[7], magnus="M4", interpolation=ex.PWC, N=7, Nc=3),
        _spec("pwc_m6_n40", "lu", 40, NEAR * TH[5], magnus="M6", interpolation=ex.PWC, N=7, Nc=6),
        _spec("linear_m4_n20", "lu", 20, NEAR * TH[7], magnus="M4", Nc=4),
        _spec("linear_m6_n20", "lu", 20, NEAR * TH[5], magnus="M6", Nc=5),
        # seed tables
        _spec("ensemble_n20", "lu", 20, NEAR * TH[9], kind="ensemble", knobs=ACTION_OFF),
        _spec("sweep_n20", "lu", 20, NEAR * TH[9], kind="sweep", seeds=3, knobs=ACTION_OFF),
        _spec("duration_n20", "lu", 20, NEAR * TH[7], kind="duration", seeds=3, knobs=ACTION_OFF),
        _spec("search_n20_free", "lu", 20, NEAR * TH[7], kind="search", seeds=3, knobs=ACTION_OFF,
              base="duration_n20", weight=0.0),
        _spec("search_n20_priced", "lu", 20, NEAR * TH[7], kind="search", seeds=3, knobs=ACTION_OFF,
              base="duration_n20", weight=0.3),
    ]
    # ---- inverse-image routes: n <= 16 (sweepi, pack8 at n <= 8, inv16_dpp where every matrix of the
    # launch is dominant - the low levels - and inv_kernel where not), latency mode, the general path
    + _pade_levels("sweepi_n8", "inverse", 8, model="inverse")
    + _pade_levels("sweepi_n16_s5", "inverse", 16, ops="gue", S=5, model="inverse")
    + [
        _spec("tile_n3", "inverse", 3, NEAR * TH[9], model="inverse", order=9, squarings=0, N=6),
        _spec("sweepi_n16_s1", "inverse", 16, NEAR * TH[13], model="inverse", order=13, squarings=0),
        _spec("sweepi_n16_s8", "inverse", 16, NEAR * TH[7], S=8, model="inverse", order=7, squarings=0),
        _spec("sweepi_n8_mixed_batch", "inverse", 8, NEAR * 4 * TH[13], model="inverse", mixed=True, order=13,
              squarings=2),
        _spec("sweep3_n12", "lu", 12, NEAR * TH[9], knobs=dict(sweep_impl=3, sweep_inverse_small=0),
              order=9, squarings=0),
        _spec("nonhermitian_n6", "inverse", 6, NEAR * TH[13], hermitian=False, model="inverse",
              order=13, squarings=0, N=6),
        _spec("complex_controls_n8", "inverse", 8, NEAR * TH[7], complex_controls=True, model="inverse",
              order=7, squarings=0),
        _spec("timedep_n8", "inverse", 8, NEAR * TH[9], timedep=True, model="inverse", N=6),
        _spec("quadratic_n12", "inverse", 12, NEAR * TH[7], quadratic=True, model="inverse"),
        _spec("latency_n8_umode1", "inverse", 8, NEAR * TH[9], knobs=dict(latency=1, sweep_umode=1),
              model="inverse", one_by_one=True, order=9, squarings=0),
        _spec("latency_n8_umode0", "inverse", 8, NEAR * TH[9], knobs=dict(latency=1, sweep_umode=0),
              model="inverse", one_by_one=True, order=9, squarings=0),
        _spec("latency_n24_umode1", "inverse", 24, 1.9 * TH[13], knobs=dict(latency=1, sweep_umode=1),
              model="inverse", one_by_one=True, order=13, squarings=1),
        _spec("latency_n24_umode0", "inverse", 24, NEAR * TH[5], knobs=dict(latency=1, sweep_umode=0),
              model="inverse", one_by_one=True, order=5, squarings=0),
        _spec("sweepd_n24_s8", "inverse", 24, NEAR * TH[9], S=8, model="inverse", order=9, squarings=0),
        _spec("general_n66", "inverse", 66, NEAR * TH[9], model="inverse", N=6),
        _spec("general_n72_level20", "inverse", 72, 20.0, model="inverse", N=6),
        _spec("general_n40_s14", "inverse", 40, NEAR * TH[7], S=14, model="inverse", N=6),
        _spec("general_n70_pwc_m4", "inverse", 70, NEAR * TH[5], model="inverse", magnus="M4",
              interpolation=ex.PWC, N=7, Nc=2),
        _spec("pwc_m6_n6", "inverse", 6, NEAR * TH[9], model="inverse", magnus="M6",
              interpolation=ex.PWC, N=7, Nc=3),
        _spec("linear_m4_n6", "inverse", 6, NEAR * TH[7], model="inverse", magnus="M4", Nc=4),
        _spec("linear_m6_n6", "inverse", 6, NEAR * TH[5], model="inverse", magnus="M6", Nc=5),
        _spec("sweep_n8", "inverse", 8, NEAR * TH[9], kind="sweep", seeds=3, model="inverse"),
        _spec("duration_n8", "inverse", 8, NEAR * TH[7], kind="duration", seeds=3, model="inverse"),
        _spec("search_n8_free", "inverse", 8, NEAR * TH[7], kind="search", seeds=3, model="inverse",
              base="duration_n8", weight=0.0),
        _spec("search_n8_priced", "inverse", 8, NEAR * TH[7], kind="search", seeds=3, model="inverse",
              base="duration_n8", weight=0.3),
    ]
    # ---- matrix-free routes: levels by the spectral-norm thresholds theta'_m, a low, a middle and the
    # highest degree the operators allow under the host's 1-norm bound <= theta_18
    + [
        _spec("action_n17_degree6", "matrix_free", 17, NEAR * THN[6], norm="two", model="action",
              degree=6),
        _spec("action_n20_degree11", "matrix_free", 20, NEAR * THN[11], norm="two", model="action",
              degree=11),
        _spec("action_n32_degree16", "matrix_free", 32, NEAR * THN[16], norm="two", model="action",
              degree=16, N=6),
        _spec("action_n20_gue_degree9", "matrix_free", 20, NEAR * THN[9], norm="two", ops="gue",
              model="action", degree=9),
        _spec("action_n20_one_norm_rule", "matrix_free", 20, NEAR * am.THETA[13], model="action",
              knobs=dict(action_degree=0), rule=0, degree=13),
        _spec("action_n17_mixed_batch", "matrix_free", 17, NEAR * THN[15], norm="two", model="action",
              mixed=True, degree=15),
        _spec("action_states_n17_s2", "matrix_free", 17, NEAR * THN[11], norm="two", S=2, model="action",
              knobs=dict(action_states=4), degree=11),
        _spec("action_states_n32_s4", "matrix_free", 32, NEAR * THN[14], norm="two", S=4, model="action",
              knobs=dict(action_states=4), degree=14, N=6),
        _spec("action_costs_n20_forbid", "matrix_free", 20, NEAR * THN[11], norm="two", model="action",
              knobs=dict(action_costs=1), forbid=True, ces=2, degree=11),
        _spec("action_wide_n33", "matrix_free", 33, NEAR * THN[8], norm="two", model="action",
              knobs=dict(action=2), degree=8, N=6),
        _spec("action_wide_n48", "matrix_free", 48, NEAR * THN[12], norm="two", model="action",
              knobs=dict(action=2), degree=12, N=6),
        _spec("action_wide_n64", "matrix_free", 64, NEAR * THN[16], norm="two", model="action",
              knobs=dict(action=2), degree=16, N=6),
        _spec("action_ensemble_n20", "matrix_free", 20, NEAR * THN[11], norm="two", kind="ensemble",
              model="action", degree=11),
    ]
)
NAMES = [s["name"] for s in SPECS]
# the self-check of the reference against mpmath at 40 digits: the smallest case of each kind, n <= 8
# and five steps. Not run on the device.
MP_SPECS = [
    _spec("mp_ladder_n8", "inverse", 8, NEAR * TH[13], N=6, S=2),
    _spec("mp_gue_n8_level20", "inverse", 8, 20.0, ops="gue", N=6),
    _spec("mp_nonhermitian_n6", "inverse", 6, NEAR * TH[13], hermitian=False, N=6),
    _spec("mp_forbid_n6_ces2", "inverse", 6, NEAR * TH[9], forbid=True, ces=2, N=6, S=2),
    _spec("mp_pwc_n6", "inverse", 6, NEAR * TH[9], interpolation=ex.PWC, N=6, Nc=4),
    _spec("mp_linear_m4_n6", "inverse", 6, NEAR * TH[7], magnus="M4", N=6, Nc=4),
    _spec("mp_linear_m6_n6", "inverse", 6, NEAR * TH[5], magnus="M6", N=6, Nc=5),
]
MPMATH_CASES = [s["name"] for s in MP_SPECS]
_ALL = NAMES + MPMATH_CASES
assert len(set(_ALL)) == len(_ALL)
TAUS = np.array([0.6, 1.0, 1.3])
TAU_BOX = (0.4, 1.6)
MEMBERS = 3
_BUILT, _EXACT = {}, {}


def ladder(rng, n):
    """A random real diagonal and nearest-neighbour coupling 0.02 sqrt(k)."""
    c = 0.02 * np.sqrt(np.arange(1.0, n))
    return (np.diag(rng.uniform(-1, 1, n)) + np.diag(c, 1) + np.diag(c, -1)).astype(np.complex128)


def unit_vectors(rng, shape):
    v = rng.standard_normal(shape) + 1j * rng.standard_normal(shape)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def spectral_bound(m):
    """rho of a Hermitian operator; the 2-norm otherwise."""
    return float(np.linalg.norm(m, 2))


def step_bounds(case, h0, g, items, dt=None):
    """(N - 1, 2): the step table's bounds of one item, |dt| (||H0|| + sum_k |r_k| ||G_k|| (+ sum_q
    |r_k r_l| ||Q_q||)) in the 1-norm and in the spectral norm, the largest over the nodes of a step
    (through mixed_pulses.magnus_norm_bound under M4 / M6, as the host does)."""
    dt = case.dt if dt is None else dt
    nodes = onp.MAGNUS_NODES[case.magnus]
    h0 = np.asarray(h0).reshape(-1, case.n, case.n)
    g = np.asarray(g).reshape(h0.shape[0] if np.asarray(g).ndim == 4 else 1, -1, case.n, case.n)
    r, _ = ex.step_controls(items, case.N, 1.0, case.interpolation, nodes)
    out = np.zeros((case.N - 1, 2))
    for which, norm in enumerate((onp.one_norm, spectral_bound)):
        hn = [norm(m) for m in h0]
        gn = [[norm(m) for m in row] for row in g]
        qn = [norm(m) for m in case.quadratic[1]] if case.quadratic else []
        for j in range(case.N - 1):
            for i in range(len(nodes)):
                row = j * len(nodes) + i
                b = hn[row if len(hn) > 1 else 0]
                b += float(np.sum(np.abs(r[j, i]) * np.array(gn[row if len(gn) > 1 else 0])))
                for q, (k, l) in enumerate(case.quadratic[0] if case.quadratic else ()):
                    b += abs(r[j, i, k] * r[j, i, l]) * qn[q]
                out[j, which] = max(out[j, which], abs(dt) * b)
    if len(nodes) > 1:
        out[:, 0] = [mp.magnus_norm_bound(len(nodes), b) for b in out[:, 0]]
    return out


def build(name):
    """The case `name` with its data (built once)."""
    if name in _BUILT:
        return _BUILT[name]
    spec = next(s for s in list(SPECS) + MP_SPECS if s["name"] == name)
    if spec["base"] is not None:  # a search runs on the data of its duration sweep
        c = SimpleNamespace(**dict(vars(build(spec["base"])), name=name, kind="search",
                                   weight=spec["weight"], base=spec["base"]))
        _BUILT[name] = c
        return c
    c = SimpleNamespace(**spec)
    rng = np.random.default_rng(zlib.crc32((c.data or name).encode()))  # (data: another case's numbers)
    n, S, K, N = c.n, c.S, c.K, c.N
    c.Nc = N if c.Nc is None else c.Nc
    draw = (lambda: ladder(rng, n)) if c.ops == "ladder" else (lambda: cases_mod.gue(rng, n))
    c.h0 = draw() * (0.01 if c.mixed else 1.0)
    c.g = [draw() for _ in range(K)]
    if not c.hermitian:  # an effective Hamiltonian with a loss term
        c.h0 = c.h0 - 0.05j * onp.one_norm(c.h0) * np.diag(np.arange(n) / n)
    c.quadratic = None
    if spec["quadratic"]:
        c.quadratic = (np.array([[0, 0], [0, 1]], dtype=np.int32), np.stack([0.5 * draw(), 0.3 * draw()]))
    if c.complex_controls:
        # H = H0 + sum_k u_k A_k + conj(u_k) A_k^H, the channels (Re u_k, Im u_k) on the slopes the
        # oracle's problem reports
        lowers = [draw() + 0.5 * np.triu(draw(), 1) for _ in range(K)]
        problem = onp.SchroedingerProblem(
            1.0, lambda u, t: c.h0 + sum(u[k] * lowers[k] + np.conj(u[k]) * lowers[k].conj().T
                                         for k in range(K)),
            np.zeros((1, n, 1)), N, control_eval_count=c.Nc, complex_controls=True, control_count=K)
        g_re, g_im = problem.hamiltonian_slopes(0.0)
        c.g = [m for pair in zip(g_re, g_im) for m in pair]
        K = c.K = 2 * K
    c.psi0 = unit_vectors(rng, (S, n))
    c.target = unit_vectors(rng, (S, n))
    c.cost_specs = [("TargetStateInfidelity", dict(target_states=c.target[:, :, None],
                                                   cost_multiplier=0.8))]
    if c.forbid:
        c.cost_specs.append(("ForbidStates", dict(
            forbidden_states=unit_vectors(rng, (S, 2, n))[:, :, :, None], system_eval_count=N,
            cost_eval_step=c.ces, cost_multiplier=0.5)))
    c.controls = c.amp * rng.standard_normal((c.seeds, c.Nc, K))
    if c.mixed:  # a quiet seed and a loud seed in one upload
        c.controls[0] *= 0.01 / c.amp
        c.controls[1] *= 1.0 / c.amp
    c.channels, c.problem_h0 = list(c.g), c.h0
    rows = None
    if c.kind in ("ensemble", "sweep", "duration"):
        rows = MEMBERS if c.kind == "ensemble" else c.seeds
        c.perturbations = [0.5 * draw()]
        c.scales = 1 + 0.05 * rng.standard_normal((rows, K))
        c.offsets = 0.3 * rng.standard_normal((rows, 1))
        c.weights = rng.uniform(0.2, 1.0, rows)
        c.channels = c.g + c.perturbations
    if c.kind == "duration":
        # tau_b times the whole Hamiltonian: the drift is the first fixed channel, the problem's own
        # h0 is zero, and the tables carry tau_b
        c.taus = TAUS[:c.seeds].copy()
        c.s0 = c.scales
        c.d0 = np.concatenate([np.ones((rows, 1)), c.offsets], axis=1)
        c.channels = c.g + [c.h0] + c.perturbations
        c.problem_h0 = np.zeros((n, n), dtype=np.complex128)
        c.scales = c.taus[:, None] * c.s0
        c.offsets = c.taus[:, None] * c.d0
    # the tables the engine reads: (nt, n, n) and (nt, K', n, n)
    c.h0_table = c.problem_h0[None]
    c.g_table = np.stack(c.channels)[None]
    if c.timedep:  # H0(t), G_k(t) at the step midpoints: nt = N - 1 under M2
        t = (np.arange(N - 1) + 0.5) / (N - 1)
        c.h0_table = np.stack([c.h0 * (1 + 0.3 * np.cos(2.0 * x)) for x in t])
        c.g_table = np.stack([np.stack(c.g) * (1 + 0.2 * np.sin(3.0 * x)) for x in t])
    # the level: dt from the largest step bound of every item at dt = 1
    c.dt = 1.0
    which = 0 if c.norm == "one" else 1
    c.dt = c.level / max(np.max(step_bounds(c, c.h0_table, c.g_table, it)[:, which])
                         for it in items_of(c))
    if NODES[c.magnus] > 1:  # (the Magnus bound is not linear in dt: a few fixed-point steps)
        for _ in range(40):
            top = max(np.max(step_bounds(c, c.h0_table, c.g_table, it)[:, 0]) for it in items_of(c))
            c.dt *= (c.level / top) ** 0.5
    c.T = c.dt * (N - 1)
    _BUILT[name] = c
    return c


def items_of(case):
    """The channel values of every item the device evolves: (items, Nc, K') - the seeds themselves, or
    [scales * u, offsets] per (seed, member) or per sweep seed."""
    u = case.controls
    if case.kind == "plain":
        return u
    rows = range(MEMBERS) if case.kind == "ensemble" else None
    out = []
    for b in range(len(u)):
        for row in (rows if rows is not None else [b]):
            out.append(np.concatenate([case.scales[row][None, :] * u[b], np.broadcast_to(
                case.offsets[row][None, :], (u.shape[1], case.offsets.shape[1]))], axis=1))
    return np.stack(out)


def oracle_costs(case):
    return [getattr(onp, kind)(**kw) for kind, kw in case.cost_specs]


def oracle_problem(case, h0=None, g=None):
    """The oracle's problem of a case with constant operators (LINEAR interpolation)."""
    h0 = case.h0 if h0 is None else h0
    g = case.g if g is None else g
    return onp.SchroedingerProblem(
        case.T, lambda u, t: h0 + sum(u[k] * g[k] for k in range(len(g))), case.psi0[:, :, None],
        case.N, control_eval_count=case.Nc, costs=oracle_costs(case), cost_eval_step=case.ces,
        magnus_policy=case.magnus, control_count=len(g))


# ---- the members ---------------------------------------------------------------------------------------

def exact_member(case, h0, g, items, **kw):
    return ex.evaluate(h0, g, items, case.T, case.N, case.psi0, oracle_costs(case), case.ces,
                       case.interpolation, case.magnus, case.hermitian, case.quadratic, **kw)


def _costs_at(case, costs, hits, psi, step, want_bar):
    value, bar = 0.0, np.zeros_like(psi)
    for c in hits.get(step, []):
        value = value + c.cost(None, psi.T[:, :, None], step)
        if want_bar:
            bar = bar + c.states_bar(None, psi.T[:, :, None], step)[:, :, 0].T
    return value, bar


def step_model(case, h0, g, items, order_shift=0, degree_shift=0, drop_squaring=False,
               keep_scale=False, orders=None, degrees=None):
    """
    The NumPy model of the case's route on one item, step by step on the generators of
    schroedinger_exact.step_hamiltonians (through the oracle's magnus_combine and its reverse rule under
    M4 / M6):

      model "pade"     tests/device_model.py: pade_uv at the order of the step table's bound (policy 13:
                       always 13), 2^s from the bound, LU with partial pivoting, 2^s solves per step,
                       the Horner Krylov adjoint krylov_abar_horner;
      model "inverse"  the same with the explicit inverse P^-1 by the blocked Gauss-Jordan elimination of
                       tests/test_general_model.py, x = P^-1 (Q psi) and P^-H lam;
      model "action"   tests/action_model.py: forward_step / adjoint_step / generator_cotangent at the
                       degrees of tests/action_degree_model.py: degree_rule (rule 0: the 1-norm alone).

    The mutations of tests/test_schroedinger_exact_host.py: order_shift -1 (one Pade order lower),
    degree_shift -3, drop_squaring (2^(s-1) sub-steps on the generator scaled by 2^-s), keep_scale (abar
    without its factor 2^-s). orders / degrees: forced per step (what a device run reported).
    Returns the namespace of schroedinger_exact.evaluate plus `orders`, `squarings`, `degrees`.
    """
    from tests.lindblad_exact import _step_hits
    items = np.asarray(items, dtype=np.float64)
    Nc, K = items.shape
    N, dt, n = case.N, case.dt, case.n
    nodes = onp.MAGNUS_NODES[case.magnus]
    costs = oracle_costs(case)
    hits = _step_hits(costs, N, case.ces)
    _, weights, hams, slopes = ex.step_hamiltonians(h0, g, items, case.T, N, case.interpolation, nodes,
                                                    case.quadratic)
    bounds = step_bounds(case, h0, g, items)
    psi = case.psi0.T.astype(np.complex128)
    tape, steps = [], [psi]
    used_orders, used_s, used_degrees = [], [], []
    for j in range(N - 1):
        gens = [-1j * h for h in hams[j]]
        a, mcache = onp.magnus_combine(case.magnus, dt, gens)
        if case.model == "action":
            m = degrees[j] if degrees is not None else adm.degree_rule(bounds[j, 0], bounds[j, 1], case.rule)
            m = max(1, m + degree_shift)
            used_degrees.append(m)
            out = [am.forward_step(a, psi[:, s], m) for s in range(psi.shape[1])]
            new = np.stack([o[0] for o in out], axis=1)
            tape.append((gens, mcache, a, m, [o[1] for o in out], psi))
        else:
            order = orders[j] if orders is not None else dm.pade_order(bounds[j, 0], case.policy)
            s = mp.squarings(bounds[j, 0]) if order == 13 else 0
            if order_shift:
                order = ORDERS[max(ORDERS.index(order) + order_shift, 0)]
            a_s = a * 2.0 ** -s
            u, v = dm.pade_uv(a_s, order)
            p, q = v - u, v + u
            if case.model == "inverse":
                from tests.test_general_model import blocked_gauss_jordan_inverse
                # (the block size: the largest divisor of n up to 16 - the elimination is the same
                # sequence of single steps at any block size, tests/test_general_model.py)
                pinv = blocked_gauss_jordan_inverse(p, max(d for d in range(1, 17) if n % d == 0))[0]
                solve = lambda y, pinv=pinv: pinv @ y
                solve_h = lambda y, pinv=pinv: pinv.conj().T @ y
            else:
                lu, perm = dm.lu_partial_pivot(p)
                solve = lambda y, lu=lu, perm=perm: dm.solve_lu(lu, perm, y)
                solve_h = lambda y, lu=lu, perm=perm: dm.solve_lu_adjoint(lu, perm, y)
            count = 2 ** (s - 1 if drop_squaring and s > 0 else s)
            subs = [psi]
            for _ in range(count):
                subs.append(solve(q @ subs[-1]))
            new = subs[-1]
            used_orders.append(order)
            used_s.append(s)
            tape.append((gens, mcache, a_s, (order, s, q, solve_h), subs, psi))
        psi = new
        steps.append(psi)
    steps = np.stack([x.T for x in steps])
    error = 0.0
    for step in sorted(hits):
        error = error + _costs_at(case, costs, hits, steps[step].T, step, False)[0]
    grad = np.zeros((Nc, K))
    step_grad = np.zeros((N - 1, len(nodes), K))
    lam = _costs_at(case, costs, hits, steps[N - 1].T, N - 1, True)[1]
    for j in range(N - 2, -1, -1):
        gens, mcache, a_s, how, kept, psi = tape[j]
        if case.model == "action":
            abar = np.zeros((n, n), dtype=np.complex128)
            new = []
            for s in range(psi.shape[1]):
                ls, w = am.adjoint_step(a_s, lam[:, s], how)
                new.append(ls)
                abar = abar + am.generator_cotangent(kept[s], w, how)
            lam = np.stack(new, axis=1)
        else:
            order, s, q, solve_h = how
            triples = []
            for sub in range(len(kept) - 2, -1, -1):
                x = solve_h(lam)
                lam = q.conj().T @ x
                triples.append((x, kept[sub], kept[sub + 1]))
            abar = dm.krylov_abar_horner(a_s, triples, order) * (1.0 if keep_scale else 2.0 ** -s)
        for i, genbar in enumerate(onp.magnus_combine_vjp(case.magnus, dt, gens, mcache, abar)):
            for k in range(K):
                step_grad[j, i, k] = np.real(np.sum(np.conj(genbar) * (-1j * slopes[j][i][k])))
            for knot, w in weights[j][i]:
                grad[knot] += w * step_grad[j, i]
        if j > 0:
            lam = lam + _costs_at(case, costs, hits, steps[j].T, j, True)[1]
    return SimpleNamespace(error=float(np.real(error)), final=steps[-1], steps=steps, grad=grad,
                           step_grad=step_grad, orders=used_orders, squarings=used_s,
                           degrees=used_degrees)


# ---- every quantity of a case ------------------------------------------------------------------------------

def results(case, member):
    """Every quantity of `case` as arrays, from member(case, h0, g, items) -> the namespace of
    schroedinger_exact.evaluate. The seed tables by the chain rule on the per-step cotangents:
    r_jk = s_k u_jk (interpolated) and r_j,K+i = delta_i at every node."""
    u = case.controls
    B, kr = u.shape[0], u.shape[2]
    items = items_of(case)
    runs = [member(case, case.h0_table, case.g_table, it) for it in items]
    nodes = onp.MAGNUS_NODES[case.magnus]
    if case.kind == "plain":
        return dict(cost=np.array([r.error for r in runs]), states=np.stack([r.final for r in runs]),
                    grad=np.stack([r.grad for r in runs]))

    def seed_values(b):  # the seed's own controls at the nodes of every step
        return ex.step_controls(u[b], case.N, case.T, case.interpolation, nodes)[0]

    if case.kind == "ensemble":
        w, M = case.weights, MEMBERS
        rows = [runs[b * M:(b + 1) * M] for b in range(B)]
        return dict(
            member_cost=np.array([[r.error for r in row] for row in rows]),
            states=np.stack([np.stack([r.final for r in row]) for row in rows]),
            cost=np.array([sum(w[m] * row[m].error for m in range(M)) for row in rows]),
            grad=np.stack([sum(w[m] * case.scales[m][None, :] * row[m].grad[:, :kr] for m in range(M))
                           for row in rows]))
    out = dict(cost=np.array([r.error for r in runs]), states=np.stack([r.final for r in runs]),
               grad=np.stack([case.scales[b][None, :] * runs[b].grad[:, :kr] for b in range(B)]),
               scale_sens=np.stack([np.sum(seed_values(b) * runs[b].step_grad[:, :, :kr], axis=(0, 1))
                                    for b in range(B)]),
               offset_sens=np.stack([np.sum(runs[b].step_grad[:, :, kr:], axis=(0, 1))
                                     for b in range(B)]))
    if case.kind in ("duration", "search"):
        out["tau_grad"] = chain_rule(case, out)
    return out


def chain_rule(case, out):
    """dE_b/dtau_b through the tables scales = tau s0, offsets = tau delta0."""
    return (np.sum(case.s0 * out["scale_sens"], axis=1) + np.sum(case.d0 * out["offset_sens"], axis=1))


def exact_results(name):
    """The exact reference of a case (computed once; a search shares its duration sweep's)."""
    case = build(name)
    key = case.base if case.kind == "search" else name
    if key not in _EXACT:
        _EXACT[key] = results(build(key), exact_member)
    return _EXACT[key]


def model_results(name, **mutation):
    case = build(name)
    if case.kind == "search":
        case = build(case.base)
    return results(case, lambda c, h0, g, it: step_model(c, h0, g, it, **mutation))


_MPMATH = {}


def mpmath_disagreement(name):
    """{cost, states, derivative}: the reference against mpmath at 40 digits on seed 0 of a case of
    MPMATH_CASES, the derivative of the error along one random direction relative to itself (absent
    under M6: schroedinger_exact.mpmath_check). Computed once."""
    if name not in _MPMATH:
        case = build(name)
        u = case.controls[0]
        direction = np.random.default_rng(zlib.crc32(name.encode()) + 1).standard_normal(u.shape)
        mine = exact_member(case, case.h0, case.g, u)
        error, final, derivative = ex.mpmath_check(
            case.h0, case.g, u, direction, case.T, case.N, case.psi0, oracle_costs(case), case.ces,
            case.interpolation, case.magnus)
        out = dict(cost=abs(error - mine.error), states=float(np.max(np.abs(final - mine.final))))
        if derivative is not None:
            out["derivative"] = abs(derivative - np.sum(mine.grad * direction)) / abs(derivative)
        _MPMATH[name] = out
    return _MPMATH[name]


def compare(got, want):
    """{quantity: error} of two result dicts as the gates measure it: costs and states absolute,
    gradients relative to the largest entry of each seed's, every other table relative to its largest
    entry."""
    out = {}
    for key in ("cost", "member_cost"):
        if key in want:
            out[key] = float(np.max(np.abs(got[key] - want[key])))
    out["states"] = float(np.max(np.abs(got["states"] - want["states"])))
    B = want["grad"].shape[0]
    out["gradient"] = float(max(
        np.max(np.abs(got["grad"][b] - want["grad"][b])) / np.max(np.abs(want["grad"][b]))
        for b in range(B)))
    for key in ("scale_sens", "offset_sens", "tau_grad"):
        if key in want and want[key].size:
            out[key] = float(np.max(np.abs(got[key] - want[key])) / np.max(np.abs(want[key])))
    return out


# ---- what the table claims, by the host's bound -----------------------------------------------------------------

def decisions(case):
    """Per item and step: dict(order_table, order_upper, order_exact, squarings, degree, bound
    (items, N - 1, 2), exact, sqfree (items, N - 1)) - the Pade order and squaring count the step table's
    bound selects, the order the step generator's own 1-norm selects (never a lower one may run), the
    order of the larger of the table's bound and the square-root-free norm max_j sum_i |re| + |im| a
    kernel without a table forms (never a higher one may run), `dominant`: the pivots of the step's Pade
    denominator are provable by that larger bound (no pivot search, no fallback), the degree of the rule."""
    items = items_of(case)
    bounds = np.stack([step_bounds(case, case.h0_table, case.g_table, it) for it in items])
    nodes = onp.MAGNUS_NODES[case.magnus]
    exact = np.empty(bounds.shape[:2])
    sqfree = np.empty(bounds.shape[:2])
    for b, it in enumerate(items):
        hams = ex.step_hamiltonians(case.h0_table, case.g_table, it, case.T, case.N,
                                    case.interpolation, nodes, case.quadratic)[2]
        for j in range(case.N - 1):
            a = onp.magnus_combine(case.magnus, case.dt, [-1j * h for h in hams[j]])[0]
            exact[b, j] = onp.one_norm(a)
            sqfree[b, j] = np.max(np.sum(np.abs(a.real) + np.abs(a.imag), axis=0))
    order = lambda v: dm.pade_order(v, case.policy)
    # qocx_lu5.h: the diagonal pivots of the Pade denominator are provable where eps_m(theta) <= 0.40
    dominant = np.array([[mp.decide([v])[2][0] for v in row] for row in np.maximum(bounds[:, :, 0], sqfree)])
    return dict(
        bound=bounds, exact=exact, sqfree=sqfree, dominant=dominant,
        order_table=np.vectorize(order)(bounds[:, :, 0]),
        order_upper=np.vectorize(order)(np.maximum(bounds[:, :, 0], sqfree)),
        order_exact=np.vectorize(order)(exact),
        squarings=np.array([[mp.squarings(v) if order(v) == 13 else 0 for v in row]
                            for row in bounds[:, :, 0]]),
        degree=np.array([[adm.degree_rule(b1, b2, case.rule) for b1, b2 in row] for row in bounds]))
