"""
CPU tests of the exact Lindblad references (tests/lindblad_exact.py), the truth of
tests/test_gpu_lindblad_exact.py:

1. the references against closed forms (T1 decay, pure dephasing, L = 0 against the Schroedinger
   oracle's expm on rho = psi psi^H, trace preservation), piecewise_constant(...) and linear(...) both;
2. the exact gradient and sensitivities against Richardson-extrapolated differences of the reference's
   own cost;
3. the NumPy model of the device scheme against the references on every case of the GPU table: the
   scheme's discretisation error, which the gates of tests/lindblad_exact.py are ten times of (or the
   device-versus-model gate, where that is larger), and which must stay below the documented parity
   tolerance (densities 1e-8, cost 1e-9);
4. proof that the references see what a kernel could get wrong: eight deliberately wrong Liouvillians
   or problems, each of which moves the exact error, final densities or gradient by at least 1e-6.
"""

import json
import os

import numpy as np
import pytest

from oracle import qoc_lindblad_numpy as ol
from oracle import qoc_numpy as onp
from tests import cases as cases_mod
from tests import lindblad_exact as ex
from tests import lindblad_exact_cases as xc
from tests import piecewise_constant as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SX = np.array([[0, 1], [1, 0]], dtype=np.complex128)
SZ = np.diag([1.0, -1.0]).astype(np.complex128)
LOWER = np.array([[0, 1], [0, 0]], dtype=np.complex128)  # |0><1|


def two_level(h0, op, gamma, rho, T, N=4):
    """The same control-free evolution through both references."""
    a = ex.piecewise_constant(h0, [SX], [op], [gamma], np.zeros((3, 1)), T, N, rho[None], [])
    b = ex.linear(h0, [SX], [op], [gamma], np.zeros((3, 1)), T, N, rho[None], [])
    assert max(b.disagreement.values()) < 1e-12
    return a.steps[:, 0], b.steps[:, 0]


# ---- 1. closed forms -------------------------------------------------------------------------------

def test_t1_decay_populations_and_coherences():
    gamma, a0, b0, T, N = 2.0, 0.3, 0.4 - 0.1j, 1.0, 4
    rho = np.array([[a0, b0], [np.conj(b0), 1 - a0]])
    for steps in two_level(np.zeros((2, 2)), LOWER, gamma, rho, T, N):
        for i, t in enumerate(np.linspace(0, T, N)):
            c = (1 - a0) * np.exp(-gamma * t)
            want = np.array([[1 - c, b0 * np.exp(-gamma * t / 2)],
                             [np.conj(b0) * np.exp(-gamma * t / 2), c]])
            assert np.max(np.abs(steps[i] - want)) < 1e-13


def test_pure_dephasing_under_a_detuning():
    gamma, omega, a0, b0, T, N = 0.7, 1.3, 0.35, 0.2 + 0.3j, 1.5, 4
    rho = np.array([[a0, b0], [np.conj(b0), 1 - a0]])
    for steps in two_level(0.5 * omega * SZ, SZ, gamma, rho, T, N):
        for i, t in enumerate(np.linspace(0, T, N)):
            # D[sigma_z] takes 2 gamma off the coherences, H = omega sigma_z / 2 turns them
            b = b0 * np.exp(-1j * omega * t - 2 * gamma * t)
            want = np.array([[a0, b], [np.conj(b), 1 - a0]])
            assert np.max(np.abs(steps[i] - want)) < 1e-13


def test_without_operators_it_is_the_schroedinger_propagator():
    rng = np.random.default_rng(11)
    n, K, N, Nc, T = 5, 2, 4, 3, 1.2
    h0 = cases_mod.gue(rng, n)
    g = [cases_mod.gue(rng, n) for _ in range(K)]
    u = rng.standard_normal((Nc, K))
    psi = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    psi /= np.linalg.norm(psi)
    out = ex.piecewise_constant(h0, g, None, None, u, T, N, np.outer(psi, psi.conj())[None], [])
    for j in range(Nc):  # Nc = N - 1: one slice per step
        psi = onp.expm_pade(-1j * (T / Nc) * (h0 + u[j, 0] * g[0] + u[j, 1] * g[1])) @ psi
        assert np.max(np.abs(out.steps[j + 1, 0] - np.outer(psi, psi.conj()))) < 1e-13


def test_the_trace_is_preserved_and_the_densities_stay_hermitian():
    for name in ("n7_l2", "n5_nc4_on_6_steps", "n6_nonhermitian_h0", "linear_n4_l2_nc5"):
        case = xc.build(name)
        if case.kind == "linear":
            steps = ex.linear(case.h0, case.g, case.operators, case.gammas, case.controls[0], case.T,
                              case.N, case.rho0, []).steps
        else:
            steps = ex.piecewise_constant(case.h0, case.g, case.operators, case.gammas,
                                          case.controls[0], case.T, case.N, case.rho0, [],
                                          want_grad=False).steps
        traces = np.trace(steps, axis1=-2, axis2=-1)
        assert np.max(np.abs(traces - 1)) < 1e-13
        if case.nonhermitian:  # (-i [H, rho] keeps the trace whatever H is, but not rho = rho^H)
            assert np.max(np.abs(steps - ex.dagger(steps))) > 1e-3
        else:
            assert np.max(np.abs(steps - ex.dagger(steps))) < 1e-13


def test_liouvillian_is_the_master_equation_entry_by_entry():
    rng = np.random.default_rng(12)
    n = 4
    h = cases_mod.gue(rng, n) - 0.1j * np.diag(rng.uniform(0, 1, n))
    ops = np.stack([cases_mod.gue(rng, n) + 0.5j * cases_mod.gue(rng, n) for _ in range(2)])
    gam = np.array([0.3, 0.7])
    rho = cases_mod.random_density(rng, n)
    want = -1j * (h @ rho - rho @ h)  # (the plain commutator, also for an H that is not Hermitian)
    for gm, op in zip(gam, ops):
        ldl = op.conj().T @ op
        want = want + gm * (op @ rho @ op.conj().T - 0.5 * (ldl @ rho + rho @ ldl))
    got = (ex.liouvillian(h, ops, gam) @ rho.reshape(-1)).reshape(n, n)
    assert np.max(np.abs(got - want)) < 1e-14
    # ... which is the right-hand side the reference integrates
    assert np.max(np.abs(got - ol.get_lindbladian(rho[None], gam, h, ops)[0])) < 1e-14


# ---- 2. the exact derivatives against differences of the reference's own cost --------------------------

def richardson(cost_of, x, h=0.05):
    return pc.richardson_differences(cost_of, x, range(np.size(x)), h).reshape(np.shape(x))


@pytest.mark.parametrize("name", ["n4_l1_pad1", "n4_forbid_ces2", "n5_nc4_on_6_steps",
                                  "n5_nc7_on_3_steps", "n6_nonhermitian_h0"])
def test_the_exact_gradient_against_richardson_differences(name):
    case = xc.build(name)
    costs = xc.oracle_costs(case)
    u = case.controls[0]

    def cost_of(x):
        return ex.piecewise_constant(case.h0, case.g, case.operators, case.gammas, x, case.T, case.N,
                                     case.rho0, costs, case.ces, want_grad=False).error
    out = ex.piecewise_constant(case.h0, case.g, case.operators, case.gammas, u, case.T, case.N,
                                case.rho0, costs, case.ces)
    want = richardson(cost_of, u)
    print(name, "gradient against differences", np.max(np.abs(out.grad - want)))
    # (O(h^6) differences of a cost evaluated to ~1e-16, divided by h: 1e-12 holds with a margin)
    assert np.max(np.abs(out.grad - want)) < 1e-12


@pytest.mark.parametrize("name", ["sweep_n4_l2", "duration_n4_l2"])
def test_the_exact_sensitivities_against_richardson_differences(name):
    case = xc.build(name)
    costs = xc.oracle_costs(case)
    b = 1
    args = (case.T, case.N, case.rho0, costs, case.ces)

    def run(scales, offsets, rates, want_grad=False):
        return ex.sweep_member(case.problem_h0, case.channels, case.operators, case.gammas,
                               case.controls[b], scales, offsets, rates, *args, want_grad=want_grad)
    s, d, c = case.scales[b], case.offsets[b], case.rate_scales[b]
    out = run(s, d, c, True)
    assert np.max(np.abs(out.scale_sens - richardson(lambda x: run(x, d, c).error, s))) < 1e-12
    assert np.max(np.abs(out.offset_sens - richardson(lambda x: run(s, x, c).error, d))) < 1e-12
    assert np.max(np.abs(out.rate_sens - richardson(lambda x: run(s, d, x).error, c))) < 1e-12
    # tau on the whole Lindbladian: scales, offsets and rates together (a duration sweep has h0 = 0)
    if case.kind == "duration":
        tau = case.taus[b]
        want = richardson(lambda x: run(x[0] * case.s0[b], x[0] * case.d0[b],
                                        x[0] * case.c0[b]).error, np.array([tau]))
        assert abs(out.tau_sens / tau - want[0]) < 1e-12
        assert abs(want[0]) > 1e-5


def test_the_directional_derivative_of_linear_against_differences():
    case = xc.build("linear_n4_l2_nc5")
    costs = xc.oracle_costs(case)
    u, d = case.controls[0], case.directions[0, 0]

    def cost_of(x):
        return ex.linear(case.h0, case.g, case.operators, case.gammas, u + x[0] * d, case.T, case.N,
                         case.rho0, costs, methods=("DOP853",)).error
    out = ex.linear(case.h0, case.g, case.operators, case.gammas, u, case.T, case.N, case.rho0, costs,
                    directions=[d], methods=("DOP853",))
    want = richardson(cost_of, np.zeros(1), h=0.1)
    # (the cost is integrated to ~1e-14 here, the quotient divides that by h / 4)
    assert abs(out.derivative[0] - want[0]) < 1e-11 and abs(want[0]) > 1e-4


# ---- 3. the model of the device scheme against the references, case by case -----------------------------

PARITY = {"cost": 1e-9, "member_cost": 1e-9, "densities": 1e-8}
GATES = {"cost": ex.GATE_COST, "member_cost": ex.GATE_COST, "densities": ex.GATE_DENSITIES,
         "gradient": ex.GATE_GRADIENT, "scale_sens": ex.GATE_SENSITIVITIES,
         "offset_sens": ex.GATE_SENSITIVITIES, "rate_sens": ex.GATE_SENSITIVITIES,
         "tau_grad": ex.GATE_SENSITIVITIES}
LINEAR_GATES = {"cost": ex.GATE_LINEAR_COST, "densities": ex.GATE_LINEAR_DENSITIES,
                "derivative": ex.GATE_LINEAR_DERIVATIVE}


@pytest.mark.parametrize("name", [n for n in xc.NAMES if xc.build(n).kind != "search"])
def test_the_model_of_the_scheme_against_the_exact_reference(name):
    """The scheme's discretisation error: the model passes every gate the engine is held to (the
    gates are ten times the committed measurement of exactly these numbers, see the next test, so
    the margin here is that factor), and stays below the documented parity tolerance."""
    case = xc.build(name)
    want = xc.exact_results(name)
    errors = xc.compare(xc.model_results(name), want)
    gates = LINEAR_GATES if case.kind == "linear" else GATES
    print(name, errors)
    for key, value in errors.items():
        assert value <= gates[key], (key, value, gates[key])
        assert value < PARITY.get(key, 1e-8), (key, value)
    for key, value in want.get("disagreement", {}).items():
        assert 10 * value <= gates[key], (key, value, gates[key])


def test_the_gate_constants_quote_the_committed_measurement():
    with open(os.path.join(ROOT, "profiles", "lindblad_exact.jsonl")) as f:
        lines = [json.loads(line) for line in f]
    worst = lines[-1]["worst"]
    assert [line["case"] for line in lines[:-1]] == xc.NAMES
    floors = {"cost": 1e-12, "densities": 1e-12, "gradient": 1e-10, "sensitivities": 1e-10}
    for quantity, constant in (("cost", ex.GATE_COST), ("densities", ex.GATE_DENSITIES),
                               ("gradient", ex.GATE_GRADIENT),
                               ("sensitivities", ex.GATE_SENSITIVITIES)):
        want = max(10 * worst[quantity]["value"], floors[quantity])
        assert want <= constant <= 1.05 * want, (quantity, constant, want)
    for quantity, constant, floor in (("cost", ex.GATE_LINEAR_COST, 1e-12),
                                      ("densities", ex.GATE_LINEAR_DENSITIES, 1e-12),
                                      ("derivative", ex.GATE_LINEAR_DERIVATIVE, 1e-10)):
        want = max(10 * worst["linear_" + quantity]["value"],
                   10 * worst["linear_two_method_" + quantity]["value"], floor)
        assert want <= constant <= 1.05 * want, (quantity, constant, want)


def test_the_sub_division_case_takes_one_two_and_four_or_more_sub_intervals():
    from tests import lindblad_model as lm
    case = xc.build("n4_l2_subdivisions")
    system = lm.StructuredLindblad(case.h0, case.g, case.gammas, case.operators)
    counts = []
    for u in case.controls:
        grid = lm.substep_grid(case.T, case.N, case.Nc + 1,
                               system.norm_bound(np.max(np.abs(u), axis=0)))
        counts.append(len(grid[0]))
    assert counts[0] == 1 and counts[1] == 2 and counts[2] >= 4, counts
    strong = xc.build("n4_l2_dissipator_dominated")
    rates = sum(g * np.linalg.norm(op, 2) ** 2 for g, op in zip(strong.gammas, strong.operators))
    assert rates > 5 * np.linalg.norm(strong.h0, 2)


def test_the_duration_sweeps_span_two_sub_division_groups():
    from tests import lindblad_model as lm
    for name in ("duration_n4_l1", "duration_n4_l2", "duration_n16_l3_complex_ops",
                 "duration_n20_l2"):
        case = xc.build(name)
        counts = set()
        for b in range(case.seeds):
            items = np.concatenate([case.scales[b][None] * case.controls[b],
                                    np.tile(case.offsets[b], (case.Nc, 1))], axis=1)
            system = lm.StructuredLindblad(case.problem_h0, case.channels,
                                           case.rate_scales[b] * case.gammas, case.operators)
            grid = lm.substep_grid(case.T, case.N, case.Nc + 1,
                                   system.norm_bound(np.max(np.abs(items), axis=0)))
            counts.add(len(grid[0]))
        assert len(counts) >= 2, (name, counts)


def test_rate_sensitivities_of_the_model_against_the_exact_ones():
    from tests import lindblad_model as lm
    from tests import lindblad_sweep_model as sm
    case = xc.build("n7_l2")
    costs = xc.oracle_costs(case)
    factors = np.array([0.5, 2.0])
    base = lm.StructuredLindblad(case.h0, case.g, case.gammas, case.operators)
    got = sm.rate_sensitivities(base, case.controls[0], case.rho0, case.T, case.N, costs,
                                factors=factors, piecewise_constant=True)[1]
    want = ex.sweep_member(case.h0, case.g, case.operators, case.gammas, case.controls[0], None, None,
                           factors, case.T, case.N, case.rho0, costs).rate_sens
    print("dE/dc model", got, "exact", want)
    assert np.max(np.abs(want)) > 1e-5
    assert np.max(np.abs(got - want)) <= ex.GATE_SENSITIVITIES / 10 * np.max(np.abs(want))


# ---- 4. the references see what a kernel could get wrong --------------------------------------------------

def moved(a, b):
    """How far a mutation moves the exact error, final densities or gradient."""
    out = max(abs(a.error - b.error), float(np.max(np.abs(a.final - b.final))))
    if hasattr(a, "grad") and a.grad.size:
        out = max(out, float(np.max(np.abs(a.grad - b.grad))))
    return out


def mutation_case():
    """n = 4, two complex operators with distinct rates, a complex G, slices that do not line up
    with the steps, a final target and a ForbidDensities step cost every second step."""
    rng = np.random.default_rng(77)
    n, K, N, Nc, T = 4, 2, 7, 4, 1.8
    gue = cases_mod.gue
    c = dict(h0=1.5 * gue(rng, n), g=[gue(rng, n) for _ in range(K)],
             ops=np.stack([gue(rng, n) + 0.5j * gue(rng, n) for _ in range(2)]),
             gam=np.array([0.3, 0.6]), u=0.7 * rng.standard_normal((Nc, K)), T=T, N=N,
             rho0=cases_mod.random_density(rng, n)[None])
    targ = cases_mod.random_density(rng, n)[None]
    forb = np.stack([cases_mod.random_density(rng, n) for _ in range(2)]).reshape(1, 2, n, n)
    c["costs"] = [ol.TargetDensityInfidelity(targ, cost_multiplier=n),
                  ol.ForbidDensities(forb, N, cost_eval_step=2, cost_multiplier=n * n)]
    return c


def exact_of(c, hook=None, **kw):
    c = dict(c, **kw)
    return ex.piecewise_constant(c["h0"], c["g"], c["ops"], c["gam"], c["u"], c["T"], c["N"],
                                 c["rho0"], c["costs"], c.get("ces", 2), step_liouvillian=hook)


def test_mutations_of_the_liouvillian_move_the_reference():
    c = mutation_case()
    good = exact_of(c)
    eye = np.eye(4)
    flipped = sum(gm * (np.kron(ex.dagger(op), op.T) - np.kron(op, op.conj()))
                  for gm, op in zip(c["gam"], c["ops"]))
    halves = sum(-0.5 * gm * (np.kron(ex.dagger(op) @ op, eye) + np.kron(eye, (ex.dagger(op) @ op).T))
                 for gm, op in zip(c["gam"], c["ops"]))
    points, _ = ex.merged_grid(c["N"], c["u"].shape[0])
    drives = [ex.hamiltonian_superoperator(x) for x in c["g"]]

    def next_slice_at_an_edge(q, j, lv):
        # an interval that ends on an interior slice edge reads the slice behind the edge
        if points[q + 1] % (c["N"] - 1) == 0 and j + 1 < c["u"].shape[0]:
            return lv + sum((c["u"][j + 1, k] - c["u"][j, k]) * drives[k] for k in range(2))
        return lv
    mutations = {
        "L^H rho L for L rho L^H": exact_of(c, lambda q, j, lv: lv + flipped),
        "an anticommutator without its 1/2": exact_of(c, lambda q, j, lv: lv + halves),
        "gamma squared": exact_of(c, gam=c["gam"] ** 2),
        "slice j + 1 read at a slice edge": exact_of(c, next_slice_at_an_edge),
        "G^T for a complex G": exact_of(c, g=[x.T for x in c["g"]]),
    }
    for what, bad in mutations.items():
        print(what, moved(good, bad))
        assert moved(good, bad) >= 1e-6, what


def test_a_step_cost_one_step_late_moves_the_reference():
    c = mutation_case()
    good = exact_of(c)
    forbid = c["costs"][1]

    class Late(object):
        """The same cost, evaluated on the densities one system step after its own steps."""
        requires_step_evaluation = True

        def cost(self, controls, densities, step):
            return forbid.cost(controls, densities, step) if step > 2 and step % 2 == 1 else 0.0

        def states_bar(self, controls, densities, step):
            if step > 2 and step % 2 == 1:
                return forbid.states_bar(controls, densities, step)
            return np.zeros_like(densities)
    bad = exact_of(c, costs=[c["costs"][0], Late()], ces=1)
    print("a step cost one step late", moved(good, bad))
    assert abs(good.error - bad.error) >= 1e-6
    assert np.max(np.abs(good.grad - bad.grad)) >= 1e-6


def test_mutations_of_the_tables_move_the_reference():
    case = xc.build("duration_n4_l2")
    costs = xc.oracle_costs(case)

    def run(b, rates):
        return ex.sweep_member(case.problem_h0, case.channels, case.operators, case.gammas,
                               case.controls[b], case.scales[b], case.offsets[b], rates, case.T,
                               case.N, case.rho0, costs)
    for b in range(1, case.seeds):
        good = run(b, case.rate_scales[b])
        # member m's rates taken from member m - 1
        assert moved(good, run(b, case.rate_scales[b - 1])) >= 1e-6
    for b in (0, 3):  # tau = 0.5 and 1.5 on the Hamiltonian but not on the rates
        assert moved(run(b, case.rate_scales[b]), run(b, case.c0[b])) >= 1e-6
