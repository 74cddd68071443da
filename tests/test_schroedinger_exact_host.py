"""
CPU tests of the exact Schroedinger reference (tests/schroedinger_exact.py), of its case table
(tests/schroedinger_exact_cases.py) and of the gates the GPU tests (tests/test_gpu_schroedinger_exact.py)
hold the engine to:

  * the NumPy model of every route sits within a tenth of its gate against exact on every case - the
    gates are ten times the models' own distance (profiles/schroedinger_exact.jsonl);
  * the reference agrees with the oracle at the oracle's gates, with mpmath at 40 digits on the smallest
    case of each kind (no gate is below ten times that disagreement), and with central differences;
  * the table reaches what it claims by the host's bound: every Pade order and 0, 1 and 2 squarings per
    Pade family, no step within 1e-9 of a threshold, three degrees and more on the matrix-free routes,
    every matrix-free case under the host's theta_18;
  * mutation proofs: the gates see one Pade order too low, three Taylor degrees too few, a dropped
    squaring, a dropped 2^-s on the generator's cotangent and a generator from the neighbouring step.
"""

import json
import os

import numpy as np
import pytest

from oracle import qoc_numpy as onp
from tests import action_model as am
from tests import mixed_pulses as mp
from tests import schroedinger_exact as ex
from tests import schroedinger_exact_cases as xc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROFILE = os.path.join(ROOT, "profiles", "schroedinger_exact.jsonl")


# ---- the gates ------------------------------------------------------------------------------------------

def profile_summary():
    with open(PROFILE) as f:
        return json.loads(f.readlines()[-1])


def test_every_gate_is_ten_times_the_profile_and_ten_times_the_mpmath_disagreement():
    """GATES = 10 x the family's worst model-against-exact number of profiles/schroedinger_exact.jsonl,
    rounded up to two digits; never below 10 x the reference's disagreement with mpmath."""
    summary = profile_summary()
    floors = dict(cost=ex.MPMATH_COST, states=ex.MPMATH_STATES, gradient=ex.MPMATH_DERIVATIVE,
                  sensitivities=ex.MPMATH_DERIVATIVE, tau_gradient=ex.MPMATH_DERIVATIVE)
    recorded = summary["mpmath_worst"]
    assert ex.MPMATH_COST >= recorded["cost"]["value"]
    assert ex.MPMATH_STATES >= recorded["states"]["value"]
    assert ex.MPMATH_DERIVATIVE >= recorded["derivative"]["value"]
    for family in ex.FAMILIES:
        for quantity, gate in ex.GATES[family].items():
            measured = summary["worst"][family].get(quantity)
            want = 10 * floors[quantity]
            if measured is not None:
                want = max(want, 10 * measured["value"])
            assert want * (1 - 1e-12) <= gate <= 1.1 * want, (family, quantity, gate, want)


@pytest.mark.parametrize("name", ["k1a_n20_ladder_4theta13", "sweepi_n16_s1", "action_wide_n64", "duration_n8"])
def test_the_tool_reproduces_its_lines_of_the_profile(name):
    """tools/measure_schroedinger_exact.py on the cases that set gates (the cases above n = 64 may move in
    their last digit with the number of BLAS threads and are left to a whole run of the tool)."""
    import importlib.util
    spec = importlib.util.spec_from_file_location(
        "measure_schroedinger_exact", os.path.join(ROOT, "tools", "measure_schroedinger_exact.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    with open(PROFILE) as f:
        recorded = [json.loads(line) for line in f]
    assert tool.measure(name) == next(line for line in recorded if line.get("case") == name)


@pytest.mark.parametrize("name", xc.NAMES)
def test_every_model_is_within_a_tenth_of_its_gate(name):
    case = xc.build(name)
    gates = ex.gates_of(case.family)
    errors = xc.compare(xc.model_results(name), xc.exact_results(name))
    for key, value in errors.items():
        assert value <= 0.1 * gates[key], (key, value, gates[key])


# ---- the reference ----------------------------------------------------------------------------------------

ORACLE_CASES = [s["name"] for s in xc.SPECS if s["kind"] == "plain" and s["interpolation"] == ex.LINEAR
                and not s["timedep"] and not s["quadratic"] and s["level"] < 6 and s["n"] <= 40]


@pytest.mark.parametrize("name", ORACLE_CASES)
def test_the_reference_agrees_with_the_oracle_at_the_oracles_gates(name):
    case = xc.build(name)
    want = xc.exact_results(name)
    for b, u in enumerate(case.controls):
        error, grads, final = onp.evaluate_with_grad(xc.oracle_problem(case), u)
        assert abs(error - want["cost"][b]) < 1e-10
        assert np.max(np.abs(final[:, :, 0] - want["states"][b])) < 1e-10
        assert np.max(np.abs(np.real(grads) - want["grad"][b])) < 1e-8 * np.max(np.abs(grads))


@pytest.mark.parametrize("name", xc.MPMATH_CASES)
def test_the_reference_agrees_with_mpmath(name):
    got = xc.mpmath_disagreement(name)
    print(name, got)
    assert got["cost"] <= ex.MPMATH_COST
    assert got["states"] <= ex.MPMATH_STATES
    assert got.get("derivative", 0.0) <= ex.MPMATH_DERIVATIVE


@pytest.mark.parametrize("name", ["mp_forbid_n6_ces2", "mp_nonhermitian_n6", "mp_linear_m6_n6"])
def test_the_exact_gradient_agrees_with_central_differences(name):
    case = xc.build(name)
    u = case.controls[0]
    grad = xc.exact_member(case, case.h0, case.g, u).grad
    h, worst = 1e-5, 0.0
    for j in range(u.shape[0]):
        for k in range(u.shape[1]):
            up, down = u.copy(), u.copy()
            up[j, k] += h
            down[j, k] -= h
            fd = (xc.exact_member(case, case.h0, case.g, up, want_grad=False).error
                  - xc.exact_member(case, case.h0, case.g, down, want_grad=False).error) / (2 * h)
            worst = max(worst, abs(fd - grad[j, k]))
    assert worst < 1e-7 * max(1.0, np.max(np.abs(grad))), worst


def test_step_states_are_the_products_of_the_step_propagators():
    case = xc.build("mp_forbid_n6_ces2")
    out = xc.exact_member(case, case.h0, case.g, case.controls[0])
    assert out.steps.shape == (case.N, case.S, case.n) and out.step_grad.shape == (case.N - 1, 1, case.K)
    assert np.array_equal(out.steps[0], case.psi0) and np.array_equal(out.steps[-1], out.final)
    # a Hermitian H: every step is unitary
    assert np.max(np.abs(np.linalg.norm(out.steps, axis=2) - 1.0)) < 1e-14


# ---- the table reaches what it claims ---------------------------------------------------------------------

PADE_FAMILIES = ("lu", "inverse")


@pytest.mark.parametrize("family", PADE_FAMILIES)
def test_every_order_and_squaring_count_occurs_by_the_hosts_bound(family):
    orders, squarings = set(), set()
    for name in xc.NAMES:
        case = xc.build(name)
        if case.family != family or case.model == "action":
            continue
        dec = xc.decisions(case)
        orders |= set(int(m) for m in dec["order_table"].ravel())
        squarings |= set(int(s) for s in dec["squarings"].ravel())
        if case.order is not None:  # the case's order is that of its loudest step
            assert case.order == int(np.max(dec["order_table"])), name
            assert case.squarings == int(np.max(dec["squarings"])), name
    assert orders == set(xc.ORDERS) and squarings >= {0, 1, 2}


@pytest.mark.parametrize("name", xc.NAMES)
def test_no_step_lies_within_1e_9_of_a_threshold(name):
    case = xc.build(name)
    dec = xc.decisions(case)
    if case.model != "action":
        for key in ("exact", "sqfree"):
            assert not mp.near_threshold(dec[key].ravel()), key
        assert not mp.near_threshold(dec["bound"][:, :, 0].ravel())
    else:
        for b1, b2 in dec["bound"].reshape(-1, 2):
            assert all(abs(b1 - th) > 1e-9 * th for th in am.THETA.values())
            assert all(abs(b2 - th) > 1e-9 * th for th in xc.THN.values())
    level = np.max(dec["bound"][:, :, 0 if case.norm == "one" else 1])
    assert abs(level - case.level) < 1e-6 * case.level, (level, case.level)


def test_the_matrix_free_cases_stay_on_their_route_and_span_the_degrees():
    tops, everything = set(), set()
    for name in xc.NAMES:
        case = xc.build(name)
        if case.model != "action":
            continue
        dec = xc.decisions(case)
        assert int(np.max(dec["degree"])) == case.degree, name
        tops.add(case.degree)
        everything |= set(int(m) for m in dec["degree"].ravel())
        # the host's knot bound (qocx_upload_controls), after the expansion of the seed tables
        items = xc.items_of(case)
        bounds = mp.host_bounds(case.problem_h0, case.channels, items, case.dt, case.N, case.Nc)
        assert min(bounds["norm_bound"], bounds["norm_bound_mid"]) <= 0.98 * am.THETA[18], name
    assert len(tops) >= 3 and max(tops) >= 16 and min(tops) <= 6
    assert len(everything) >= 8


def test_ladder_norms_nearly_coincide_and_gue_norms_do_not():
    ladder, gue = xc.build("k1a_n20_ladder_order9"), xc.build("k1a_n20_gue_order9")
    ratio = lambda c: onp.one_norm(c.h0) / xc.spectral_bound(c.h0)
    assert ratio(ladder) < 1.25 and ratio(gue) > 1.8
    # real couplings: the device's |re| + |im| column bound is the 1-norm
    dec = xc.decisions(ladder)
    assert np.max(np.abs(dec["sqfree"] - dec["exact"])) < 1e-15


# ---- mutation proofs ------------------------------------------------------------------------------------
# A mutation is seen when some quantity of the case leaves its gate by a factor of ten; every test prints
# the factor of every quantity (DESIGN.md section 10 lists them).

def mutation_ratio(name, **mutation):
    """The largest (error of the mutated model against exact) / gate over the quantities."""
    case = xc.build(name)
    gates = ex.gates_of(case.family)
    errors = xc.compare(xc.model_results(name, **mutation), xc.exact_results(name))
    return {key: errors[key] / gates[key] for key in errors}


@pytest.mark.parametrize("name", ["k1a_n20_ladder_order5", "k1a_n20_ladder_order7", "k1a_n20_ladder_order13",
                                  "sweepi_n8_ladder_order5", "sweepi_n8_ladder_order7",
                                  "sweepi_n8_ladder_order13"])
def test_the_gates_see_one_pade_order_too_low(name):
    ratios = mutation_ratio(name, order_shift=-1)
    print(name, ratios)
    assert max(ratios.values()) >= 10


@pytest.mark.parametrize("name", ["k1a_n20_ladder_order9", "sweepi_n8_ladder_order9"])
def test_one_order_too_low_at_order_9_is_printed_not_asserted(name):
    """Order 9 -> 7 just below theta_9 moves the states by about 1e-12: DESIGN.md section 10 lists what
    the gates make of it."""
    print(name, "order 9 -> 7:", mutation_ratio(name, order_shift=-1))


@pytest.mark.parametrize("name", ["action_n17_degree6", "action_n20_degree11", "action_wide_n48",
                                  "action_states_n17_s2", "action_costs_n20_forbid"])
def test_the_gates_see_three_taylor_degrees_too_few(name):
    ratios = mutation_ratio(name, degree_shift=-3)
    print(name, ratios)
    assert max(ratios.values()) >= 10


@pytest.mark.parametrize("name", ["action_n32_degree16", "action_wide_n64", "action_states_n32_s4",
                                  "action_n20_one_norm_rule"])
def test_three_degrees_too_few_at_the_high_degrees_is_printed_not_asserted(name):
    """theta'_m bounds the remainder of every eigenvalue up to beta; at degrees 13 and above the last
    three terms weigh 1e-14 .. 1e-12 on these states: DESIGN.md section 10 lists what the gates make of
    it."""
    print(name, "degree - 3:", mutation_ratio(name, degree_shift=-3))


@pytest.mark.parametrize("name", ["k1a_n20_ladder_level20", "k1a_n20_ladder_1p9theta13",
                                  "sweepi_n8_ladder_4theta13", "general_n72_level20"])
def test_the_gates_see_a_dropped_squaring_and_a_dropped_scale(name):
    ratios = mutation_ratio(name, drop_squaring=True)
    assert ratios["states"] >= 10 and ratios["gradient"] >= 10, ratios
    ratios = mutation_ratio(name, keep_scale=True)
    print(name, ratios)
    assert ratios["gradient"] >= 10 and ratios["states"] <= 0.1, ratios


@pytest.mark.parametrize("name", ["k1a_n20_ladder_order7", "sweepi_n8_ladder_order9", "action_n20_degree11",
                                  "mp_pwc_n6"])
def test_the_gates_see_a_generator_from_the_neighbouring_step(name):
    """Through the hook of the reference: step 1 evolves under the generator of step 2."""
    case = xc.build(name)
    kept = {}

    def record(step, a):
        kept[step] = a
        return a

    u = case.controls[0]
    want = xc.exact_member(case, case.h0, case.g, u, step_generator=record)
    got = xc.exact_member(case, case.h0, case.g, u, step_generator=lambda j, a: kept[2] if j == 1 else a)
    gates = ex.gates_of(case.family)
    states = np.max(np.abs(got.final - want.final))
    gradient = np.max(np.abs(got.grad - want.grad)) / np.max(np.abs(want.grad))
    assert states >= 10 * gates["states"] and gradient >= 10 * gates["gradient"], (states, gradient)
