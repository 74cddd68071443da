"""
GPU tests (-m gpu) of the Schroedinger engine, through the C ABI, against a reference that does not share
its scheme (tests/schroedinger_exact.py): products of the exact step propagators exp(-i dt H) by
eigendecomposition and their Daleckii-Krein derivatives - cost, final states, the full gradient, and the
sensitivities of ensembles, sweeps, duration sweeps and duration searches.

The cases are the table of tests/schroedinger_exact_cases.py: every kernel route of DESIGN.md section 3
at the smallest sizes that reach it, on transmon-like "ladder" operators and on GUE operators, with the
largest step bound at 0.97 of every Pade threshold, at 1.9 and 0.97 x 4 theta_13 and at 20, and for the
matrix-free routes at 0.97 of three spectral-norm thresholds. The gates are the constants of
tests/schroedinger_exact.py, measured on the CPU by the NumPy models of the routes against the same
reference (profiles/schroedinger_exact.jsonl), never by the engine. Every test prints its worst error over
its gate and the orders / degrees the engine executed.
"""

import numpy as np
import pytest

from tests import schroedinger_exact as ex
from tests import schroedinger_exact_cases as xc

pytestmark = pytest.mark.gpu

BITS_CASES = ("k1a_n20_ladder_level20", "sweepi_n8_ladder_order13", "action_n20_degree11")


@pytest.fixture(scope="module")
def engine():
    from qoc_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


def set_problem(engine, case):
    from tests import gpu_helpers as gh
    engine.set_schroedinger_problem(
        case.n, case.S, len(case.channels), case.Nc, case.N, case.T, case.h0_table, case.g_table,
        case.psi0, costs=gh.device_costs(case)[0], cost_eval_step=case.ces, magnus_policy=case.magnus,
        interpolation=case.interpolation)
    if case.quadratic is not None:
        engine.set_quadratic_terms(*case.quadratic)


class Evidence(object):
    """What the engine says it executed, summed over the evaluations of a case."""

    def __init__(self, engine):
        self.engine = engine
        self.orders = {m: 0 for m in xc.ORDERS}
        self.degrees = {m: 0 for m in range(1, 19)}
        self.fallbacks = 0
        self.reruns = engine.action_reruns()

    def take(self):
        for m, count in self.engine.pade_orders().items():
            self.orders[m] += count
        for m, count in self.engine.action_degrees().items():
            self.degrees[m] += count
        self.fallbacks += self.engine.lu_fallbacks()

    def rerun_count(self):
        return self.engine.action_reruns() - self.reruns


def evaluate(engine, case, evidence, want_grad=True):
    """engine.evaluate on the case's seeds; latency mode takes one control set at a time."""
    u = case.controls
    if not case.one_by_one:
        out = engine.evaluate(u, want_grad)
        evidence.take()
        return out
    outs = []
    for b in range(len(u)):
        outs.append(engine.evaluate(u[b:b + 1], want_grad))
        evidence.take()
    return tuple(None if outs[0][i] is None else np.concatenate([o[i] for o in outs]) for i in range(3))


def device_results(engine, case, evidence):
    """The quantities of tests/schroedinger_exact_cases.results from the engine."""
    set_problem(engine, case)
    if case.kind == "plain":
        cost, grads, final = evaluate(engine, case, evidence)
        return dict(cost=cost, states=final, grad=grads)
    if case.kind == "ensemble":
        engine.set_ensemble(case.scales, case.offsets, case.weights)
        cost, grads, final = evaluate(engine, case, evidence)
        return dict(cost=cost, grad=grads, states=final, member_cost=engine.ensemble_member_costs())
    engine.set_sweep(case.scales, case.offsets)
    if case.kind == "search":
        engine.sweep_set_durations(case.taus, case.s0, case.d0, xc.TAU_BOX[0], xc.TAU_BOX[1], case.weight)
    cost, grads, final = evaluate(engine, case, evidence)
    scale_sens, offset_sens = engine.sweep_sensitivities()
    out = dict(cost=cost, grad=grads, states=final, scale_sens=scale_sens, offset_sens=offset_sens)
    if case.kind == "duration":
        out["tau_grad"] = xc.chain_rule(case, out)
    if case.kind == "search":
        tau, tau_grad = engine.sweep_download_durations()
        assert np.max(np.abs(tau - case.taus)) < 1e-15
        # the price of time, lambda tau_b on the cost and lambda on the gradient, taken off again: what
        # is left is held to the exact E_b and dE_b/dtau_b
        out["cost"] = cost - case.weight * tau
        out["tau_grad"] = tau_grad - case.weight
        if case.weight:
            assert np.max(np.abs(tau_grad - xc.chain_rule(case, out) - case.weight)) < 1e-14
    return out


def run_with_knobs(engine, case, body):
    try:
        for knob, value in dict(xc.KNOB_DEFAULTS, **case.knobs).items():
            engine.set_knob(knob, value)
        return body()
    finally:
        for knob, value in xc.KNOB_DEFAULTS.items():
            engine.set_knob(knob, value)
        engine.set_chunk(0)
        engine.set_pipeline(0)


def assert_route(case, evidence):
    """The approximant the case is about ran: Pade orders between what the step generators' own
    1-norms ask for and what the host's bounds allow, the case's order among them; or the degrees of the
    matrix-free route, the case's degree the highest, and nothing handed back to the Pade route."""
    dec = xc.decisions(case)
    steps = dec["exact"].size
    executed_degrees = {m: c for m, c in evidence.degrees.items() if c}
    executed_orders = {m: c for m, c in evidence.orders.items() if c}
    print(case.name, "orders", executed_orders, "degrees", executed_degrees, "lu fallbacks",
          evidence.fallbacks, "reruns", evidence.rerun_count())
    if case.model == "action":
        assert sum(executed_degrees.values()) == steps, executed_degrees
        assert evidence.rerun_count() == 0
        assert max(executed_degrees) == case.degree == int(np.max(dec["degree"])), executed_degrees
        return
    assert not executed_degrees, executed_degrees
    assert sum(executed_orders.values()) == steps, executed_orders
    for m in xc.ORDERS:
        taken = sum(c for order, c in executed_orders.items() if order >= m)
        assert np.sum(dec["order_exact"] >= m) <= taken <= np.sum(dec["order_upper"] >= m), (
            m, executed_orders)
    if case.order is not None and case.order == int(np.max(dec["order_upper"])):
        assert executed_orders.get(case.order, 0) > 0, executed_orders
    # where the host's bound proves the diagonal pivots of every denominator, no factorisation may have
    # left its form; elsewhere the count is printed above
    if np.all(dec["dominant"]):
        assert evidence.fallbacks == 0


@pytest.mark.parametrize("name", xc.NAMES)
def test_the_engine_against_the_exact_reference(engine, name):
    case = xc.build(name)
    want = xc.exact_results(name)
    evidence = Evidence(engine)
    got = run_with_knobs(engine, case, lambda: device_results(engine, case, evidence))
    gates = ex.gates_of(case.family)
    errors = xc.compare(got, want)
    ratios = {key: errors[key] / gates[key] for key in errors}
    worst = max(ratios, key=ratios.get)
    print(name, "family", case.family, "worst error over its gate: %s %.3g / %.3g = %.3g" % (
        worst, errors[worst], gates[worst], ratios[worst]), errors)
    assert_route(case, evidence)
    if case.kind in ("sweep", "duration", "search"):  # every table carries a signal
        for key in ("scale_sens", "offset_sens"):
            assert np.max(np.abs(want[key])) > 1e-7
    for key in sorted(errors):
        assert errors[key] <= gates[key], (key, errors[key], gates[key])


@pytest.mark.parametrize("prefix", ["k1a_n20_ladder", "sweepi_n8_ladder"])
def test_every_order_and_squaring_count_is_executed_on_each_family(engine, prefix):
    """The level cases of the LU and of the inverse-image family on ladder operators (table bound,
    norm and square-root-free norm agree on every order), run again without gradients: every Pade order
    is executed, and the steps the host's bound gives 0, 1 and 2 squarings are."""
    orders, squarings = set(), set()
    for name in xc.NAMES:
        if not name.startswith(prefix + "_"):
            continue
        case = xc.build(name)
        evidence = Evidence(engine)

        def body():
            set_problem(engine, case)
            evaluate(engine, case, evidence, want_grad=False)
        run_with_knobs(engine, case, body)
        assert sum(evidence.orders.values()) == case.controls.shape[0] * (case.N - 1)
        orders |= {m for m, c in evidence.orders.items() if c}
        squarings |= set(int(s) for s in xc.decisions(case)["squarings"].ravel())
    assert orders == set(xc.ORDERS), orders
    assert squarings >= {0, 1, 2}, squarings


@pytest.mark.parametrize("name", ["forbid_n20_ces2", "sweepi_n16_s5_gue_level20", "nonhermitian_n6"])
def test_kept_step_states_against_the_exact_step_states(engine, name):
    """qocx_set_keep_step_states: the states at every system step, at the gate of the final states."""
    case = xc.build(name)
    want = np.stack([xc.exact_member(case, case.h0_table, case.g_table, u, want_grad=False).steps
                     for u in case.controls])

    def body():
        set_problem(engine, case)
        engine.set_keep_step_states(True)
        try:
            engine.evaluate(case.controls, True)
            return engine.download_step_states()
        finally:
            engine.set_keep_step_states(False)
    got = run_with_knobs(engine, case, body)
    error, gate = np.max(np.abs(got - want)), ex.GATES[case.family]["states"]
    print(name, "step states %.3g / %.3g = %.3g" % (error, gate, error / gate))
    assert got.shape == want.shape and error <= gate


@pytest.mark.parametrize("name", BITS_CASES)
def test_chunks_and_segments_give_the_bits_of_the_plain_evaluation(engine, name):
    """Chunks of one seed and two time segments: scheduling alone."""
    case = xc.build(name)

    def body():
        set_problem(engine, case)
        plain = engine.evaluate(case.controls, True)
        engine.set_chunk(1)
        engine.set_pipeline(2)
        split = engine.evaluate(case.controls, True)
        return plain, split
    plain, split = run_with_knobs(engine, case, body)
    for x, y in zip(plain, split):
        assert np.array_equal(x, y)
