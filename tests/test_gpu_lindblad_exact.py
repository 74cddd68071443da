"""
GPU tests (-m gpu) of the Lindblad engine, through the C ABI, against references that do not share its
scheme (tests/lindblad_exact.py): products of exponentials of the n^2 x n^2 superoperator and their
Frechet derivatives for PIECEWISE_CONSTANT controls - cost, final densities, the full gradient, and the
sensitivities to scales, offsets, rates and duration -, and two unrelated solve_ivp methods with a
forward sensitivity equation for LINEAR controls and h0(t).

The cases are the table of tests/lindblad_exact_cases.py: every kernel route (one tile, the tile kernel
above n = 16, one-wave kernels, the classic launch, recomputed stage values), sub-division counts,
slices that do not line up with the steps, a long horizon, ensembles with rates, sweeps, duration sweeps
and duration searches. The gates are the constants of tests/lindblad_exact.py, measured on the CPU by
the NumPy model of the scheme against the same references (profiles/lindblad_exact.jsonl), never by the
engine. Every test prints its worst error over its gate.
"""

import numpy as np
import pytest

from tests import gpu_helpers as gh
from tests import lindblad_exact as ex
from tests import lindblad_exact_cases as xc

pytestmark = pytest.mark.gpu

DEFAULT_KNOBS = dict(lindblad_pad_operator=1, lindblad_chain=1, lindblad_q2=1, lindblad_two_sided=1,
                     lindblad_hermitian=1, lindblad_real_ops=1, lindblad_4t=1)
PWC = "piecewise_constant"
GATES = {"cost": ex.GATE_COST, "member_cost": ex.GATE_COST, "densities": ex.GATE_DENSITIES,
         "gradient": ex.GATE_GRADIENT, "scale_sens": ex.GATE_SENSITIVITIES,
         "offset_sens": ex.GATE_SENSITIVITIES, "rate_sens": ex.GATE_SENSITIVITIES,
         "tau_grad": ex.GATE_SENSITIVITIES}
LINEAR_GATES = {"cost": ex.GATE_LINEAR_COST, "densities": ex.GATE_LINEAR_DENSITIES,
                "derivative": ex.GATE_LINEAR_DERIVATIVE}
TAU_BOX = (0.4, 1.6)


@pytest.fixture(scope="module")
def engine():
    from qoc_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


def set_problem(engine, case, h0, g, interpolation=PWC, **kw):
    L = 0 if case.operators is None else len(case.operators)
    engine.set_lindblad_problem(
        case.n, case.S, len(g), case.Nc, case.N, case.T, h0, g, case.gammas if L else None,
        case.operators if L else None, case.rho0, costs=gh.lindblad_device_costs(case),
        cost_eval_step=case.ces, interpolation=interpolation, **kw)


def chain_rule(case, out):
    """dE_b/dtau_b through the tables scales = tau s0, offsets = tau delta0, rates = tau c0."""
    return (np.sum(case.s0 * out["scale_sens"], axis=1) + np.sum(case.d0 * out["offset_sens"], axis=1)
            + np.sum(case.c0 * out["rate_sens"], axis=1))


def device_results(engine, case):
    """The quantities of tests/lindblad_exact_cases.results from the engine."""
    from qoc_amd.engine import Engine
    u = case.controls
    if case.kind == "linear":
        kw = {}
        if case.h0_of_t is not None:
            times = Engine.lindblad_stage_times(case.T, case.N, case.Nc, case.K, case.subdivision)
            kw = dict(fixed_subdivision=case.subdivision,
                      h0_stages=np.stack([case.h0_of_t(t) for t in times]))
        set_problem(engine, case, case.h0, case.g, interpolation="linear", **kw)
        cost, grads, final = engine.evaluate_lindblad(u)
        return dict(cost=cost, final=final, derivative=np.array(
            [[np.sum(grads[b] * d) for d in case.directions[b]] for b in range(len(u))]))
    if case.kind == "plain":
        set_problem(engine, case, case.h0, case.g)
        if case.debug is not None:
            engine.debug_lindblad_knobs(*case.debug)
        cost, grads, final = engine.evaluate_lindblad(u)
        return dict(cost=cost, final=final, grad=grads)
    set_problem(engine, case, case.problem_h0, case.channels)
    if case.kind == "ensemble":
        engine.set_lindblad_ensemble(case.scales, case.offsets, case.weights)
        engine.set_lindblad_ensemble_rates(case.rate_scales)
        cost, grads, final = engine.evaluate_lindblad(u)
        return dict(cost=cost, grad=grads, final=final,
                    member_cost=engine.lindblad_ensemble_member_costs())
    engine.set_lindblad_sweep(case.scales, case.offsets, case.rate_scales)
    if case.kind == "search":
        engine.lindblad_sweep_set_durations(case.taus, case.s0, case.d0, case.c0, TAU_BOX[0],
                                            TAU_BOX[1], case.weight)
    engine.lindblad_sweep_want_rate_sensitivities(True)
    try:
        cost, grads, final = engine.evaluate_lindblad(u)
        scale_sens, offset_sens, rate_sens = engine.lindblad_sweep_sensitivities()
    finally:
        engine.lindblad_sweep_want_rate_sensitivities(False)
    assert rate_sens is not None, "the rate sensitivities did not run (not two-sided)"
    out = dict(cost=cost, grad=grads, final=final, scale_sens=scale_sens, offset_sens=offset_sens,
               rate_sens=rate_sens)
    if case.kind == "duration":
        out["tau_grad"] = chain_rule(case, out)
    if case.kind == "search":
        tau, tau_grad = engine.lindblad_sweep_download_durations()
        assert np.max(np.abs(tau - case.taus)) < 1e-15
        # the price of time, lambda tau_b on the cost and lambda on the gradient, taken off again:
        # what is left is held to the exact E_b and dE_b/dtau_b
        out["cost"] = cost - case.weight * tau
        out["tau_grad"] = tau_grad - case.weight
        if case.weight:
            assert np.max(np.abs(tau_grad - chain_rule(case, out) - case.weight)) < 1e-14
    return out


def sub_intervals_per_seed(engine, case):
    counts = []
    for b in range(case.controls.shape[0]):
        engine.evaluate_lindblad(case.controls[b:b + 1], want_grad=False)
        counts.append(engine.lindblad_last_subintervals())
    return counts


@pytest.mark.parametrize("name", xc.NAMES)
def test_the_engine_against_the_exact_reference(engine, name):
    case = xc.build(name)
    want = xc.exact_results(name)
    try:
        for knob, value in dict(DEFAULT_KNOBS, **case.knobs).items():
            engine.set_knob(knob, value)
        got = device_results(engine, case)
        counts = sub_intervals_per_seed(engine, case) if case.amplitudes is not None else None
    finally:
        for knob, value in DEFAULT_KNOBS.items():
            engine.set_knob(knob, value)
        engine.debug_lindblad_knobs(0, 256, 0)
    gates = dict(LINEAR_GATES if case.kind == "linear" else GATES)
    if case.kind == "linear":
        # a reference is accepted only as far as its two integrators agree
        for key, value in want["disagreement"].items():
            assert 10 * value <= gates[key], (key, value)
    errors = xc.compare(got, want)
    ratios = {key: errors[key] / gates[key] for key in errors}
    worst = max(ratios, key=ratios.get)
    print(name, "worst error over its gate: %s %.3g / %.3g = %.3g" % (
        worst, errors[worst], gates[worst], ratios[worst]), errors)
    if case.kind in ("sweep", "duration", "search"):  # every table carries a signal
        for key in ("scale_sens", "offset_sens", "rate_sens"):
            assert np.max(np.abs(want[key])) > 1e-7
    if counts is not None:  # 1, 2 and >= 4 sub-intervals per step in one batch
        steps = case.N - 1
        print("sub-intervals per seed", counts)
        assert counts[0] == steps and counts[1] == 2 * steps and counts[2] >= 4 * steps
    for key in sorted(errors):
        assert errors[key] <= gates[key], (key, errors[key], gates[key])
