"""
CPU tests (-m "not gpu") of tests/action_features.py, by the oracle and the NumPy model alone - what
tests/test_gpu_action_features.py holds the matrix-free route to could not be passed by a plausibly wrong
kernel, and is reachable by a correct one:

  * every case stays on the route: the host's knot bound of its controls - after the ensemble, sweep or
    duration expansion - is <= 0.9 theta_18, and the degrees of its steps take >= 3 values;
  * the extended model (action_model.evaluate_features: any K, any Nc, piecewise constant, several states,
    step costs) agrees with the oracle on every case to 1e-12 in cost and final states and 1e-11 of the
    largest gradient entry: the project's gates (1e-10, 1e-8) are reachable by a Taylor implementation;
  * every mutant of the model - controls k >= 2 dropped from the generator or from the gradient or read
    at the wrong step, a second image at K = 1, a slice index off by one, the two knot weights
    transposed, the seed-0 scalar on every item of an ensemble - misses one of the project's gates by a
    factor of 100 on some case.

The cases of the n <= 16 kernel (qocx_action16.hip, tag "small") are held to the same three proofs, the
control mutants also at its own boundaries - k >= 1 (registers / LDS) and k >= 4 (LDS / streamed) -, and its
one final incoherent target of scale 0.7 to a scale mutant.
"""

import numpy as np
import pytest

from tests import action_features as af
from tests import action_model as am
from tests.helpers import rel_err

CASES = [c + (af.LINEAR, af.N) for c in af.CONTROL_COUNTS] + af.INTERPOLATIONS
TABLES = dict(ensemble=af.ensemble, sweep=af.sweep, durations=af.durations)
TABLES.update({"small-ensemble": lambda: af.ensemble("small"), "small-sweep": lambda: af.sweep("small"),
               "small-durations": lambda: af.durations("small"), "small-ensemble-streamed": af.ensemble_streamed})
STARTS = [(v, "one") for v in af.OPTIMISER_STARTS] + [(v, "small") for v in af.OPTIMISER_STARTS]
# the boundaries of qocx_action16.hip, for the mutants that drop or misplace the controls k >= first:
# 1 (registers / LDS) where K > 1, 4 (LDS / streamed) where K > 4
SMALL_FIRSTS = (1, 4)


def case_id(case):
    return "{}-n{}-K{}-S{}-{}-Nc{}".format(*case)


def model(p, controls, **kw):
    return am.evaluate_features(p["h0"], p["g"], p["psi0"], af.oracle_costs(p), af.N, p["T"], controls,
                                p["interpolation"], p["ces"], **kw)


def misses(out, ref):
    """By how much the model's answer misses the project's gates (1e-10, 1e-10, 1e-8): the largest ratio."""
    return max(abs(out["cost"] - ref[0]) / 1e-10, np.abs(out["final"] - ref[2][:, :, 0]).max() / 1e-10,
               rel_err(out["grads"], ref[1]) / 1e-8)


def expanded(p):
    return p.get("expanded", p)


# ---- 1. the inputs ------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_a_case_stays_on_the_route_and_spans_three_degrees(case):
    p = af.build(*case)
    assert abs(am.onp.one_norm(p["h0"]) - 1) < 1e-14 and all(abs(am.onp.one_norm(m) - 1) < 1e-14 for m in p["g"])
    assert p["controls"].shape == (3, case[5], case[2])
    bound = af.host_bound(p)
    assert bound <= 0.9 * am.THETA[18] and bound <= 0.55 + 1e-12, bound
    degrees = set()
    for u in p["controls"]:
        ustep, _ = am.step_controls(u, af.N, p["T"], p["interpolation"])
        degrees |= {am.degree_for(af.DT * (1 + np.sum(np.abs(row)))) for row in ustep}
    assert len(degrees) >= 3 and max(degrees) <= 15, degrees


@pytest.mark.parametrize("name", sorted(TABLES))
def test_a_seed_table_stays_on_the_route_and_spans_three_degrees(name):
    p = TABLES[name]()
    q = expanded(p)
    bound = af.host_bound(q, p["items"])
    assert bound <= 0.9 * am.THETA[18], bound
    gn = np.array([am.onp.one_norm(m) for m in q["g"]])
    degrees = set()
    for r in p["items"]:
        ustep, _ = am.step_controls(r, af.N, p["T"])
        degrees |= {am.degree_for(af.DT * (am.onp.one_norm(q["h0"]) + np.abs(row) @ gn)) for row in ustep}
    assert len(degrees) >= 3, degrees


@pytest.mark.parametrize("variant, kernel", STARTS, ids=[v if k == "one" else k + "-" + v for v, k in STARTS])
def test_an_optimiser_start_stays_on_the_route_and_its_clip_binds(variant, kernel):
    """The bound of the upload and the bound opt_clip commits from its norms (a complex control: both
    channels up to the modulus) are <= 0.9 theta_18, and the loud seed starts outside the norms."""
    p = af.optimiser_start(variant, kernel)
    assert p["kernel"] == kernel and p["n"] == af.TABLE_SIZE[kernel]
    channels = np.repeat(p["max_norms"], 2) if variant == "complex" else p["max_norms"]
    assert p["controls"].shape == (3, p["Nc"], len(channels)) and len(channels) == len(p["g"])
    assert af.host_bound(p) <= 0.9 * am.THETA[18]
    assert af.DT * (1 + np.sum(channels)) <= 0.9 * am.THETA[18]
    if variant == "complex":
        assert np.hypot(p["controls"][..., 0], p["controls"][..., 1]).max() > p["max_norms"][0]
    else:
        assert np.abs(p["controls"]).max() > p["max_norms"].max()
    if variant == "basis":
        assert p["matrix"].shape == (9, 4) and p["coefficients"].shape == (3, 4, 3)
        assert np.linalg.matrix_rank(p["matrix"]) == 4
    u = np.clip(p["controls"][2], -channels, channels)  # (a point inside the norms: the oracle takes it)
    assert_model((variant, 2), model(p, u), af.reference(p, u))


# ---- 2. the model agrees with the oracle ------------------------------------------------------------

def assert_model(tag, out, ref):
    worst = (abs(out["cost"] - ref[0]), np.abs(out["final"] - ref[2][:, :, 0]).max(), rel_err(out["grads"], ref[1]))
    assert worst[0] < 1e-12 and worst[1] < 1e-12 and worst[2] < 1e-11, (tag, worst)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_the_model_agrees_with_the_oracle(case):
    p = af.build(*case)
    for b, ref in enumerate(af.references(p)):
        assert_model((case, b), model(p, p["controls"][b]), ref)


@pytest.mark.parametrize("name", sorted(TABLES))
def test_the_model_agrees_with_the_oracle_on_the_items_of_a_seed_table(name):
    p = TABLES[name]()
    q = expanded(p)
    for i, ref in enumerate(af.item_reference(q, p["items"])):
        assert_model((name, i), model(q, p["items"][i]), ref)


def test_the_piecewise_constant_reference_is_the_central_difference_of_the_slices():
    """The twin-knot reference against Reference A of tests/piecewise_constant.py (the pulse folded into
    a control-free callable, differentiated numerically), where the slices cut the steps: Nc = 3."""
    from tests import piecewise_constant as pc
    p = af.build("one", 17, 3, 1, af.PWC, 3)
    c = p["controls"][1]
    cost, grads, final = af.references(p)[1]
    h = af.hamiltonian(p)
    a = pc.reference_a(h, c, p["T"], p["psi0"][:, :, None], af.N, af.oracle_costs(p))
    assert abs(a[0] - cost) < 1e-13 and np.abs(a[1] - final).max() < 1e-13
    fd = pc.reference_a_gradient(h, c, p["T"], p["psi0"][:, :, None], af.N, af.oracle_costs(p))
    assert rel_err(grads, fd) < 1e-7


# ---- 3. no plausibly wrong kernel could pass ----------------------------------------------------------

def test_no_mutant_passes():
    """A mutant is run on the cases where it can differ; the worst miss of each is >= 100 gates."""
    applies = {
        "generator without k >= 2": lambda c: c[2] > 2,
        "gradient without k >= 2": lambda c: c[2] > 2,
        "wrong step for k >= 2": lambda c: c[2] > 2,
        "second image at K = 1": lambda c: c[2] == 1,
        "slice off by one": lambda c: c[4] == af.PWC,
        "transposed knot weights": lambda c: c[4] == af.LINEAR and c[5] != af.N,
    }
    assert set(applies) == set(am.MUTANTS)
    for mutant, on in applies.items():
        worst, count = 0.0, 0
        for case in CASES:
            if not on(case):
                continue
            p = af.build(*case)
            for b, ref in enumerate(af.references(p)):
                miss = misses(model(p, p["controls"][b], mutant=mutant, ghost=p["ghost"]), ref)
                worst = max(worst, miss)
                count += 1
                # every kernel and every size the mutant applies to catches it at the ordinary seed
                if b == 1:
                    assert miss >= 100, (mutant, case, miss)
        print("{}: {} evaluations, worst miss {:.1e} gates".format(mutant, count, worst))
        assert count and worst >= 100, (mutant, worst)
    # the same three control mutants at the boundaries of the small kernel
    for first in SMALL_FIRSTS:
        for mutant in am.MUTANTS[:3]:
            worst, least, count = 0.0, np.inf, 0
            for case in CASES:
                if case[0] != "small" or case[2] <= first:
                    continue
                p = af.build(*case)
                for b, ref in enumerate(af.references(p)):
                    miss = misses(model(p, p["controls"][b], mutant=mutant, first=first), ref)
                    worst = max(worst, miss)
                    count += 1
                    if b == 1:
                        least = min(least, miss)
                        assert miss >= 100, (mutant, first, case, miss)
            print("{} at first = {}: {} evaluations, worst miss {:.1e} gates, least on an ordinary seed {:.1e}"
                  .format(mutant, first, count, worst, least))
            assert count and worst >= 100, (mutant, first, worst)


def test_transposed_knot_weights_pass_at_one_knot_per_grid_point():
    """Why Nc = N alone could not see them: both weights are 1 / 2 there."""
    p = af.build("one", 17, 3)
    out = model(p, p["controls"][1], mutant="transposed knot weights")
    assert misses(out, af.references(p)[1]) < 1


def test_the_scalar_of_seed_0_on_every_item_of_an_ensemble_cannot_pass():
    """The unit adjoint scales the gradient of item i by its own scalar, lam_scale[i * S]: with that of
    item 0 on every item, the weighted sums of the ensemble miss the gradient gate."""
    p = af.ensemble()
    refs = af.item_reference(p, p["items"])
    kr, M = p["kr"], p["M"]
    scalar0 = model(p, p["items"][0])["scalar"]
    assert scalar0 is not None
    worst = 0.0
    for b in range(p["B"]):
        want = sum(p["weights"][m] * p["scales"][m] * refs[b * M + m][1][:, :kr] for m in range(M))
        right = sum(p["weights"][m] * p["scales"][m] * model(p, p["items"][b * M + m])["grads"][:, :kr]
                    for m in range(M))
        wrong = sum(p["weights"][m] * p["scales"][m]
                    * model(p, p["items"][b * M + m], scalar=scalar0)["grads"][:, :kr] for m in range(M))
        assert rel_err(right, want) < 1e-11
        worst = max(worst, rel_err(wrong, want) / 1e-8)
    assert worst >= 100, worst


# ---- 4. one final incoherent target of scale 0.7 on the small kernel ---------------------------------

@pytest.mark.parametrize("kernel, n", af.INCOHERENT_TARGETS)
def test_the_incoherent_target_stays_on_the_route_and_the_model_agrees(kernel, n):
    p = af.incoherent(kernel, n)
    costs = af.oracle_costs(p)
    assert len(costs) == 1 and costs[0].neglect_relative_pahse and costs[0].cost_multiplier == 0.7
    assert not costs[0].requires_step_evaluation
    assert af.descriptors(p) == [dict(kind=1, step_cost=0, scale=0.7, vectors=p["target"])]
    assert af.host_bound(p) <= 0.9 * am.THETA[18]
    degrees = set()
    for b, ref in enumerate(af.references(p)):
        out = model(p, p["controls"][b])
        degrees |= set(out["degrees"])
        assert_model((kernel, n, b), out, ref)
    assert len(degrees) >= 3, degrees


@pytest.mark.parametrize("kernel, n", af.INCOHERENT_TARGETS)
def test_no_wrong_scalar_of_the_incoherent_target_passes(kernel, n):
    """Two ways to get the scalar of the unit adjoint wrong under an incoherent target at S = 1.
    The coherent scalar, -2 scale sum_s <t_s|psi_s> / S^2, in place of the incoherent one, -2 scale
    <t_s|psi_s> / S: at ONE state the two costs are the same function of the state - the same value and
    the same cotangent -, so this mutant cannot differ and no test at S = 1 can see it; asserted here
    as an equality. The scale mutant - 1 in place of 0.7, in the cost and in the scalar - must miss a gate
    by a factor of 100 on every seed."""
    p = af.incoherent(kernel, n)
    target = p["target"][:, :, None]
    coherent = [am.onp.TargetStateInfidelity(target, cost_multiplier=af.INCOHERENT_SCALE)]
    unscaled = [am.onp.TargetStateInfidelity(target, neglect_relative_pahse=True)]

    def run(costs, u):
        return am.evaluate_features(p["h0"], p["g"], p["psi0"], costs, af.N, p["T"], u, p["interpolation"], 1)

    for b, ref in enumerate(af.references(p)):
        same = misses(run(coherent, p["controls"][b]), ref)
        wrong = misses(run(unscaled, p["controls"][b]), ref)
        print("n={} seed {}: coherent scalar {:.1e} gates, scale 1 {:.1e} gates".format(n, b, same, wrong))
        assert same < 1
        assert wrong >= 100, (n, b, wrong)
