"""
CPU tests (not gpu) of the inputs tests/test_gpu_mixed_steps.py runs on the device: the pulses of
tests/mixed_pulses.py mix Pade orders, squaring counts and pivoting regimes inside one seed and
one upload, stay clear of every decision threshold, and the algorithm the kernels run (order by
norm: tests/device_model.py) agrees with the oracle on them to a tenth of each parity gate - so a
failure on the device at the gates themselves would be the device's.

The conditions are conditions, not measurements: a problem that stops meeting them is repaired in
tests/mixed_pulses.py (seed, amplitudes), not here.
"""

import numpy as np
import pytest

from oracle import qoc_numpy as onp
from tests import device_model as dm
from tests import mixed_pulses as mp

THETA5 = dm.PADE_THETA[5]


def input_failures(p, controls, tabs):
    """The claims of the mixed batch of one problem; returns the list of those that do not hold."""
    bad = []
    # what the algorithm needs (exact norms): every K1a kernel takes the order from the norm of the
    # matrix or from a bound above it
    order = np.concatenate([t["order_exact"] for t in tabs])
    sq = np.concatenate([t["sq_exact"] for t in tabs])
    for m in mp.ORDERS:
        if np.mean(order == m) < 0.05:
            bad.append("order %d at %.3f of the steps" % (m, np.mean(order == m)))
    for s in (0, 1, 2):
        if not np.any(sq == s):
            bad.append("no step with %d squarings" % s)
    by_name = dict(zip(mp.FAMILIES, tabs))
    for name in ("ramp", "bell"):
        for key in ("order_exact", "order_bound") if p["nodes"] == 1 else ("order_exact",):
            if set(by_name[name][key]) != set(mp.ORDERS):
                bad.append("%s: %s has %s" % (name, key, sorted(set(by_name[name][key]))))
    for key in ("dominant_exact", "dominant_bound"):
        if set(by_name["bell"][key]) != {True, False}:
            bad.append("bell: one value of " + key)
    quiet = by_name["quiet"]
    for key in ("exact", "bound") if p["nodes"] == 1 else ("exact",):
        if set(quiet["order_" + key]) != {3, 5}:
            bad.append("quiet: order_%s has %s" % (key, sorted(set(quiet["order_" + key]))))
        if not np.all(quiet["dominant_" + key]):
            bad.append("quiet: a step not dominant by " + key)
    for name, t in by_name.items():
        for key in ("bound", "exact", "sqfree"):
            if mp.near_threshold(t[key]):
                bad.append("%s: a step's %s within 1e-9 of a threshold" % (name, key))
        # the square-root-free norm of the two-wave K1a without a step table (17 <= n <= 32, M4 / M6)
        # never asks for a higher order than the bound
        if 16 < p["n"] <= 32 and p["nodes"] > 1 and np.any(t["order_sqfree"] > t["order_bound"]):
            bad.append("%s: |re| + |im| norm above the bound's order" % name)
        if np.any(t["exact"] > t["bound"] * (1 + 1e-12)):  # (equal where the controls are zero)
            bad.append("%s: the bound is no bound" % name)
    hb = mp.host_bounds(p["h0"], p["g"], controls, p["dt"], p["N"], p["Nc"], p["nodes"])
    if hb["sbound"] > 10:
        bad.append("the upload would be rejected: sbound %d" % hb["sbound"])
    if max(np.max(t["bound"]) for t in tabs) > hb["norm_bound"] * (1 + 1e-12):
        bad.append("a step bound above the host's norm_bound")
    # alone, quiet takes the prefer_low / all_dominant routes; in the batch it does not
    hq = mp.host_bounds(p["h0"], p["g"], controls[:1], p["dt"], p["N"], p["Nc"], p["nodes"])
    if p["nodes"] == 1 and not (hq["norm_bound"] < THETA5 < hb["norm_bound"]):
        bad.append("quiet alone is not below theta_5 / the batch not above")
    if not (mp.pade_eps_max(hq["norm_bound"]) <= mp.DOMINANCE_MARGIN < mp.pade_eps_max(hb["norm_bound"])):
        bad.append("quiet alone is not all_dominant / the batch is")
    return bad


def check_parity(problem, controls, tag, capsys=None):
    """The device model against the oracle at a tenth of each gate; also the final-state norm of a
    non-unitary evolution (above ~10 the relative gates stop meaning what they say)."""
    worst = dict(cost=0.0, states=0.0, grad=0.0, grad_channel=0.0)
    for b in range(len(controls)):
        ref = onp.evaluate_with_grad(problem, controls[b])
        err, gr, fin = mp.model_evaluate_with_grad(problem, controls[b])
        fr = mp.gate_fractions(ref, (err, gr, fin[:, :, 0]))
        for key in worst:
            worst[key] = max(worst[key], fr[key])
        assert np.max(np.linalg.norm(ref[2][:, :, 0], axis=1)) < 10.0, (tag, b)
    print("{}: model/oracle worst/gate {}".format(tag, {k: "%.2e" % v for k, v in worst.items()}))
    for key, value in worst.items():
        assert value <= 0.1, (tag, key, value)


@pytest.mark.parametrize("name", mp.PROBLEM_NAMES)
def test_mixed_batch_mixes_what_it_claims(name):
    p = mp.named_problem(name)
    controls = mp.mixed_controls(p)
    assert input_failures(p, controls, mp.tables(p, controls)) == []


@pytest.mark.parametrize("name", mp.PROBLEM_NAMES)
def test_device_model_matches_oracle_on_mixed_batch(name):
    p = mp.named_problem(name)
    check_parity(p["oracle"], mp.mixed_controls(p), name)


def test_problem_matrix_covers_the_routes():
    specs = list(mp.PROBLEMS.values())
    assert {s["n"] for s in specs} >= {8, 16, 20, 32, 48, 72}
    assert {s["magnus"] for s in specs} == {"M2", "M4", "M6"}
    assert {s["hermitian"] for s in specs} == {True, False}
    assert {s["S"] for s in specs} == {1, 3}
    assert any(s["Nc"] == s["N"] for s in specs) and any(s["Nc"] < s["N"] for s in specs)
    assert all(s["N"] - 1 <= 129 for s in specs)


def test_families_are_what_their_names_say():
    rng = np.random.default_rng(5)
    fam = mp.families(49, 3, 40.0, rng)
    assert set(fam) == set(mp.FAMILIES) and all(v.shape == (49, 3) for v in fam.values())
    assert np.all(fam["bell"][0] == 0) and np.all(fam["bell"][-1] == 0)
    assert np.isclose(np.max(np.abs(fam["bell"])), 40.0)
    assert np.count_nonzero(fam["spike"]) == 2
    assert np.max(fam["spike"]) == 5.0 and np.min(fam["spike"]) == -40.0
    assert np.all(fam["square"][0] == 0) and np.all(fam["square"][-1] == 0)
    assert set(np.unique(fam["square"])) == {-40.0, 0.0, 40.0 / 3}
    r = np.abs(fam["ramp"][:, -1])
    assert np.isclose(r[0], 1e-3) and np.isclose(r[-1], 40.0) and np.allclose(r[1:] / r[:-1], r[1] / r[0])
    assert np.any(fam["ramp"][:, -1] > 0) and np.any(fam["ramp"][:, -1] < 0)
    assert np.max(np.abs(fam["quiet"])) < 0.1


def test_step_table_model_against_the_generators():
    """The model's bound is a bound, its exact norm the oracle's, on a problem of each policy."""
    for name in ("n8_M2_S3_nonherm", "n20_M4_S3_nonherm", "n16_M6_S1"):
        p = mp.named_problem(name)
        u = mp.mixed_controls(p)[4]
        t = mp.step_table(p["h0"], p["g"], u, p["dt"], p["N"], p["Nc"], p["nodes"])
        for step in (0, p["N"] // 2, p["N"] - 2):
            _, cache = onp.evolve_step(p["oracle"], u, p["oracle"].initial_states, step * p["dt"], True)
            a = cache["ecache"]["a"] * 2.0 ** cache["ecache"]["s"]
            assert np.isclose(onp.one_norm(a), t["exact"][step], rtol=1e-12)
            assert cache["ecache"]["s"] == t["sq_exact"][step] or t["order_exact"][step] < 13
        assert np.all(t["exact"] <= t["bound"] * (1 + 1e-12)) and np.all(t["exact"] <= t["sqfree"])


def test_midpoint_problems_sit_where_they_claim():
    mid, counter, plateau = mp.midpoint_problems()
    p, u = mid["p"], mid["u"]
    assert p["hermitian"] and p["magnus"] == "M2" and p["Nc"] == p["N"] and 17 <= p["n"] <= 32
    hb = mp.host_bounds(p["h0"], p["g"], u, p["dt"], p["N"], p["Nc"])
    assert THETA5 < hb["norm_bound"] < 2 * THETA5
    assert hb["norm_bound_mid"] < THETA5
    tabs = mp.tables(p, u)
    assert all(np.all(t["exact"] < THETA5) and np.all(t["bound"] < THETA5) for t in tabs)
    assert not any(mp.near_threshold(t["bound"]) or mp.near_threshold(t["exact"]) for t in tabs)
    check_parity(p["oracle"], u, "midpoint")
    # the counter-problem: a step sits on the spike and needs more than order 5
    p, u = counter["p"], counter["u"]
    assert p["Nc"] < p["N"]
    hb = mp.host_bounds(p["h0"], p["g"], u, p["dt"], p["N"], p["Nc"])
    assert THETA5 < hb["norm_bound"] < 2 * THETA5 and hb["norm_bound_mid"] == 1e300
    tabs = mp.tables(p, u)
    assert all(np.any(t["exact"] > THETA5) for t in tabs)
    assert not any(mp.near_threshold(t["bound"]) or mp.near_threshold(t["exact"]) for t in tabs)
    check_parity(p["oracle"], u, "counter")
    # the plateau: the midpoint bound applies and itself says "above theta_5"
    p, u = plateau["p"], plateau["u"]
    hb = mp.host_bounds(p["h0"], p["g"], u, p["dt"], p["N"], p["Nc"])
    assert THETA5 < hb["norm_bound_mid"] < 2 * THETA5 and hb["norm_bound_mid"] / 2 < THETA5
    tabs = mp.tables(p, u)
    assert all(np.any(t["exact"] > THETA5) for t in tabs)
    check_parity(p["oracle"], u, "plateau")


def test_deep_squaring_problem():
    """A single spike needing mp.DEEP_S = 6 squarings among order-3 steps: the device model stays
    within a tenth of the gates at s = 6, so 6 it is."""
    d = mp.deep_problem()
    p, u = d["p"], d["u"]
    assert p["N"] - 1 <= 17 and p["n"] <= 16
    t = mp.tables(p, u)[0]
    assert np.max(t["sq_exact"]) == mp.DEEP_S and np.max(t["sq_bound"]) == mp.DEEP_S
    assert set(t["order_bound"]) == {3, 13} and set(t["order_exact"]) == {3, 13}
    assert not mp.near_threshold(t["bound"]) and not mp.near_threshold(t["exact"])
    check_parity(p["oracle"], u, "deep")
