"""
GPU tests (-m gpu): pulses that mix Pade orders, squaring counts and pivoting regimes inside one
seed and one upload (tests/mixed_pulses.py; tests/test_mixed_pulses_host.py proves on the CPU that
they do, and that the algorithm itself holds a tenth of the gates on them).

The engine decides per step (step_table_kernel, the K1a kernels) and per upload (norm_bound,
norm_bound_mid, sbound, slot_cap: prefer_low, the three-wave K1a with order_max 5, all_dominant,
pack8) from bounds; a bound too small for some step fails nothing - it costs the 6th to 9th digit.
Every other fixture draws sigma * standard_normal controls, one regime per launch. Here: the six
families in one upload against the oracle (per seed and per control channel), the orders actually
taken between what the norms allow and what the bounds demand, the midpoint bound and its
counter-problems, a seed alone against the same seed in the batch (other routes), chunks and time
segments, the resident (clipped) route, and six squarings inside an order-3 pulse.
Gates: cost and states 1e-10 relative, gradient 1e-8. Run with -s for worst/gate.
"""

import numpy as np
import pytest

from oracle import qoc_numpy as onp
from tests import device_model as dm
from tests import mixed_pulses as mp

pytestmark = pytest.mark.gpu

THETA5 = dm.PADE_THETA[5]
QUIET, LOUD, SQUARE = (mp.FAMILIES.index(name) for name in ("quiet", "loud", "square"))


@pytest.fixture(scope="module")
def engine():
    from qoc_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


_problems, _oracle = {}, {}


def mixed(name):
    """(problem, controls, per-seed oracle results) of a named problem, computed once."""
    if name not in _problems:
        p = mp.named_problem(name)
        u = mp.mixed_controls(p)
        _problems[name] = (p, u)
        _oracle[name] = [onp.evaluate_with_grad(p["oracle"], u[b]) for b in range(len(u))]
    return _problems[name] + (_oracle[name],)


def assert_parity(tag, refs, out, seeds=None):
    """out = (cost[B], grads[B], final[B]) against the oracle's refs, seed by seed."""
    worst = dict(cost=0.0, states=0.0, grad=0.0, grad_channel=0.0)
    fails = []
    for b, ref in enumerate(refs):
        fr = mp.gate_fractions(ref, (out[0][b], out[1][b], out[2][b]))
        for key, value in fr.items():
            worst[key] = max(worst[key], value)
            if not value < 1.0:
                fails.append((b if seeds is None else seeds[b], key, value))
    print("{}: worst/gate {}".format(tag, " ".join("%s=%.2e" % kv for kv in worst.items())))
    assert not fails, (tag, fails)


def assert_close(a, b, tag):
    """cost, gradient and final state to 1e-12 max(1, max|.|): other kernels, other summation order."""
    for x, y, what in zip(a, b, ("cost", "grads", "final")):
        assert np.abs(x - y).max() <= 1e-12 * max(1.0, np.abs(y).max()), (tag, what, np.abs(x - y).max())


def assert_identical(a, b, tag):
    for x, y in zip(a, b):
        assert np.array_equal(x, y), tag


# ---- a. parity of the mixed batch ----------------------------------------------------------------------

@pytest.mark.parametrize("pade_order", [0, 13])
@pytest.mark.parametrize("name", mp.PROBLEM_NAMES)
def test_mixed_batch_against_oracle(engine, name, pade_order):
    """All six families in one upload, order by norm and always [13/13], at the parity gates; the
    gradient per seed and per control channel (a wrong quiet channel must not hide behind a loud one)."""
    p, u, refs = mixed(name)
    mp.set_engine_problem(engine, p)
    engine.set_knob("pade_order", pade_order)
    try:
        out = engine.evaluate(u, True)
        orders = engine.pade_orders()
    finally:
        engine.set_knob("pade_order", 0)
    assert sum(orders.values()) == len(u) * (p["N"] - 1)
    assert pade_order == 0 or orders[13] == sum(orders.values())
    assert_parity("{} pade_order={}".format(name, pade_order), refs, out)


# ---- b. orders actually taken ----------------------------------------------------------------------------

@pytest.mark.parametrize("name", mp.PROBLEM_NAMES)
def test_orders_between_norm_and_bound(engine, name):
    """Never a lower order than the norm allows, never a higher one than the bound demands (what
    check_pade_factor of test_gpu_engine.py asserts per matrix), counted over the batch; the quiet
    seed alone stays on orders 3 and 5 and on the diagonal-pivot factorisation."""
    p, u, _ = mixed(name)
    tabs = mp.tables(p, u)
    mp.set_engine_problem(engine, p)
    engine.evaluate(u, True)
    orders = engine.pade_orders()
    assert sum(orders.values()) == len(u) * (p["N"] - 1)
    exact = np.concatenate([t["order_exact"] for t in tabs])
    bound = np.concatenate([t["order_bound"] for t in tabs])
    for m in (5, 7, 9, 13):
        taken = sum(count for order, count in orders.items() if order >= m)
        print("{}: order >= {}: norm {} <= taken {} <= bound {}".format(
            name, m, int(np.sum(exact >= m)), taken, int(np.sum(bound >= m))))
        assert np.sum(exact >= m) <= taken <= np.sum(bound >= m), (m, orders)
        # M2, where check_pade_factor names the source of the order: the step table's bound for the
        # two-wave K1a (17 <= n <= 32), the norm of the matrix everywhere else
        if p["nodes"] == 1:
            assert taken == np.sum((bound if 16 < p["n"] <= 32 else exact) >= m), (m, orders)
    engine.evaluate(u[QUIET:QUIET + 1], True)
    orders = engine.pade_orders()
    assert orders[7] == orders[9] == orders[13] == 0 and orders[3] + orders[5] == p["N"] - 1
    if p["nodes"] == 1:  # (by the norm or by the step table: both say 3 and 5)
        assert orders[3] > 0 and orders[5] > 0
    assert engine.lu_fallbacks() == 0


# ---- c. the bound at the step midpoints ------------------------------------------------------------------

def test_midpoint_bound_route(engine):
    """
    Nc == N, single-knot spikes: the knot bound exceeds theta_5, norm_bound_mid does not, and the
    three-wave K1a (orders 3 and 5 only, order_max = 5) is taken on its strength. Against the
    two-wave kernel with the checked factorisation to 1e-12 (the gate of
    test_three_wave_pade_kernel_equals_two_wave_kernel), both at the gates of the oracle.
    """
    d = mp.midpoint_problems()[0]
    p, u = d["p"], d["u"]
    refs = [onp.evaluate_with_grad(p["oracle"], ub) for ub in u]
    mp.set_engine_problem(engine, p)
    try:
        engine.set_knob("k1a_three", 1)
        three = engine.evaluate(u, True)
        orders = engine.pade_orders()
        engine.set_knob("k1a_three", 0)
        engine.set_knob("lu_dpp", 0)
        two = engine.evaluate(u, True)
        assert engine.pade_orders() == orders
    finally:
        engine.set_knob("k1a_three", 1)
        engine.set_knob("lu_dpp", 1)
    assert orders[3] > 0 and orders[5] > 0 and orders[7] == orders[9] == orders[13] == 0
    assert abs(three[0] - two[0]).max() <= 1e-12
    assert np.abs(three[1] - two[1]).max() <= 1e-12 * max(1.0, np.abs(two[1]).max())
    assert np.abs(three[2] - two[2]).max() <= 1e-12
    assert_parity("midpoint three-wave", refs, three)
    assert_parity("midpoint two-wave", refs, two)


@pytest.mark.parametrize("which", ["counter", "plateau"])
def test_midpoint_bound_counter_problems(engine, which):
    """
    counter: the same spikes with Nc < N, a step sits on each spike and needs order 7 - no midpoint
    bound applies. plateau: Nc == N, the spike two knots wide - the midpoint bound applies and is
    itself above theta_5. Either way a too-optimistic order_max = 5 would run these steps at order 5.
    """
    d = mp.midpoint_problems()[1 if which == "counter" else 2]
    p, u = d["p"], d["u"]
    tabs = mp.tables(p, u)
    need = int(sum(np.sum(t["order_exact"] >= 7) for t in tabs))
    assert need >= len(u)
    refs = [onp.evaluate_with_grad(p["oracle"], ub) for ub in u]
    mp.set_engine_problem(engine, p)
    out = engine.evaluate(u, True)
    orders = engine.pade_orders()
    assert orders[7] + orders[9] + orders[13] >= need, orders
    assert_parity(which, refs, out)


# ---- d. a seed does not depend on its batch ---------------------------------------------------------------

@pytest.mark.parametrize("name", mp.PROBLEM_NAMES)
def test_seed_alone_equals_seed_in_batch(engine, name):
    """Alone, quiet takes the prefer_low, all_dominant and pack8 routes; beside loud it does not."""
    p, u, _ = mixed(name)
    mp.set_engine_problem(engine, p)
    batch = engine.evaluate(u, True)
    assert_identical(batch, engine.evaluate(u, True), "the same batch twice")
    for b, family in enumerate(mp.FAMILIES):
        alone = engine.evaluate(u[b:b + 1], True)
        assert_close(alone, [x[b:b + 1] for x in batch], family + " alone")
    for pair in ((QUIET, LOUD), (LOUD, QUIET)):
        out = engine.evaluate(u[list(pair)], True)
        assert_close(out, [x[list(pair)] for x in batch], "quiet and loud %s" % (pair,))


# ---- e. chunks and time segments ---------------------------------------------------------------------------

def check_chunks_and_segments(engine, u, tag):
    ref = engine.evaluate(u, True)
    try:
        for chunk in (1, 4):
            engine.set_chunk(chunk)
            assert_identical(ref, engine.evaluate(u, True), (tag, "chunk", chunk))
        engine.set_chunk(0)
        for pipe in (1, 2, 3):
            engine.set_pipeline(pipe)
            assert_identical(ref, engine.evaluate(u, True), (tag, "pipeline", pipe))
    finally:
        engine.set_chunk(0)
        engine.set_pipeline(0)
    return ref


@pytest.mark.parametrize("name", mp.PROBLEM_NAMES)
def test_chunks_and_segments_of_the_mixed_batch(engine, name):
    """Sub-step slots of unequal occupancy across chunk and time-segment boundaries: bit for bit the
    default evaluation (as test_chunked_equals_unchunked and test_multi_state_sweep_segments ask)."""
    p, u, _ = mixed(name)
    mp.set_engine_problem(engine, p)
    check_chunks_and_segments(engine, u, name)


# ---- f. the resident route -----------------------------------------------------------------------------------

@pytest.mark.parametrize("name", mp.PROBLEM_NAMES)
def test_resident_route_after_clip(engine, name):
    """
    opt_clip raises norm_bound (and the slot layout) behind the upload from the clip bound alone: the
    quiet seed under a clip bound above theta_13 equals its plain evaluation; the mixed batch clipped
    on the device equals the evaluation of the controls clipped on the host.
    """
    from qoc_amd.engine import host_clip_controls
    p, u, refs = mixed(name)
    gn = np.array([onp.one_norm(m) for m in p["g"]])
    mp.set_engine_problem(engine, p)
    quiet = u[QUIET:QUIET + 1]
    plain = engine.evaluate(quiet, True)
    # sum_k norms_k ||G_k||_1 dt = 1.2 theta_13 (and quiet far below every norms_k)
    norms = 1.2 * onp.THETA_13 / (p["dt"] * gn * p["K"])
    assert np.all(np.abs(quiet) < 0.1 * norms)
    engine.upload_controls(quiet)
    engine.opt_begin()
    engine.opt_clip(norms)
    engine.eval_resident(True)
    out = engine.download_results(True)
    assert_close(out, plain, "quiet under a wide clip")
    assert_parity(name + " resident quiet", refs[QUIET:QUIET + 1], out)
    # norms that cut loud and square but not quiet
    norms = np.full(p["K"], 0.25 * p["amp_hi"])
    clipped = np.ascontiguousarray(u.copy())
    host_clip_controls(clipped, norms)
    assert np.array_equal(clipped[QUIET], u[QUIET])
    assert not np.array_equal(clipped[LOUD], u[LOUD]) and not np.array_equal(clipped[SQUARE], u[SQUARE])
    ref = engine.evaluate(clipped, True)
    engine.upload_controls(u)
    engine.opt_begin()
    engine.opt_clip(norms)
    engine.eval_resident(True)
    assert_close(engine.download_results(True), ref, "mixed batch clipped on the device")


# ---- g. deep squaring inside a quiet pulse ----------------------------------------------------------------------

def test_deep_squaring_inside_quiet_pulse(engine):
    """One seed, 16 steps at n = 8: order-3 steps around a spike whose two steps need s = 6 squarings
    (tests/test_mixed_pulses_host.py: the device model holds a tenth of the gates at s = 6). Oracle
    parity, and chunks / time segments bit for bit."""
    d = mp.deep_problem()
    p, u = d["p"], d["u"]
    refs = [onp.evaluate_with_grad(p["oracle"], u[0])]
    mp.set_engine_problem(engine, p)
    out = check_chunks_and_segments(engine, u, "deep")
    orders = engine.pade_orders()
    assert orders[13] == 2 and orders[3] == p["N"] - 3, orders
    assert_parity("deep s=%d" % mp.DEEP_S, refs, out)


# ---- fuzz ----------------------------------------------------------------------------------------------------------

def test_random_shapes_fuzz_with_pulse_shapes(engine):
    """tests/fuzz_parity.py with shapes=True: 40 random problems whose two seeds each take a pulse
    family and an amplitude of their own, against the oracle at the parity tolerances."""
    from tests import fuzz_parity
    rng = np.random.default_rng(4040)
    checked, overall = 0, 0.0
    for index in range(40):
        worst, tag = fuzz_parity.one(engine, rng, index, shapes=True)
        if worst is None:  # more than 2^10 squarings per step: rejected by design
            continue
        checked += 1
        overall = max(overall, worst)
        assert worst <= 1.0, tag
    print("fuzz with shapes: {} of 40 checked, worst/gate {:.2e}".format(checked, overall))
    # (the host's capacity rule, restated in mixed_pulses.host_bounds, admits all 40 draws of this seed,
    # one of them at exactly 2^10)
    assert checked >= 39
