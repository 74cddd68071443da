"""
GPU tests (-m gpu): drive operators G_k(t) that depend on time (tests/time_dependent_drive.py), on
every kernel route that reads the time-indexed g tables - K1a generator assembly (one wave, pack8,
two / sixteen tiles, the general path), the gradient contraction K3 in its forms, the Magnus node
generators and their cotangents, the augmented tables of quadratic terms and ensembles - against the
oracle on the callable H(u, t). tests/test_time_dependent_drive_host.py proves on the CPU that a
table read at a wrong time (frozen, a step late, nodes swapped, in the gradient alone) moves the
oracle's numbers by >= 1e-3 relative on every problem run here.
Gates: cost and states 1e-10 relative, gradient 1e-8. Run with -s for worst/gate.
Every batch holds a quiet seed (bound below theta_5) and a loud one, and every seed is also evaluated
alone: the routes an upload takes (pack8, the three-wave K1a, the dominant-diagonal factorisation)
follow from its largest bound.
"""

import numpy as np
import pytest

from oracle import qoc_numpy as onp
from tests import time_dependent_drive as tdd

pytestmark = pytest.mark.gpu

KNOB_DEFAULTS = dict(pack8=1, k1a_three=1, k1a_herm4=1, general_skew=1, latency=0, sweep_umode=1,
                     sweep_impl=1, sweep_dense=1, magnus_4w=1, pade_order=0)


@pytest.fixture(scope="module")
def engine():
    from qoc_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


_cache = {}


def problem(name, hermitian=True, costs="general", B=2):
    """(problem, controls, per-seed oracle results), computed once."""
    key = (name, hermitian, costs, B)
    if key not in _cache:
        p = tdd.configured(name, hermitian, costs)
        u = tdd.config_controls(p, B)
        _cache[key] = (p, u, [onp.evaluate_with_grad(p["oracle"], ub) for ub in u])
    return _cache[key]


def assert_parity(tag, refs, out):
    """out = (cost[B], grads[B], final[B]) against the oracle's refs, seed by seed."""
    worst, fails = dict(cost=0.0, states=0.0, grad=0.0), []
    for b, ref in enumerate(refs):
        for key, value in tdd.gate_fractions(ref, (out[0][b], out[1][b], out[2][b])).items():
            worst[key] = max(worst[key], value)
            if not value < 1.0:
                fails.append((b, key, value))
    print("{}: worst/gate {}".format(tag, " ".join("%s=%.2e" % kv for kv in worst.items())))
    assert not fails, (tag, fails)


def assert_identical(a, b, tag):
    for x, y in zip(a, b):
        assert np.array_equal(x, y), tag


class knobs(object):
    def __init__(self, engine, values):
        self.engine, self.values = engine, values

    def __enter__(self):
        for name, value in self.values.items():
            self.engine.set_knob(name, value)

    def __exit__(self, *exc):
        for name in self.values:
            self.engine.set_knob(name, KNOB_DEFAULTS[name])


def run_route(engine, name, hermitian, costs, settings, check_orders=None):
    """The batch and every seed alone (with latency = 1: one control set at a time only), order by
    norm and always [13/13], under each knob setting, at the gates."""
    p, u, refs = problem(name, hermitian, costs)
    steps = p["N"] - 1
    for setting in settings:
        for pade_order in (0, 13):
            tag = "{} herm={} {} {} pade_order={}".format(name, hermitian, costs, setting, pade_order)
            with knobs(engine, dict(setting, pade_order=pade_order)):
                tdd.set_engine_problem(engine, p)
                if not setting.get("latency"):
                    out = engine.evaluate(u, True)
                    orders = engine.pade_orders()
                    assert sum(orders.values()) == len(u) * steps
                    assert pade_order == 0 or orders[13] == len(u) * steps
                    assert_parity(tag, refs, out)
                    if check_orders and pade_order == 0:
                        check_orders(orders, None)
                for b in range(len(u)):
                    alone = engine.evaluate(u[b:b + 1], True)
                    orders = engine.pade_orders()
                    assert sum(orders.values()) == steps
                    assert_parity(tag + " seed %d alone" % b, refs[b:b + 1], alone)
                    if check_orders and pade_order == 0:
                        check_orders(orders, b)


# ---- routes at M2 -----------------------------------------------------------------------------------------

def two_tile_orders(orders, seed):
    """The quiet seed alone stays on orders 3 / 5 (the three-wave K1a with order_max = 5 where the knob
    allows it), the loud one and the batch need 7 and more (the two-wave kernel)."""
    high = orders[7] + orders[9] + orders[13]
    if seed == 0:
        assert high == 0 and orders[3] + orders[5] > 0, orders
    else:
        assert high > 0, orders


ROUTES = (
    [("wave_n%d" % n, [{}], None) for n in (1, 5, 16)]
    + [(name, [dict(pack8=1), dict(pack8=0)], None)
       for name in ("pack8_n8_N6", "pack8_n8_N7", "pack8_n3_N6", "pack8_n3_N7")]
    + [("two_n%d" % n, [dict(k1a_three=1), dict(k1a_three=0)], two_tile_orders) for n in (17, 20, 32)]
    + [("four_n%d" % n, [dict(k1a_herm4=1), dict(k1a_herm4=0)], None) for n in (33, 40, 64)]
    + [("general_n%d" % n, [dict(general_skew=1), dict(general_skew=0)], None) for n in (66, 72)]
    + [("general_n40_S20", [{}], None),
       ("sweep_n24", [dict(latency=1, sweep_umode=1), dict(latency=1, sweep_umode=0),
                      dict(sweep_impl=3)], None),
       ("dense_n24_S8", [dict(sweep_dense=1), dict(sweep_dense=0)], None),
       ("edge_K1", [{}], None), ("edge_K8", [{}], None), ("edge_Nc2", [{}], None),
       ("edge_Nc_above_N", [{}], None)])


@pytest.mark.parametrize("hermitian, costs", tdd.VARIANTS,
                         ids=["%s_%s" % ("herm" if h else "nonherm", c) for h, c in tdd.VARIANTS])
@pytest.mark.parametrize("name, settings, check_orders", ROUTES, ids=[r[0] for r in ROUTES])
def test_m2_routes_against_oracle(engine, name, settings, check_orders, hermitian, costs):
    run_route(engine, name, hermitian, costs, settings, check_orders)


# ---- Magnus M4 / M6: the node generators [step][node] and their cotangents ------------------------------------

MAGNUS = [("%s_n%d" % (policy, n), [dict(magnus_4w=1), dict(magnus_4w=0)] if n == 20 else [{}])
          for policy in ("M4", "M6") for n in (6, 20, 40, 70)]


@pytest.mark.parametrize("hermitian, costs", [(True, "general"), (False, "final")],
                         ids=["herm_general", "nonherm_final"])
@pytest.mark.parametrize("name, settings", MAGNUS, ids=[m[0] for m in MAGNUS])
def test_magnus_routes_against_oracle(engine, name, settings, hermitian, costs):
    """K = 3 (K = 1 at n = 40); the tables are time dependent, so M4 never runs as a linear system."""
    run_route(engine, name, hermitian, costs, settings)


# ---- pipeline and batching ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [8, 24, 40, 72])
def test_chunks_segments_and_batch_independence(engine, n):
    """N = 14, three seeds: memory chunks of one seed and 1 / 3 / 6 time segments (n <= 64: the general
    path has no time segments), and the loudest seed alone, bit for bit the default evaluation of the
    batch - which is at the gates."""
    p, u, refs = problem("pipe_n%d" % n, False, "general", B=3)
    tdd.set_engine_problem(engine, p)
    ref = engine.evaluate(u, True)
    assert_parity("pipe_n%d" % n, refs, ref)
    try:
        engine.set_chunk(1)
        assert_identical(ref, engine.evaluate(u, True), ("chunk", 1))
        engine.set_chunk(0)
        for pipe in ((1, 3, 6) if n <= 64 else ()):
            engine.set_pipeline(pipe)
            assert_identical(ref, engine.evaluate(u, True), ("pipeline", pipe))
    finally:
        engine.set_chunk(0)
        engine.set_pipeline(0)
    alone = engine.evaluate(u[1:2], True)
    assert_identical(alone, [x[1:2] for x in ref], "seed 1 alone")


@pytest.mark.parametrize("n", [8, 24, 40])
def test_resident_route_after_clip(engine, n):
    """opt_clip + eval_resident against the evaluation of the controls clipped on the host, bit for
    bit. opt_clip bounds the step generators from the clip norms alone and keeps the larger of that and
    the upload's bound; tdd.clip_controls makes the three coincide (one knot of a seed sits at the
    norms in every channel, no knot sum exceeds them), so both sides decide every route alike - where
    the bounds differ the suite asks 1e-12 (test_gpu_mixed_steps.py::test_resident_route_after_clip)."""
    from qoc_amd.engine import host_clip_controls
    p = tdd.configured("pipe_n%d" % n, False, "general")
    norms, u = tdd.clip_controls(p)
    clipped = np.ascontiguousarray(u.copy())
    host_clip_controls(clipped, norms)
    assert np.array_equal(clipped[0], u[0])
    for b in (1, 2):
        assert np.array_equal(clipped[b, 0], u[b, 0]) and np.all(np.abs(u[b, 0]) == norms)
        assert np.all(np.sum(np.abs(clipped[b]) != np.abs(u[b]), axis=1)[1:] == 1)
        assert np.all(np.max(np.abs(clipped[b]) / norms, axis=0) == 1.0)
    tdd.set_engine_problem(engine, p)
    ref = engine.evaluate(clipped, True)
    assert_parity("clipped n=%d" % n, [onp.evaluate_with_grad(p["oracle"], c) for c in clipped], ref)
    engine.upload_controls(u)
    engine.opt_begin()
    engine.opt_clip(norms)
    engine.eval_resident(True)
    assert_identical(engine.download_results(True), ref, "clipped on the device")


# ---- norms that vary with time ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [20, 40])
def test_growing_envelope(engine, n):
    """G_k(t) grows 20-fold over the pulse: the host's bounds take the largest sample of ||G_k(t)||_1,
    the loud seed's last steps need squarings and its first ones none (test_time_dependent_drive_host.py)
    - no QOCX_ERR_CAPACITY, at least two orders in the call, results at the gates."""
    for hermitian in (True, False):
        p, u, refs = problem("envelope_n%d" % n, hermitian, "general")
        for pade_order in (0, 13):
            with knobs(engine, dict(pade_order=pade_order)):
                tdd.set_engine_problem(engine, p)
                out = engine.evaluate(u, True)
                orders = engine.pade_orders()
                assert_parity("envelope n=%d herm=%s pade_order=%d" % (n, hermitian, pade_order), refs, out)
                if pade_order == 0:
                    assert sum(1 for count in orders.values() if count) >= 2, orders
                    assert orders[13] > 0, orders
                for b in range(2):
                    assert_parity("envelope n=%d seed %d alone" % (n, b), refs[b:b + 1],
                                  engine.evaluate(u[b:b + 1], True))


# ---- quadratic terms and ensembles: the augmented tables [nt][G_0 .. G_K-1, Q_0 ..] ------------------------------------

def augmented_problem(n, ensemble):
    """K_r = 3 seed channels (+ J = 2 perturbation channels D_j(t), rotating like the G_k), M2."""
    key = ("augmented", n, ensemble)
    if key not in _cache:
        p = tdd.configured(("ensemble_n%d" if ensemble else "quadratic_n%d") % n)
        _cache[key] = (p, tdd.controls(p, 2, channels=3))
    return _cache[key]


@pytest.mark.parametrize("n", [24, 72])
def test_quadratic_terms_on_time_dependent_tables(engine, n):
    """H_lin(u, t) + sum_q r_k r_l Q_q with two terms: qocx_set_quadratic_terms interleaves the Q_q
    into every time row of the three g images."""
    p, u = augmented_problem(n, False)
    quad = tdd.quadratic_terms(p)
    refs = [onp.evaluate_with_grad(tdd.member_oracle(p, ub, quad), ub) for ub in u]
    plain = [onp.evaluate_with_grad(p["oracle"], ub) for ub in u]
    assert abs(refs[1][0] - plain[1][0]) > 1e-4  # the terms matter
    tdd.set_engine_problem(engine, p)
    engine.set_quadratic_terms(*quad)
    assert_parity("quadratic n=%d" % n, refs, engine.evaluate(u, True))
    for b in range(2):
        assert_parity("quadratic n=%d seed %d alone" % (n, b), refs[b:b + 1], engine.evaluate(u[b:b + 1], True))
    engine.set_quadratic_terms(np.zeros((0, 2)), None)  # cleared: the linear problem again
    assert_parity("quadratic terms cleared n=%d" % n, plain, engine.evaluate(u, True))


def check_ensemble(engine, p, u, quad, ens, tag):
    scales, offsets, weights = ens
    out = engine.evaluate(u, True)
    members = engine.ensemble_member_costs()
    B, M = len(u), len(weights)
    assert members.shape == (B, M) and out[2].shape == (B, M, p["S"], p["n"])
    for b in range(B):
        refs = [onp.evaluate_with_grad(tdd.member_oracle(p, u[b], quad, scales[m], offsets[m]), u[b])
                for m in range(M)]
        fr = dict(cost=0.0, states=0.0)
        for m, (err, _, fin) in enumerate(refs):  # every member against the oracle of that member
            fr["cost"] = max(fr["cost"], abs(err - members[b, m]) / max(1.0, abs(err)) / 1e-10)
            fr["states"] = max(fr["states"], np.max(np.abs(fin[:, :, 0] - out[2][b, m]))
                               / np.max(np.abs(fin)) / 1e-10)
        want = sum(weights[m] * members[b, m] for m in range(M))  # the reduction, in member order
        assert abs(out[0][b] - want) <= 1e-14 * abs(want)
        grad = sum(weights[m] * refs[m][1] for m in range(M))
        fr["grad"] = np.max(np.abs(grad - out[1][b])) / max(np.max(np.abs(grad)), 1e-3) / 1e-8
        print("{} seed {}: worst/gate {}".format(tag, b, " ".join("%s=%.2e" % kv for kv in fr.items())))
        assert all(v < 1.0 for v in fr.values()), (tag, b, fr)


@pytest.mark.parametrize("n", [24, 72])
def test_ensemble_on_time_dependent_tables(engine, n):
    """M = 3 members, J = 2 perturbation channels D_j(t) that vary in time as the G_k do."""
    p, u = augmented_problem(n, True)
    ens = tdd.ensemble_of(p)
    tdd.set_engine_problem(engine, p)
    engine.set_ensemble(*ens)
    check_ensemble(engine, p, u, None, ens, "ensemble n=%d" % n)


@pytest.mark.parametrize("order", ["quadratic_first", "ensemble_first"])
def test_ensemble_with_quadratic_terms_on_time_dependent_tables(engine, order):
    p, u = augmented_problem(24, True)
    ens, quad = tdd.ensemble_of(p), tdd.quadratic_terms(p)
    tdd.set_engine_problem(engine, p)
    if order == "quadratic_first":
        engine.set_quadratic_terms(*quad)
        engine.set_ensemble(*ens)
    else:
        engine.set_ensemble(*ens)
        engine.set_quadratic_terms(*quad)
    check_ensemble(engine, p, u, quad, ens, "ensemble + quadratic, " + order)


# ---- fuzz ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nmin, nmax, count, seed", [(1, 32, 12, 3201), (33, 64, 4, 6433), (65, 100, 3, 10065)])
def test_random_shapes_fuzz_with_time_dependent_drive(engine, nmin, nmax, count, seed):
    """tests/fuzz_parity.py with drive=True: random shapes, grids, Magnus policies and time steps, every
    draw with G_k(t) rotating at its own frequency, against the oracle at the parity tolerances."""
    from tests import fuzz_parity
    rng = np.random.default_rng(seed)
    checked, overall = 0, 0.0
    for index in range(count):
        worst, tag = fuzz_parity.one(engine, rng, index, nmin=nmin, nmax=nmax, drive=True)
        if worst is None:  # more than 2^10 squarings per step: rejected by design
            continue
        checked += 1
        overall = max(overall, worst)
        assert worst <= 1.0, tag
    print("fuzz with drive, n in {}..{}: {} of {} checked, worst/gate {:.2e}".format(
        nmin, nmax, checked, count, overall))
    assert checked >= count - 1


# ---- the host API: probe_hamiltonian's tables through the entry points ----------------------------------------------

def api_problems():
    """name: (hamiltonian, initial_states, target_states, K, Nc, N, T, complex_controls, start controls
    (3, Nc, K)). A two-level system driven in a frame that rotates against the drive,
    u (s- e^{i w t} + h.c.), with a real and with a complex control, and n = 24 from the builder."""
    from qoc_amd.standard import get_annihilation_operator, get_creation_operator
    a, ad = get_annihilation_operator(2), get_creation_operator(2)
    h_sys = 0.35 * np.matmul(ad, a)
    N, Nc, T, w = 11, 6, 4.0, 1.9  # dt = 0.4, w dt = 0.76
    zero, one = np.array([[[1], [0]]], dtype=np.complex128), np.array([[[0], [1]]], dtype=np.complex128)
    rng = np.random.default_rng(2222)

    def real_drive(u, t):
        return h_sys + u[0] * (np.exp(1j * w * t) * a + np.exp(-1j * w * t) * ad)

    def complex_drive(u, t):
        return h_sys + u[0] * np.exp(1j * w * t) * a + np.conjugate(u[0]) * np.exp(-1j * w * t) * ad

    p = tdd.drive_problem(24, 9, 6, 2, 2, costs="final", seed=5)
    u24 = tdd.controls(p, 3, loud=1.5)
    return {
        "two_level_real": (real_drive, zero, one, 1, Nc, N, T, False,
                           0.4 * rng.standard_normal((3, Nc, 1))),
        "two_level_complex": (complex_drive, zero, one, 1, Nc, N, T, True,
                              0.4 * (rng.standard_normal((3, Nc, 1)) + 1j * rng.standard_normal((3, Nc, 1)))),
        "n24": (p["hamiltonian"], p["init"][:, :, None], p["descs"][0]["vectors"][:, :, None], 2, 6, 9,
                p["T"], False, u24)}


@pytest.mark.parametrize("name", ["two_level_real", "two_level_complex", "n24"])
def test_entry_points_against_the_oracle_backend(name):
    """evolve_schroedinger_discrete, three iterations of grape_schroedinger_discrete and of
    grape_schroedinger_discrete_batch (B = 3, Adam: the resident route) on the device against the same
    runs on tests/oracle_backend.py, at the trajectory tolerances of tests/test_gpu_api.py."""
    import qoc_amd
    from qoc_amd.core import batch as batch_mod
    from qoc_amd.standard import Adam, TargetStateInfidelity
    from tests import helpers
    from tests.helpers import rel_err
    from tests.oracle_backend import OracleBackend
    hamiltonian, init, target, K, Nc, N, T, cplx, u0 = api_problems()[name]
    norms = np.full(K, 1.5 * np.max(np.abs(u0)))
    taken = []

    def runs():
        costs = [TargetStateInfidelity(target)]
        evolved = [qoc_amd.evolve_schroedinger_discrete(T, hamiltonian, init, N, controls=u, costs=costs)
                   for u in u0[:2]]
        trace = []

        class Recorder(object):
            def __init__(self, inner):
                self.inner = inner

            def run(self, function, iteration_count, initial_params, jacobian, args=()):
                def jac(params, *a):
                    grads, stop = jacobian(params, *a)
                    trace.append((a[1].error, grads.copy()))
                    return grads, stop
                return self.inner.run(function, iteration_count, initial_params, jac, args=args)

        single = qoc_amd.grape_schroedinger_discrete(
            K, Nc, costs, T, hamiltonian, init, N, complex_controls=cplx, initial_controls=u0[1].copy(),
            iteration_count=3, log_iteration_step=0, optimizer=Recorder(Adam(learning_rate=2e-2)),
            max_control_norms=norms)
        resident = batch_mod.run_batch_resident

        def counted(*a, **k):
            taken.append("resident")
            return resident(*a, **k)
        batch_mod.run_batch_resident = counted
        try:
            batch = qoc_amd.grape_schroedinger_discrete_batch(
                K, Nc, costs, T, hamiltonian, init, N, u0.copy(), complex_controls=cplx, iteration_count=3,
                log_iteration_step=0, optimizer=Adam(learning_rate=2e-2), max_control_norms=norms)
        finally:
            batch_mod.run_batch_resident = resident
        return evolved, single, trace, batch

    helpers.set_backend_factory(None)
    gpu = runs()
    assert taken == ["resident"]
    helpers.set_backend_factory(OracleBackend)
    try:
        cpu = runs()
    finally:
        helpers.set_backend_factory(None)
    assert taken == ["resident"]  # the oracle backend takes the host loop
    for g, c in zip(gpu[0], cpu[0]):
        assert abs(g.error - c.error) < 1e-10 * max(1, abs(c.error))
        assert rel_err(g.final_states, c.final_states) < 1e-10
    assert len(gpu[2]) == len(cpu[2]) == 3
    for (ge, gg), (ce, cg) in zip(gpu[2], cpu[2]):
        assert abs(ge - ce) < 1e-9 * max(1, abs(ce))
        assert rel_err(gg, cg) < 1e-7
    assert gpu[1].best_iteration == cpu[1].best_iteration
    assert rel_err(gpu[1].best_controls, cpu[1].best_controls) < 1e-7
    assert np.array_equal(gpu[3].best_iteration, cpu[3].best_iteration)
    for s in range(3):
        assert abs(gpu[3].best_error[s] - cpu[3].best_error[s]) < 1e-9 * max(1, abs(cpu[3].best_error[s]))
        assert rel_err(gpu[3].best_controls[s], cpu[3].best_controls[s]) < 1e-7
    # the rotation matters: the drive frozen at t = 0 evolves elsewhere
    frozen = qoc_amd.evolve_schroedinger_discrete(T, lambda u, t: hamiltonian(u, 0.0), init, N, controls=u0[1],
                                                  costs=[TargetStateInfidelity(target)])
    assert rel_err(frozen.final_states, gpu[0][1].final_states) > 1e-3


# ---- the tests bite -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["pack8_n8_N7", "two_n20", "four_n40", "general_n72", "M4_n20", "M6_n70"])
def test_a_table_read_at_the_wrong_time_is_seen(engine, name):
    """The engine handed a g table frozen at its first sample, or one step late, against the oracle
    of the true problem: what a kernel with such an index would compute. Both miss every gate by
    more than three orders of magnitude (the CPU tests prove >= 1e5 gates for the gradient)."""
    p, u, refs = problem(name)
    nodes = p["nodes"]
    for what, g in (("frozen", np.repeat(p["g"][:1], len(p["g"]), axis=0)),
                    ("late", np.concatenate([p["g"][nodes:], p["g"][-nodes:]]))):
        tdd.set_engine_problem(engine, dict(p, g=g))
        out = engine.evaluate(u, True)
        for b, ref in enumerate(refs):
            fr = tdd.gate_fractions(ref, (out[0][b], out[1][b], out[2][b]))
            print("{} {} seed {}: {}".format(name, what, b, " ".join("%s=%.2e" % kv for kv in fr.items())))
            assert fr["grad"] > 1e3 and fr["states"] > 1e3, (name, what, b, fr)
