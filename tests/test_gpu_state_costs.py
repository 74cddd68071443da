"""
GPU tests (-m gpu): every state-cost descriptor on every sweep route (tests/state_costs.py). The cost
code turns states into the error and into the cotangent that seeds the adjoint sweep; it exists in
several hand-written copies - eval_costs, unit_adjoint_scales and unit_adjoint_seed of
qocx_sweep_common.h under the choreography of six sweep kernels, eval_costs_g of qocx_general.hip,
effctl_cotangent of qocx_effctl.hip, the scalar application of the scatter kernel, density_costs of
the two Lindblad cores - and every other problem of the suite hands them the same costs. Here nine
descriptor sets (a sole incoherent final cost, step coherent costs, ragged forbid counts, a second
forbid, descriptors behind a ragged sum, two finals, a final forbid) run on every row of the route
table at N = 7 and 8 with cost_eval_step 3 - the final step is a cost step in one and not in the other -
against the oracle on DescriptorCosts. tests/test_state_costs_host.py proves on the CPU that a misread
table moves the oracle's gradient by >= 1e-3 relative on every one of these problems.
Gates: cost and states 1e-10 relative, gradient 1e-8 of max(|g|, 1e-3), per seed and
per control channel. Run with -s for the worst fraction of each gate per row and set.
"""

import numpy as np
import pytest

from tests import state_costs as sc

pytestmark = pytest.mark.gpu

KNOB_DEFAULTS = dict(sweep_inverse_small=1, sweep_dense=1, sweep_impl=1, sweep_one=1, latency=0, sweep_umode=1,
                     unit_adjoint=1, lindblad_4t=1)


@pytest.fixture(scope="module")
def engine():
    from qoc_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


class knobs(object):
    def __init__(self, engine, values):
        self.engine, self.values = engine, values

    def __enter__(self):
        for name, value in self.values.items():
            self.engine.set_knob(name, value)

    def __exit__(self, *exc):
        for name in self.values:
            self.engine.set_knob(name, KNOB_DEFAULTS[name])


_refs = {}


def references(p, name):
    """The oracle's (error, grads, final) of every seed for a set, computed once per problem."""
    key = (p["n"], p["S"], p["kind"], p["N"], name)
    if key not in _refs:
        costs = sc.descriptor_set(name, p)
        _refs[key] = [sc.evaluate(p, costs, b) for b in range(len(p["controls"]))]
    return _refs[key]


def set_problem(engine, p, costs):
    engine.set_schroedinger_problem(p["n"], p["S"], p["K"], p["Nc"], p["N"], p["T"], p["h0"][None],
                                    p["g"][None], p["init"], costs=[c.descriptor() for c in costs],
                                    cost_eval_step=p["ces"], magnus_policy=p["policy"])
    if p["quadratic"] is not None:
        engine.set_quadratic_terms(*p["quadratic"])


def run(engine, p):
    """(cost[B], grads[B], final[B]) of the row's seeds: upload, qocx_eval_resident, download. Latency
    mode takes one control set at a time."""
    u = p["controls"]
    if not p["row"]["knobs"].get("latency"):
        return engine.evaluate(u, True)
    outs = [engine.evaluate(u[b:b + 1], True) for b in range(len(u))]
    return tuple(np.concatenate([o[i] for o in outs]) for i in range(3))


def assert_identical(a, b, tag):
    for x, y in zip(a, b):
        assert np.array_equal(x, y), tag


def assert_close(a, b, tag, tol=1e-12):
    """cost, gradient and states within `tol` of the larger magnitude."""
    for x, y in zip(a, b):
        assert np.max(np.abs(x - y)) <= tol * np.max(np.abs(y)), tag


# ---- against the oracle ------------------------------------------------------------------------------------

@pytest.mark.parametrize("row", sc.ROWS, ids=[r["name"] for r in sc.ROWS])
def test_every_set_on_every_route_against_the_oracle(engine, row):
    fails = []
    with knobs(engine, row["knobs"]):
        for name in sc.SETS:
            if (name, row["name"]) in sc.REFUSED:
                continue
            worst = dict(cost=0.0, states=0.0, grad=0.0, grad_channel=0.0)
            for N in sc.STEP_COUNTS:
                p = sc.build(row, N)
                set_problem(engine, p, sc.descriptor_set(name, p))
                out = run(engine, p)
                for b, ref in enumerate(references(p, name)):
                    for key, value in sc.gate_fractions(ref, (out[0][b], out[1][b], out[2][b])).items():
                        worst[key] = max(worst[key], value)
                        if not value < 1.0:
                            fails.append((name, N, b, key, value))
            print("state costs {} {}: worst/gate {}".format(
                row["name"], name, " ".join("%s=%.2e" % kv for kv in worst.items())))
    assert not fails, (row["name"], fails)


# ---- unit adjoint on and off ---------------------------------------------------------------------------------

@pytest.mark.parametrize("row", sc.ROWS, ids=[r["name"] for r in sc.ROWS])
def test_unit_adjoint_on_and_off(engine, row):
    """Where the unit adjoint applies - final_coherent; final_incoherent on one state - the classic
    order (knob unit_adjoint 0) gives the same cost and final states bit for bit and the same gradient
    within 1e-12 relative (the numbers of test_gpu_engine.py::test_unit_adjoint_and_two_sided_pipeline),
    and one time segment against three is scheduling alone: bit for bit."""
    with knobs(engine, row["knobs"]):
        for name in ("final_coherent", "final_incoherent"):
            if not sc.unit_adjoint_applies(name, row["S"]):
                continue
            for N in sc.STEP_COUNTS:
                p = sc.build(row, N)
                set_problem(engine, p, sc.descriptor_set(name, p))
                try:
                    unit = run(engine, p)
                    engine.set_knob("unit_adjoint", 0)
                    classic = run(engine, p)
                    engine.set_knob("unit_adjoint", 1)
                    assert np.array_equal(classic[0], unit[0]) and np.array_equal(classic[2], unit[2]), (name, N)
                    assert np.max(np.abs(classic[1] - unit[1])) <= 1e-12 * np.max(np.abs(classic[1])), (name, N)
                    engine.set_pipeline(1)
                    one = run(engine, p)
                    engine.set_pipeline(3)
                    assert_identical(one, run(engine, p), (name, N, "pipeline 1 against 3"))
                    assert_identical(one, unit, (name, N, "pipeline 1 against the default"))
                finally:
                    engine.set_knob("unit_adjoint", 1)
                    engine.set_pipeline(0)


ONE_STATE_ROWS = [r for r in sc.ROWS if r["S"] == 1]


@pytest.mark.parametrize("row", ONE_STATE_ROWS, ids=[r["name"] for r in ONE_STATE_ROWS])
def test_incoherent_equals_coherent_on_one_state(engine, row):
    """On one state the two kinds are the same function: the incoherent branch of unit_adjoint_scales
    and what stands behind it against the coherent one on the same targets and scale, cost, states
    and gradient within 1e-12 relative. (The arithmetic is the same, too: whether the results are
    bit-identical is printed, not asserted.)"""
    with knobs(engine, row["knobs"]):
        for N in sc.STEP_COUNTS:
            p = sc.build(row, N)
            inc = sc.descriptor_set("final_incoherent", p)[0]
            out = {}
            for kind in (sc.INCOHERENT, sc.COHERENT):
                set_problem(engine, p, [sc.DescriptorCost(kind, 0, inc.scale, inc.vectors)])
                out[kind] = run(engine, p)
            assert_close(out[sc.INCOHERENT], out[sc.COHERENT], (row["name"], N))
            print("state costs {} N={}: incoherent against coherent bit-identical: {}".format(
                row["name"], N, all(np.array_equal(a, b) for a, b in zip(out[sc.INCOHERENT], out[sc.COHERENT]))))


TWO_TILE_ROWS = [r for r in sc.ROWS if 17 <= r["n"] <= 32 and r["S"] >= 2]


@pytest.mark.parametrize("row", TWO_TILE_ROWS, ids=[r["name"] for r in TWO_TILE_ROWS])
def test_segments_and_chunks_with_step_costs(engine, row):
    """17 <= n <= 32 with several states - the waves of a workgroup share the states, and wave 0's cost
    evaluation stands between their steps -, a ragged forbid, a step target and a final one: one time
    segment against two and chunks of one seed against one chunk, bit for bit."""
    assert len(TWO_TILE_ROWS) == 8
    with knobs(engine, row["knobs"]):
        for N in sc.STEP_COUNTS:
            p = sc.build(row, N)
            set_problem(engine, p, sc.descriptor_set("target_after_ragged_forbid", p))
            try:
                engine.set_pipeline(1)
                ref = run(engine, p)
                engine.set_pipeline(2)
                assert_identical(ref, run(engine, p), (N, "pipeline 1 against 2"))
                engine.set_pipeline(0)
                engine.set_chunk(1)
                one = run(engine, p)
                engine.set_chunk(0)
                assert_identical(one, run(engine, p), (N, "chunk 1 against 0"))
                assert_identical(one, ref, (N, "chunk against pipeline"))
            finally:
                engine.set_pipeline(0)
                engine.set_chunk(0)


# ---- the tests bite -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["chain2_n20_S5", "sweepd_n24_S8", "chain4_n40_S5", "general_n66_S3"])
def test_a_misread_table_is_seen(engine, name):
    """The engine handed what a kernel with a wrong table would read - the kinds of two_finals swapped,
    forbid_ragged with the count of state 0 for every state - against the oracle of the true set: both
    miss the gradient gate by more than three orders of magnitude at every seed (the CPU tests prove
    >= 1e5 gates)."""
    row = sc.ROW_BY_NAME[name]
    p = sc.build(row, 8)
    D = sc.DescriptorCost
    finals, forbid = sc.descriptor_set("two_finals", p), sc.descriptor_set("forbid_ragged", p)[0]
    first = forbid.counts[0]
    wrong = {"two_finals": [D(1 - c.kind, 0, c.scale, c.vectors) for c in finals],
             "forbid_ragged": [D(sc.FORBID, 1, forbid.scale, forbid.vectors[:first * p["S"]], [first] * p["S"])]}
    with knobs(engine, row["knobs"]):
        for set_name, costs in wrong.items():
            set_problem(engine, p, costs)
            out = run(engine, p)
            for b, ref in enumerate(references(p, set_name)):
                fr = sc.gate_fractions(ref, (out[0][b], out[1][b], out[2][b]))
                assert fr["grad"] > 1e3 and fr["states"] < 1.0, (set_name, b, fr)


# ---- the host API -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("S", [1, 2])
def test_grape_with_incoherent_costs_against_the_oracle_backend(S):
    """grape_schroedinger_discrete, three iterations at n = 17, on the device against the same run on
    tests/oracle_backend.py, at the trajectory tolerances of tests/test_gpu_api.py: S = 1 with
    TargetStateInfidelity(neglect_relative_pahse=True) - the unit adjoint of an incoherent cost -, S = 2
    with it and a coherent TargetStateInfidelityTime."""
    import qoc_amd
    from qoc_amd.standard import Adam, TargetStateInfidelity, TargetStateInfidelityTime
    from tests import helpers
    from tests.helpers import rel_err
    from tests.oracle_backend import OracleBackend
    p = sc.build(sc._row("api", 17, S), 8)
    h0, g = p["h0"], p["g"]
    init, targ = p["init"][:, :, None], p["vec"]["A"][:, :, None]

    def runs():
        costs = [TargetStateInfidelity(targ, neglect_relative_pahse=True)]
        if S == 2:
            costs.append(TargetStateInfidelityTime(p["N"], p["vec"]["B"][:, :, None], neglect_relative_pahse=False,
                                                   cost_eval_step=p["ces"]))
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

        result = qoc_amd.grape_schroedinger_discrete(
            p["K"], p["Nc"], costs, p["T"], lambda u, t: h0 + u[0] * g[0] + u[1] * g[1], init, p["N"],
            cost_eval_step=p["ces"], initial_controls=p["controls"][1].copy(), iteration_count=3,
            log_iteration_step=0, optimizer=Recorder(Adam(learning_rate=2e-2)),
            max_control_norms=np.full(p["K"], 1.5 * np.max(np.abs(p["controls"][1]))))
        return result, trace

    helpers.set_backend_factory(None)
    gpu = runs()
    helpers.set_backend_factory(OracleBackend)
    try:
        cpu = runs()
    finally:
        helpers.set_backend_factory(None)
    assert len(gpu[1]) == len(cpu[1]) == 3
    for (ge, gg), (ce, cg) in zip(gpu[1], cpu[1]):
        assert abs(ge - ce) < 1e-9 * max(1, abs(ce))
        assert rel_err(gg, cg) < 1e-7
    assert gpu[0].best_iteration == cpu[0].best_iteration
    assert rel_err(gpu[0].best_controls, cpu[0].best_controls) < 1e-7
    assert rel_err(gpu[0].best_final_states, cpu[0].best_final_states) < 1e-9


# ---- Lindblad companion -------------------------------------------------------------------------------------

_lindblad_refs = {}


@pytest.mark.parametrize("ces", [1, 2])
@pytest.mark.parametrize("shape", sc.LINDBLAD_SHAPES,
                         ids=["n{}_L{}{}".format(s["n"], s["L"], "".join("_%s%d" % kv for kv in s["knobs"].items()))
                              for s in sc.LINDBLAD_SHAPES])
def test_lindblad_descriptor_sets_against_the_model(engine, shape, ces):
    """density_costs of qocx_lindblad_core.h and its twin of qocx_lindblad4t_core.h: one final target, two
    final targets (no unit adjoint; the second on matrices that are not Hermitian, so tr(T^H rho)
    carries a phase), two ragged forbids ([1, 3] and [2, 1]) and a step target, against
    tests/lindblad_model.py with DescriptorDensityCosts at that file's gates: 1e-12 absolute for cost
    and final densities, 1e-10 of max(|g|, 1e-3) for the gradient."""
    q = sc.lindblad_problem(shape["n"], shape["L"])
    fails = []
    with knobs(engine, shape["knobs"]):
        for name in sc.LINDBLAD_SETS:
            costs = sc.lindblad_set(name, q, ces)
            key = (shape["n"], shape["L"], ces, name)
            if key not in _lindblad_refs:
                _lindblad_refs[key] = [sc.lindblad_model_run(q, costs, ces, b) for b in range(len(q["controls"]))]
            engine.set_lindblad_problem(q["n"], q["S"], q["K"], q["Nc"], q["N"], q["T"], q["h0"], q["g"], q["gam"],
                                        q["ops"], q["rho0"], costs=[c.descriptor() for c in costs],
                                        cost_eval_step=ces)
            cost, grads, final = engine.evaluate_lindblad(q["controls"])
            worst = dict(cost=0.0, final=0.0, grad=0.0)
            for b, (m_err, m_grads, m_final) in enumerate(_lindblad_refs[key]):
                fr = dict(cost=abs(cost[b] - m_err) / 1e-12, final=np.max(np.abs(final[b] - m_final)) / 1e-12,
                          grad=np.max(np.abs(grads[b] - m_grads)) / max(np.max(np.abs(m_grads)), 1e-3) / 1e-10)
                for k, v in fr.items():
                    worst[k] = max(worst[k], v)
                    if not v < 1.0:
                        fails.append((name, b, k, v))
            print("state costs lindblad n={} L={} {} ces={} {}: worst/gate {}".format(
                q["n"], q["L"], shape["knobs"], ces, name, " ".join("%s=%.2e" % kv for kv in worst.items())))
    assert not fails, fails


# ---- fuzz -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nmin, nmax, count, seed", [(1, 32, 30, 3301), (33, 80, 10, 8033)])
def test_random_descriptors_fuzz(engine, nmin, nmax, count, seed):
    """tests/fuzz_parity.py with costs=True: random shapes, grids, Magnus policies and time steps, every
    draw with 1 to 4 random descriptors (kinds, step or final, ragged counts from 1 to 4) against the
    oracle on DescriptorCosts, every draw at the parity gates."""
    from tests import fuzz_parity
    rng = np.random.default_rng(seed)
    checked, overall = 0, 0.0
    for index in range(count):
        worst, tag = fuzz_parity.one(engine, rng, index, nmin=nmin, nmax=nmax, costs=True)
        if worst is None:  # more than 2^10 squarings per step: rejected by design
            continue
        checked += 1
        overall = max(overall, worst)
        assert worst <= 1.0, tag
    print("state costs fuzz, n in {}..{}: {} of {} checked, worst/gate {:.2e}".format(
        nmin, nmax, checked, count, overall))
    assert checked >= count - 1
