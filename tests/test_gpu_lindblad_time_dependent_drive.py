"""
GPU tests (-m gpu): drive operators G_k(t) that depend on time on the Lindblad path - g_stages, the
table gp_tab the host builds from it (qocx_api_lindblad.hip) and the stage loops that index it - with
h0_stages constant, against the NumPy model of the device algorithm (tests/lindblad_model.py with
g_of_t, subdivision = fixed_subdivision; tests/test_time_dependent_drive_host.py pins its gradient on
finite differences). Below n = 17 no other test passes a varying g_stages at all; above, one compares
two kernels with each other. Tolerances of test_lindblad_edge_shapes_against_model: cost and
densities 1e-12, gradients 1e-10 relative. Problems: tests/time_dependent_drive.py:
lindblad_drive_problem - N = 3 .. 4, Nc = 2 .. 3, three seeds of different amplitude.
"""

import numpy as np
import pytest

from tests import lindblad_model as lm
from tests import time_dependent_drive as tdd

pytestmark = pytest.mark.gpu

KNOB_DEFAULTS = dict(lindblad_pad_operator=1, lindblad_two_sided=1, lindblad_q2=1, lindblad_4t=1)


@pytest.fixture(scope="module")
def engine():
    from qoc_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


_cache = {}


def problem(**spec):
    """(problem, per-seed model results), computed once."""
    from qoc_amd.engine import Engine
    key = tuple(sorted(spec.items()))
    if key not in _cache:
        q = tdd.lindblad_drive_problem(stage_times=Engine.lindblad_stage_times, **spec)
        system = tdd.lindblad_model_system(q)
        refs = [lm.evaluate_with_grad(system, u, q["rho0"], q["T"], q["N"], q["mcosts"], 1,
                                      want_grad=True, subdivision=q["subdivision"])
                for u in q["controls"]]
        _cache[key] = (q, refs)
    return _cache[key]


def assert_model(tag, refs, out):
    worst = dict(cost=0.0, densities=0.0, grad=0.0)
    for b, (m_err, m_grads, m_final) in enumerate(refs):
        worst["cost"] = max(worst["cost"], abs(out[0][b] - m_err) / 1e-12)
        worst["densities"] = max(worst["densities"], np.max(np.abs(out[2][b] - m_final)) / 1e-12)
        worst["grad"] = max(worst["grad"], np.max(np.abs(out[1][b] - m_grads))
                            / max(np.max(np.abs(m_grads)), 1e-3) / 1e-10)
    print("{}: worst/tolerance {}".format(tag, " ".join("%s=%.2e" % kv for kv in worst.items())))
    assert all(v < 1.0 for v in worst.values()), (tag, worst)


def evaluate(engine, q, settings=None, launch=(0, 256, 0)):
    """One evaluation under knob settings (read when the problem is set and when it is evaluated) and
    launch variants (qocx_debug_lindblad_knobs)."""
    settings = settings or {}
    try:
        for name, value in settings.items():
            engine.set_knob(name, value)
        engine.set_lindblad_problem(*q["args"], **q["kwargs"])
        engine.debug_lindblad_knobs(*launch)
        return engine.evaluate_lindblad(q["controls"])
    finally:
        for name in settings:
            engine.set_knob(name, KNOB_DEFAULTS[name])
        engine.debug_lindblad_knobs(0, 256, 0)


LAUNCHES = [("default", (0, 256, 0)), ("recompute", (1, 256, 0)), ("one wave", (0, 256, 1)),
            ("several waves", (0, 256, 2))]


def run_variants(engine, spec, tile_knob=False):
    """Forbid step costs (the classic forward-then-adjoint launch) and one final target (the two-sided
    route, with its knobs), each under every launch variant."""
    tag = " ".join("%s=%s" % kv for kv in sorted(spec.items()))
    tiles = [dict(lindblad_4t=1), dict(lindblad_4t=0)] if tile_knob else [{}]
    pads = [dict(lindblad_pad_operator=1), dict(lindblad_pad_operator=0)] if spec["L"] == 1 and spec["n"] <= 16 else [{}]
    for costs in ("general", "final"):
        q, refs = problem(costs=costs, **spec)
        sides = ([dict(lindblad_two_sided=1, lindblad_q2=1), dict(lindblad_two_sided=1, lindblad_q2=0),
                  dict(lindblad_two_sided=0)] if costs == "final" else [{}])
        for tile in tiles:
            for pad in pads:
                for side in sides:
                    settings = dict(tile, **dict(pad, **side))
                    # (the launch variants once per cost set, on the default knobs)
                    launches = LAUNCHES if settings == dict(tiles[0], **dict(pads[0], **sides[0])) else LAUNCHES[:1]
                    for name, launch in launches:
                        out = evaluate(engine, q, settings, launch)
                        assert_model("{} {} {} {}".format(tag, costs, settings, name), refs, out)


# ---- n <= 16: the path no test ran with a varying g_stages ------------------------------------------------------

SMALL = [
    dict(n=1, N=3, Nc=2, K=1, S=1, L=0, subdivision=1),
    dict(n=1, N=4, Nc=3, K=8, S=2, L=2, subdivision=4, complex_ops=False),
    dict(n=4, N=4, Nc=3, K=1, S=2, L=1, subdivision=1),                      # one operator: padded or not
    dict(n=4, N=3, Nc=3, K=8, S=1, L=3, subdivision=4),                      # chained loop
    dict(n=4, N=4, Nc=2, K=2, S=2, L=5, subdivision=1, complex_ops=False),   # one-wave kernels
    dict(n=4, N=3, Nc=2, K=2, S=1, L=2, subdivision=4, complex_ops=False),
    dict(n=16, N=3, Nc=3, K=8, S=2, L=0, subdivision=4),
    dict(n=16, N=4, Nc=2, K=1, S=1, L=1, subdivision=4, complex_ops=False),
    dict(n=16, N=3, Nc=2, K=2, S=2, L=2, subdivision=1),
    dict(n=16, N=4, Nc=3, K=2, S=1, L=3, subdivision=1, complex_ops=False),
    dict(n=16, N=3, Nc=3, K=1, S=2, L=5, subdivision=4),
]


def spec_id(s):
    return "n{n}_S{S}_K{K}_L{L}_sub{subdivision}_{ops}".format(
        ops="real" if s.get("complex_ops") is False else "complex", **s)


@pytest.mark.parametrize("spec", SMALL, ids=spec_id)
def test_one_tile_against_model(engine, spec):
    run_variants(engine, spec)


# ---- 17 <= n <= 32 ------------------------------------------------------------------------------------------------------

TILES = [
    dict(n=17, N=3, Nc=2, K=2, S=1, L=1, subdivision=4),
    dict(n=21, N=4, Nc=3, K=2, S=2, L=3, subdivision=1),
    dict(n=32, N=3, Nc=3, K=1, S=2, L=3, subdivision=4, complex_ops=False),
    dict(n=32, N=3, Nc=2, K=2, S=1, L=1, subdivision=1),
]


@pytest.mark.parametrize("spec", TILES, ids=spec_id)
def test_tile_kernel_and_one_wave_form_against_model(engine, spec):
    run_variants(engine, spec, tile_knob=True)


# ---- together with time-dependent lindblad_data --------------------------------------------------------------------------

@pytest.mark.parametrize("spec", [dict(n=4, N=4, Nc=3, K=2, S=2, L=2, subdivision=4),
                                  dict(n=16, N=3, Nc=2, K=2, S=1, L=3, subdivision=1),
                                  dict(n=21, N=3, Nc=3, K=2, S=2, L=3, subdivision=4)], ids=spec_id)
def test_with_time_dependent_lindblad_data(engine, spec):
    """g_stages beside diss_stages / op_stages: three time-indexed tables in one stage loop."""
    for costs in ("general", "final"):
        q, refs = problem(costs=costs, data_stages=True, **spec)
        assert_model("{} data {}".format(spec_id(spec), costs), refs, evaluate(engine, q))


# ---- the resident route ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("spec", [SMALL[3], SMALL[8], TILES[1]], ids=spec_id)
def test_resident_evaluation_equals_evaluate_lindblad(engine, spec):
    q, refs = problem(costs="general", **spec)
    engine.set_lindblad_problem(*q["args"], **q["kwargs"])
    ref = engine.evaluate_lindblad(q["controls"])
    assert_model(spec_id(spec), refs, ref)
    engine.lindblad_upload_controls(q["controls"])
    engine.eval_lindblad_resident(True)
    out = engine.lindblad_download_results(True)
    for a, b in zip(out, ref):
        assert np.array_equal(a, b)


def test_resident_grape_equals_host_loop_with_a_rotating_drive(monkeypatch):
    """grape_lindblad_discrete_batch, three iterations of Adam on the device against the host loop, on
    a Hamiltonian whose drive operators rotate (H0 constant): bit for bit, as
    test_gpu_lindblad_batch.py::test_time_dependent_resident_equals_host_loop asks of a modulated H0."""
    import qoc_amd
    from qoc_amd.core import batch as batch_mod
    from qoc_amd.standard import Adam
    from tests import cases as cases_mod
    from tests import helpers
    from tests.test_gpu_lindblad_batch import PluginAdam, assert_same_runs, problem as api_problem, starts
    taken = {"resident": 0, "host": 0}
    resident, host = batch_mod.run_batch_resident, batch_mod.run_batch_host

    def run_resident(*a, **k):
        taken["resident"] += 1
        return resident(*a, **k)

    def run_host(*a, **k):
        taken["host"] += 1
        return host(*a, **k)
    monkeypatch.setattr(batch_mod, "run_batch_resident", run_resident)
    monkeypatch.setattr(batch_mod, "run_batch_host", run_host)
    helpers.set_backend_factory(None)
    case = cases_mod.lindblad_case_by_name("lindblad_timedep")
    rng = np.random.default_rng(881)
    quad = [cases_mod.gue(rng, case.n) for _ in range(case.K)]
    dt = case.T / (case.N - 1)
    omegas = [(2.0 + k) / dt for k in range(case.K)]

    def hamiltonian(u, t):
        return case.h0 + sum(u[k] * (np.cos(omegas[k] * t + k) * case.g_re[k] + np.sin(omegas[k] * t) * quad[k])
                             for k in range(case.K))

    u0 = starts(case, 3, 0.6, 96, bound=1.2)
    args, kw = api_problem(case)
    kw.update(hamiltonian=hamiltonian, iteration_count=3, max_control_norms=np.full(case.K, 1.2))
    a = qoc_amd.grape_lindblad_discrete_batch(*args, u0.copy(), optimizer=Adam(learning_rate=5e-2), **kw)
    b = qoc_amd.grape_lindblad_discrete_batch(*args, u0.copy(), optimizer=PluginAdam(learning_rate=5e-2), **kw)
    assert taken == {"resident": 1, "host": 1}
    assert_same_runs(a, b, 3)
    # and the rotation matters: the frozen drive gives other errors
    kw["hamiltonian"] = lambda u, t: hamiltonian(u, 0.0)
    frozen = qoc_amd.grape_lindblad_discrete_batch(*args, u0.copy(), optimizer=Adam(learning_rate=5e-2), **kw)
    assert np.max(np.abs(frozen.best_error - a.best_error)) > 1e-4


@pytest.mark.parametrize("spec", [SMALL[5], SMALL[8], TILES[1]], ids=spec_id)
def test_a_frozen_table_is_seen(engine, spec):
    """The tests bite: with g_stages frozen at its first sample (t = 0) the engine misses the model of
    the true problem by >= 1e-6 in the densities and >= 1e-10 in the gradient, as
    test_time_dependent_drive_host.py::test_lindblad_wrong_stage_cannot_pass says it must."""
    q, refs = problem(costs="general", **spec)
    g = q["kwargs"]["g_stages"]
    frozen = dict(q, kwargs=dict(q["kwargs"], g_stages=np.repeat(g[:1], len(g), axis=0)))
    out = evaluate(engine, frozen)
    for b in (1, 2):
        assert np.max(np.abs(out[2][b] - refs[b][2])) >= 1e-6
        assert np.max(np.abs(out[1][b] - refs[b][1])) >= 1e-10
