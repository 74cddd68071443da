"""
GPU tests (-m gpu) of ControlBasis on the device (qocx_control_basis_apply, qocx_opt_begin_basis and
its Lindblad twin, qoc_amd/csrc/qocx_ctrlbasis.hip): the two kernels give the bits of
ControlBasis.expand / project, and the device-resident multi-start route under a basis walks the host
loop's trajectory bit for bit - errors, best iterations, best controls, best coefficients, final
states - the host loop being forced by a trivial subclass of the optimizer.

Small problems in the mould of tests/test_gpu_lbfgs.py (n <= 8 on the Schroedinger path, <= 41 system
steps, <= 6 seeds, 6 iterations). As there, max_control_norms sits at the scale of the pulses: the
resident route derives the evaluation's norm bound from max_control_norms alone, the host loop from
the controls it uploads, so under a wide clip the two routes' evaluations differ in rounding.
"""

import numpy as np
import pytest

import qoc_amd
import qoc_amd.standard.costs as product_costs
from qoc_amd.standard import LBFGS, SGD, Adam, ControlBasis
from qoc_amd.standard.costs import ControlNorm, ControlVariation
from tests import cases as cases_mod
from tests import helpers
from tests.test_control_basis_host import KERNEL_SHAPES, kernel_case
from tests.test_gpu_ensemble import transmon_ensemble
from tests.test_gpu_lbfgs import assert_same_runs, lindblad_problem, routes  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def real_engine():
    helpers.set_backend_factory(None)
    yield
    helpers.set_backend_factory(None)


@pytest.fixture
def engine():
    from qoc_amd.engine import Engine
    out = Engine(0)
    yield out
    out.close()


# ---- the kernels ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", KERNEL_SHAPES)
def test_kernels_give_the_bits_of_the_host_maps(engine, shape):
    basis, c, g = kernel_case(shape)
    up = engine.control_basis_apply(basis.matrix, c)
    down = engine.control_basis_apply(basis.matrix, g, transpose=True)
    assert up.shape == g.shape and down.shape == c.shape
    assert np.array_equal(up, basis.expand(c))
    assert np.array_equal(down, basis.project(g))


def test_a_seed_does_not_depend_on_its_batch(engine):
    basis, c, g = kernel_case((65, 33, 3, 2))
    rng = np.random.default_rng(6)
    many_c = np.concatenate([c, rng.standard_normal((5,) + c.shape[1:])])
    many_g = np.concatenate([rng.standard_normal((5,) + g.shape[1:]), g])
    up = engine.control_basis_apply(basis.matrix, many_c)
    down = engine.control_basis_apply(basis.matrix, many_g, transpose=True)
    for b in range(2):
        assert np.array_equal(up[b], engine.control_basis_apply(basis.matrix, c[b:b + 1])[0])
        assert np.array_equal(down[5 + b],
                              engine.control_basis_apply(basis.matrix, g[b:b + 1], transpose=True)[0])
    assert np.array_equal(up[:2], basis.expand(c))
    assert np.array_equal(down[5:], basis.project(g))


# ---- the resident route against the host loop -------------------------------------------------------

class HostAdam(Adam):  # not type(...) is Adam: the host loop
    pass


class HostSGD(SGD):
    pass


class HostLBFGS(LBFGS):
    pass


OPTIMIZERS = {
    "adam": (lambda: Adam(learning_rate=5e-2), lambda: HostAdam(learning_rate=5e-2)),
    "sgd": (lambda: SGD(learning_rate=0.5), lambda: HostSGD(learning_rate=0.5)),
    "lbfgs": (LBFGS, HostLBFGS),
}


def both_routes(run, args, c0, taken, optimizer, **kw):
    kw = dict(dict(iteration_count=6, log_iteration_step=0), **kw)
    resident, host = OPTIMIZERS[optimizer]
    before = dict(taken)
    a = run(*args, c0.copy(), optimizer=resident(), **kw)
    assert taken == {"resident": before["resident"] + 1, "host": before["host"]}
    b = run(*args, c0.copy(), optimizer=host(), **kw)
    assert taken == {"resident": before["resident"] + 1, "host": before["host"] + 1}
    return a, b


def assert_same_runs_and_coefficients(a, b, basis, finals="best_final_states"):
    assert_same_runs(a, b, finals=finals)
    for s in range(len(a.best_error)):
        assert a.best_coefficients[s].shape == (basis.coefficient_count,
                                                a.best_controls[s].shape[1])
        assert np.array_equal(a.best_coefficients[s], b.best_coefficients[s])


def schroedinger_problem(n=8, N=21, Nc=10, K=2, h_seed=41):
    case = cases_mod.case_random("ctrlbasis", n, N, 1, h_seed, S=2, K=K, Nc=Nc, dt=0.3,
                                 full_unitary=True)
    costs = [getattr(product_costs, kind)(**kw) for kind, kw in case.cost_specs]
    return (case.K, case.Nc, costs, case.T, case.hamiltonian(), case.initial_states, case.N)


def starts(basis, seeds, K, sigma, seed, bound, complex_controls=False):
    """Coefficients [seeds, P, K] of scale sigma, a seed scaled down where its pulse would pass
    0.95 bound: start pulses must conform to max_control_norms."""
    rng = np.random.default_rng(seed)
    shape = (seeds, basis.coefficient_count, K)
    c = sigma * rng.standard_normal(shape)
    if complex_controls:
        c = c + 1j * sigma * rng.standard_normal(shape)
    for b in range(seeds):
        top = np.max(np.abs(basis.expand(c[b])))
        if top > 0.95 * bound:
            c[b] *= 0.95 * bound / top
    return c


@pytest.mark.parametrize("optimizer", ["adam", "sgd", "lbfgs"])
def test_sine_basis_real_controls_with_the_clip_engaged(routes, optimizer):  # noqa: F811
    """P = 5 of Nc = 10. The coefficients move on unclipped, so pulses pass max_control_norms = 0.5
    and the evaluated (best) pulses sit at the bound."""
    args = schroedinger_problem()
    basis = ControlBasis.sine(10, 5)
    c0 = starts(basis, 6, args[0], 0.25, 21, 0.5)
    a, b = both_routes(qoc_amd.grape_schroedinger_discrete_batch, args, c0, routes, optimizer,
                       max_control_norms=np.full(args[0], 0.5), control_basis=basis)
    assert_same_runs_and_coefficients(a, b, basis)
    assert np.any(a.best_iteration > 0)
    engaged = 0
    for s in range(6):
        pulse = basis.expand(a.best_coefficients[s])
        assert np.all(a.best_controls[s][0] == 0.0) and np.all(a.best_controls[s][-1] == 0.0)
        assert np.max(np.abs(a.best_controls[s])) <= 0.5
        assert np.array_equal(np.clip(pulse, -0.5, 0.5), a.best_controls[s])
        engaged += int(a.best_iteration[s] > 0 and np.max(np.abs(pulse)) > 0.5)
    assert engaged > 0  # the clip acted on a best pulse that came out of an update


@pytest.mark.parametrize("optimizer", ["adam", "lbfgs"])
def test_complex_controls(routes, optimizer):  # noqa: F811
    n, K, N, Nc, B = 8, 2, 31, 10, 4
    rng = np.random.default_rng(704)
    h0 = cases_mod.gue(rng, n)
    g_re = [cases_mod.gue(rng, n) for _ in range(K)]
    g_im = [cases_mod.gue(rng, n) for _ in range(K)]

    def hamiltonian(u, t):
        out = h0
        for k in range(K):
            out = out + u[k].real * g_re[k] + u[k].imag * g_im[k]
        return out
    psi0 = cases_mod.column_states(np.eye(n)[:, :2])
    target = cases_mod.column_states(cases_mod.random_unitary(rng, n)[:, :2])
    args = (K, Nc, [product_costs.TargetStateInfidelity(target)], 0.3 * (N - 1), hamiltonian,
            psi0, N)
    basis = ControlBasis.sine(Nc, 4)
    c0 = starts(basis, B, K, 0.15, 22, 10.0, complex_controls=True)
    a, b = both_routes(qoc_amd.grape_schroedinger_discrete_batch, args, c0, routes, optimizer,
                       complex_controls=True, max_control_norms=np.full(K, 10.0),
                       control_basis=basis)
    assert_same_runs_and_coefficients(a, b, basis)
    assert np.all(a.best_iteration > 0)
    assert all(np.iscomplexobj(c) and c.shape == (4, K) for c in a.best_coefficients)
    assert all(np.iscomplexobj(c) and c.shape == (Nc, K) for c in a.best_controls)


def test_gaussian_filter_with_as_many_coefficients_as_knots(routes):  # noqa: F811
    args = schroedinger_problem(n=6, N=41, Nc=33, K=2, h_seed=42)
    basis = ControlBasis.gaussian_filter(33, 2.0)
    c0 = starts(basis, 4, args[0], 0.5, 23, 0.6)
    a, b = both_routes(qoc_amd.grape_schroedinger_discrete_batch, args, c0, routes, "adam",
                       max_control_norms=np.full(args[0], 0.6), control_basis=basis)
    assert_same_runs_and_coefficients(a, b, basis)
    assert np.any(a.best_iteration > 0)


def test_control_costs_on_the_device(routes):  # noqa: F811
    """ControlVariation and ControlNorm of the expanded, clipped pulse: on the device (resident) and
    through their Python classes (host loop); their gradients are projected with the pulse's."""
    args = schroedinger_problem(h_seed=44)
    K, Nc = args[0], args[1]
    mx = np.full(K, 0.5)
    costs = args[2] + [ControlNorm(K, Nc, cost_multiplier=0.5, max_control_norms=mx),
                       ControlVariation(K, Nc, cost_multiplier=0.4, order=1)]
    args = args[:2] + (costs,) + args[3:]
    basis = ControlBasis.sine(Nc, 5)
    c0 = starts(basis, 4, K, 0.25, 24, 0.5)
    a, b = both_routes(qoc_amd.grape_schroedinger_discrete_batch, args, c0, routes, "adam",
                       max_control_norms=mx, control_basis=basis)
    assert_same_runs_and_coefficients(a, b, basis)


def test_hamiltonian_ensemble_of_three(routes):  # noqa: F811
    K, N, Nc, S, T, n = 3, 31, 10, 2, 1.5, 8
    e, rng = transmon_ensemble(n, K, M=3, J=1, seed=5, complex_controls=False)
    psi0 = cases_mod.column_states(np.eye(n)[:, :S])
    target = cases_mod.column_states(cases_mod.random_unitary(rng, n)[:, :S])
    args = (K, Nc, [product_costs.TargetStateInfidelity(target)], T, e, psi0, N)
    basis = ControlBasis.sine(Nc, 5)
    c0 = starts(basis, 4, K, 0.4, 25, 1.0)
    a, b = both_routes(qoc_amd.grape_schroedinger_discrete_batch, args, c0, routes, "lbfgs",
                       max_control_norms=np.full(K, 1.0), control_basis=basis)
    assert_same_runs_and_coefficients(a, b, basis)
    for s in range(4):
        assert a.best_final_states[s].shape == (3, S, n, 1)
        assert np.array_equal(a.member_errors[s], b.member_errors[s])


@pytest.mark.parametrize("optimizer", ["adam", "lbfgs"])
def test_lindblad(routes, optimizer):  # noqa: F811
    args, kw = lindblad_problem()  # K = 2, Nc = 4, max_control_norms = 2
    basis = ControlBasis.sine(args[1], 2)
    c0 = starts(basis, 6, args[0], 0.8, 26, 2.0)
    a, b = both_routes(qoc_amd.grape_lindblad_discrete_batch, args, c0, routes, optimizer,
                       control_basis=basis, **kw)
    assert_same_runs_and_coefficients(a, b, basis, finals="best_final_densities")
    assert np.any(a.best_iteration > 0)


# ---- the engine's calls ---------------------------------------------------------------------------------

def test_engine_rejections_and_lbfgs_state_sized_by_the_coefficients(engine):
    """Both paths: begin_basis without uploaded controls, P = 0, a NaN in the matrix; then L-BFGS
    begun after begin_basis - two steps, whose second keeps the coefficients the first one made:
    they are LBFGS.update of the projected gradient on the host, so the state has P * channels
    entries per seed and the kernel's element order is the host's."""
    from qoc_amd.engine import QocxError
    from tests import gpu_helpers as gh
    for lindblad in (False, True):
        if lindblad:
            case = cases_mod.lindblad_case_by_name("lindblad_n4")
            gh.setup_lindblad_engine(engine, case)
            prefix = "lindblad_"
            evaluate, results = engine.eval_lindblad_resident, engine.lindblad_download_results
        else:
            case = cases_mod.case_random("ctrlbasis", 6, 21, 1, 47, S=2, K=2, Nc=10, dt=0.3,
                                         full_unitary=True)
            gh.setup_engine(engine, case)
            prefix = ""
            evaluate, results = engine.eval_resident, engine.download_results
        call = lambda name: getattr(engine, prefix + name)  # noqa: E731
        B, P, K = 3, 3, case.K
        basis = ControlBasis.sine(case.Nc, P)
        c0 = starts(basis, B, K, 0.2, 27, 0.9)
        with pytest.raises(QocxError):  # no uploaded controls
            call("opt_begin_basis")(False, basis.matrix, c0)
        call("upload_controls")(basis.expand(c0))
        with pytest.raises(QocxError):
            call("opt_begin_basis")(False, np.zeros((case.Nc, 0)), c0)
        broken = np.array(basis.matrix)
        broken[case.Nc // 2, 1] = np.nan
        with pytest.raises(QocxError):
            call("opt_begin_basis")(False, broken, c0)
        with pytest.raises(QocxError):  # no basis stands after the failures
            call("opt_download_best_params")()
        call("opt_begin_basis")(False, basis.matrix, c0)
        call("opt_lbfgs_begin")(4)
        seeds = [LBFGS(history=4) for _ in range(B)]
        ones = np.ones(B, dtype=bool)
        expect = c0.reshape(B, -1)
        for _ in range(3):
            call("opt_clip")(np.full(K, 1.0))
            evaluate(True)
            cost, grads, _ = results(True, False)
            o = seeds[0]
            finished = call("opt_lbfgs_step")(ones, ones, o.first_step, o.armijo, o.shrink,
                                              o.max_backtracks)
            kept = call("opt_download_best_params")()  # (every seed `improved`: what was evaluated)
            assert kept.shape == (B, P, K)
            assert np.array_equal(kept.reshape(B, -1), expect)
            evaluated, _ = call("opt_download_best")()
            assert np.array_equal(evaluated, np.clip(basis.expand(kept), -1.0, 1.0))
            projected = basis.project(grads).reshape(B, -1)
            expect = np.stack([seeds[b].update(projected[b], expect[b], cost[b])
                               for b in range(B)])
            assert np.array_equal(finished, [s.finished for s in seeds])
        call("opt_begin")()  # a plain begin clears the basis
        with pytest.raises(QocxError):
            call("opt_download_best_params")()
