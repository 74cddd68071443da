"""
CPU tests of ControlBasis (qoc_amd/standard/controlbasis.py): the class and its two maps in their
defined summation order, the control_basis keyword of the four GRAPE entry points on the host loop
with the oracle backend (tests/oracle_backend.py), and the device-resident loop's driver logic on a
NumPy stand-in for the engine's resident calls. The kernels and the real resident route run in
tests/test_gpu_control_basis.py, which takes its kernel inputs from kernel_case() below.
"""

import math

import numpy as np
import pytest

import qoc_amd
from qoc_amd.core import batch as batch_mod
from qoc_amd.core.common import clip_control_norms
from qoc_amd.core.device import SchroedingerEvaluator
from qoc_amd.core.schroedingerdiscrete import GrapeSchroedingerBatchResult
from qoc_amd.models import MagnusPolicy
from qoc_amd.standard import LBFGS, SGD, Adam, ControlBasis
from tests import cases as cases_mod
from tests import helpers
from tests.oracle_backend import OracleBackend
from tests.test_host_api import product_cost_list
from tests.test_lindblad_host_api import product_cost_list as lindblad_cost_list


@pytest.fixture(autouse=True)
def oracle_engine():
    helpers.set_backend_factory(OracleBackend)
    yield
    helpers.set_backend_factory(None)


# ---- the class -------------------------------------------------------------------------------------

@pytest.mark.parametrize("matrix", [
    np.zeros(5), np.zeros((5, 0)), np.zeros((0, 3)), np.zeros((2, 3, 4)),
    np.ones((4, 2)) * (1 + 1j), np.array([[1.0, np.nan]]), np.array([[np.inf], [0.0]]),
    np.array([["a", "b"]])])
def test_constructor_rejects(matrix):
    with pytest.raises(ValueError):
        ControlBasis(matrix)


def test_fields_and_shapes():
    basis = ControlBasis(np.arange(12).reshape(4, 3))
    assert basis.matrix.dtype == np.float64 and basis.matrix.shape == (4, 3)
    assert (basis.knot_count, basis.coefficient_count) == (4, 3)
    assert basis.expand(np.ones((3, 2))).shape == (4, 2)
    assert basis.expand(np.ones((5, 7, 3, 2))).shape == (5, 7, 4, 2)
    assert basis.project(np.ones((5, 4, 2))).shape == (5, 3, 2)
    assert np.iscomplexobj(basis.expand(np.ones((3, 1)) * 1j))
    for bad in (np.ones((4, 2)), np.ones(3)):
        with pytest.raises(ValueError):
            basis.expand(bad)
    with pytest.raises(ValueError):
        basis.project(np.ones((3, 2)))
    for bad in ((1, 3), (5, 0)):
        with pytest.raises(ValueError):
            ControlBasis.sine(*bad)
    for bad in ((0, 1.0), (5, 0.0), (5, np.inf)):
        with pytest.raises(ValueError):
            ControlBasis.gaussian_filter(*bad)


def test_sine_end_points_are_exactly_zero():
    basis = ControlBasis.sine(33, 6)
    assert basis.matrix.shape == (33, 6)
    assert np.all(basis.matrix[0] == 0.0) and np.all(basis.matrix[-1] == 0.0)
    j = np.arange(33)
    for p in range(1, 7):
        assert np.allclose(basis.matrix[:, p - 1], np.sin(np.pi * p * j / 32), atol=1e-15, rtol=0)
    rng = np.random.default_rng(2)
    pulse = basis.expand(rng.standard_normal((4, 6, 3)) + 1j * rng.standard_normal((4, 6, 3)))
    assert np.all(pulse[:, 0] == 0.0) and np.all(pulse[:, -1] == 0.0)
    assert np.max(np.abs(pulse)) > 0.5


def test_gaussian_filter_rows_sum_to_one():
    for count, sigma in ((33, 2.0), (1001, 8.0), (7, 50.0)):
        basis = ControlBasis.gaussian_filter(count, sigma)
        assert basis.matrix.shape == (count, count)
        sums = np.array([math.fsum(row) for row in basis.matrix])
        assert np.max(np.abs(sums - 1.0)) <= 1e-15
        assert np.all(basis.matrix >= 0) and np.array_equal(np.argmax(basis.matrix, axis=1),
                                                           np.arange(count))
    # a constant comes through unchanged, a spike is spread out
    basis = ControlBasis.gaussian_filter(33, 2.0)
    assert np.allclose(basis.expand(np.ones((33, 1))), 1.0, atol=1e-15, rtol=0)
    spike = np.zeros((33, 1))
    spike[16] = 1.0
    assert 0.15 < basis.expand(spike)[16, 0] < 0.25


def test_fit_recovers_coefficients():
    rng = np.random.default_rng(3)
    basis = ControlBasis.sine(33, 5)  # orthogonal columns: well conditioned
    assert np.linalg.cond(basis.matrix) < 1.0 + 1e-9
    for c in (rng.standard_normal((5, 2)), rng.standard_normal((3, 5, 2)),
              rng.standard_normal((5, 1)) + 1j * rng.standard_normal((5, 1))):
        fitted = basis.fit(basis.expand(c))
        assert fitted.shape == c.shape and np.iscomplexobj(fitted) == np.iscomplexobj(c)
        assert np.max(np.abs(fitted - c)) <= 1e-10
    with pytest.raises(ValueError):
        basis.fit(np.ones((5, 2)))


# ---- the maps against the reference arithmetic -------------------------------------------------------

KERNEL_SHAPES = [(2, 1, 1, 1), (3, 3, 2, 2), (65, 33, 3, 2), (257, 257, 2, 3), (1001, 12, 4, 2)]


def wide_range(rng, shape):
    """standard_normal * 10^integers(-3, 4): sums whose rounding depends on their order."""
    return rng.standard_normal(shape) * 10.0 ** rng.integers(-3, 4, size=shape)


def kernel_case(shape):
    """(basis, coefficients [B, P, C], gradients [B, Nc, C]) of one (Nc, P, C, B) of KERNEL_SHAPES;
    (3, 3, 2, 2) has a non-symmetric permutation matrix, under which a transposed index shows."""
    nc, P, C, B = shape
    rng = np.random.default_rng(1000 + nc + P)
    if (nc, P) == (3, 3):
        matrix = np.array([[0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [1.0, 0.0, 0.0]])
        assert not np.array_equal(matrix, matrix.T)
    else:
        matrix = wide_range(rng, (nc, P))
    return ControlBasis(matrix), wide_range(rng, (B, P, C)), wide_range(rng, (B, nc, C))


@pytest.mark.parametrize("shape", KERNEL_SHAPES)
def test_maps_agree_with_matmul(shape):
    """1e-13 relative to the magnitude sum |M| |c|: a sum of n <= 1001 terms in any order is within
    n 2^-53 of that (first order), and far closer for rounding errors of mixed sign."""
    basis, c, g = kernel_case(shape)
    m = basis.matrix
    up, down = basis.expand(c), basis.project(g)
    assert up.shape == g.shape and down.shape == c.shape
    assert np.max(np.abs(up - m @ c) / (np.abs(m) @ np.abs(c))) <= 1e-13
    assert np.max(np.abs(down - m.T @ g) / (np.abs(m.T) @ np.abs(g))) <= 1e-13
    z = c + 1j * c[::-1]
    assert np.array_equal(basis.expand(z).real, up)
    assert np.array_equal(basis.expand(z).imag, up[::-1])
    # the defined order, spelled out with Python floats for the first seed's first channel
    for j in (0, shape[0] - 1):
        acc = 0.0
        for p in range(shape[1]):
            acc = acc + float(m[j, p]) * float(c[0, p, 0])
        assert up[0, j, 0] == acc
    for p in (0, shape[1] - 1):
        acc = 0.0
        for j in range(shape[0]):
            acc = acc + float(m[j, p]) * float(g[0, j, 0])
        assert down[0, p, 0] == acc


def test_maps_are_adjoint():
    """<M c, g> = <c, M^T g>. Positive inputs, so that neither inner product cancels and 1e-14 of the
    larger one is some fifty roundings; the inner products themselves are summed exactly."""
    rng = np.random.default_rng(5)
    basis = ControlBasis(rng.uniform(0.5, 1.5, (33, 5)))
    c, g = rng.uniform(0.5, 1.5, (3, 5, 2)), rng.uniform(0.5, 1.5, (3, 33, 2))
    left = math.fsum((basis.expand(c) * g).ravel())
    right = math.fsum((c * basis.project(g)).ravel())
    assert abs(left - right) <= 1e-14 * max(abs(left), abs(right))
    z, w = c + 1j * c[::-1], g - 2j * g
    left = np.sum(basis.expand(z) * np.conj(w))
    right = np.sum(z * np.conj(basis.project(w)))
    assert abs(left - right) <= 1e-13 * abs(left)


@pytest.mark.parametrize("shape", KERNEL_SHAPES)
def test_reversed_summation_order_gives_other_bits(shape):
    """The guard of the bit-identity tests: for these inputs the order matters, so an implementation
    that sums in another order does not pass them. A sum of one or two terms is the same in both
    orders (the addition commutes) and the permutation matrix has one term per sum."""
    basis, c, g = kernel_case(shape)
    nc, P = shape[:2]
    random_matrix = (nc, P) != (3, 3)
    m = basis.matrix
    reverse_expand = ControlBasis(m[:, ::-1]).expand(c[:, ::-1])
    reverse_project = ControlBasis(m[::-1]).project(g[:, ::-1])
    assert np.allclose(reverse_expand, basis.expand(c), rtol=0,
                       atol=1e-12 * np.max(np.abs(m) @ np.abs(c)))
    if random_matrix and P > 2:
        assert not np.array_equal(reverse_expand, basis.expand(c))
    else:
        assert np.array_equal(reverse_expand, basis.expand(c))
    if random_matrix and nc > 2:
        assert not np.array_equal(reverse_project, basis.project(g))
    else:
        assert np.array_equal(reverse_project, basis.project(g))


# ---- the drivers on the oracle backend ----------------------------------------------------------------

def real_problem(bound=2.0):
    case = cases_mod.case_by_name("ctrlcosts_r")  # K = 2, Nc = 17
    args = (case.K, case.Nc, product_cost_list(case), case.T, case.hamiltonian(),
            case.initial_states, case.N)
    kw = dict(cost_eval_step=case.cost_eval_step, log_iteration_step=0,
              max_control_norms=np.full(case.K, bound),
              magnus_policy=getattr(MagnusPolicy, case.magnus))
    return case, args, kw


def complex_problem(bound=2.0):
    case = cases_mod.case_by_name("small_complex_M2")  # K = 1, Nc = 7
    args = (case.K, case.Nc, product_cost_list(case), case.T, case.hamiltonian(),
            case.initial_states, case.N)
    kw = dict(cost_eval_step=case.cost_eval_step, log_iteration_step=0, complex_controls=True,
              max_control_norms=np.full(case.K, bound),
              magnus_policy=getattr(MagnusPolicy, case.magnus))
    return case, args, kw


def lindblad_problem(bound=2.0):
    case = cases_mod.lindblad_case_by_name("lindblad_n4")  # K = 2, Nc = 11
    args = (case.K, case.Nc, lindblad_cost_list(case), case.T, case.initial_densities, case.N)
    kw = dict(cost_eval_step=case.cost_eval_step, hamiltonian=case.hamiltonian(),
              lindblad_data=case.lindblad_data(), log_iteration_step=0,
              max_control_norms=np.full(case.K, bound))
    return case, args, kw


def coefficients(seed, seeds, P, K, sigma, complex_controls=False):
    rng = np.random.default_rng(seed)
    c = sigma * rng.standard_normal((seeds, P, K))
    if complex_controls:
        c = c + 1j * sigma * rng.standard_normal((seeds, P, K))
    return c


def clipped(controls, max_control_norms):
    out = np.array(controls)
    clip_control_norms(out, max_control_norms)
    return out


def test_single_seed_with_a_sine_basis():
    case, args, kw = real_problem(bound=0.5)
    basis = ControlBasis.sine(case.Nc, 5)
    c0 = coefficients(7, 1, 5, case.K, 0.08)[0]
    assert np.max(np.abs(basis.expand(c0))) <= 0.5
    plain = qoc_amd.grape_schroedinger_discrete(*args, initial_controls=basis.expand(c0),
                                                optimizer=Adam(learning_rate=5e-2),
                                                iteration_count=1, **kw)
    assert plain.best_coefficients is None
    out = qoc_amd.grape_schroedinger_discrete(*args, initial_controls=c0.copy(),
                                              optimizer=Adam(learning_rate=5e-2),
                                              iteration_count=12, control_basis=basis, **kw)
    assert out.best_iteration > 0 and out.best_error < plain.best_error
    assert out.best_controls.shape == (case.Nc, case.K)
    assert out.best_coefficients.shape == (5, case.K)
    assert np.all(out.best_controls[0] == 0.0) and np.all(out.best_controls[-1] == 0.0)
    expanded = basis.expand(out.best_coefficients)
    assert np.array_equal(clipped(expanded, kw["max_control_norms"]), out.best_controls)
    # the clip acted on the best pulse, and the coefficients behind it were left alone
    assert np.max(np.abs(expanded)) > 0.5 and np.max(np.abs(out.best_controls)) == 0.5
    assert not np.array_equal(out.best_coefficients, c0)


class Probe(object):
    """An optimizer plugin that takes the gradient at the start and central differences of the error
    in every parameter, through the driver's own function / jacobian callbacks."""

    def __init__(self, step):
        self.step = step

    def run(self, function, iteration_count, initial_params, jacobian, args=()):
        x = np.array(initial_params, dtype=np.float64)
        self.grads = np.array(jacobian(x.copy(), *args)[0])
        self.differences = np.zeros_like(x)
        for i in range(len(x)):
            up, down = x.copy(), x.copy()
            up[i] += self.step
            down[i] -= self.step
            self.differences[i] = (function(up, *args)[0] - function(down, *args)[0]) / (2 * self.step)


def test_coefficient_gradient_against_central_differences():
    """The FD gate of DESIGN section 10: 1e-7 relative to max |g|, with the clip inactive."""
    case, args, kw = real_problem(bound=5.0)
    basis = ControlBasis.sine(case.Nc, 5)
    c0 = coefficients(8, 1, 5, case.K, 0.3)[0]
    assert np.max(np.abs(basis.expand(c0))) < 4.0
    probe = Probe(1e-5)
    qoc_amd.grape_schroedinger_discrete(*args, initial_controls=c0, optimizer=probe,
                                        control_basis=basis, **kw)
    assert probe.grads.shape == (5 * case.K,)
    scale = np.max(np.abs(probe.grads))
    print("max |g|", scale, "max |g - fd|", np.max(np.abs(probe.grads - probe.differences)))
    assert scale > 1e-3
    assert np.max(np.abs(probe.grads - probe.differences)) <= 1e-7 * scale
    # complex controls: the parameters are [Re(c) ..., Im(c) ...]
    case, args, kw = complex_problem(bound=5.0)
    basis = ControlBasis.sine(case.Nc, 3)
    c0 = coefficients(9, 1, 3, case.K, 0.3, complex_controls=True)[0]
    probe = Probe(1e-5)
    qoc_amd.grape_schroedinger_discrete(*args, initial_controls=c0, optimizer=probe,
                                        control_basis=basis, **kw)
    assert probe.grads.shape == (2 * 3 * case.K,)
    scale = np.max(np.abs(probe.grads))
    print("complex: max |g|", scale, "max |g - fd|",
          np.max(np.abs(probe.grads - probe.differences)))
    assert np.max(np.abs(probe.grads - probe.differences)) <= 1e-7 * max(scale, 1e-3)


def test_lindblad_coefficient_gradient_against_central_differences():
    """The directional check and tolerance of
    tests/test_gpu_lindblad.py::test_lindblad_gradient_vs_finite_differences, in the coefficients."""
    case, args, kw = lindblad_problem(bound=5.0)
    basis = ControlBasis.sine(case.Nc, 4)
    c0 = coefficients(10, 1, 4, case.K, 0.3)[0]
    direction = np.random.default_rng(3).standard_normal(c0.size)
    h = 1e-4

    class Directional(object):
        def run(self, function, iteration_count, initial_params, jacobian, args=()):
            x = np.array(initial_params, dtype=np.float64)
            self.slope = float(np.sum(jacobian(x.copy(), *args)[0] * direction))
            self.fd = (function(x + h * direction, *args)[0]
                       - function(x - h * direction, *args)[0]) / (2 * h)

    probe = Directional()
    qoc_amd.grape_lindblad_discrete(*args, initial_controls=c0, optimizer=probe,
                                    control_basis=basis, **kw)
    print("lindblad: slope", probe.slope, "fd", probe.fd)
    assert abs(probe.slope) > 1e-4
    assert abs(probe.fd - probe.slope) < 1e-8 * max(1.0, abs(probe.fd) / 1e-3)


def assert_seed_equals_single(full, one, b, finals="best_final_states"):
    assert one.best_error == full.best_error[b]
    assert one.best_iteration == full.best_iteration[b]
    assert np.array_equal(one.best_controls, full.best_controls[b])
    assert np.array_equal(one.best_coefficients, full.best_coefficients[b])
    assert np.array_equal(getattr(one, finals), getattr(full, finals)[b])


@pytest.mark.parametrize("complex_controls", [False, True], ids=["real", "complex"])
@pytest.mark.parametrize("optimizer", [lambda: Adam(learning_rate=5e-2), LBFGS, lambda: SGD(0.3)],
                         ids=["adam", "lbfgs", "sgd"])
def test_host_batch_equals_single_seed_runs(optimizer, complex_controls):
    case, args, kw = complex_problem(0.6) if complex_controls else real_problem(0.5)
    P, B = (3, 4) if complex_controls else (5, 4)
    basis = ControlBasis.sine(case.Nc, P)
    c0 = coefficients(11, B, P, case.K, 0.08, complex_controls)
    full = qoc_amd.grape_schroedinger_discrete_batch(*args, c0.copy(), optimizer=optimizer(),
                                                     iteration_count=7, control_basis=basis, **kw)
    assert np.any(full.best_iteration > 0)
    assert np.iscomplexobj(full.best_coefficients[0]) == complex_controls
    for b in range(B):
        one = qoc_amd.grape_schroedinger_discrete(*args, initial_controls=c0[b].copy(),
                                                  optimizer=optimizer(), iteration_count=7,
                                                  control_basis=basis, **kw)
        assert_seed_equals_single(full, one, b)
    best = full.best
    b = int(np.argmin(full.best_error))
    assert np.array_equal(best.best_coefficients, full.best_coefficients[b])


def test_lindblad_host_batch_equals_single_seed_runs():
    case, args, kw = lindblad_problem(0.5)
    basis = ControlBasis.gaussian_filter(case.Nc, 1.5)
    c0 = coefficients(12, 3, case.Nc, case.K, 0.3)
    full = qoc_amd.grape_lindblad_discrete_batch(*args, c0.copy(), optimizer=Adam(learning_rate=5e-2),
                                                 iteration_count=5, control_basis=basis, **kw)
    for b in range(3):
        one = qoc_amd.grape_lindblad_discrete(*args, initial_controls=c0[b].copy(),
                                              optimizer=Adam(learning_rate=5e-2), iteration_count=5,
                                              control_basis=basis, **kw)
        assert_seed_equals_single(full, one, b, finals="best_final_densities")


def test_control_conditions_act_on_the_expanded_pulse():
    case, args, kw = real_problem(0.5)
    basis = ControlBasis.gaussian_filter(case.Nc, 1.5)
    c0 = coefficients(13, 2, case.Nc, case.K, 0.3)
    seen = []

    def pin_ends(controls):
        seen.append(controls.shape)
        controls = np.array(controls)
        controls[0] = controls[-1] = 0.0
        return controls

    out = qoc_amd.grape_schroedinger_discrete_batch(
        *args, c0.copy(), optimizer=Adam(learning_rate=5e-2), iteration_count=3,
        control_basis=basis, impose_control_conditions=pin_ends, **kw)
    assert set(seen) == {(case.Nc, case.K)}
    for b in range(2):
        assert np.all(out.best_controls[b][0] == 0.0) and np.all(out.best_controls[b][-1] == 0.0)
        assert np.any(basis.expand(out.best_coefficients[b])[0] != 0.0)


# ---- the resident loop on a NumPy stand-in --------------------------------------------------------------

class NumpyResidentOps(object):
    """What run_batch_resident calls, with the engine's resident state as NumPy arrays: the evaluation
    is the evaluator's evaluate_batch, the basis calls are ControlBasis.expand / project, the
    optimizer kernels the arithmetic of the host steppers. Parameters are kept in the optimizer's
    host format ([Re ..., Im ...] rows for complex controls)."""

    def __init__(self, evaluator, complex_controls):
        self.evaluator = evaluator
        self.complex_controls = complex_controls
        self.basis = None
        self.log = []

    def upload_controls(self, controls):
        self.controls = np.array(controls)
        self.log.append(("upload", self.controls.shape))

    def opt_begin(self):
        raise AssertionError("a run with a basis begins with opt_begin_basis")

    def opt_begin_basis(self, basis, coefficients):
        assert np.array_equal(self.controls, basis.expand(coefficients))
        self.basis = basis
        self.coefficient_shape = coefficients.shape
        self.params = batch_mod._strip_batch(self.complex_controls, np.array(coefficients))
        self.moment = np.zeros_like(self.params)
        self.square_moment = np.zeros_like(self.params)
        B = self.params.shape[0]
        self.best_controls = np.zeros_like(self.controls)
        self.best_params = np.zeros_like(self.params)
        self.best_finals = [None] * B
        self.log.append(("begin_basis", self.params.shape))

    def _coefficients(self, params):
        if self.complex_controls:
            half = params.shape[1] // 2
            params = params[:, :half] + 1j * params[:, half:]
        return params.reshape(self.coefficient_shape)

    def opt_clip(self, max_norms):
        self.controls = self.basis.expand(self._coefficients(self.params))
        for b in range(self.controls.shape[0]):
            clip_control_norms(self.controls[b], max_norms)

    def eval_resident(self, want_grad):
        self.errors, self.grads, self.finals, _ = self.evaluator.evaluate_batch(
            self.controls, want_grad=True)

    def download_costs(self):
        return np.array(self.errors)

    def _keep_best(self, improved):
        for b in np.nonzero(improved)[0]:
            self.best_controls[b] = self.controls[b]
            self.best_params[b] = self.params[b]
            self.best_finals[b] = np.array(self.finals[b])
        return batch_mod._strip_batch(self.complex_controls,
                                      self.basis.project(np.asarray(self.grads)))

    def opt_step(self, kind, improved, update, learning_rate, beta_1=0.0, beta_2=0.0, epsilon=0.0,
                 corr_1=1.0, corr_2=1.0, clip_grads=None):
        grads = self._keep_best(improved)
        assert grads.shape == self.params.shape == self.moment.shape
        for b in np.nonzero(update)[0]:
            g = grads[b]
            if kind == 0:
                self.params[b] = self.params[b] - learning_rate * g
                continue
            if clip_grads is not None:
                g = np.clip(g, -clip_grads, clip_grads)
            self.moment[b] = beta_1 * self.moment[b] + (1 - beta_1) * g
            self.square_moment[b] = beta_2 * self.square_moment[b] + (1 - beta_2) * (g * g)
            hat = self.moment[b] / corr_1
            den = np.sqrt(self.square_moment[b] / corr_2) + epsilon
            self.params[b] = self.params[b] - learning_rate * (hat / den)

    def opt_lbfgs_begin(self, history):
        self.seeds = [LBFGS(history=history) for _ in range(self.params.shape[0])]
        self.log.append(("lbfgs_begin", history))

    def opt_lbfgs_step(self, improved, update, first_step, armijo, shrink, max_backtracks):
        grads = self._keep_best(improved)
        finished = np.zeros(len(self.seeds), dtype=bool)
        for b, seed in enumerate(self.seeds):
            seed.first_step, seed.armijo, seed.shrink = first_step, armijo, shrink
            seed.max_backtracks = max_backtracks
            if update[b]:
                self.params[b] = seed.update(grads[b], self.params[b], self.errors[b])
            finished[b] = seed.finished
        return finished

    def opt_download_best(self):
        finals = [f if f is not None else np.zeros_like(self.finals[0]) for f in self.best_finals]
        return self.best_controls, np.stack(finals)

    def opt_download_best_params(self):
        return self._coefficients(self.best_params)

    def finish(self):
        self.log.append(("finish",))


@pytest.mark.parametrize("which", ["adam_real", "sgd_real", "adam_complex", "lbfgs_real",
                                   "lbfgs_complex", "lbfgs_finishing"])
def test_resident_loop_walks_the_host_loop(which):
    complex_controls = which.endswith("complex")
    case, args, kw = complex_problem(0.6) if complex_controls else real_problem(0.5)
    P, B, iterations = (3 if complex_controls else 5), 4, 8
    basis = ControlBasis.sine(case.Nc, P)
    c0 = coefficients(14, B, P, case.K, 0.08, complex_controls)
    if which.startswith("adam"):
        make = lambda: Adam(learning_rate=5e-2)  # noqa: E731
    elif which.startswith("sgd"):
        make = lambda: SGD(0.3)  # noqa: E731
    elif which == "lbfgs_finishing":
        make = lambda: LBFGS(first_step=1e3, max_backtracks=1)  # noqa: E731
    else:
        make = lambda: LBFGS(history=3)  # noqa: E731

    def run(resident):
        comm, pstate, params = batch_mod.prepare_seeds(
            c0.copy(), complex_controls, case.K, case.Nc, case.T, kw["max_control_norms"], None,
            None, basis)
        assert params.shape == (B, P * case.K * (2 if complex_controls else 1))
        evaluator = SchroedingerEvaluator(
            case.T, case.hamiltonian(), case.initial_states, case.N, control_count=case.K,
            control_eval_count=case.Nc, complex_controls=complex_controls,
            costs=product_cost_list(case), cost_eval_step=case.cost_eval_step,
            magnus_policy=kw["magnus_policy"], need_gradients=True, latency_mode=True)
        optimizer = make()
        stepper = batch_mod.batched_stepper(optimizer, params)
        # the oracle backend has no resident calls: the entry points take the host loop on it
        assert not batch_mod.resident_route(stepper, optimizer, pstate, evaluator, B)
        result = GrapeSchroedingerBatchResult(B)
        tail = (pstate, iterations, 0, 0, comm, result)
        if not resident:
            return batch_mod.run_batch_host(evaluator, stepper, optimizer, params, *tail), None
        ops = NumpyResidentOps(evaluator, complex_controls)
        return batch_mod.run_batch_resident(ops, optimizer, params, *tail), ops

    host, _ = run(False)
    resident, ops = run(True)
    assert ops.log[0] == ("upload", (B, case.Nc, case.K))
    assert ops.log[1] == ("begin_basis", (B, P * case.K * (2 if complex_controls else 1)))
    assert ops.log[-1] == ("finish",)
    assert np.array_equal(host.best_error, resident.best_error)
    assert np.array_equal(host.best_iteration, resident.best_iteration)
    assert np.array_equal(host.iterations_run, resident.iterations_run)
    print(which, "best iterations", host.best_iteration, "iterations run", host.iterations_run)
    if which != "lbfgs_finishing":
        assert np.any(host.best_iteration > 0)
    for b in range(B):
        assert np.array_equal(host.best_controls[b], resident.best_controls[b])
        assert np.array_equal(host.best_coefficients[b], resident.best_coefficients[b])
        assert np.array_equal(host.best_final_states[b], resident.best_final_states[b])
        assert resident.best_coefficients[b].shape == (P, case.K)
    if which == "lbfgs_finishing":
        assert np.any(host.iterations_run < iterations)  # a seed finished at its accepted point
    if which in ("adam_real", "lbfgs_real"):
        assert any(np.max(np.abs(c)) == 0.5 for c in host.best_controls)  # the clip acted


def test_stand_in_backend_without_the_basis_calls_takes_the_host_loop():
    class Evaluator(object):
        def __init__(self, backend):
            self.backend = backend

        def resident_capable(self):
            return True

        def resident_lbfgs_capable(self):
            return True

        def resident_basis_capable(self):
            return (hasattr(self.backend, "opt_begin_basis")
                    and hasattr(self.backend, "opt_download_best_params"))

    class Old(object):
        pass

    class New(object):
        opt_begin_basis = opt_download_best_params = None

    params = np.zeros((2, 6))
    with_basis, without = batch_mod.Dummy(), batch_mod.Dummy()
    for pstate in (with_basis, without):
        pstate.impose_control_conditions = None
    with_basis.control_basis = ControlBasis.sine(5, 3)
    optimizer = Adam()
    stepper = batch_mod.batched_stepper(optimizer, params)
    assert batch_mod.resident_route(stepper, optimizer, without, Evaluator(Old()), 2)
    assert not batch_mod.resident_route(stepper, optimizer, with_basis, Evaluator(Old()), 2)
    assert batch_mod.resident_route(stepper, optimizer, with_basis, Evaluator(New()), 2)


# ---- rejections -------------------------------------------------------------------------------------------

def test_rejections():
    case, args, kw = real_problem(0.5)
    basis = ControlBasis.sine(case.Nc, 5)
    good = coefficients(15, 2, 5, case.K, 0.1)
    single, many = qoc_amd.grape_schroedinger_discrete, qoc_amd.grape_schroedinger_discrete_batch
    with pytest.raises(NotImplementedError, match="save"):
        single(*args, initial_controls=good[0], control_basis=basis, save_file_path="x.h5", **kw)
    lcase, largs, lkw = lindblad_problem(0.5)
    lbasis = ControlBasis.sine(lcase.Nc, 4)
    with pytest.raises(NotImplementedError, match="save"):
        qoc_amd.grape_lindblad_discrete(*largs, initial_controls=np.zeros((4, lcase.K)),
                                        control_basis=lbasis, save_file_path="x.h5", **lkw)
    with pytest.raises(ValueError):  # no coefficients
        single(*args, control_basis=basis, **kw)
    with pytest.raises(ValueError):
        many(*args, None, control_basis=basis, **kw)
    with pytest.raises(ValueError):  # knots where coefficients belong
        single(*args, initial_controls=np.zeros((case.Nc, case.K)), control_basis=basis, **kw)
    with pytest.raises(ValueError):
        many(*args, np.zeros((2, case.Nc, case.K)), control_basis=basis, **kw)
    with pytest.raises(ValueError):
        many(*args, good[0], control_basis=basis, **kw)
    with pytest.raises(ValueError):  # a basis for another knot count
        single(*args, initial_controls=good[0], control_basis=ControlBasis.sine(case.Nc + 1, 5),
               **kw)
    with pytest.raises(ValueError):
        many(*args, good, control_basis=ControlBasis.sine(case.Nc + 1, 5), **kw)
    with pytest.raises(ValueError):  # the expanded start pulse exceeds max_control_norms
        single(*args, initial_controls=10.0 * np.ones((5, case.K)), control_basis=basis, **kw)
    with pytest.raises(ValueError):
        many(*args, 10.0 * np.ones((2, 5, case.K)), control_basis=basis, **kw)
    with pytest.raises(ValueError):  # complex coefficients go with complex_controls
        single(*args, initial_controls=good[0] * (1 + 1j), control_basis=basis, **kw)
    with pytest.raises(ValueError):
        qoc_amd.grape_lindblad_discrete(*largs, control_basis=lbasis, **lkw)
    with pytest.raises(ValueError):
        qoc_amd.grape_lindblad_discrete_batch(*largs, np.zeros((2, lcase.Nc, lcase.K)),
                                              control_basis=lbasis, **lkw)
