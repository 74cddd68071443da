"""
Host tests (no GPU) of the costs of the controls alone on the resident multi-start route: the
descriptors the four classes hand to the engine, the NumPy model of the device arithmetic
(tests/control_cost_model.py) against cost() / controls_bar(), when the evaluators answer
resident_capable(), the batch drivers on a NumPy stand-in of the resident entry points, and the ABI.

Gates (eps = 2^-52, T = number of terms a sum runs over): costs to 4 T eps relative; gradients of
ControlNorm / ControlArea to 8 eps of the largest entry, of ControlVariation to 16 * 2^order * eps,
ControlBandwidthMax cost and gradient to Nc eps.
"""

import os
import subprocess

import numpy as np
import pytest

import qoc_amd
from qoc_amd import engine
from qoc_amd.core import batch as batch_mod
from qoc_amd.core import device, structure
from qoc_amd.standard import SGD, Adam
from qoc_amd.standard.costs import (ControlArea, ControlBandwidthMax, ControlNorm,
                                    ControlVariation, TargetStateInfidelity)
from tests import cases as cases_mod
from tests import control_cost_model as model
from tests import helpers
from tests.oracle_backend import OracleBackend

EPS = 2.0 ** -52
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. descriptors --------------------------------------------------------------------------------

def test_descriptors_of_the_four_classes():
    K, Nc = 3, 8
    mx, w = np.array([1.0, 2.0, 0.5]), np.array([1.0, 0.0, 3.0])
    d = ControlNorm(K, Nc, control_weights=w, cost_multiplier=0.3,
                    max_control_norms=mx).control_descriptor(K, Nc, False)
    assert d["kind"] == engine.CONTROL_NORM and d["multiplier"] == 0.3 / (K * Nc)
    assert np.array_equal(d["max_norms"], mx) and np.array_equal(d["weights"], w)
    d = ControlNorm(K, Nc).control_descriptor(K, Nc, True)
    assert d["max_norms"] is None and d["weights"] is None and d["multiplier"] == 1.0 / (K * Nc)
    d = ControlVariation(K, Nc, cost_multiplier=2.0, max_control_norms=mx,
                         order=2).control_descriptor(K, Nc, False)
    assert d["kind"] == engine.CONTROL_VARIATION and d["order"] == 2
    assert d["multiplier"] == 2.0 / (K * (Nc - 2) * 4) and np.array_equal(d["max_norms"], mx)
    d = ControlArea(K, Nc, cost_multiplier=0.7, max_control_norms=mx).control_descriptor(K, Nc, False)
    assert d["kind"] == engine.CONTROL_AREA and d["multiplier"] == 0.7 / (K * Nc)
    assert np.array_equal(d["max_norms"], mx)
    T = 2.0
    freqs = np.fft.fftfreq(Nc, d=T / (Nc - 1))
    bw = np.array([freqs[2], freqs[3] - 1e-9, -1e9])
    d = ControlBandwidthMax(K, Nc, T, bw, cost_multiplier=1.5).control_descriptor(K, Nc, False)
    assert d["kind"] == engine.CONTROL_BANDWIDTH_MAX and d["multiplier"] == 1.5 / K
    assert [list(b) for b in d["bins"]] == [[2, 3], [3], list(range(Nc))]


def test_descriptors_the_host_keeps():
    K, Nc = 2, 6
    # ControlArea without max_control_norms: cost() raises the reference's NameError
    area = ControlArea(K, Nc)
    assert area.control_descriptor(K, Nc, False) is None
    with pytest.raises(NameError):
        area.cost(np.zeros((Nc, K)), None, 0)
    # no DFT bin at or above the bandwidth
    assert ControlBandwidthMax(K, Nc, 1.0, [1.0, 1e9]).control_descriptor(K, Nc, False) is None
    # shapes that do not match the problem
    assert ControlNorm(K, Nc + 1).control_descriptor(K, Nc, False) is None
    assert ControlNorm(K, Nc, max_control_norms=np.ones(K + 1)).control_descriptor(K, Nc, False) is None
    assert ControlNorm(K, Nc, control_weights=np.ones((Nc, K))).control_descriptor(K, Nc, False) is None
    assert ControlVariation(K, Nc + 1).control_descriptor(K, Nc, False) is None
    assert ControlVariation(K, Nc, order=Nc).control_descriptor(K, Nc, False) is None
    assert ControlArea(K + 1, Nc, max_control_norms=np.ones(K + 1)).control_descriptor(K, Nc, False) is None
    assert ControlBandwidthMax(K, Nc + 1, 1.0, [0.0, 0.0]).control_descriptor(K, Nc, False) is None
    assert ControlBandwidthMax(K, Nc, 1.0, [0.0]).control_descriptor(K, Nc, False) is None


# ---- 2. the model of the device arithmetic against the Python classes ------------------------------

def random_controls(rng, Nc, K, cplx):
    u = rng.standard_normal((Nc, K))
    return u + 1j * rng.standard_normal((Nc, K)) if cplx else u


def check_against_class(cost, u, cplx, terms, grad_gate):
    """The model on the descriptor of `cost` against cost.cost() / cost.controls_bar() at `u`;
    returns the two relative deviations."""
    Nc, K = u.shape
    desc = cost.control_descriptor(K, Nc, cplx)
    assert desc is not None
    value, grad = model.control_costs(structure.to_real_controls(u, cplx), [desc], cplx)
    want = cost.cost(u, None, 0)
    want_grad = structure.to_real_controls(cost.controls_bar(u, None, 0), cplx)
    dev_cost = abs(value - want) / abs(want) if want != 0 else abs(value)
    scale = np.max(np.abs(want_grad))
    dev_grad = np.max(np.abs(grad - want_grad)) / scale if scale > 0 else np.max(np.abs(grad))
    assert dev_cost <= 4 * terms * EPS, (type(cost).__name__, dev_cost / EPS)
    assert dev_grad <= grad_gate, (type(cost).__name__, dev_grad / EPS)
    return dev_cost, dev_grad


@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("Nc", [2, 3, 9, 64, 1001])
def test_model_equals_the_python_classes(Nc, cplx):
    K = 3
    rng = np.random.default_rng(40 + Nc + cplx)
    u = random_controls(rng, Nc, K, cplx)
    mx, w = rng.uniform(0.5, 2.0, K), rng.uniform(0.0, 2.0, K)
    check_against_class(ControlNorm(K, Nc, control_weights=w, cost_multiplier=0.3,
                                    max_control_norms=mx), u, cplx, Nc * K * (1 + cplx), 8 * EPS)
    check_against_class(ControlNorm(K, Nc), u, cplx, Nc * K * (1 + cplx), 8 * EPS)
    check_against_class(ControlArea(K, Nc, cost_multiplier=1.7, max_control_norms=mx), u, cplx,
                        Nc * K, 8 * EPS)
    for order in (1, 2, 3):
        if order < Nc:
            for norms in (None, mx):
                check_against_class(
                    ControlVariation(K, Nc, cost_multiplier=0.9, max_control_norms=norms, order=order),
                    u, cplx, (Nc - order) * K * (1 + cplx), 16 * 2 ** order * EPS)
    T = 3.0
    freqs = np.fft.fftfreq(Nc, d=T / (Nc - 1))
    # every control with at least two bins (one bin alone: the cost is identically 1 and its
    # gradient nothing but rounding noise); at Nc = 2, 3 that means all bins
    if Nc <= 3:
        bw = np.full(K, -1e9)
    else:
        bw = np.array([freqs[Nc // 4], freqs[Nc // 3] - 1e-9, -1e9])
    bandwidth = ControlBandwidthMax(K, Nc, T, bw, cost_multiplier=1.3)
    assert all(len(b) >= 2 for b in bandwidth.control_descriptor(K, Nc, cplx)["bins"])
    desc = bandwidth.control_descriptor(K, Nc, cplx)
    value, grad = model.control_costs(structure.to_real_controls(u, cplx), [desc], cplx)
    want = bandwidth.cost(u, None, 0)
    want_grad = structure.to_real_controls(bandwidth.controls_bar(u, None, 0), cplx)
    assert abs(value - want) <= Nc * EPS * abs(want), abs(value - want) / abs(want) / EPS
    dev = np.max(np.abs(grad - want_grad)) / np.max(np.abs(want_grad))
    assert dev <= Nc * EPS, dev / EPS


def test_model_zero_area_sum_and_tied_maximum():
    Nc, K = 4, 2
    u = np.array([[1.0, 0.3], [-1.0, 0.2], [0.5, -0.1], [-0.5, 0.4]])
    area = ControlArea(K, Nc, max_control_norms=np.array([2.0, 1.0]))
    _, grad = model.control_costs(u, [area.control_descriptor(K, Nc, False)], False)
    assert np.all(grad[:, 0] == 0.0) and np.all(grad[:, 1] != 0.0)
    assert np.array_equal(grad, area.controls_bar(u, None, 0))
    uc = u[:, :1] + 1j * np.array([[2.0], [-2.0], [0.25], [-0.25]])
    area = ControlArea(1, Nc, max_control_norms=np.array([2.0]))
    _, grad = model.control_costs(structure.to_real_controls(uc, True),
                                  [area.control_descriptor(1, Nc, True)], True)
    assert np.all(grad == 0.0)
    # a pulse at the first knot: every bin has the same modulus, the first one is "the" maximum
    Nc = 8
    u = np.zeros((Nc, 1))
    u[0, 0] = 0.7
    bandwidth = ControlBandwidthMax(1, Nc, 1.0, [-1e9])
    desc = bandwidth.control_descriptor(1, Nc, False)
    value, grad = model.control_costs(u, [desc], False)
    assert value == bandwidth.cost(u, None, 0) == 1.0
    want = bandwidth.controls_bar(u, None, 0)
    assert np.max(np.abs(grad - want)) <= Nc * EPS * np.max(np.abs(want))
    assert np.max(np.abs(want)) > 0.1


def test_model_of_the_complex_clip():
    rng = np.random.default_rng(3)
    z = rng.standard_normal((5, 7, 2)) + 1j * rng.standard_normal((5, 7, 2))
    mx = np.array([0.8, 1.5])
    want = z.copy()
    for i, m in enumerate(mx):  # clip_control_norms of the product (core/batch.py)
        col = want[:, :, i]
        mod = np.abs(col)
        over = np.less(m, mod)
        col[over] = (col[over] / mod[over]) * m
    got = model.clip_complex(structure.to_real_controls(z, True), mx)
    assert np.max(np.abs(got - structure.to_real_controls(want, True))) <= 4 * EPS * 1.5
    assert np.any(np.abs(z) > mx) and np.any(np.abs(z) < mx)


# ---- 3. resident_capable ---------------------------------------------------------------------------

class ResidentOracle(OracleBackend):
    """The oracle backend with the resident entry points of the Schroedinger path: optimizer
    states as NumPy arrays, the control costs and the complex clip from the model."""

    def __init__(self):
        super().__init__()
        self.control_costs = []
        self.cplx = False

    def set_control_costs(self, path, complex_controls, descriptors):
        assert path == engine.PATH_SCHROEDINGER
        self.control_costs, self.cplx = list(descriptors), bool(complex_controls)

    def _begin(self, complex_mode):
        self.params = np.stack(self.controls).copy()
        self.complex_mode = complex_mode
        self.m, self.v = np.zeros_like(self.params), np.zeros_like(self.params)
        self.best_controls = np.zeros_like(self.params)
        self.best_final = None

    def opt_begin(self):
        self._begin(False)

    def opt_begin_complex(self):
        self._begin(True)

    clipped_entries = 0  # (of all instances: the tests read it to see that a clip acted)

    def opt_clip(self, max_norms):
        if self.complex_mode:
            self.controls = list(model.clip_complex(self.params, max_norms))
            ResidentOracle.clipped_entries += int(np.sum(np.stack(self.controls) != self.params))
            return
        mod = np.abs(self.params)
        over = np.less(max_norms, mod)
        ResidentOracle.clipped_entries += int(np.sum(over))
        clipped = (self.params / np.where(over, mod, 1.0)) * max_norms
        self.params = np.where(over, clipped, self.params)
        self.controls = list(self.params)

    def eval_resident(self, want_grad=True):
        super().eval_resident(want_grad)
        for b, u in enumerate(self.controls):
            if self.control_costs:
                value, grad = model.control_costs(u, self.control_costs, self.cplx, want_grad)
                self.cost[b] = self.cost[b] + value
                if want_grad:
                    self.grads[b] = self.grads[b] + grad

    def download_costs(self):
        return np.array(self.cost, dtype=np.float64)

    def opt_step(self, kind, improved, update, learning_rate, beta_1=0.0, beta_2=0.0, epsilon=0.0,
                 corr_1=1.0, corr_2=1.0, clip_grads=None):
        final = np.stack(self.final)
        if self.best_final is None:
            self.best_final = np.zeros_like(final)
        improved, update = np.asarray(improved, dtype=bool), np.asarray(update, dtype=bool)
        self.best_controls[improved] = np.stack(self.controls)[improved]
        self.best_final[improved] = final[improved]
        g = np.stack(self.grads)
        if kind == 0:
            new = self.params - learning_rate * g
        else:
            if clip_grads is not None:
                g = np.clip(g, -clip_grads, clip_grads)
            m = beta_1 * self.m + (1 - beta_1) * g
            v = beta_2 * self.v + (1 - beta_2) * (g * g)
            new = self.params - learning_rate * ((m / corr_1) / (np.sqrt(v / corr_2) + epsilon))
            self.m[update], self.v[update] = m[update], v[update]
        self.params[update] = new[update]
        if not self.complex_mode:
            self.controls = list(self.params)

    def opt_download_best(self):
        return self.best_controls.copy(), self.best_final.copy()


def evaluator(backend, costs, complex_controls=False, K=2, Nc=6, n=3, N=7):
    rng = np.random.default_rng(11)
    h0 = cases_mod.gue(rng, n)
    gs = [cases_mod.gue(rng, n) for _ in range(2 * K)]

    def hamiltonian(u, t):
        out = h0
        for k in range(K):
            out = out + (u[k].real * gs[2 * k] + u[k].imag * gs[2 * k + 1] if complex_controls
                         else u[k] * gs[k])
        return out
    psi0 = cases_mod.column_states(np.eye(n)[:, :1])
    target = cases_mod.column_states(np.roll(np.eye(n), 1, axis=0)[:, :1])
    all_costs = [TargetStateInfidelity(target)] + list(costs)
    ev = device.SchroedingerEvaluator(1.0, hamiltonian, psi0, N, control_count=K,
                                      control_eval_count=Nc, complex_controls=complex_controls,
                                      costs=all_costs, backend=backend)
    return ev, (K, Nc, all_costs, 1.0, hamiltonian, psi0, N)


def test_resident_capable_needs_descriptors_and_entry_points():
    K, Nc = 2, 6
    variation = ControlVariation(K, Nc, order=2)

    class TodaysStandIn(OracleBackend):  # the resident entry points of the parent commit only
        def opt_step(self, *args, **kwargs):
            raise AssertionError("not reached")

    ev, _ = evaluator(TodaysStandIn(), [variation])
    assert ev.host_costs == [variation] and not ev.resident_capable()
    assert not evaluator(TodaysStandIn(), [], complex_controls=True)[0].resident_capable()
    assert evaluator(TodaysStandIn(), [])[0].resident_capable()
    ev, _ = evaluator(ResidentOracle(), [variation, ControlNorm(K, Nc)])
    assert ev.resident_capable()
    assert [d["kind"] for d in ev.control_cost_descriptors] == [engine.CONTROL_VARIATION,
                                                                engine.CONTROL_NORM]
    assert evaluator(ResidentOracle(), [variation], complex_controls=True)[0].resident_capable()
    ev, _ = evaluator(ResidentOracle(), [variation, ControlArea(K, Nc)])  # (no max_control_norms)
    assert ev.control_cost_descriptors[1] is None and not ev.resident_capable()

    class UserCost(ControlNorm):
        control_descriptor = None

    assert not evaluator(ResidentOracle(), [UserCost(K, Nc)])[0].resident_capable()


def test_lindblad_resident_capable_needs_descriptors_and_entry_points():
    case = cases_mod.lindblad_case_by_name("lindblad_n4")
    norm = ControlNorm(case.K, case.Nc)

    class Today(OracleBackend):
        def lindblad_opt_step(self, *args, **kwargs):
            raise AssertionError("not reached")

    class Resident(Today):
        def set_control_costs(self, *args):
            raise AssertionError("not reached")

        def lindblad_opt_begin_complex(self):
            raise AssertionError("not reached")

    def make(backend, costs):
        return device.LindbladEvaluator(
            case.T, case.initial_densities, case.N, hamiltonian=case.hamiltonian(),
            lindblad_data=case.lindblad_data(), control_count=case.K, control_eval_count=case.Nc,
            costs=costs, backend=backend)
    assert make(Today(), []).resident_capable()
    assert not make(Today(), [norm]).resident_capable()
    assert make(Resident(), [norm]).resident_capable()
    assert not make(Resident(), [norm, ControlArea(case.K, case.Nc)]).resident_capable()


# ---- 4. the batch driver on the stand-in of the resident entry points ------------------------------

class PluginAdam(Adam):  # not type(...) is Adam: takes the host loop
    pass


@pytest.fixture
def routes(monkeypatch):
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
    return taken


@pytest.fixture
def resident_oracle():
    helpers.set_backend_factory(ResidentOracle)
    ResidentOracle.clipped_entries = 0
    yield
    helpers.set_backend_factory(None)


def both_routes(args, u0, routes, **kw):
    kw = dict(dict(iteration_count=5, log_iteration_step=0), **kw)
    a = qoc_amd.grape_schroedinger_discrete_batch(*args, u0.copy(),
                                                  optimizer=Adam(learning_rate=5e-2), **kw)
    assert routes == {"resident": 1, "host": 0}
    b = qoc_amd.grape_schroedinger_discrete_batch(*args, u0.copy(),
                                                  optimizer=PluginAdam(learning_rate=5e-2), **kw)
    assert routes == {"resident": 1, "host": 1}
    return a, b


def test_complex_controls_resident_equals_host_loop_bit_for_bit(routes, resident_oracle):
    _, args = evaluator(ResidentOracle(), [], complex_controls=True)
    K, Nc = args[0], args[1]
    rng = np.random.default_rng(21)
    u0 = 0.2 * (rng.standard_normal((3, Nc, K)) + 1j * rng.standard_normal((3, Nc, K)))
    a, b = both_routes(args, u0, routes, complex_controls=True, max_control_norms=np.full(K, 5.0))
    assert np.array_equal(a.best_error, b.best_error)
    assert np.array_equal(a.best_iteration, b.best_iteration)
    for s in range(3):
        assert np.iscomplexobj(a.best_controls[s]) and a.best_controls[s].shape == (Nc, K)
        assert np.max(np.abs(a.best_controls[s])) < 5.0  # (the clip never acted)
        assert np.array_equal(a.best_controls[s], b.best_controls[s])
        assert np.array_equal(a.best_final_states[s], b.best_final_states[s])


@pytest.mark.parametrize("cplx", [False, True])
def test_control_costs_resident_equals_host_loop(cplx, routes, resident_oracle):
    K, Nc = 2, 6
    mx = np.array([0.5, 0.7])
    costs = [ControlVariation(K, Nc, cost_multiplier=0.5, order=2),
             ControlBandwidthMax(K, Nc, 1.0, [0.8, -1e9], cost_multiplier=0.2),
             ControlNorm(K, Nc, cost_multiplier=0.03, max_control_norms=mx),
             ControlArea(K, Nc, cost_multiplier=0.04, max_control_norms=mx)]
    _, args = evaluator(ResidentOracle(), costs, complex_controls=cplx)
    rng = np.random.default_rng(22)
    u0 = 0.45 * rng.standard_normal((3, Nc, K))
    if cplx:
        u0 = u0 + 0.45j * rng.standard_normal((3, Nc, K))
    u0[np.abs(u0) > mx] *= 0.3
    # entries next to the bound, both signs: Adam steps of 5e-2 take some of them beyond it
    u0[0, :, 0] = 0.495 * (1 - 0.1 * rng.uniform(size=Nc)) * (np.exp(0.3j) if cplx else 1.0)
    u0[1, :, 0] = -u0[0, :, 0]
    a, b = both_routes(args, u0, routes, complex_controls=cplx, max_control_norms=mx)
    assert np.array_equal(a.best_iteration, b.best_iteration)
    for s in range(3):
        assert abs(a.best_error[s] - b.best_error[s]) < 1e-12
        assert helpers.rel_err(a.best_controls[s], b.best_controls[s]) < 1e-10
        assert np.all(np.abs(a.best_controls[s]) <= mx * (1 + 4 * EPS))
    assert ResidentOracle.clipped_entries > 0


def test_finish_clears_the_control_costs_when_the_loop_fails(resident_oracle):
    K, Nc = 2, 6
    backend = ResidentOracle()
    ev, args = evaluator(backend, [ControlNorm(K, Nc)])
    from qoc_amd.core.schroedingerdiscrete import _ResidentOps
    ops = _ResidentOps(backend, ev.control_cost_descriptors, False)
    ops.opt_clip = None  # the first call of the loop after the upload fails
    comm, pstate, params = batch_mod.prepare_seeds(np.zeros((2, Nc, K)), False, K, Nc, 1.0, None,
                                                   None, None)
    with pytest.raises(TypeError):
        batch_mod.run_batch_resident(ops, SGD(), params, pstate, 2, 0, 0, comm,
                                     qoc_amd.core.schroedingerdiscrete.GrapeSchroedingerBatchResult(2))
    assert backend.control_costs == []


# ---- 5. ABI ----------------------------------------------------------------------------------------

NEW_SYMBOLS = ("qocx_set_control_costs", "qocx_eval_control_costs", "qocx_opt_begin_complex",
               "qocx_lindblad_opt_begin_complex")


def test_the_abi_declares_the_entry_points():
    header = open(os.path.join(ROOT, "include", "qocx.h")).read()
    lib = engine.load_library()
    for name in NEW_SYMBOLS:
        assert "int {}(".format(name) in header
        assert name in engine.SIGNATURES
        assert hasattr(lib, name)
    exported = subprocess.run(["nm", "-D", "--defined-only", engine.LIBRARY_PATH],
                              capture_output=True, text=True, check=True).stdout
    for name in NEW_SYMBOLS:
        assert " T {}\n".format(name) in exported
    for method in ("set_control_costs", "eval_control_costs", "opt_begin_complex",
                   "lindblad_opt_begin_complex"):
        assert hasattr(engine.Engine, method)
    for name, value in (("QOCX_CONTROL_NORM", engine.CONTROL_NORM),
                        ("QOCX_CONTROL_VARIATION", engine.CONTROL_VARIATION),
                        ("QOCX_CONTROL_AREA", engine.CONTROL_AREA),
                        ("QOCX_CONTROL_BANDWIDTH_MAX", engine.CONTROL_BANDWIDTH_MAX),
                        ("QOCX_PATH_SCHROEDINGER", engine.PATH_SCHROEDINGER),
                        ("QOCX_PATH_LINDBLAD", engine.PATH_LINDBLAD)):
        assert "#define {} {}".format(name, value) in header


def test_the_control_cost_kernels_do_not_spill():
    from tests.test_build_resources import resources
    table = resources("qocx_ctrlcost.hip")
    kernels = [k for k in table if "kernel" in k]
    assert len(kernels) == 9, kernels  # seed kernel, weights, add, 2 forward and 4 backward forms
    for name in kernels:
        assert table[name]["ScratchSize"] == 0 and table[name]["VGPRs Spill"] == 0, name
        assert table[name]["LDS Size"] <= 64 * 1024, name
