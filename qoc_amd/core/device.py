"""
device.py - the bridge between the reference-shaped host API and the HIP engine.

`SchroedingerEvaluator` plays the role of `_evaluate_schroedinger_discrete` and of
`ans_jacobian(_evaluate_schroedinger_discrete, 0)` (qoc/core/schroedingerdiscrete.py:318-319,
:356-438): given controls it returns the total error, its gradient and the final states - for
one control array or for a batch of independent seeds - by ONE call into libqocx.
"""

import numpy as np

from qoc_amd.core import structure
from qoc_amd.models.policies import InterpolationPolicy, MagnusPolicy
from qoc_amd.standard.hamiltonians import (HamiltonianEnsemble, HamiltonianSweep, LindbladSweep,
                                            QuadraticHamiltonian)

def make_backend(device=-1):
    """The HIP engine. There is no CPU fallback: this raises when libqocx.so or the GPU is
    missing."""
    from qoc_amd.engine import Engine
    return Engine(device)


_FD_STEP = 1e-6

# matrix_free="states" / "all": the most states per seed that take the matrix-free route (the engine's
# knob "action_states"). The engine accepts up to 4; this is the largest count at which the route's median
# evaluation was below the Pade route's fastest one in every run (n = 32, 256 seeds x 1000 steps: 10.9 ms
# against 11.3 at two states, 18.4 against 13.5 at three - tools/bench_action_states.py,
# profiles/action_states.jsonl).
ACTION_STATES_DEFAULT = 2
MATRIX_FREE_VALUES = ("default", "wide", "states", "all", "costs")
# ... and the value that opts n <= 16 in (knob "action_small"), beside the tuple existing callers enumerate
MATRIX_FREE_SMALL = "small"
# ... and the value that opts problems on effective controls in (knob "action_eff"): M4 on a time-independent
# system, a QuadraticHamiltonian under M2
MATRIX_FREE_EFFECTIVE = "effective"
# Every accepted value and the engine knobs it sets, in the order they are set
MATRIX_FREE_KNOBS = {
    "default": (),
    "wide": (("action", 2),),
    "states": (("action_states", ACTION_STATES_DEFAULT),),
    "all": (("action", 2), ("action_states", ACTION_STATES_DEFAULT)),
    "costs": (("action_costs", 1),),
    MATRIX_FREE_SMALL: (("action_small", 1),),
    MATRIX_FREE_EFFECTIVE: (("action_eff", 1),),
}


def interpolation_keywords(backend, setter, interpolation_policy):
    """The keyword a backend's problem setter takes for `interpolation_policy`: none for LINEAR
    (every backend's default), interpolation="piecewise_constant" otherwise - from a backend
    whose setter takes it; there is no fallback to another policy."""
    if interpolation_policy == InterpolationPolicy.LINEAR:
        return {}
    import inspect
    if "interpolation" not in inspect.signature(getattr(backend, setter)).parameters:
        raise NotImplementedError("the backend {!r} does not evaluate the interpolation policy {}"
                                  "".format(backend, interpolation_policy))
    return dict(interpolation=interpolation_policy.short)


def control_cost_descriptors(host_costs, control_count, control_eval_count, complex_controls):
    """One entry per cost of the controls alone: the dict engine.set_control_costs() takes, or None
    where only the host can evaluate the cost (a user plugin without control_descriptor(), or a
    built-in one that declines)."""
    out = []
    for cost in host_costs:
        hook = getattr(cost, "control_descriptor", None)
        out.append(None if hook is None
                   else hook(control_count, control_eval_count, complex_controls))
    return out


def controls_stay_resident(backend, descriptors, complex_controls, begin_complex):
    """The resident drivers can take these costs of the controls (every one has a descriptor and
    the backend evaluates them) and this kind of controls (complex ones need the backend's complex
    clip, `begin_complex`)."""
    if complex_controls and not hasattr(backend, begin_complex):
        return False
    if not descriptors:
        return True
    return (all(d is not None for d in descriptors) and hasattr(backend, "set_control_costs"))


def reject_costless_lindblad_ensemble(hamiltonian, costs):
    """An ensemble on the Lindblad path needs at least one cost: its error is the weighted sum of
    the members' costs and member_errors is what it returns - with no cost there is nothing to
    weigh."""
    if isinstance(hamiltonian, HamiltonianEnsemble) and len(list(costs)) == 0:
        raise NotImplementedError(
            "a HamiltonianEnsemble on the Lindblad path needs at least one cost: its error is the "
            "weighted sum of the members' costs (costs is empty)")


def reject_sweep(hamiltonian, where, hint="", lindblad_sweep_ok=False):
    """The entry points that do not take a HamiltonianSweep say so by name. lindblad_sweep_ok: this
    one takes a LindbladSweep (the batch entry points of the Lindblad path)."""
    if lindblad_sweep_ok and isinstance(hamiltonian, LindbladSweep):
        return
    if isinstance(hamiltonian, HamiltonianSweep):
        raise NotImplementedError("a {} is not evaluated by {}{}".format(
            type(hamiltonian).__name__, where, hint))


LINDBLAD_SWEEP_HINT = (": a duration there scales the dissipation rates as well, which a plain "
                       "HamiltonianSweep does not state (a LindbladSweep does: pass one to "
                       "grape_lindblad_discrete_batch or LindbladEvaluator)")


def reject_lindblad_sweep(hamiltonian):
    """The Schroedinger entry points: a LindbladSweep scales dissipation rates, and there are none."""
    if isinstance(hamiltonian, LindbladSweep):
        raise ValueError(
            "a LindbladSweep scales the dissipation rates of lindblad_data: the Schroedinger path "
            "has none, so there is nothing to scale (use the Lindblad entry points, or a "
            "HamiltonianSweep)")


def user_states_bar(cost, controls, states, step):
    """
    d cost / d Re(states) + i d cost / d Im(states) of a user Cost: its states_bar() hook when it
    has one, else central differences of cost() (4 evaluations per state component; the
    reference gets this from autograd).
    """
    hook = getattr(cost, "states_bar", None)
    if hook is not None:
        out = hook(controls, states, step)
        if out is not None:
            return np.asarray(out, dtype=np.complex128).reshape(states.shape)
    states = np.array(states, dtype=np.complex128)
    out = np.zeros_like(states)
    flat, oflat = states.reshape(-1), out.reshape(-1)
    for idx in range(flat.size):
        keep = flat[idx]
        h = _FD_STEP * max(1.0, abs(keep))
        vals = []
        for delta in (h, -h, 1j * h, -1j * h):
            flat[idx] = keep + delta
            vals.append(cost.cost(controls, states, step))
        flat[idx] = keep
        oflat[idx] = (vals[0] - vals[1]) / (2 * h) + 1j * (vals[2] - vals[3]) / (2 * h)
    return out


def user_controls_bar(cost, controls, states, step):
    """The same for the explicit dependence of a user Cost on the controls (`uses_controls = False`
    on the class skips it; a controls_bar() hook replaces the finite differences)."""
    if getattr(cost, "uses_controls", True) is False:
        return 0.0
    hook = getattr(cost, "controls_bar", None)
    if hook is not None:
        out = hook(controls, states, step)
        if out is not None:
            return np.asarray(out)
    controls = np.array(controls)
    out = np.zeros(controls.shape, dtype=np.complex128)
    flat, oflat = controls.reshape(-1), out.reshape(-1)
    deltas = (1.0, 1j) if np.iscomplexobj(controls) else (1.0,)
    for idx in range(flat.size):
        keep = flat[idx]
        h = _FD_STEP * max(1.0, abs(keep))
        for d in deltas:
            flat[idx] = keep + d * h
            up = cost.cost(controls, states, step)
            flat[idx] = keep - d * h
            down = cost.cost(controls, states, step)
            oflat[idx] += d * (up - down) / (2 * h)
        flat[idx] = keep
    return out


class _Evaluator(object):
    """
    What the Schroedinger and the Lindblad evaluator share: cost triage, the batch protocol of
    evaluate_batch (one or two device passes, step states kept for exactly as long as they are
    needed), the host's share of the costs and the resident-capability test. "States" are state
    vectors or densities. A subclass probes and sets its problem and supplies
      _pass(controls_batch, device_controls, want_grad, again) -> (cost, grads, final),
      _download_steps(), _set_cotangents(steps, bars), _problem_stays_resident(),
      _set_linearized_problem(controls, device_controls),
    and the class attributes below.
    """

    opt_prefix = ""           # of the backend's resident-driver methods (opt_step, ...)
    subtotal_costs = True     # the order in which evaluate_batch sums the host's costs (see there)
    linearized_route = ""     # names the linearised route in an error message
    linearized_hamiltonian = None
    _cost_controls = None     # controls the costs see in place of the evaluated ones
    ensemble = None           # the HamiltonianEnsemble being evaluated
    sweep = None              # the HamiltonianSweep being evaluated
    ensemble_setter = "set_ensemble"                 # the backend's entry points for one
    ensemble_member_costs = "ensemble_member_costs"
    sweep_setter = "set_sweep"                       # ... and for a sweep

    # -- Hamiltonian ensembles ------------------------------------------------------------------
    def _ensemble_base(self, ensemble, control_count, complex_controls, backend,
                       quadratic_ok=False):
        """Checks an ensemble against this problem and the backend, keeps it with the arguments
        of the backend's setter (self._ensemble_args) and returns its base Hamiltonian.
        quadratic_ok: this path takes a QuadraticHamiltonian base on this backend."""
        base = ensemble.hamiltonian
        if control_count == 0:
            raise NotImplementedError("a HamiltonianEnsemble needs at least one control "
                                      "(control_count = 0)")
        if isinstance(base, (HamiltonianEnsemble, HamiltonianSweep)) or (
                isinstance(base, QuadraticHamiltonian) and not quadratic_ok):
            raise NotImplementedError(self._ensemble_base_message.format(base))
        if not hasattr(backend, self.ensemble_setter):
            raise NotImplementedError("the backend {!r} does not evaluate Hamiltonian ensembles "
                                      "(no {})".format(backend, self.ensemble_setter))
        if ensemble.hilbert_size is not None and ensemble.hilbert_size != self.hilbert_size:
            raise ValueError("perturbations are {0} x {0}, the system is {1} x {1}".format(
                ensemble.hilbert_size, self.hilbert_size))
        scales = ensemble.real_channel_scales(control_count, complex_controls)
        self.ensemble = ensemble
        self._ensemble_scales = scales
        self._ensemble_args = (scales if ensemble.control_scales is not None else None,
                               ensemble.offsets, ensemble.weights)
        return base

    def _reject_opaque_ensemble_costs(self):
        if self.opaque_costs:
            raise NotImplementedError(
                "a HamiltonianEnsemble takes costs evaluated on the device (with a "
                "device_descriptor()) and costs of the controls alone; {} is neither"
                "".format(self.opaque_costs[0]))

    def _append_perturbations(self, g):
        """G (nt, K_r, n, n) -> [G_1 .. G_K_r, D_1 .. D_J] in every one of the nt tables."""
        d = self.ensemble.perturbations if self.ensemble is not None else self._sweep_matrices
        if d is None:
            return g
        g = np.asarray(g, dtype=np.complex128)
        return np.concatenate([g, np.broadcast_to(d[None], (g.shape[0],) + d.shape)], axis=1)

    def member_errors(self):
        """The unweighted device cost of every member of every seed of the last evaluation,
        (B, M)."""
        return getattr(self.backend, self.ensemble_member_costs)()

    # -- Hamiltonian sweeps -----------------------------------------------------------------------
    def _sweep_base(self, sweep, control_count, complex_controls, backend, times):
        """Checks a sweep against this problem and the backend, keeps it with the arguments of the
        backend's setter (self._sweep_args) and its fixed matrices, and returns its base."""
        base = sweep.hamiltonian
        if control_count == 0:
            raise NotImplementedError("a HamiltonianSweep needs at least one control "
                                      "(control_count = 0)")
        if isinstance(base, (HamiltonianEnsemble, HamiltonianSweep, QuadraticHamiltonian)):
            raise NotImplementedError(
                "a HamiltonianSweep needs a plain base hamiltonian linear in the controls (sweep x "
                "ensemble and sweep x QuadraticHamiltonian are not evaluated), got {!r}"
                "".format(base))
        if not hasattr(backend, self.sweep_setter):
            raise NotImplementedError("the backend {!r} does not evaluate Hamiltonian sweeps "
                                      "(no {})".format(backend, self.sweep_setter))
        if sweep.searches_duration and not hasattr(backend, self.durations_setter):
            raise NotImplementedError(
                "the backend {!r} does not search the durations of a sweep (no "
                "{}): drop time_bounds, or use the engine".format(backend, self.durations_setter))
        matrices = sweep.resolve(control_count, complex_controls, self.hilbert_size, times)
        if matrices is not None and matrices.shape[1] != self.hilbert_size:
            raise ValueError("perturbations are {0} x {0}, the system is {1} x {1}".format(
                matrices.shape[1], self.hilbert_size))
        self.sweep = sweep
        self._sweep_matrices = matrices
        self._sweep_args = (sweep.real_channel_scales(control_count, complex_controls),
                            sweep.offsets)
        if sweep.searches_duration:
            # tau_b is a parameter of seed b on the device (qocx_sweep_set_durations): the tables
            # before the factor tau, and the durations the next evaluation runs at
            self._duration_tables = sweep.base_tables(control_count, complex_controls)
            self._tau = np.array(sweep._tau, dtype=np.float64)
            self._tau_grad = None
        return base

    def _reject_sweep_costs(self):
        if self.opaque_costs:
            raise NotImplementedError(
                "a HamiltonianSweep takes costs evaluated on the device (with a "
                "device_descriptor()) and costs of the controls alone; {} is neither (user costs "
                "without a device descriptor)".format(self.opaque_costs[0]))
        if self.sweep.time_scaled:
            from qoc_amd.standard.costs import ControlBandwidthMax
            for cost in self.host_costs:
                if isinstance(cost, ControlBandwidthMax):
                    raise NotImplementedError(
                        "ControlBandwidthMax with a duration sweep: its frequency bins depend on "
                        "the evolution time, which differs from seed to seed")

    # -- duration search of a sweep (HamiltonianSweep.durations(time_bounds=...)) -----------------
    _time_term_resident = False
    durations_setter = "sweep_set_durations"         # the backend's entry points for the search
    durations_getter = "sweep_download_durations"

    def _duration_rate_tables(self):
        """What the backend's setter takes between the base offsets and the box (the Lindblad path:
        the base rate factors)."""
        return ()

    def _device_time_weight(self):
        """The price of time joins the error LAST, after the costs of the controls alone. Where the
        host adds those (evaluate_batch) it adds the time term after them, the same product and the
        same sum, and the device is given a weight of zero; where the device adds them (the resident
        loop, time_term_resident) or there are none, the device adds the time term."""
        if self.host_costs and not self._time_term_resident:
            return 0.0
        return self.sweep.time_weight

    def _set_durations(self):
        s0, d0 = self._duration_tables
        lo, hi = self.sweep.tau_bounds
        getattr(self.backend, self.durations_setter)(
            self._tau, s0, d0, *self._duration_rate_tables(), lo, hi, self._device_time_weight())
        self._tau = np.array(getattr(self.backend, self.durations_getter)(want_grad=False)[0])
        self._tau_grad = None

    def _require_search(self):
        if self.sweep is None or not self.sweep.searches_duration:
            raise ValueError("durations are set and read on a duration search "
                             "(HamiltonianSweep.durations(time_bounds=...), "
                             "LindbladSweep.duration_search)")

    def time_term_resident(self, on):
        """The resident loop adds the costs of the controls on the device, so the price of time
        must be added there too (run_batch_resident brackets its loop with this)."""
        self._require_search()
        if bool(on) != self._time_term_resident:
            self._time_term_resident = bool(on)
            if self.host_costs:
                self._set_durations()

    def set_durations(self, tau):
        """tau_b = T_b / reference_time of every seed for the evaluations from here on (B,); the
        engine clips them to the box."""
        self._require_search()
        tau = np.array(tau, dtype=np.float64).reshape(-1)
        if tau.shape[0] != self.sweep.seed_count:
            raise ValueError("a sweep of {} seeds takes that many durations, got {}".format(
                self.sweep.seed_count, tau.shape[0]))
        if not np.all(np.isfinite(tau)):
            raise ValueError("durations are not finite")
        self._tau = tau
        self._set_durations()

    def set_evolution_times(self, times):
        """T_b of every seed for the evaluations from here on (B,), clipped to time_bounds."""
        self._require_search()
        self.set_durations(np.asarray(times, dtype=np.float64) / self.sweep.reference_time)

    def durations(self):
        """tau_b (B,) the evaluations run at (the last evaluation's, once there is one)."""
        self._require_search()
        return self._tau.copy()

    def evolution_times(self):
        """T_b = tau_b * reference_time (B,) the evaluations run at."""
        return self.durations() * self.sweep.reference_time

    def duration_gradients(self):
        """d (error_b + time_weight * tau_b) / d tau_b (B,) of the last evaluation with gradients:
        the engine's chain rule through the tables (qocx_duration.hip, on the Lindblad path
        qocx_lindblad_duration.hip) plus time_weight."""
        self._require_search()
        if self._tau_grad is None:
            raise ValueError("duration gradients need an evaluation with gradients")
        return self._tau_grad.copy()

    def evolution_time_gradients(self):
        """d (error_b + time_weight * tau_b) / d T_b (B,): duration_gradients() / reference_time."""
        return self.duration_gradients() / self.sweep.reference_time

    def _finish_search(self, out, want_grad):
        """The tail of evaluate_batch with a duration search: the durations the evaluation ran at,
        their gradient, and the price of time where the host adds it (_device_time_weight)."""
        if self.sweep is None or not self.sweep.searches_duration:
            return out
        errors, grads, final, steps = out
        tau, tau_grad = getattr(self.backend, self.durations_getter)(want_grad=bool(want_grad))
        weight = self.sweep.time_weight
        if weight != 0.0 and self._device_time_weight() == 0.0:
            errors = errors + weight * tau
            if tau_grad is not None:
                tau_grad = tau_grad + weight
        self._tau = np.array(tau)
        self._tau_grad = None if tau_grad is None else np.array(tau_grad)
        return errors, grads, final, steps

    def _triage_costs(self, item_count):
        """Splits self.costs into device_costs (they have a device_descriptor(); returns those
        descriptors), host_costs (of the controls alone) and opaque_costs (user costs of the
        states, evaluated on the host)."""
        self.device_costs, self.host_costs, self.opaque_costs = [], [], []
        descriptors = []
        for cost in self.costs:
            desc = cost.device_descriptor(item_count, self.hilbert_size) \
                if hasattr(cost, "device_descriptor") else None
            if desc is not None:
                self.device_costs.append(cost)
                descriptors.append(desc)
            elif (getattr(cost, "uses_states", True) is False
                  and not cost.requires_step_evaluation):
                self.host_costs.append(cost)
            else:
                self.opaque_costs.append(cost)
        # the same costs as the resident multi-start driver hands them to the engine
        self.control_cost_descriptors = control_cost_descriptors(
            self.host_costs, self.control_count, self.control_eval_count, self.complex_controls)
        return descriptors

    def resident_capable(self):
        """True when a multi-start driver may keep controls and optimizer states on the device
        (engine.opt_* / engine.lindblad_opt_*): a problem the device holds in structured form
        (_problem_stays_resident), every cost evaluated on the device - the built-in costs of the
        controls alone included, through their control_descriptor() -, and a backend that has the
        entry points (the real engine; complex controls need its complex clip)."""
        return (self.linearized_hamiltonian is None and self._problem_stays_resident()
                and self.control_count > 0 and not self.opaque_costs
                and hasattr(self.backend, self.opt_prefix + "opt_step")
                and controls_stay_resident(self.backend, self.control_cost_descriptors,
                                           self.complex_controls,
                                           self.opt_prefix + "opt_begin_complex"))

    def resident_lbfgs_capable(self):
        """resident_capable() with a backend that also has the L-BFGS calls of the resident driver."""
        return self.resident_capable() and hasattr(self.backend, self.opt_prefix + "opt_lbfgs_step")

    def resident_basis_capable(self):
        """resident_capable() with a backend that also has the ControlBasis calls of the resident
        driver."""
        return (self.resident_capable()
                and hasattr(self.backend, self.opt_prefix + "opt_begin_basis")
                and hasattr(self.backend, self.opt_prefix + "opt_download_best_params"))

    def _prepare(self, device_controls):
        """Before the first pass of an evaluation (the Lindblad time tables)."""

    def _kept_pass(self, controls_batch, device_controls, want_grad, need_steps):
        """One pass -> (cost, grads, final, step states or None); the backend keeps step states
        during it when they are needed, and never after it (an engine error included)."""
        if need_steps:
            self.backend.set_keep_step_states(True)
        try:
            cost, grads, final = self._pass(controls_batch, device_controls, want_grad)
            return cost, grads, final, self._download_steps() if need_steps else None
        finally:
            if need_steps:
                self.backend.set_keep_step_states(False)

    def _evaluate_linearized(self, controls_batch, device_controls, want_grad, need_steps):
        """One control array at a time: the tangent problem of the callable at THAT array, set as
        a structured time-dependent problem (_set_linearized_problem) and evaluated at it - the
        route of callables that are not linear in the controls, which the reference evaluates one
        control array at a time as well. The backend is left holding the tangent problem of the
        LAST array."""
        outs = []
        for b in range(controls_batch.shape[0]):
            self._set_linearized_problem(controls_batch[b], device_controls[b])
            out = self._kept_pass(controls_batch[b:b + 1], device_controls[b:b + 1], want_grad,
                                  need_steps)
            outs.append([None if x is None else x[0] for x in out])
        costs, grads, finals, steps = zip(*outs)
        return (np.array(costs), np.stack(grads) if want_grad else None, np.stack(finals),
                np.stack(steps) if need_steps else None)

    def evaluate_batch(self, controls_batch, want_grad=True, want_step_states=False):
        """
        controls_batch :: (B x Nc x K) (or None / an int B when control_count == 0).
        Returns (errors[B], grads[B x Nc x K] or None, final states, step states or None): final
        states [B x S x n x 1] and step states [B x N x S x n x 1] on the Schroedinger path (with
        an ensemble a member axis M follows B), densities [B x S x n x n] and [B x N x S x n x n]
        on the Lindblad path.
        """
        if self.control_count == 0:
            batch = 1 if controls_batch is None else int(controls_batch)
            want_grad = False
            device_controls = batch
        else:
            controls_batch = np.asarray(controls_batch)
            batch = controls_batch.shape[0]
            if self.sweep is not None and batch != self.sweep.seed_count:
                raise ValueError("a HamiltonianSweep of {} seeds takes a batch of exactly that "
                                 "many control arrays, got {}".format(self.sweep.seed_count, batch))
            device_controls = structure.to_real_controls(controls_batch, self.complex_controls)
        self._prepare(device_controls)
        need_steps = want_step_states or bool(self.opaque_costs)
        two_pass = want_grad and bool(self.opaque_costs)
        if self.linearized_hamiltonian is not None:
            if two_pass:
                raise NotImplementedError(
                    "user costs without a device descriptor together with a hamiltonian that is "
                    "not linear in the controls " + self.linearized_route)
            run = self._evaluate_linearized
        else:
            run = self._kept_pass
        cost, grads, final, step_states = run(controls_batch, device_controls,
                                              want_grad and not two_pass, need_steps)
        opaque_grads = None
        if two_pass:
            # User costs without a device descriptor: the host supplies the cotangent of the
            # states at every cost step (the cost's own states_bar() hook, else central
            # differences of its cost()), the engine's adjoint sweep carries it back.
            steps, bars, opaque_grads = self._opaque_cotangents(controls_batch, step_states)
            self._set_cotangents(steps, bars)
            try:
                cost, grads, final = self._pass(controls_batch, device_controls, True, again=True)
            finally:
                self._set_cotangents(None, None)
        errors = np.array(cost, dtype=np.float64)
        if grads is not None:
            grads = structure.from_real_gradients(grads, self.complex_controls)
            if not self.complex_controls:
                grads = np.array(grads, dtype=np.float64)
            if opaque_grads is not None:
                grads = grads + (opaque_grads if self.complex_controls
                                 else np.real(opaque_grads))
        # The host's share of the costs: those of the controls alone, then the user's cost() at its
        # steps. The two paths round differently and each keeps its order: with subtotal_costs the
        # host costs are summed from 0.0 and each user cost over its steps from 0.0 before they
        # join errors[b] / grads[b]; without, every term is added to errors[b] / grads[b] in turn.
        device_share = self._device_control_costs(device_controls, want_grad)
        for b in range(batch):
            controls = None if self.control_count == 0 else controls_batch[b]
            if self._cost_controls is not None:
                controls = self._cost_controls
            if device_share is not None:  # (the costs of the controls as the resident route adds them)
                errors[b] = errors[b] + device_share[0][b]
                if want_grad:
                    grads[b] = grads[b] + device_share[1][b]
            elif self.subtotal_costs:
                value, host_grad = self._add_host_costs(0.0, None, controls, want_grad)
                errors[b] += value
                if host_grad is not None:
                    grads[b] = grads[b] + host_grad
                for cost in self.opaque_costs:
                    errors[b] += self._add_user_cost(0.0, cost, controls, step_states[b])
            else:
                errors[b], host_grad = self._add_host_costs(
                    errors[b], grads[b] if want_grad else None, controls, want_grad)
                if host_grad is not None:
                    grads[b] = host_grad
                for cost in self.opaque_costs:
                    errors[b] = self._add_user_cost(errors[b], cost, controls, step_states[b])
        return errors, grads, final, step_states

    def _device_control_costs(self, device_controls, want_grad):
        """(costs (B,), gradients in the cost-function format or None) of the costs of the controls
        alone where evaluate_batch takes them from the device instead of the host; None: the host
        adds them (_add_host_costs)."""
        return None

    def _add_host_costs(self, value, grad, controls, want_grad):
        """(value + c_1 + c_2 + ..., grad + bar_1 + bar_2 + ...) over the costs of the controls
        alone, left to right; grad = None starts the second sum at bar_1."""
        for cost in self.host_costs:
            value = value + cost.cost(controls, None, self.final_system_eval_step)
            if want_grad:
                bar = cost.controls_bar(controls, None, self.final_system_eval_step)
                if bar is None:
                    raise NotImplementedError("cost {} has no controls_bar()".format(cost))
                grad = bar if grad is None else grad + bar
        return value, grad

    def _add_user_cost(self, value, cost, controls, states_by_step):
        """value + the user's cost() at each of its steps, in step order."""
        for step in self._cost_steps(cost):
            value = value + cost.cost(controls, states_by_step[step], step)
        return value

    def _cost_steps(self, cost):
        if not cost.requires_step_evaluation:
            return [self.final_system_eval_step]
        return list(range(self.cost_eval_step, self.system_eval_count, self.cost_eval_step))

    def _opaque_cotangents(self, controls_batch, step_states):
        """(steps, bars[B, len(steps)] + cotangent_shape, control_grads[B, Nc, K] complex) of the
        user costs."""
        steps = sorted({st for c in self.opaque_costs for st in self._cost_steps(c)})
        row = {st: r for r, st in enumerate(steps)}
        batch = controls_batch.shape[0]
        bars = np.zeros((batch, len(steps)) + self.cotangent_shape, dtype=np.complex128)
        cgrads = np.zeros(controls_batch.shape, dtype=np.complex128)
        for b in range(batch):
            for cost in self.opaque_costs:
                for st in self._cost_steps(cost):
                    states = step_states[b][st]
                    bars[b, row[st]] += user_states_bar(
                        cost, controls_batch[b], states, st).reshape(self.cotangent_shape)
                    cgrads[b] += user_controls_bar(cost, controls_batch[b], states, st)
        return steps, bars, cgrads

    def evaluate(self, controls, want_grad=True, want_step_states=False):
        """Single control array, the reference's calling convention."""
        batch = None if controls is None else np.asarray(controls)[None]
        errors, grads, final, steps = self.evaluate_batch(batch, want_grad, want_step_states)
        return (float(errors[0]), None if grads is None else grads[0], final[0],
                None if steps is None else steps[0])


class SchroedingerEvaluator(_Evaluator):
    linearized_route = "under MagnusPolicy.M4 / M6"

    def __init__(self, evolution_time, hamiltonian, initial_states, system_eval_count,
                 control_count=0, control_eval_count=0, complex_controls=False, costs=(),
                 cost_eval_step=1, interpolation_policy=InterpolationPolicy.LINEAR,
                 magnus_policy=MagnusPolicy.M2, need_gradients=True, backend=None,
                 latency_mode=False, matrix_free="default"):
        """
        matrix_free: "default" leaves the engine's route decision as it is (matrix-free Taylor
        sweeps for one-state Hermitian problems at 17 <= n <= 32, knob "action" untouched); "wide"
        also takes them at 33 <= n <= 64 (knob "action" = 2 on a backend with set_knob; opt-in
        because the default route there is what existing callers measure and assert on); "states"
        also takes them for 2 .. ACTION_STATES_DEFAULT states per seed at 17 <= n <= 32 under one
        coherent final TargetStateInfidelity (knob "action_states"; a wave per state, opt-in for the
        same reason); "all" asks for both. A problem of that many states asked for with "states" or
        "all" is not put into latency mode, which the route yields to. "costs" takes them for one
        state at 17 <= n <= 32 under any set of costs the device evaluates - step costs
        (TargetStateInfidelityTime, ForbidStates), several costs, an incoherent target - instead of
        the one final TargetStateInfidelity (knob "action_costs" = 1; opt-in, not part of "all"); such
        a problem is not put into latency mode either. "small" takes them for one-state Hermitian
        problems at n <= 16 under the one final TargetStateInfidelity (knob "action_small" = 1; a
        wave per seed whose four rows of 16 lanes do the four real products of a complex one;
        opt-in because the Pade route there is what existing callers measure and assert on, and
        not part of "all"); latency mode keeps its route, the new one yields to it as "wide" does.
        "effective" takes them for one-state problems under the one final TargetStateInfidelity
        whose step generator is linear in EFFECTIVE controls: MagnusPolicy.M4 on a time-independent
        Hermitian system, and a QuadraticHamiltonian under M2 (knob "action_eff" = 1, at 17 <= n <=
        32; opt-in because the Pade route is what existing callers measure and assert on for these
        problems, and not part of "all"); latency mode keeps its route here too.
        A backend without knobs ignores it; any other value is a ValueError.
        latency_mode: the evaluator will be asked for ONE control array at a time (the
        reference's evolve_* / grape_* entry points). Where the cost is a single final
        TargetStateInfidelity the engine then runs its two-sided pipeline (round 3: forward and
        adjoint sweep of the one seed side by side, knob "latency": 3.6 ms per forward + gradient
        evaluation at n = 32 / 1000 steps against 6.4 ms). Otherwise, for 17 <= n <= 32, its
        blocked-inverse sweep (four wavefronts per seed, 1.5x faster per step when the sweep has
        the chip to itself: qocx_debug_set_knob "sweep_impl" = 3); batched evaluation keeps the
        default, and so do n <= 16 (one seed, 1000 steps: 3.3 ms with the column-chain sweep
        against 4.1 ms with the blocked one - a single 16 x 16 block leaves nothing to overlap)
        and n > 32 (not built there).
        """
        if not isinstance(interpolation_policy, InterpolationPolicy):
            raise NotImplementedError("The interpolation policy {} is not yet supported for this "
                                      "method.".format(interpolation_policy))
        self.interpolation_policy = interpolation_policy
        if not isinstance(magnus_policy, MagnusPolicy):
            raise ValueError("Unrecognized magnus policy {}.".format(magnus_policy))
        if not (isinstance(matrix_free, str) and matrix_free in MATRIX_FREE_KNOBS):
            names = ['"{}"'.format(value) for value in MATRIX_FREE_KNOBS]
            raise ValueError("matrix_free must be {} or {}, not {!r}.".format(
                ", ".join(names[:-1]), names[-1], matrix_free))
        self.matrix_free = matrix_free
        initial_states = np.asarray(initial_states)
        self.state_count = initial_states.shape[0]
        self.hilbert_size = initial_states.shape[1]
        self.cotangent_shape = (self.state_count, self.hilbert_size)
        self.control_count = control_count
        self.control_eval_count = control_eval_count
        self.complex_controls = complex_controls
        self.system_eval_count = system_eval_count
        self.final_system_eval_step = system_eval_count - 1
        self.costs = list(costs)
        self.magnus_policy = magnus_policy
        dt = evolution_time / (system_eval_count - 1)
        times = [step * dt + dt * c for step in range(system_eval_count - 1)
                 for c in magnus_policy.nodes]
        # A Hamiltonian that is real-linear in the controls goes to the device in structured form
        # (H0, G_k; the engine builds every step generator itself). Anything else - the
        # reference takes ANY callable, e.g. the epsilon^2 term of report.tex:22-32 - is sampled
        # by the host at every step of every evaluation, as the reference does, and the engine
        # takes the generators as they are (qocx_upload_generators).
        self.opaque_hamiltonian = None
        # ... and under MagnusPolicy.M4 / M6, where the step generator is a commutator expression
        # of several node generators, the host hands the engine the TANGENT of the callable at the
        # current controls instead (structure.linearize_hamiltonian: a structured, time-dependent
        # problem with the same cost and the same control gradient), one control array at a time.
        self.linearized_hamiltonian = None
        self._problem_static = None
        # A QuadraticHamiltonian under M2, on an engine that takes quadratic terms: the linear part
        # goes in structured form and the r_k r_l Q_kl terms to qocx_set_quadratic_terms - the
        # engine evaluates it as linear in the effective controls (r_k, r_k r_l), the callable is
        # never called per evaluation. Elsewhere it is just a callable (the routes below).
        self.quadratic_terms = None
        # A HamiltonianEnsemble: its linear base goes in structured form with the perturbation
        # matrices D_j appended to the G_k as J extra channels, and the engine expands every seed
        # into the M members' (K_r + J)-channel controls (qocx_set_ensemble). Evaluations return
        # the weighted seed costs and gradients, and final states with a member axis. A
        # QuadraticHamiltonian base under M2 goes on into the quadratic route above: its terms
        # index the seeds' K_r channels and act on the members' scaled controls.
        self.ensemble = None
        if isinstance(hamiltonian, HamiltonianEnsemble):
            if hamiltonian.rate_scales is not None:
                raise ValueError(
                    "rate_scales scale the dissipation rates of lindblad_data: the Schroedinger "
                    "path has none, so there is nothing to scale (use the Lindblad entry points, "
                    "or drop rate_scales)")
            if backend is None:
                backend = make_backend()
            hamiltonian = self._ensemble_base(hamiltonian, control_count, complex_controls,
                                              backend, magnus_policy)
        # A HamiltonianSweep: the same structured problem - the base with the fixed matrices D_j
        # appended as J channels - but seed b is item b, with scales and offsets of its own
        # (qocx_set_sweep); evaluations take exactly B control arrays and return B errors and
        # gradients, and sweep_sensitivities() the derivatives with respect to the tables.
        self.sweep = None
        reject_lindblad_sweep(hamiltonian)
        if isinstance(hamiltonian, HamiltonianSweep):
            if backend is None:
                backend = make_backend()
            hamiltonian = self._sweep_base(hamiltonian, control_count, complex_controls, backend,
                                           times)
        if isinstance(hamiltonian, QuadraticHamiltonian) and backend is None:
            backend = make_backend()  # (the route depends on what the backend takes)
        if (isinstance(hamiltonian, QuadraticHamiltonian) and magnus_policy == MagnusPolicy.M2
                and control_count > 0 and hasattr(backend, "set_quadratic_terms")):
            hamiltonian.check_real_control_count(
                control_count * (2 if complex_controls else 1), self.hilbert_size)
            self.quadratic_terms = (hamiltonian.pairs, hamiltonian.matrices)
            probed = hamiltonian.linear_hamiltonian
        else:
            probed = hamiltonian
        try:
            h0, g = structure.probe_hamiltonian(probed, self.hilbert_size, control_count,
                                                complex_controls, times)
        except structure.NonLinearHamiltonianError as exc:
            if self.ensemble is not None:
                raise NotImplementedError(
                    "a HamiltonianEnsemble needs a base hamiltonian linear in the controls "
                    "({})".format(exc))
            if self.sweep is not None:
                raise NotImplementedError(
                    "a HamiltonianSweep needs a base hamiltonian linear in the controls "
                    "({})".format(exc))
            if self.quadratic_terms is not None:
                raise
            if magnus_policy != MagnusPolicy.M2:
                self.linearized_hamiltonian = hamiltonian
                self._node_times = times
                self._evolution_time = evolution_time
                h0 = np.zeros((1, self.hilbert_size, self.hilbert_size), dtype=np.complex128)
                g = np.zeros((1, control_count * (2 if complex_controls else 1),
                              self.hilbert_size, self.hilbert_size), dtype=np.complex128)
            else:
                self.opaque_hamiltonian = hamiltonian
                self._dt = dt
                self._mid_times = times
                self._rows = structure.interpolation_rows(evolution_time, control_eval_count, times,
                                                          interpolation_policy)
                h0 = np.zeros((1, self.hilbert_size, self.hilbert_size), dtype=np.complex128)
                g = None
        descriptors = self._triage_costs(self.state_count)
        if self.ensemble is not None:
            self._reject_opaque_ensemble_costs()
            g = self._append_perturbations(g)
        if self.sweep is not None:
            self._reject_sweep_costs()
            g = self._append_perturbations(g)
        self.backend = backend if backend is not None else make_backend()
        if hasattr(self.backend, "set_knob"):
            knobs = dict(MATRIX_FREE_KNOBS[matrix_free])
            if "action_states" in knobs and 2 <= self.state_count <= knobs["action_states"]:
                latency_mode = False  # (the route asked for yields to it)
            if "action_costs" in knobs and self._takes_action_costs(descriptors):
                latency_mode = False
            self.backend.set_knob(
                "sweep_impl", 3 if (latency_mode and 16 < self.hilbert_size <= 32) else 1)
            self.backend.set_knob("latency", 1 if latency_mode else 0)
            for name, value in knobs.items():
                self.backend.set_knob(name, value)
        self.kr = control_count * (2 if complex_controls else 1)
        device_k = 0 if self.opaque_hamiltonian is not None else self.kr
        if self.ensemble is not None:
            device_k += self.ensemble.perturbation_count
        if self.sweep is not None:
            device_k += self.sweep.perturbation_count
        self._problem_static = (
            (self.hilbert_size, self.state_count, device_k, control_eval_count if device_k else 0,
             system_eval_count, evolution_time),
            initial_states.reshape(self.state_count, self.hilbert_size),
            dict(costs=descriptors, cost_eval_step=cost_eval_step,
                 magnus_policy=magnus_policy.short,
                 **interpolation_keywords(self.backend, "set_schroedinger_problem",
                                          interpolation_policy)))
        self._set_problem(h0, g)
        self.cost_eval_step = cost_eval_step

    def _takes_action_costs(self, descriptors):
        """matrix_free="costs": one state, 17 <= n <= 32, every cost of the states a device
        descriptor, and not the single final target (which has kernels of its own)."""
        single_final_target = (len(descriptors) == 1 and not descriptors[0]["step_cost"]
                               and descriptors[0]["kind"] in (0, 1))  # COHERENT, INCOHERENT
        return (self.state_count == 1 and 17 <= self.hilbert_size <= 32 and len(descriptors) >= 1
                and not self.opaque_costs and not single_final_target)

    def _set_problem(self, h0, g):
        head, psi0, kw = self._problem_static
        self.backend.set_schroedinger_problem(*head, h0, g, psi0, **kw)
        if self.quadratic_terms is not None:
            self.backend.set_quadratic_terms(*self.quadratic_terms)
        if self.ensemble is not None:
            self.backend.set_ensemble(*self._ensemble_args)
            if (self.quadratic_terms is not None and len(self.quadratic_terms[0])
                    and self.ensemble.quadratic_scales is not None):
                self.backend.set_ensemble_quadratic_scales(self.ensemble.quadratic_scales)
        if self.sweep is not None:
            self.backend.set_sweep(*self._sweep_args)
            if self.sweep.searches_duration:
                self._set_durations()

    def evaluate_batch(self, controls_batch, want_grad=True, want_step_states=False):
        """_Evaluator.evaluate_batch; a duration search evaluates at the current durations and its
        errors include the price of time, time_weight * tau_b, added last."""
        return self._finish_search(
            _Evaluator.evaluate_batch(self, controls_batch, want_grad, want_step_states), want_grad)

    # -- Hamiltonian sweeps -----------------------------------------------------------------------
    def sweep_sensitivities(self):
        """Of the last evaluation with gradients: dict(control_scales = d error_b / d s_bk
        (B x control_count; a complex control's two channels added), offsets = d error_b /
        d delta_bj (B x J)), and for a duration sweep evolution_time_gradients = d error_b / d T_b
        (B). Costs of the controls alone do not depend on the tables and do not enter, and neither
        does the price of time of a duration search (evolution_time_gradients() has it)."""
        scales, offsets = self.backend.sweep_sensitivities()
        scales, offsets = np.asarray(scales), np.asarray(offsets)
        if self.complex_controls:
            scales = scales[:, 0::2] + scales[:, 1::2]
        out = dict(control_scales=scales, offsets=offsets)
        if self.sweep.time_scaled:
            out["evolution_time_gradients"] = self.sweep.time_gradients(scales, offsets)
        return out

    # -- Hamiltonian ensembles ------------------------------------------------------------------
    _ensemble_base_message = (
        "a HamiltonianEnsemble needs a base hamiltonian linear in the controls (or a "
        "QuadraticHamiltonian under MagnusPolicy.M2 on a backend that takes quadratic "
        "terms and their member scales), got {!r}")

    def _ensemble_base(self, ensemble, control_count, complex_controls, backend, magnus_policy):
        """_Evaluator._ensemble_base; a quadratic base goes under M2, on a backend that takes
        quadratic terms and ensembles (and the members' term scales, where the ensemble has
        them)."""
        quadratic_ok = (
            isinstance(ensemble.hamiltonian, QuadraticHamiltonian)
            and magnus_policy == MagnusPolicy.M2
            and hasattr(backend, "set_quadratic_terms") and hasattr(backend, "set_ensemble")
            and (ensemble.quadratic_scales is None
                 or hasattr(backend, "set_ensemble_quadratic_scales")))
        return _Evaluator._ensemble_base(self, ensemble, control_count, complex_controls, backend,
                                         quadratic_ok)

    # -- device round trip: structured controls, or generators sampled from an opaque callable ----
    def _upload(self, controls_batch, device_controls):
        if self.opaque_hamiltonian is None:
            self.backend.upload_controls(device_controls)
            return
        gens = [structure.sample_generators(self.opaque_hamiltonian, controls, self._rows,
                                            self._mid_times, self._dt, self.hilbert_size)[0]
                for controls in controls_batch]
        self.backend.upload_generators(np.stack(gens))

    def _download(self, controls_batch, want_grad):
        if self.opaque_hamiltonian is None:
            return self.backend.download_results(want_grad=want_grad)
        cost, _, final = self.backend.download_results(want_grad=False)
        grads = None
        if want_grad:
            bars = self.backend.download_generator_cotangents()
            grads = np.stack([structure.generator_gradients(
                self.opaque_hamiltonian, controls, self._rows, self._mid_times, self._dt,
                bars[b], self.complex_controls) for b, controls in enumerate(controls_batch)])
            grads = structure.to_real_controls(grads, self.complex_controls) \
                if self.complex_controls else grads
        return cost, grads, final

    def _set_linearized_problem(self, controls, device_controls):
        """The tangent of the callable at `controls` on the node times of the Magnus policy. Host
        cost per array: (4 K + 1) evaluations of the callable per node time, one re-upload of the
        nsteps x nodes x (1 + K) tables and a one-seed evaluation."""
        self._set_problem(*structure.linearize_hamiltonian(
            self.linearized_hamiltonian, controls, self._evolution_time, self._node_times,
            self.hilbert_size, self.complex_controls, self.interpolation_policy))

    def _pass(self, controls_batch, device_controls, want_grad, again=False):
        """again: the second pass of one evaluation, the backend still holds the controls."""
        if not again:
            self._upload(controls_batch, device_controls)
        self.backend.eval_resident(want_grad)
        cost, grads, final = self._download(controls_batch, want_grad)
        return cost, grads, final[..., None]

    def _download_steps(self):
        return self.backend.download_step_states()[..., None]

    def _set_cotangents(self, steps, bars):
        self.backend.set_state_cotangents(steps, bars)

    def _problem_stays_resident(self):
        return self.opaque_hamiltonian is None


class LindbladEvaluator(_Evaluator):
    """
    Plays the role of `_evaluate_lindblad_discrete` and of its `ans_jacobian`
    (qoc/core/lindbladdiscrete.py:321-322, :357-441) through qocx_eval_lindblad.
    """

    MAX_HILBERT_SIZE = 32
    WIDE_HILBERT_SIZE = 64    # with wide=True (knob "lindblad_wide"): static problems, classic launch
    opt_prefix = "lindblad_"
    subtotal_costs = False
    _frozen_slices = None     # (callable, controls) of piecewise-constant frozen controls
    linearized_route = "on the Lindblad GRAPE path"
    MAX_CHANNELS = 8          # QOCX_LINDBLAD_MAX_K: real control channels of a Lindblad problem
    ensemble_setter = "set_lindblad_ensemble"
    ensemble_member_costs = "lindblad_ensemble_member_costs"
    ensemble_rates_setter = "set_lindblad_ensemble_rates"
    sweep_setter = "set_lindblad_sweep"
    durations_setter = "lindblad_sweep_set_durations"
    durations_getter = "lindblad_sweep_download_durations"
    _ensemble_base_message = (
        "a HamiltonianEnsemble on the Lindblad path needs a base hamiltonian linear in the "
        "controls (the tangent and frozen-controls routes evaluate one control array at a "
        "time), got {!r}")

    def __init__(self, evolution_time, initial_densities, system_eval_count, hamiltonian=None,
                 lindblad_data=None, control_count=0, control_eval_count=0,
                 complex_controls=False, costs=(), cost_eval_step=1,
                 interpolation_policy=InterpolationPolicy.LINEAR, need_gradients=True,
                 backend=None, control_bounds=None, frozen_controls=None, wide=False):
        """
        wide: False refuses hilbert_size > 32, as ever. True takes 33 <= hilbert_size <= 64 on the
        sixteen-wave kernel (knob "lindblad_wide" = 1 on a backend with set_knob; an evaluator
        with wide=False sets it to 0, so a shared backend never leaks the opt-in). That kernel
        evaluates time-independent systems in the classic launch only: above 32 a time-dependent
        hamiltonian or lindblad_data (stage tables; so also a hamiltonian that is not linear in the
        controls), rate_scales of an ensemble or a sweep, LindbladSweep.durations and a
        duration_search are refused by name, and sweep_sensitivities() has no rate_scales and no
        evolution_time_gradients (nothing runs two-sided).

        frozen_controls :: (Nc x K) or None. Forward-only evaluation of ONE control array under a
        hamiltonian(controls, time) that is not linear in the controls (the reference calls any
        callable per RHS evaluation, lindbladdiscrete.py:479-483): the controls are folded into a
        control-free, time-dependent Hamiltonian t -> hamiltonian(u(t), t), which the engine takes
        as per-stage samples like any other time dependence. Costs still see the controls.

        hamiltonian may be a HamiltonianEnsemble whose base is linear in the controls: the
        perturbation matrices D_j go to the engine as J constant channels behind the K_r real
        channels of the seeds (K_r + J <= 8, the Lindblad engine's channel limit), the engine
        expands every seed into its M members (qocx_lindblad_set_ensemble), and evaluations
        return the weighted seed errors and gradients and final densities with a member axis
        (B x M x S x n x n). An ensemble on this path needs at least one cost: the error IS the
        weighted sum of the members' costs. Densities and costs are the same for all members,
        and so is lindblad_data unless the ensemble has rate_scales (M x L): member m then decays
        with the rates c_m * dissipators (qocx_lindblad_set_ensemble_rates). Those need a
        time-independent system: with a time-dependent hamiltonian or lindblad_data the engine
        holds the control-free generator in per-stage tables, one set, not M.

        hamiltonian may be a LindbladSweep whose base is linear in the controls: its fixed
        matrices D_j go to the engine as J constant channels behind the K_r real channels of the
        seeds (K_r + J <= 8), seed b is item b with scales, offsets and rate factors of its own
        (qocx_lindblad_set_sweep), evaluations take exactly B control arrays and return B errors,
        gradients and final densities (B x S x n x n, no member axis), and sweep_sensitivities()
        the derivatives with respect to the tables. costs may be empty. With rates of its own
        (rate_scales, or any duration sweep) the system must be time independent, as above.
        """
        if not isinstance(interpolation_policy, InterpolationPolicy):
            raise NotImplementedError("This operation does not yet support the interpolation "
                                      "policy {}.".format(interpolation_policy))
        self.interpolation_policy = interpolation_policy
        reject_sweep(hamiltonian, "the Lindblad path", LINDBLAD_SWEEP_HINT, lindblad_sweep_ok=True)
        sweep = hamiltonian if isinstance(hamiltonian, LindbladSweep) else None
        if sweep is not None and frozen_controls is not None:
            raise NotImplementedError(
                "a LindbladSweep needs a base hamiltonian linear in the controls (the frozen-"
                "controls route evaluates one control array at a time)")
        self.sweep = None
        ensemble = hamiltonian if isinstance(hamiltonian, HamiltonianEnsemble) else None
        if ensemble is not None:
            reject_costless_lindblad_ensemble(ensemble, costs)
            if frozen_controls is not None:
                raise NotImplementedError(self._ensemble_base_message.format(ensemble.hamiltonian))
        if frozen_controls is not None:
            if need_gradients:
                raise structure.NonLinearHamiltonianError(
                    "gradients through a hamiltonian(controls, time) that is not linear in the "
                    "controls are available on the Schroedinger path only")
            frozen_controls = np.asarray(frozen_controls)
            self._cost_controls = frozen_controls
            user_hamiltonian, frozen_nc = hamiltonian, frozen_controls.shape[0]
            if interpolation_policy == InterpolationPolicy.PIECEWISE_CONSTANT:
                self._frozen_slices = (user_hamiltonian, frozen_controls)

            def hamiltonian(_, time):
                rows = structure.interpolation_rows(evolution_time, frozen_nc, [time],
                                                    interpolation_policy)
                return user_hamiltonian(structure.controls_at(frozen_controls, rows, [time])[0],
                                        time)
            # one dummy control with a zero coupling keeps the control knots in the integrator's
            # grid: u(t) has kinks there, and a sub-interval that straddled one would lose the
            # integrator's order (the engine cuts sub-intervals at knots only when it has controls;
            # piecewise constant it cuts at the slice edges, where u(t) jumps)
            control_count, control_eval_count, complex_controls = 1, frozen_nc, False
        initial_densities = np.asarray(initial_densities)
        self.density_count = initial_densities.shape[0]
        self.hilbert_size = initial_densities.shape[1]
        self.wide = bool(wide)
        size_limit = self.WIDE_HILBERT_SIZE if self.wide else self.MAX_HILBERT_SIZE
        if self.hilbert_size > size_limit:
            raise NotImplementedError(
                "the MI355X Lindblad engine handles hilbert_size <= {} (got {}); there is no "
                "CPU fallback.".format(size_limit, self.hilbert_size))
        above_32 = self.hilbert_size > self.MAX_HILBERT_SIZE
        if above_32:
            self._reject_above_32(ensemble, sweep, frozen_controls)
        self.control_count = control_count
        self.control_eval_count = control_eval_count
        self.complex_controls = complex_controls
        self.system_eval_count = system_eval_count
        self.final_system_eval_step = system_eval_count - 1
        self.cost_eval_step = cost_eval_step
        self.costs = list(costs)
        self.backend = backend if backend is not None else make_backend()
        if self.wide and not hasattr(self.backend, "set_knob"):
            raise NotImplementedError(
                "wide=True needs a backend with set_knob (the knob lindblad_wide), got "
                "{!r}".format(self.backend))
        if hasattr(self.backend, "set_knob"):
            self.backend.set_knob("lindblad_wide", 1 if self.wide else 0)
        self.kr = control_count * (2 if complex_controls else 1)
        self.device_k = self.kr   # the problem's channels: with an ensemble K_r + J
        if ensemble is not None:
            hamiltonian = self._ensemble_base(ensemble, control_count, complex_controls,
                                              self.backend)
            self.device_k = self.kr + ensemble.perturbation_count
            if self.device_k > self.MAX_CHANNELS:
                raise NotImplementedError(
                    "the Lindblad engine takes up to {} real control channels: this ensemble "
                    "needs K_r + J = {} + {}".format(self.MAX_CHANNELS, self.kr,
                                                     ensemble.perturbation_count))
            if (ensemble.rate_scales is not None
                    and not hasattr(self.backend, self.ensemble_rates_setter)):
                raise NotImplementedError(
                    "the backend {!r} does not take per-member dissipation rates (no {})".format(
                        self.backend, self.ensemble_rates_setter))
        # time dependence is decided on the integrator's own grid: every stage time of the
        # coarsest sub-division (12 per sub-interval), never on a handful of equispaced probes
        # (piecewise constant: the edges of Nc slices are the cut points of Nc + 1 linear knots)
        self._stage_knots = control_eval_count + (
            1 if interpolation_policy == InterpolationPolicy.PIECEWISE_CONSTANT else 0)
        self._coarse_times = self.backend.lindblad_stage_times(
            evolution_time, system_eval_count, self._stage_knots, self.kr, 1)
        if sweep is not None:
            try:
                hamiltonian = self._sweep_base(sweep, control_count, complex_controls,
                                               self.backend, list(self._coarse_times))
            except ValueError as exc:
                if sweep.time_scaled and "time-independent" in str(exc):
                    # (the sweep's own probe; here it is the rates' refusal, as _check_rate_scales)
                    raise NotImplementedError(
                        "rate_scales need a time-independent system (a duration sweep scales every "
                        "seed's rates): the hamiltonian (base or drives) is time dependent, so the "
                        "engine holds the control-free generator in per-stage tables "
                        "(fixed_subdivision > 0) - one set, not one per seed")
                raise
            self.device_k = self.kr + sweep.perturbation_count
            if self.device_k > self.MAX_CHANNELS:
                raise NotImplementedError(
                    "the Lindblad engine takes up to {} real control channels: this sweep needs "
                    "K_r + J = {} + {}".format(self.MAX_CHANNELS, self.kr,
                                               sweep.perturbation_count))
        # A hamiltonian(controls, time) that is not linear in the controls (the reference takes any
        # callable, lindbladdiscrete.py:486-489): the engine gets the TANGENT of the callable at the
        # control array being evaluated, sampled at the integrator's stage times
        # (structure.linearize_hamiltonian) - a structured time-dependent problem with the same
        # cost and the same control gradient -, one control array at a time.
        self.linearized_hamiltonian = None
        self._evolution_time = evolution_time
        probe = lambda h: structure.probe_static_lindblad_system(  # noqa: E731
            h, lindblad_data, self.hilbert_size, control_count, complex_controls, evolution_time,
            probe_times=self._coarse_times)
        try:
            h0, g, dissipators, operators, self.time_dependent, data_dependent = probe(hamiltonian)
        except structure.NonLinearHamiltonianError:
            if self.ensemble is not None:
                raise NotImplementedError(self._ensemble_base_message.format(hamiltonian))
            if self.sweep is not None:
                raise NotImplementedError(
                    "a LindbladSweep needs a base hamiltonian linear in the controls (the tangent "
                    "route evaluates one control array at a time), got {!r}".format(hamiltonian))
            if frozen_controls is not None or control_count == 0:
                raise
            if above_32:
                raise NotImplementedError(self._above_32_message(
                    "a hamiltonian that is not linear in the controls (its tangent goes to the "
                    "engine as stage tables)"))
            self.linearized_hamiltonian = hamiltonian
            h0, g, dissipators, operators, _, data_dependent = probe(None)
            self.time_dependent = True
            hamiltonian = None
        if above_32 and (self.time_dependent or data_dependent):
            raise NotImplementedError(self._above_32_message(
                "a time-dependent hamiltonian or lindblad_data (the engine holds them in stage "
                "tables, fixed_subdivision > 0)"))
        if self.ensemble is not None and self.ensemble.rate_scales is not None:
            self._check_rate_scales(self.ensemble.rate_scales, dissipators, data_dependent,
                                    "(M, L)", "member")
        if self.sweep is not None:
            rates = self.sweep.resolved_rate_scales(0 if dissipators is None else len(dissipators))
            if rates is not None:
                self._check_rate_scales(rates, dissipators, data_dependent, "(B, L)", "seed")
            self._sweep_args = self._sweep_args + (rates,)
        # a time-dependent lindblad_data is sampled at the stage times like the Hamiltonian
        self._lindblad_data = lindblad_data if data_dependent else None
        self.cotangent_shape = (self.density_count, self.hilbert_size, self.hilbert_size)
        descriptors = self._triage_costs(self.density_count)
        if self.ensemble is not None:
            self._reject_opaque_ensemble_costs()
            g = self._append_perturbations(np.asarray(g)[None])[0]
        if self.sweep is not None:
            self._reject_sweep_costs()
            if self.sweep.searches_duration:
                self._reject_one_sided_search(dissipators)
                self._base_rates = self.sweep.base_rates(len(dissipators))
            g = self._append_perturbations(np.asarray(g)[None])[0]
        self._problem_args = (self.hilbert_size, self.density_count, self.device_k,
                              control_eval_count, system_eval_count, evolution_time, h0, g,
                              dissipators, operators, initial_densities)
        self._problem_kw = dict(costs=descriptors, cost_eval_step=cost_eval_step,
                                **interpolation_keywords(self.backend, "set_lindblad_problem",
                                                         interpolation_policy))
        self._hamiltonian = hamiltonian
        self._table_bounds = None
        self._coarse_samples = None
        self._coarse_lindblad = None
        if self.linearized_hamiltonian is not None:
            pass  # the tables depend on the controls: set per evaluation (_set_linearized_problem)
        elif not self.time_dependent:
            self._set_problem()
        elif control_bounds is not None:  # GRAPE: max_control_norms bound the controls for good
            bounds = np.repeat(np.asarray(control_bounds, dtype=np.float64),
                               2 if complex_controls else 1)
            self._set_time_dependent_problem(bounds)

    @staticmethod
    def _above_32_message(what):
        return ("{} is not available at hilbert_size > 32: the wide=True kernel (33 <= "
                "hilbert_size <= 64) evaluates time-independent systems in the classic launch "
                "only".format(what))

    def _reject_above_32(self, ensemble, sweep, frozen_controls):
        """What has kernels of its own at hilbert_size <= 32 only, by name, before the backend
        sees a problem."""
        if frozen_controls is not None:
            raise NotImplementedError(self._above_32_message(
                "a hamiltonian that is not linear in the controls (frozen controls go to the "
                "engine as stage tables)"))
        if ensemble is not None and ensemble.rate_scales is not None:
            raise NotImplementedError(self._above_32_message(
                "rate_scales of a HamiltonianEnsemble (per-member rates)"))
        if sweep is not None:
            if sweep.searches_duration:
                raise NotImplementedError(self._above_32_message(
                    "duration_search of a LindbladSweep (it needs the two-sided evaluation)"))
            if sweep.time_scaled:
                raise NotImplementedError(self._above_32_message(
                    "durations of a LindbladSweep (every seed's rates scale with its duration)"))
            if sweep.rate_scales is not None:
                raise NotImplementedError(self._above_32_message(
                    "rate_scales of a LindbladSweep (per-seed rates)"))

    def _set_problem(self, **tables):
        """The problem (with its stage tables, if any) to the backend, then the ensemble or the
        sweep: a new problem clears them."""
        self.backend.set_lindblad_problem(*self._problem_args, **tables, **self._problem_kw)
        if self.sweep is not None:
            getattr(self.backend, self.sweep_setter)(*self._sweep_args)
            if self.sweep.searches_duration:
                self._set_durations()
        if self.ensemble is not None:
            self.backend.set_lindblad_ensemble(*self._ensemble_args)
            if self.ensemble.rate_scales is not None:
                getattr(self.backend, self.ensemble_rates_setter)(self.ensemble.rate_scales)

    def _duration_rate_tables(self):
        return (self._base_rates,)

    def _device_control_costs(self, device_controls, want_grad):
        """A duration search keeps its two loops on the same numbers: where the resident route
        could run (every cost of the controls has a control_descriptor() and the backend takes
        them), evaluate_batch adds the costs of the controls as that route does - the engine's
        kernel on the seeds' controls, one sum onto the error and one onto every gradient entry -
        and not NumPy's cost(), which rounds the same value differently. The engine keeps the
        descriptors only for the call: its resident evaluations add what is set."""
        if (self.sweep is None or not self.sweep.searches_duration or not self.host_costs
                or not hasattr(self.backend, "eval_control_costs")
                or not controls_stay_resident(self.backend, self.control_cost_descriptors,
                                              self.complex_controls,
                                              self.opt_prefix + "opt_begin_complex")):
            return None
        from qoc_amd.engine import PATH_LINDBLAD
        self.backend.set_control_costs(PATH_LINDBLAD, self.complex_controls,
                                       self.control_cost_descriptors)
        try:
            cost, grads = self.backend.eval_control_costs(PATH_LINDBLAD, device_controls,
                                                          want_grad=bool(want_grad))
        finally:
            self.backend.set_control_costs(PATH_LINDBLAD, self.complex_controls, [])
        if grads is not None:
            grads = structure.from_real_gradients(grads, self.complex_controls)
        return cost, grads

    def _reject_one_sided_search(self, dissipators):
        """A duration search (LindbladSweep.duration_search) needs dE/dtau_b with its rate part,
        which exists only where the engine's evaluation runs two-sided; what can be known here is
        refused by name before the backend sees a problem."""
        from qoc_amd.standard.costs import TargetDensityInfidelity
        L = 0 if dissipators is None else len(dissipators)
        if L == 0:
            raise NotImplementedError(
                "a duration search on the Lindblad path needs 1 to 4 Lindblad operators, "
                "lindblad_data has none: without dissipation this is a closed system - use the "
                "Schroedinger search (HamiltonianSweep.duration_search with "
                "grape_schroedinger_discrete_batch)")
        if L > 4:
            raise NotImplementedError(
                "a duration search on the Lindblad path takes 1 to 4 Lindblad operators (the "
                "rate sensitivities behind dE/dT exist for those), lindblad_data has {}".format(L))
        ok = (len(self.device_costs) == 1
              and isinstance(self.device_costs[0], TargetDensityInfidelity)
              and not self.device_costs[0].requires_step_evaluation)
        if not ok:
            raise NotImplementedError(
                "a duration search on the Lindblad path takes exactly one cost of the densities, a "
                "final TargetDensityInfidelity (costs of the controls alone may join it): the rate "
                "part of dE/dT exists only on the engine's two-sided route, which evaluates that "
                "cost alone; got {}".format(self.device_costs))

    def _check_rate_scales(self, rates, dissipators, data_dependent, shape, each):
        """rate_scales (an ensemble's (M, L), a sweep's (B, L)) against the probed lindblad_data,
        before the backend sees a problem: L operators, and a time-independent system."""
        L = 0 if dissipators is None else len(dissipators)
        if rates.shape[1] != L:
            raise ValueError("rate_scales must be {} with L = {} Lindblad operators of "
                             "lindblad_data, got shape {}".format(shape, L, rates.shape))
        if self.time_dependent:
            raise NotImplementedError(
                "rate_scales need a time-independent system: {} is time dependent, so the engine "
                "holds the control-free generator in per-stage tables (fixed_subdivision > 0) - "
                "one set, not one per {}".format(
                    "lindblad_data" if data_dependent else "the hamiltonian (base or drives)",
                    each))

    def _item_bounds(self, bounds):
        """Bounds of the seeds' K_r channels -> bounds of the evaluated channels: with an ensemble
        those of the items, bound_k max_m |s_mk| and max_m |delta_mj| for the J fixed channels (a
        sweep: the maxima over its seeds)."""
        if self.sweep is not None:
            scales, offsets = self._sweep_args[0], self._sweep_args[1]
        elif self.ensemble is not None:
            scales, offsets = self._ensemble_scales, self.ensemble.offsets
        else:
            return bounds
        scaled = np.asarray(bounds, dtype=np.float64) * np.max(np.abs(scales), axis=0)
        if offsets is None:
            return scaled
        return np.concatenate([scaled, np.max(np.abs(offsets), axis=0)])

    def _set_stage_tables(self, coarse_samples, bounds, sample):
        """The tail of both table builders. coarse_samples :: (h0, g) on the coarsest stage grid:
        their norms and `bounds` on the controls give the sub-division; sample(times) ->
        (h0_stages, g_stages) on its stage times; a time-dependent lindblad_data is sampled there
        as well, and the engine takes the lot."""
        (n, _, kr, nc, n_eval, evolution_time, _, _, dissipators, operators, _) = self._problem_args
        dt = evolution_time / (n_eval - 1)
        h_probe, g_probe = coarse_samples
        h_norm = max(np.linalg.norm(m, 2) for m in h_probe)
        g_norms = [max(np.linalg.norm(g_probe[t, k], 2) for t in range(g_probe.shape[0]))
                   for k in range(kr)]
        pairs = [(dissipators, operators)]
        if self._lindblad_data is not None:  # the largest dissipative norm over the coarse grid
            if self._coarse_lindblad is None:
                self._coarse_lindblad = structure.sample_lindblad_data(
                    self._lindblad_data, n, list(self._coarse_times))
            pairs = list(zip(*self._coarse_lindblad))
        ksub = max(structure.lindblad_subdivision(h_norm, g_norms, bounds, d, o, dt)
                   for d, o in pairs)
        times = self.backend.lindblad_stage_times(evolution_time, n_eval, self._stage_knots, kr,
                                                  ksub)
        h0_stages, g_stages = sample(times)
        extra = {}
        if self._lindblad_data is not None:
            diss_stages, op_stages = structure.sample_lindblad_data(self._lindblad_data, n, times)
            extra = dict(diss_stages=diss_stages, op_stages=op_stages)
        self._set_problem(fixed_subdivision=ksub, h0_stages=h0_stages, g_stages=g_stages, **extra)

    def _set_time_dependent_problem(self, bounds):
        """Sample the time-dependent Hamiltonian at the stage times of a sub-division fine
        enough for controls up to `bounds` and hand the samples to the engine."""
        n, kr, h0 = self._problem_args[0], self.kr, self._problem_args[6]

        def with_perturbations(tables):
            """(h0, g) samples of the base -> those of the problem: with an ensemble the D_j are
            repeated in every table of g (none where g is constant: the problem's own g has
            them)."""
            h, g = tables
            if (self.ensemble is None and self.sweep is None) or g is None:
                return h, g
            return h, self._append_perturbations(g)
        if self._coarse_samples is None and self._hamiltonian is None:
            self._coarse_samples = (np.asarray(h0, dtype=np.complex128)[None],
                                    np.zeros((1, kr, n, n), dtype=np.complex128))
        if self._coarse_samples is None:  # H on the coarsest stage grid: norms for the bound
            self._coarse_samples = with_perturbations(structure.probe_hamiltonian(
                self._hamiltonian, n, self.control_count, self.complex_controls,
                list(self._coarse_times)))

        def sample(times):
            if self._frozen_slices is not None:
                # piecewise-constant frozen controls: by sub-interval, not by time - a stage ON a
                # slice edge belongs to the slice of its sub-interval
                call, controls = self._frozen_slices
                rows = structure.lindblad_stage_rows(
                    self._evolution_time, controls.shape[0], times, self.interpolation_policy)
                u = structure.controls_at(controls, rows, times)
                return np.stack([np.asarray(call(u[q], t), dtype=np.complex128)
                                 for q, t in enumerate(times)]), None
            if self._hamiltonian is None:
                return np.repeat(np.asarray(h0, dtype=np.complex128)[None], len(times), axis=0), None
            return with_perturbations(structure.sample_lindblad_hamiltonian(
                self._hamiltonian, n, self.control_count, self.complex_controls, times))
        self._set_stage_tables(self._coarse_samples, self._item_bounds(bounds), sample)
        self._table_bounds = np.asarray(bounds, dtype=np.float64)

    def _set_linearized_problem(self, controls, device_controls):
        """Tangent of the non-linear callable at `controls` (Nc x K) on the stage grid of a
        sub-division fine enough for this control array, handed to the engine as tables."""
        lin = lambda times: structure.linearize_hamiltonian(  # noqa: E731
            self.linearized_hamiltonian, controls, self._evolution_time, list(times),
            self.hilbert_size, self.complex_controls, self.interpolation_policy,
            rows=structure.lindblad_stage_rows(self._evolution_time, controls.shape[0], times,
                                               self.interpolation_policy))
        bounds = np.max(np.abs(device_controls.reshape(-1, self.kr)), axis=0)
        self._set_stage_tables(lin(self._coarse_times), bounds, lin)

    def _prepare(self, device_controls):
        """A time-dependent problem's tables cover the controls seen so far: widen them first."""
        if not self.time_dependent or self.linearized_hamiltonian is not None:
            return
        if self.control_count == 0:
            need = np.zeros(0)
        else:
            need = np.max(np.abs(device_controls.reshape(-1, self.kr)), axis=0)
        if self._table_bounds is None or np.any(need > self._table_bounds):
            old = np.zeros_like(need) if self._table_bounds is None else self._table_bounds
            self._set_time_dependent_problem(np.maximum(old, need))

    def _pass(self, controls_batch, device_controls, want_grad, again=False):
        return self.backend.evaluate_lindblad(device_controls, want_grad=want_grad)

    def _download_steps(self):
        return self.backend.download_step_densities()

    def _set_cotangents(self, steps, bars):
        self.backend.set_density_cotangents(steps, bars)

    def _problem_stays_resident(self):
        """Time-dependent Hamiltonians included once their tables cover max_control_norms, which
        the resident driver's clip enforces; not the frozen controls of a forward evaluation."""
        return (self._cost_controls is None
                and (not self.time_dependent or self._table_bounds is not None))

    def evaluate_batch(self, controls_batch, want_grad=True, want_step_densities=False):
        """_Evaluator.evaluate_batch; the step states are densities [B x N x S x n x n] (with an
        ensemble a member axis M follows B, in the final densities too). A duration search
        (LindbladSweep.duration_search) evaluates at the current durations and its errors include
        the price of time, time_weight * tau_b, added last."""
        return self._finish_search(
            _Evaluator.evaluate_batch(self, controls_batch, want_grad, want_step_densities),
            want_grad)

    # -- Lindblad sweeps ------------------------------------------------------------------------
    def want_rate_sensitivities(self, on):
        """Ask the evaluations from here on for the sweep's rate sensitivities (one more kernel
        launch per piece of an evaluation with gradients); sweep_sensitivities() returns them.
        Above hilbert_size 32 nothing runs two-sided, so nothing is asked for (the engine refuses
        the request by name) and sweep_sensitivities() keeps its rule: rate_scales is None."""
        if self.hilbert_size > self.MAX_HILBERT_SIZE:
            return
        if hasattr(self.backend, "lindblad_sweep_want_rate_sensitivities"):
            self.backend.lindblad_sweep_want_rate_sensitivities(bool(on))

    def sweep_sensitivities(self):
        """Of the last evaluation with gradients: dict(control_scales = d error_b / d s_bk
        (B x control_count; a complex control's two channels added), offsets = d error_b /
        d delta_bj (B x J), rate_scales = d error_b / d c_bl (B x L)), and for a duration sweep
        evolution_time_gradients = d error_b / d T_b (B). Costs of the controls alone do not depend
        on the tables and do not enter. rate_scales, and with it evolution_time_gradients, is None
        unless the evaluation was asked for it (want_rate_sensitivities) and ran two-sided in
        every piece: one final TargetDensityInfidelity and no other cost, 1 to 4 Lindblad
        operators, a time-independent system, stage values that fit the device memory. Without
        Lindblad operators rate_scales is (B x 0) and the time gradients are the Hamiltonian part."""
        scales, offsets, rates = self.backend.lindblad_sweep_sensitivities()
        scales, offsets = np.asarray(scales), np.asarray(offsets)
        if self.complex_controls:
            scales = scales[:, 0::2] + scales[:, 1::2]
        if rates is None and len(self._problem_args[8] if self._problem_args[8] is not None
                                 else ()) == 0:
            rates = np.zeros((scales.shape[0], 0))
        out = dict(control_scales=scales, offsets=offsets,
                   rate_scales=None if rates is None else np.asarray(rates))
        if self.sweep.time_scaled:
            out["evolution_time_gradients"] = (
                None if rates is None else self.sweep.time_gradients(scales, offsets, rates))
        return out

    def evaluate(self, controls, want_grad=True, want_step_densities=False):
        if self._cost_controls is not None:  # frozen controls: the device's dummy control is zero
            controls = np.zeros((self.control_eval_count, 1))
        return _Evaluator.evaluate(self, controls, want_grad, want_step_densities)
