"""
schroedingerdiscrete.py - evolve_schroedinger_discrete and grape_schroedinger_discrete.

Same positional/keyword signatures, result objects, side effects (stdout table, save file) and
optimizer-callback protocol as qoc/core/schroedingerdiscrete.py:28-353. The time loop, the
matrix exponential and the gradient (the reference's :356-502 traced by autograd) run on the
MI355X through qoc_amd.core.device.SchroedingerEvaluator.
"""

import numpy as np

from qoc_amd.core import batch
from qoc_amd.core.common import (_coefficients_of, _cost_format, _param_gradient,
                                 initialize_coefficients, initialize_controls,
                                 reject_basis_save, strip_controls)
from qoc_amd.core.device import SchroedingerEvaluator, reject_lindblad_sweep, reject_sweep
from qoc_amd.engine import PATH_SCHROEDINGER
from qoc_amd.models import (Dummy, EvolveSchroedingerDiscreteState, EvolveSchroedingerResult,
                            GrapeSchroedingerDiscreteState, GrapeSchroedingerResult,
                            InterpolationPolicy, MagnusPolicy)
from qoc_amd.standard.hamiltonians import HamiltonianEnsemble, HamiltonianSweep
from qoc_amd.standard.optimizers import Adam


_SWEEP_HINT = (": it is B systems with controls of their own - pass it to "
               "grape_schroedinger_discrete_batch, or evaluate one of its systems as "
               "sweep.member(b)")


def _check_ensemble_save(hamiltonian, save_file_path):
    if isinstance(hamiltonian, HamiltonianEnsemble) and save_file_path is not None:
        raise NotImplementedError("save files are not written for a HamiltonianEnsemble "
                                  "(save_file_path must be None)")


def evolve_schroedinger_discrete(evolution_time, hamiltonian, initial_states, system_eval_count,
                                 controls=None, cost_eval_step=1, costs=list(),
                                 interpolation_policy=InterpolationPolicy.LINEAR,
                                 magnus_policy=MagnusPolicy.M2, save_file_path=None,
                                 save_intermediate_states=False, matrix_free="default"):
    """
    Evolve state vectors under the Schroedinger equation and compute the optimization error.

    Arguments as in the reference (schroedingerdiscrete.py:28-84):
    evolution_time :: float; hamiltonian :: (controls (control_count), time) -> (n x n);
    initial_states :: (state_count x n x 1); system_eval_count :: int >= 2;
    controls :: (control_eval_count x control_count) or None; costs :: iterable(Cost).
    Returns EvolveSchroedingerResult{error, final_states}. With a HamiltonianEnsemble
    (qoc_amd.standard) the error is the weighted sum over its members, final_states gains a
    member axis (M x state_count x n x 1) and the result's member_errors holds each member's
    unweighted device cost.
    matrix_free: SchroedingerEvaluator's keyword ("default", "wide", "states", "all", "costs", "small" or
    "effective").
    """
    reject_lindblad_sweep(hamiltonian)
    reject_sweep(hamiltonian, "evolve_schroedinger_discrete", _SWEEP_HINT)
    _check_ensemble_save(hamiltonian, save_file_path)
    if controls is not None:
        controls = np.asarray(controls)
        control_eval_count, control_count = controls.shape[0], controls.shape[1]
    else:
        control_eval_count, control_count = 0, 0
    pstate = EvolveSchroedingerDiscreteState(control_eval_count, cost_eval_step, costs,
                                             evolution_time, hamiltonian, initial_states,
                                             interpolation_policy, magnus_policy, save_file_path,
                                             save_intermediate_states, system_eval_count)
    pstate.save_initial(controls)
    evaluator = SchroedingerEvaluator(
        evolution_time, hamiltonian, initial_states, system_eval_count,
        control_count=control_count, control_eval_count=control_eval_count,
        complex_controls=controls is not None and np.iscomplexobj(controls), costs=costs,
        cost_eval_step=cost_eval_step, interpolation_policy=interpolation_policy,
        magnus_policy=magnus_policy, need_gradients=False, latency_mode=True,
        matrix_free=matrix_free)
    error, _, final_states, step_states = evaluator.evaluate(
        controls, want_grad=False, want_step_states=pstate.save_intermediate_states_)
    if pstate.save_intermediate_states_:
        pstate.save_all_intermediate_states(0, step_states)
    member_errors = None
    if getattr(evaluator, "ensemble", None) is not None:
        member_errors = evaluator.member_errors()[0]
    return EvolveSchroedingerResult(error=error, final_states=final_states,
                                    member_errors=member_errors)


def grape_schroedinger_discrete(control_count, control_eval_count, costs, evolution_time,
                                hamiltonian, initial_states, system_eval_count,
                                complex_controls=False, cost_eval_step=1,
                                impose_control_conditions=None, initial_controls=None,
                                interpolation_policy=InterpolationPolicy.LINEAR,
                                iteration_count=1000, log_iteration_step=10,
                                magnus_policy=MagnusPolicy.M2, max_control_norms=None,
                                min_error=0, optimizer=Adam(), save_file_path=None,
                                save_intermediate_states=False, save_iteration_step=0,
                                control_basis=None, matrix_free="default"):
    """
    Optimize time-discrete controls for the evolution of a set of states (GRAPE).
    Arguments as in the reference (schroedingerdiscrete.py:106-212).
    control_basis (qoc_amd.standard.ControlBasis, optional): the optimizer's parameters are the
    coefficients (P x control_count) of the pulse in that basis and initial_controls holds their
    start. Each iteration evaluates the expanded pulse clipped to max_control_norms (the
    coefficients are never clipped; the derivative of the clip is ignored, as for complex
    controls); costs of the controls and impose_control_conditions act on that pulse. The result's
    best_controls is the evaluated pulse, best_coefficients the coefficients behind it.
    Returns GrapeSchroedingerResult{best_controls, best_error, best_final_states, best_iteration}.
    With a HamiltonianEnsemble the error is the weighted sum over its members, best_final_states
    has a member axis, and member_errors holds each member's unweighted device cost at
    best_controls (one forward evaluation after the loop).
    matrix_free: SchroedingerEvaluator's keyword ("default", "wide", "states", "all", "costs", "small" or
    "effective").
    """
    reject_lindblad_sweep(hamiltonian)
    reject_sweep(hamiltonian, "grape_schroedinger_discrete", _SWEEP_HINT)
    _check_ensemble_save(hamiltonian, save_file_path)
    reject_basis_save(control_basis, save_file_path)
    coefficients = None
    if control_basis is not None:
        coefficients, initial_controls, max_control_norms = initialize_coefficients(
            control_basis, complex_controls, control_count, control_eval_count, evolution_time,
            initial_controls, max_control_norms)
    else:
        initial_controls, max_control_norms = initialize_controls(
            complex_controls, control_count, control_eval_count, evolution_time,
            initial_controls, max_control_norms)
    pstate = GrapeSchroedingerDiscreteState(
        complex_controls, control_count, control_eval_count, cost_eval_step, costs,
        evolution_time, hamiltonian, impose_control_conditions, initial_controls, initial_states,
        interpolation_policy, iteration_count, log_iteration_step, max_control_norms,
        magnus_policy, min_error, optimizer, save_file_path, save_intermediate_states,
        save_iteration_step, system_eval_count)
    pstate.control_basis = control_basis
    if control_basis is not None:
        pstate.coefficients_shape = coefficients.shape
    pstate.evaluator = SchroedingerEvaluator(
        evolution_time, hamiltonian, initial_states, system_eval_count,
        control_count=control_count, control_eval_count=control_eval_count,
        complex_controls=complex_controls, costs=costs, cost_eval_step=cost_eval_step,
        interpolation_policy=interpolation_policy, magnus_policy=magnus_policy,
        need_gradients=True, latency_mode=True, matrix_free=matrix_free)
    pstate.log_and_save_initial()
    reporter = Dummy()
    reporter.iteration = 0
    result = GrapeSchroedingerResult()
    flat_controls = strip_controls(pstate.complex_controls, pstate.initial_controls
                                   if control_basis is None else coefficients)
    pstate.optimizer.run(_esd_wrap, pstate.iteration_count, flat_controls, _esdj_wrap,
                         args=(pstate, reporter, result))
    if (getattr(pstate.evaluator, "ensemble", None) is not None
            and result.best_controls is not None):
        pstate.evaluator.evaluate(result.best_controls, want_grad=False)
        result.member_errors = pstate.evaluator.member_errors()[0]
    return result


def _esd_wrap(controls, pstate, reporter, result):
    """function(params, *args) -> (error, terminate); used by optimizers that ask for values."""
    controls = _cost_format(controls, pstate)
    error, _, final_states, _ = pstate.evaluator.evaluate(controls, want_grad=False)
    reporter.error = error
    reporter.final_states = final_states
    return error, bool(error <= pstate.min_error)


def _esdj_wrap(controls, pstate, reporter, result):
    """jacobian(params, *args) -> (grads, terminate); one device evaluation per call."""
    params = controls
    controls = _cost_format(controls, pstate)
    save_states = pstate.save_intermediate_states_
    error, grads, final_states, step_states = pstate.evaluator.evaluate(
        controls, want_grad=True, want_step_states=save_states)
    reporter.error = error
    reporter.final_states = final_states
    if save_states:
        pstate.save_all_intermediate_states(reporter.iteration, step_states)
    if error < result.best_error:  # strict, as schroedingerdiscrete.py:333
        result.best_controls = controls
        result.best_coefficients = _coefficients_of(params, pstate)
        result.best_error = error
        result.best_final_states = final_states
        result.best_iteration = reporter.iteration
    pstate.log_and_save(controls, error, final_states, grads, reporter.iteration)
    reporter.iteration += 1
    return _param_gradient(grads, pstate), bool(error <= pstate.min_error)


# ---- multi-start GRAPE: B independent optimisations in lock step ---------------

class GrapeSchroedingerBatchResult(batch.BatchResult):
    """Per-seed bests of grape_schroedinger_discrete_batch; `best` is the overall winner as a
    GrapeSchroedingerResult. With a communicator the arrays hold this rank's seeds and
    `global_best_error` the minimum over all ranks."""

    single_result = GrapeSchroedingerResult
    final_field = "best_final_states"


def _ResidentOps(engine, control_costs=(), complex_controls=False):
    """engine.opt_* as the resident loop of core/batch.py calls it (final states [B, S, n, 1]).
    A function under the name of the class it replaced: tools and tests build their ops with it."""
    return batch.ResidentOps(engine, PATH_SCHROEDINGER, control_costs, complex_controls)


def grape_schroedinger_discrete_batch(control_count, control_eval_count, costs, evolution_time,
                                      hamiltonian, initial_states, system_eval_count,
                                      initial_controls, complex_controls=False, cost_eval_step=1,
                                      impose_control_conditions=None,
                                      interpolation_policy=InterpolationPolicy.LINEAR,
                                      iteration_count=1000, log_iteration_step=10,
                                      magnus_policy=MagnusPolicy.M2, max_control_norms=None,
                                      min_error=0, optimizer=Adam(), comm=None,
                                      control_basis=None, matrix_free="default"):
    """
    Multi-start GRAPE: B = len(initial_controls) independent optimisations of the same problem,
    one batched device evaluation per iteration (the engine's batch axis; the reference runs one
    control set per process). Seed b follows EXACTLY the iteration of
    grape_schroedinger_discrete (reference :293-353 per seed): clip -> conditions -> evaluate ->
    best-so-far (strict <) -> optimizer update, its own optimizer state (a deep copy of
    `optimizer`), its own termination at error <= min_error (a finished seed is frozen and no
    longer updated; the batch ends when every seed has finished or after iteration_count
    iterations).

    initial_controls :: (B x control_eval_count x control_count), each conforming to
    max_control_norms. comm (qoc_amd.parallel communicator, optional): the seed axis is sharded
    over its ranks, every rank optimises its own block, and the logged error is the all-reduced
    sum (the path's single collective); result arrays are rank local.
    With a HamiltonianEnsemble (qoc_amd.standard) every seed is evaluated over its M members: the
    errors are the weighted sums, the final states have a member axis, and member_errors[b] holds
    seed b's unweighted member costs at its best controls (one forward evaluation of all seeds
    after the loop).
    optimizer: any step-wise plugin (update(grads, params)); Adam, SGD and LBFGS also run with their
    state resident on the device. With LBFGS a seed whose line search is exhausted is `finished`:
    frozen at its last accepted point like a seed stopped by min_error. LBFGSB (SciPy's loop) is
    single-seed only.
    control_basis (qoc_amd.standard.ControlBasis, optional): as in grape_schroedinger_discrete, per
    seed - initial_controls holds the coefficients (B x P x control_count), the result's
    best_coefficients[b] the coefficients behind best_controls[b]. On the resident route the
    coefficients, the optimizer state sized by them and the map itself stay on the device
    (qocx_opt_begin_basis, qocx_ctrlbasis.hip).
    With a HamiltonianSweep (qoc_amd.standard) of B seeds, B = len(initial_controls) over all ranks,
    seed b is optimised on the sweep's system b (with a communicator every rank sets its block,
    sweep.slice); max_control_norms bound the seeds' own controls. The result's
    sweep_sensitivities holds d error_b / d control_scales (B x control_count) and / d offsets
    (B x J) at the seeds' best controls (one evaluation with gradients after the loop), and for a
    duration sweep evolution_time_gradients (B). User costs without a device descriptor, and
    ControlBandwidthMax with a duration sweep, are refused.
    With a duration search (HamiltonianSweep.durations(time_bounds=..., time_weight=...)) the
    duration of every seed is optimised with its controls: tau_b = T_b / evolution_time is one more
    parameter of seed b (the last entry of its flat vector on the host loop; beside the controls
    on the device), clipped in place to the box every iteration and stepped with the controls'
    rule and learning rate. best_error includes the price of time, best_evolution_times (B) is T_b
    at every seed's best iteration, and sweep_sensitivities is evaluated at the best controls and
    best durations. Adam and SGD keep tau_b resident; LBFGS and plugin optimizers take the host
    loop.
    matrix_free: SchroedingerEvaluator's keyword - "wide" opts one-state Hermitian problems at
    33 <= n <= 64 into the matrix-free Taylor sweeps (more than 128 evaluated items: the route
    yields to the latency mode of smaller batches); "states" opts Hermitian problems of two to
    device.ACTION_STATES_DEFAULT states per seed at 17 <= n <= 32 under one coherent final
    TargetStateInfidelity into them (any batch size); "all" asks for both; "costs" opts one-state
    Hermitian problems at 17 <= n <= 32 into them under any costs the device evaluates (step costs,
    several costs, forbidden states; any batch size); "small" opts one-state Hermitian problems at
    n <= 16 into them (more than 128 evaluated items, as "wide"); "effective" opts one-state
    problems under MagnusPolicy.M4 on a time-independent Hermitian system, or with a
    QuadraticHamiltonian under M2, into them at 17 <= n <= 32 (more than 128 evaluated items).
    Returns GrapeSchroedingerBatchResult.
    """
    reject_lindblad_sweep(hamiltonian)
    if isinstance(hamiltonian, HamiltonianSweep):
        initial_controls = np.asarray(initial_controls)
        if initial_controls.ndim == 3:  # (prepare_seeds reports any other shape)
            hamiltonian = batch.rank_sweep(hamiltonian, initial_controls.shape[0], comm)
    comm, pstate, params = batch.prepare_seeds(
        initial_controls, complex_controls, control_count, control_eval_count, evolution_time,
        max_control_norms, impose_control_conditions, comm, control_basis)
    B = params.shape[0]
    # (latency mode up to 128 evaluated items: an ensemble evaluates M per seed)
    items = B * (hamiltonian.member_count if isinstance(hamiltonian, HamiltonianEnsemble) else 1)
    evaluator = SchroedingerEvaluator(
        evolution_time, hamiltonian, initial_states, system_eval_count,
        control_count=control_count, control_eval_count=control_eval_count,
        complex_controls=complex_controls, costs=costs, cost_eval_step=cost_eval_step,
        interpolation_policy=interpolation_policy, magnus_policy=magnus_policy,
        need_gradients=True, latency_mode=items <= 128, matrix_free=matrix_free)
    stepper = batch.batched_stepper(optimizer, params)
    if getattr(evaluator, "sweep", None) is not None and evaluator.sweep.searches_duration:
        pstate.duration_search = evaluator  # (both loops carry tau_b beside the controls)
    result = GrapeSchroedingerBatchResult(B)
    run = (iteration_count, log_iteration_step, min_error, comm, result)
    # Device-resident form: controls, gradients, Adam moments and the best
    # so far stay in HBM; per iteration the host sees B costs and sends 2 B flags. The same
    # iteration, the same arithmetic (qocx_optim.hip: IEEE operations in the reference's order);
    # the built-in costs of the controls alone are evaluated there too (qocx_ctrlcost.hip).
    if batch.resident_route(stepper, optimizer, pstate, evaluator, B):
        ops = _ResidentOps(evaluator.backend, evaluator.control_cost_descriptors, complex_controls)
        out = batch.run_batch_resident(ops, optimizer, params, pstate, *run)
    else:
        out = batch.run_batch_host(evaluator, stepper, optimizer, params, pstate, *run)
    if getattr(evaluator, "ensemble", None) is not None:
        _ensemble_member_errors(evaluator, out)
    if getattr(evaluator, "sweep", None) is not None:
        batch.sweep_sensitivities(evaluator, out)
    return out


def _ensemble_member_errors(evaluator, result):
    """result.member_errors[b]: the members' unweighted costs at seed b's best controls, from one
    forward evaluation of every seed that has best controls."""
    seeds = [b for b in range(len(result.best_controls)) if result.best_controls[b] is not None]
    if not seeds:
        return
    evaluator.evaluate_batch(np.stack([result.best_controls[b] for b in seeds]), want_grad=False)
    members = evaluator.member_errors()
    for i, b in enumerate(seeds):
        result.member_errors[b] = members[i]
