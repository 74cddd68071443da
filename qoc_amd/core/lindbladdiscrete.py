"""
lindbladdiscrete.py - evolve_lindblad_discrete, grape_lindblad_discrete and its multi-start form
grape_lindblad_discrete_batch.

Same positional/keyword signatures, result objects, side effects (stdout table, save file) and
optimizer-callback protocol as qoc/core/lindbladdiscrete.py:31-257. The integration of the
master equation and the gradient (the reference's :357-441 and the adaptive RKDP5 of
mathmethods.py:352-480, traced by autograd) run on the MI355X through
qoc_amd.core.device.LindbladEvaluator (fixed-step DOP853 + discrete adjoint; DESIGN.md 9 for
the parity tolerances that follow from replacing an adaptive integrator).
"""

import numpy as np

from qoc_amd.core import batch
from qoc_amd.core.common import (_coefficients_of, _cost_format, _param_gradient,
                                 initialize_coefficients, initialize_controls,
                                 reject_basis_save, strip_controls)
from qoc_amd.core.device import (LINDBLAD_SWEEP_HINT, LindbladEvaluator,
                                 reject_costless_lindblad_ensemble, reject_sweep)
from qoc_amd.core.structure import NonLinearHamiltonianError
from qoc_amd.engine import PATH_LINDBLAD
from qoc_amd.models import (Dummy, EvolveLindbladDiscreteState, EvolveLindbladResult,
                            GrapeLindbladDiscreteState, GrapeLindbladResult,
                            InterpolationPolicy)
from qoc_amd.standard.hamiltonians import HamiltonianEnsemble, LindbladSweep
from qoc_amd.standard.optimizers import Adam


_SWEEP_HINT = (": it is B open systems with controls of their own - pass it to "
               "grape_lindblad_discrete_batch, or evaluate one of its systems as sweep.member(b) "
               "with sweep.member_lindblad_data(b, lindblad_data); save files go with these "
               "entry points and are not written for a sweep")


def _check_ensemble(hamiltonian, costs, save_file_path=None, where=None):
    """Before any save file is touched and before a backend is made: a HamiltonianEnsemble on the
    Lindblad path needs at least one cost (its error is the weighted sum of the members' costs)
    and writes no save file. A plain HamiltonianSweep is refused everywhere on this path, a
    LindbladSweep by the single-problem entry points (`where` names one)."""
    if where is not None and isinstance(hamiltonian, LindbladSweep):
        reject_sweep(hamiltonian, where, _SWEEP_HINT)
    reject_sweep(hamiltonian, "the Lindblad entry points", LINDBLAD_SWEEP_HINT,
                 lindblad_sweep_ok=True)
    if not isinstance(hamiltonian, HamiltonianEnsemble):
        return
    reject_costless_lindblad_ensemble(hamiltonian, costs)
    if save_file_path is not None:
        raise NotImplementedError("save files are not written for a HamiltonianEnsemble on the "
                                  "Lindblad path (save_file_path must be None)")


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


def evolve_lindblad_discrete(evolution_time, initial_densities, system_eval_count,
                             controls=None, cost_eval_step=1, costs=list(), hamiltonian=None,
                             interpolation_policy=InterpolationPolicy.LINEAR, lindblad_data=None,
                             save_file_path=None, save_intermediate_densities=False, wide=False):
    """
    Evolve density matrices under the Lindblad master equation and compute the optimization
    error. Arguments as in the reference (lindbladdiscrete.py:31-91):
    initial_densities :: (density_count x n x n); hamiltonian :: (controls, time) -> (n x n);
    lindblad_data :: (time) -> (dissipators (L), operators (L x n x n)).
    Returns EvolveLindbladResult{error, final_densities}. With a HamiltonianEnsemble
    (qoc_amd.standard) whose base is linear in the controls every member evolves under the same
    lindblad_data: the error is the weighted sum over the members, final_densities gains a member
    axis (M x density_count x n x n) and the result's member_errors holds each member's
    unweighted device cost. Such an ensemble needs at least one cost (costs of the densities with
    a device descriptor, and costs of the controls alone), K_r + J <= 8 real control channels and
    perturbations, and no save file. An ensemble with rate_scales (M x L) gives member m the
    dissipation rates rate_scales[m] * dissipators of lindblad_data (an uncertain T1 / T2); that
    needs a hamiltonian and a lindblad_data without explicit time dependence.
    wide=True takes 33 <= n <= 64 (time-independent systems without rates or durations of their
    own; LindbladEvaluator); the default refuses n > 32.
    """
    _check_ensemble(hamiltonian, costs, save_file_path, "evolve_lindblad_discrete")
    if controls is not None:
        controls = np.asarray(controls)
        control_eval_count, control_count = controls.shape[0], controls.shape[1]
    else:
        control_eval_count, control_count = 0, 0
    pstate = EvolveLindbladDiscreteState(control_eval_count, cost_eval_step, costs,
                                         evolution_time, hamiltonian, initial_densities,
                                         interpolation_policy, lindblad_data, save_file_path,
                                         save_intermediate_densities, system_eval_count)
    pstate.save_initial(controls)
    common = dict(hamiltonian=hamiltonian, lindblad_data=lindblad_data, costs=costs,
                  cost_eval_step=cost_eval_step, interpolation_policy=interpolation_policy,
                  need_gradients=False, wide=wide)
    try:
        evaluator = LindbladEvaluator(
            evolution_time, initial_densities, system_eval_count, control_count=control_count,
            control_eval_count=control_eval_count,
            complex_controls=controls is not None and np.iscomplexobj(controls), **common)
        device_controls = controls
    except NonLinearHamiltonianError:
        # not linear in the controls: fold this control array into a time-dependent Hamiltonian
        evaluator = LindbladEvaluator(evolution_time, initial_densities, system_eval_count,
                                      frozen_controls=controls, **common)
        device_controls = None
    error, _, final_densities, step_densities = evaluator.evaluate(
        device_controls, want_grad=False,
        want_step_densities=pstate.save_intermediate_densities_)
    if pstate.save_intermediate_densities_:
        pstate.save_all_intermediate_densities(0, step_densities)
    member_errors = None
    if evaluator.ensemble is not None:
        member_errors = evaluator.member_errors()[0]
    return EvolveLindbladResult(error=error, final_densities=final_densities,
                                member_errors=member_errors)


def grape_lindblad_discrete(control_count, control_eval_count, costs, evolution_time,
                            initial_densities, system_eval_count, complex_controls=False,
                            cost_eval_step=1, hamiltonian=None, impose_control_conditions=None,
                            initial_controls=None,
                            interpolation_policy=InterpolationPolicy.LINEAR,
                            iteration_count=1000, lindblad_data=None, log_iteration_step=10,
                            max_control_norms=None, min_error=0, optimizer=Adam(),
                            save_file_path=None, save_intermediate_densities=False,
                            save_iteration_step=0, control_basis=None, wide=False):
    """
    Optimize time-discrete controls for the evolution of a set of densities under the Lindblad
    equation (GRAPE). Arguments as in the reference (lindbladdiscrete.py:106-212).
    control_basis (qoc_amd.standard.ControlBasis, optional): as in grape_schroedinger_discrete -
    initial_controls holds the coefficients (P x control_count), the expanded pulse clipped to
    max_control_norms is evaluated, the result gains best_coefficients.
    Returns GrapeLindbladResult{best_controls, best_error, best_final_densities,
    best_iteration}. With a HamiltonianEnsemble (robust GRAPE under decoherence; conditions as in
    evolve_lindblad_discrete: at least one cost, K_r + J <= 8, no save file) the error is the
    weighted sum over its members, best_final_densities has a member axis, and member_errors
    holds each member's unweighted device cost at best_controls (one forward evaluation after the
    loop).
    wide=True takes 33 <= n <= 64 (as in evolve_lindblad_discrete); the default refuses n > 32.
    """
    _check_ensemble(hamiltonian, costs, save_file_path, "grape_lindblad_discrete")
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
    pstate = GrapeLindbladDiscreteState(
        complex_controls, control_count, control_eval_count, cost_eval_step, costs,
        evolution_time, hamiltonian, impose_control_conditions, initial_controls,
        initial_densities, interpolation_policy, iteration_count, lindblad_data,
        log_iteration_step, max_control_norms, min_error, optimizer, save_file_path,
        save_intermediate_densities, save_iteration_step, system_eval_count)
    pstate.control_basis = control_basis
    if control_basis is not None:
        pstate.coefficients_shape = coefficients.shape
    pstate.evaluator = LindbladEvaluator(
        evolution_time, initial_densities, system_eval_count, hamiltonian=hamiltonian,
        lindblad_data=lindblad_data, control_count=control_count,
        control_eval_count=control_eval_count, complex_controls=complex_controls, costs=costs,
        cost_eval_step=cost_eval_step, interpolation_policy=interpolation_policy,
        need_gradients=True, control_bounds=max_control_norms, wide=wide)
    pstate.log_and_save_initial()
    reporter = Dummy()
    reporter.iteration = 0
    result = GrapeLindbladResult()
    flat_controls = strip_controls(pstate.complex_controls, pstate.initial_controls
                                   if control_basis is None else coefficients)
    pstate.optimizer.run(_eld_wrap, pstate.iteration_count, flat_controls, _eldj_wrap,
                         args=(pstate, reporter, result))
    if pstate.evaluator.ensemble is not None and result.best_controls is not None:
        pstate.evaluator.evaluate(result.best_controls, want_grad=False)
        result.member_errors = pstate.evaluator.member_errors()[0]
    return result


def _eld_wrap(controls, pstate, reporter, result):
    controls = _cost_format(controls, pstate)
    error, _, final_densities, _ = pstate.evaluator.evaluate(controls, want_grad=False)
    reporter.error = error
    reporter.final_densities = final_densities
    return error, bool(error <= pstate.min_error)


def _eldj_wrap(controls, pstate, reporter, result):
    params = controls
    controls = _cost_format(controls, pstate)
    save_densities = pstate.save_intermediate_densities_
    error, grads, final_densities, step_densities = pstate.evaluator.evaluate(
        controls, want_grad=True, want_step_densities=save_densities)
    reporter.error = error
    reporter.final_densities = final_densities
    if save_densities:
        pstate.save_all_intermediate_densities(reporter.iteration, step_densities)
    if error < result.best_error:  # strict, as lindbladdiscrete.py:334
        result.best_controls = controls
        result.best_coefficients = _coefficients_of(params, pstate)
        result.best_error = error
        result.best_final_densities = final_densities
        result.best_iteration = reporter.iteration
    pstate.log_and_save(controls, error, final_densities, grads, reporter.iteration)
    reporter.iteration += 1
    return _param_gradient(grads, pstate), bool(error <= pstate.min_error)


# ---- multi-start GRAPE: B independent optimisations in lock step (core/batch.py) -----------------

class GrapeLindbladBatchResult(batch.BatchResult):
    """Per-seed bests of grape_lindblad_discrete_batch; `best` is the overall winner as a
    GrapeLindbladResult. With a communicator the arrays hold this rank's seeds and
    `global_best_error` the minimum over all ranks."""

    single_result = GrapeLindbladResult
    final_field = "best_final_densities"


def _ResidentOps(engine, control_costs=(), complex_controls=False):
    """engine.lindblad_* (the Lindblad problem's resident buffers) as the resident loop of
    core/batch.py calls them. A function under the name of the class it replaced."""
    return batch.ResidentOps(engine, PATH_LINDBLAD, control_costs, complex_controls)


def grape_lindblad_discrete_batch(control_count, control_eval_count, costs, evolution_time,
                                  initial_densities, system_eval_count, initial_controls,
                                  complex_controls=False, cost_eval_step=1, hamiltonian=None,
                                  impose_control_conditions=None,
                                  interpolation_policy=InterpolationPolicy.LINEAR,
                                  iteration_count=1000, lindblad_data=None, log_iteration_step=10,
                                  max_control_norms=None, min_error=0, optimizer=Adam(),
                                  comm=None, control_basis=None, wide=False):
    """
    Multi-start Lindblad GRAPE: B = len(initial_controls) independent optimisations of the same
    problem, one batched device evaluation per iteration. Seed b follows EXACTLY the iteration of
    grape_lindblad_discrete (reference lindbladdiscrete.py:297-352 per seed): clip -> conditions ->
    evaluate -> best-so-far (strict <) -> optimizer update with its own optimizer state, its own
    termination at error <= min_error (a finished seed is frozen; the batch ends when every seed
    has finished or after iteration_count iterations).

    Arguments as grape_lindblad_discrete without the save-file ones; initial_controls ::
    (B x control_eval_count x control_count), each conforming to max_control_norms. comm
    (qoc_amd.parallel communicator, optional): the seed axis is sharded over its ranks, result
    arrays are rank local. With costs the device evaluates (the built-in density costs and the four
    built-in costs of the controls), a Hamiltonian linear in the controls, the built-in Adam / SGD /
    LBFGS and no control conditions, controls, gradients, optimizer states and the best so far stay in HBM
    (qocx_lindblad_opt_*; real or complex controls); otherwise the host drives
    LindbladEvaluator.evaluate_batch. Both routes give the same numbers to rounding (bit for bit
    without costs of the controls and without a clip acting on a complex control).
    control_basis (qoc_amd.standard.ControlBasis, optional): as in
    grape_schroedinger_discrete_batch - initial_controls holds the coefficients
    (B x P x control_count), the result gains best_coefficients per seed
    (qocx_lindblad_opt_begin_basis on the resident route).
    With a HamiltonianEnsemble (conditions as in evolve_lindblad_discrete: at least one cost,
    K_r + J <= 8) every seed is evaluated over its M members on either route: the errors are the
    weighted sums, the final densities have a member axis, and member_errors[b] holds seed b's
    unweighted member costs at its best controls (one forward evaluation of all seeds after the
    loop).
    With a LindbladSweep (qoc_amd.standard) of B seeds, B = len(initial_controls) over all ranks,
    seed b is optimised on the sweep's open system b - its own scales, offsets and rate factors
    (with a communicator every rank sets its block, sweep.slice) - on either route;
    max_control_norms bound the seeds' own controls, costs may be empty, and the final densities
    have no member axis. The result's sweep_sensitivities holds d error_b / d control_scales
    (B x control_count), / d offsets (B x J) and / d rate_scales (B x L) at the seeds' best
    controls (one evaluation with gradients after the loop), and for a duration sweep
    evolution_time_gradients (B). The last two are None unless that evaluation ran two-sided: ONE
    cost, a final TargetDensityInfidelity (no step cost), 1 to 4 Lindblad operators, a
    time-independent system and stage values that fit the device memory. Refused: user costs
    without a device descriptor, ControlBandwidthMax with a duration sweep, a QuadraticHamiltonian,
    ensemble, sweep or non-linear base, K_r + J > 8, and - with rates of its own, so for every
    duration sweep - a time-dependent hamiltonian or lindblad_data.
    With a duration search (LindbladSweep.duration_search) the duration of every seed is optimised
    with its controls (minimum-time GRAPE under T1 / T2): tau_b = T_b / evolution_time is one more
    parameter of seed b (the last entry of its flat vector on the host loop; beside the controls on
    the device), clipped in place to the box every iteration and stepped with the controls' rule
    and learning rate. best_error includes the price of time, best_evolution_times (B) is T_b at
    every seed's best iteration, and sweep_sensitivities is evaluated at the best controls and best
    durations. Adam and SGD keep tau_b resident; LBFGS and plugin optimizers take the host loop.
    The search needs the two-sided evaluation: exactly one cost of the densities, a final
    TargetDensityInfidelity (costs of the controls alone may join it), and 1 to 4 Lindblad
    operators; anything else is refused by name.
    wide=True takes 33 <= n <= 64 on either route: time-independent systems, ensembles and sweeps
    without rates, durations or a duration search; sweep_sensitivities then holds the channel tables
    only (rate_scales and evolution_time_gradients are None: nothing runs two-sided above 32).
    Returns GrapeLindbladBatchResult.
    """
    _check_ensemble(hamiltonian, costs)
    if isinstance(hamiltonian, LindbladSweep):
        initial_controls = np.asarray(initial_controls)
        if initial_controls.ndim == 3:  # (prepare_seeds reports any other shape)
            hamiltonian = batch.rank_sweep(hamiltonian, initial_controls.shape[0], comm)
    comm, pstate, params = batch.prepare_seeds(
        initial_controls, complex_controls, control_count, control_eval_count, evolution_time,
        max_control_norms, impose_control_conditions, comm, control_basis)
    B = params.shape[0]
    evaluator = LindbladEvaluator(
        evolution_time, initial_densities, system_eval_count, hamiltonian=hamiltonian,
        lindblad_data=lindblad_data, control_count=control_count,
        control_eval_count=control_eval_count, complex_controls=complex_controls, costs=costs,
        cost_eval_step=cost_eval_step, interpolation_policy=interpolation_policy,
        need_gradients=True, control_bounds=pstate.max_control_norms, wide=wide)
    stepper = batch.batched_stepper(optimizer, params)
    if evaluator.sweep is not None and evaluator.sweep.searches_duration:
        pstate.duration_search = evaluator  # (both loops carry tau_b beside the controls)
    result = GrapeLindbladBatchResult(B)
    run = (iteration_count, log_iteration_step, min_error, comm, result)
    if batch.resident_route(stepper, optimizer, pstate, evaluator, B):
        ops = _ResidentOps(evaluator.backend, evaluator.control_cost_descriptors, complex_controls)
        out = batch.run_batch_resident(ops, optimizer, params, pstate, *run)
    else:
        out = batch.run_batch_host(evaluator, stepper, optimizer, params, pstate, *run)
    if evaluator.ensemble is not None:
        _ensemble_member_errors(evaluator, out)
    if evaluator.sweep is not None:
        batch.sweep_sensitivities(evaluator, out)
    return out
