"""
lindbladmodels.py - program states and results of the Lindblad entry points.

Behaviour follows qoc/models/lindbladmodels.py: result field names (:105-122, :342-366), the
stdout table (:232-238, :311-313) and the HDF5 layout (:60-90, :254-309). One deliberate
difference: intermediate densities of a GRAPE run are stored at the save step (the dataset has
save_count rows); the reference indexes that dataset by the iteration number (:336), which
overruns it whenever save_iteration_step > 1.
"""

import numpy as np

from qoc_amd.models.policies import ProgramType
from qoc_amd.models.programstate import GrapeState, ProgramState
from qoc_amd.models.schroedingermodels import _h5


class EvolveLindbladDiscreteState(ProgramState):
    method = "evolve_lindblad_discrete"

    def __init__(self, control_eval_count, cost_eval_step, costs, evolution_time, hamiltonian,
                 initial_densities, interpolation_policy, lindblad_data, save_file_path,
                 save_intermediate_densities_, system_eval_count):
        super().__init__(control_eval_count, cost_eval_step, costs, evolution_time, hamiltonian,
                         interpolation_policy, ProgramType.EVOLVE, save_file_path,
                         system_eval_count)
        self.initial_densities = initial_densities
        self.lindblad_data = lindblad_data
        self.save_intermediate_densities_ = (save_intermediate_densities_
                                             and save_file_path is not None)

    def save_initial(self, controls):
        if self.save_file_path is None:
            return
        h5py, FileLock, Timeout = _h5()
        print("QOC is saving this evolution to {}.".format(self.save_file_path))
        try:
            with FileLock(self.save_file_lock_path):
                with h5py.File(self.save_file_path, "w") as f:
                    f["controls"] = controls
                    f["cost_eval_step"] = self.cost_eval_step
                    f["costs"] = np.array(["{}".format(c) for c in self.costs])
                    f["evolution_time"] = self.evolution_time
                    f["initial_densities"] = self.initial_densities
                    f["interpolation_policy"] = "{}".format(self.interpolation_policy)
                    if self.save_intermediate_densities_:
                        f["intermediate_densities"] = np.zeros(
                            (self.system_eval_count, *self.initial_densities.shape),
                            dtype=np.complex128)
                    f["method"] = self.method
                    f["program_type"] = self.program_type.value
                    f["system_eval_count"] = self.system_eval_count
        except Timeout:
            print("Timeout while locking {}.".format(self.save_file_lock_path))

    def save_all_intermediate_densities(self, iteration, step_densities):
        """step_densities :: (system_eval_count x density_count x n x n)."""
        if self.save_file_path is None:
            return
        h5py, FileLock, Timeout = _h5()
        try:
            with FileLock(self.save_file_lock_path):
                with h5py.File(self.save_file_path, "a") as f:
                    f["intermediate_densities"][...] = step_densities.astype(np.complex128)
        except Timeout:
            print("Timeout while locking {} while saving intermediate densities on iteration "
                  "{}.".format(self.save_file_lock_path, iteration))


class EvolveLindbladResult(object):
    """member_errors: with a HamiltonianEnsemble, the unweighted device cost of each member (M,);
    None otherwise."""

    def __init__(self, error=None, final_densities=None, member_errors=None):
        super().__init__()
        self.error = error
        self.final_densities = final_densities
        self.member_errors = member_errors


class GrapeLindbladDiscreteState(GrapeState):
    method = "grape_lindblad_discrete"

    def __init__(self, complex_controls, control_count, control_eval_count, cost_eval_step, costs,
                 evolution_time, hamiltonian, impose_control_conditions, initial_controls,
                 initial_densities, interpolation_policy, iteration_count, lindblad_data,
                 log_iteration_step, max_control_norms, min_error, optimizer, save_file_path,
                 save_intermediate_densities_, save_iteration_step, system_eval_count):
        super().__init__(complex_controls, control_count, control_eval_count, cost_eval_step,
                         costs, evolution_time, hamiltonian, impose_control_conditions,
                         initial_controls, interpolation_policy, iteration_count,
                         log_iteration_step, max_control_norms, min_error, optimizer,
                         save_file_path, save_iteration_step, system_eval_count)
        self.hilbert_size = initial_densities[0].shape[0]
        self.initial_densities = initial_densities
        self.lindblad_data = lindblad_data
        self.save_intermediate_densities_ = self.should_save and save_intermediate_densities_

    def _is_save_iteration(self, iteration):
        return self.should_save and (np.mod(iteration, self.save_iteration_step) == 0
                                     or iteration == self.final_iteration)

    def log_and_save(self, controls, error, final_densities, grads, iteration):
        if iteration > self.final_iteration:
            return
        if self.should_log and (np.mod(iteration, self.log_iteration_step) == 0
                                or iteration == self.final_iteration):
            print("{:^6d} | {:^1.8e} | {:^1.8e}".format(iteration, error, np.linalg.norm(grads)))
        if self._is_save_iteration(iteration):
            h5py, FileLock, Timeout = _h5()
            save_step, _ = np.divmod(iteration, self.save_iteration_step)
            try:
                with FileLock(self.save_file_lock_path):
                    with h5py.File(self.save_file_path, "a") as f:
                        f["controls"][save_step, ] = controls
                        f["error"][save_step, ] = error
                        f["final_densities"][save_step, ] = final_densities
                        f["grads"][save_step, ] = grads
            except Timeout:
                print("Timeout while locking {}, could not perform save after iteration {}."
                      "".format(self.save_file_lock_path, iteration))

    def log_and_save_initial(self):
        if self.should_save:
            h5py, FileLock, Timeout = _h5()
            print("QOC is saving this optimization run to {}.".format(self.save_file_path))
            save_count, remainder = np.divmod(self.iteration_count, self.save_iteration_step)
            if remainder != 0:
                save_count += 1
            density_count = len(self.initial_densities)
            ctype = self.initial_controls.dtype
            try:
                with FileLock(self.save_file_lock_path):
                    with h5py.File(self.save_file_path, "w") as f:
                        f["complex_controls"] = self.complex_controls
                        f["control_count"] = self.control_count
                        f["control_eval_count"] = self.control_eval_count
                        f["controls"] = np.zeros((save_count, self.control_eval_count,
                                                  self.control_count), dtype=ctype)
                        f["cost_eval_step"] = self.cost_eval_step
                        f["cost_names"] = np.array([np.bytes_("{}".format(c)) for c in self.costs])
                        f["error"] = np.repeat(np.finfo(np.float64).max, save_count)
                        f["evolution_time"] = self.evolution_time
                        f["final_densities"] = np.zeros(
                            (save_count, density_count, self.hilbert_size, self.hilbert_size),
                            dtype=np.complex128)
                        f["grads"] = np.zeros((save_count, self.control_eval_count,
                                               self.control_count), dtype=ctype)
                        f["initial_controls"] = self.initial_controls
                        f["initial_densities"] = self.initial_densities
                        if self.save_intermediate_densities_:
                            f["intermediate_densities"] = np.zeros(
                                (save_count, self.system_eval_count,
                                 *np.shape(self.initial_densities)), dtype=np.complex128)
                        f["interpolation_policy"] = "{}".format(self.interpolation_policy)
                        f["iteration_count"] = self.iteration_count
                        f["max_control_norms"] = self.max_control_norms
                        f["method"] = self.method
                        f["optimizer"] = "{}".format(self.optimizer)
                        f["program_type"] = self.program_type.value
                        f["system_eval_count"] = self.system_eval_count
            except Timeout:
                print("Timeout while locking {}.".format(self.save_file_lock_path))
        if self.should_log:
            print("iter   |   total error  |    grads_l2   \n"
                  "=========================================")

    def save_all_intermediate_densities(self, iteration, step_densities):
        if iteration > self.final_iteration or not self._is_save_iteration(iteration):
            return
        h5py, FileLock, Timeout = _h5()
        save_step, _ = np.divmod(iteration, self.save_iteration_step)
        try:
            with FileLock(self.save_file_lock_path):
                with h5py.File(self.save_file_path, "a") as f:
                    f["intermediate_densities"][save_step] = step_densities.astype(np.complex128)
        except Timeout:
            print("Timeout while locking {} while saving intermediate densities on iteration "
                  "{}.".format(self.save_file_lock_path, iteration))


class GrapeLindbladResult(object):
    """member_errors: with a HamiltonianEnsemble, the unweighted device cost of each member (M,)
    at best_controls, from one forward evaluation after the optimisation; None otherwise."""

    def __init__(self, best_controls=None, best_error=np.finfo(np.float64).max,
                 best_final_densities=None, best_iteration=None, member_errors=None):
        super().__init__()
        self.best_controls = best_controls
        self.best_error = best_error
        self.best_final_densities = best_final_densities
        self.best_iteration = best_iteration
        self.member_errors = member_errors
        # with a ControlBasis: the coefficients (P x control_count) behind best_controls
        self.best_coefficients = None
