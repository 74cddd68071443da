"""
batch.py - the multi-start GRAPE loop shared by grape_schroedinger_discrete_batch and
grape_lindblad_discrete_batch: B independent optimisations of one problem in lock step, one
batched device evaluation per iteration.

Seed b follows EXACTLY the iteration of the single-seed driver (the reference's
schroedingerdiscrete.py:293-353 / lindbladdiscrete.py:297-352 per seed): clip -> conditions ->
evaluate -> best-so-far (strict <) -> optimizer update with its own optimizer state, its own
termination at error <= min_error (a finished seed is frozen). Two routes: the host loop (any
evaluator, any step-wise optimizer plugin) and the device-resident one, where controls, gradients,
optimizer state (Adam moments, the L-BFGS history) and the best so far stay in HBM and the host sees
B costs per iteration. An optimizer with `needs_error` (LBFGS) also takes the seed's error and may
declare a seed `finished`: such a seed leaves the loop as one stopped by min_error does.
"""

import numpy as np

from qoc_amd.core import structure
from qoc_amd.core.common import (initialize_coefficients, initialize_controls, slap_controls,
                                 strip_controls)
from qoc_amd.engine import PATH_LINDBLAD
from qoc_amd.models import Dummy
from qoc_amd.standard.optimizers import LBFGS, SGD, Adam


class BatchResult(object):
    """Per-seed bests of a multi-start driver; `best` is the overall winner as the single-seed
    result class. With a communicator the arrays hold this rank's seeds and `global_best_error` the
    minimum over all ranks. Subclasses name the single-seed result and its final-state field."""

    single_result = None
    final_field = None

    def __init__(self, seed_count):
        self.best_controls = [None] * seed_count
        self.best_error = np.repeat(np.finfo(np.float64).max, seed_count)
        setattr(self, self.final_field, [None] * seed_count)
        self.best_iteration = np.full(seed_count, -1, dtype=np.int64)
        self.iterations_run = np.zeros(seed_count, dtype=np.int64)
        self.global_best_error = None
        # Hamiltonian ensembles: per seed, the members' unweighted costs at the best controls
        self.member_errors = [None] * seed_count
        # with a ControlBasis: per seed, the coefficients (P x control_count) behind best_controls
        self.best_coefficients = [None] * seed_count
        # with a HamiltonianSweep: dict(control_scales (B x control_count), offsets (B x J)[,
        # evolution_time_gradients (B)]) at every seed's best controls; a LindbladSweep adds
        # rate_scales (B x L), which - with evolution_time_gradients - is None where the
        # sensitivity evaluation did not run two-sided
        self.sweep_sensitivities = None
        # with a duration search (HamiltonianSweep.durations(time_bounds=...)): T_b at every seed's
        # best iteration, (B,); NaN for a seed without one
        self.best_evolution_times = None

    @property
    def best(self):
        b = int(np.argmin(self.best_error))
        out = self.single_result(
            best_controls=self.best_controls[b], best_error=float(self.best_error[b]),
            best_iteration=int(self.best_iteration[b]),
            **{self.final_field: getattr(self, self.final_field)[b]})
        if self.member_errors[b] is not None:
            out.member_errors = self.member_errors[b]
        out.best_coefficients = self.best_coefficients[b]
        return out


def _optimizer_clone(optimizer, flat_controls):
    """A private copy of a step-wise optimizer plugin, initialised as its run() would."""
    import copy
    if not hasattr(optimizer, "update"):
        raise NotImplementedError(
            "the multi-start GRAPE drivers step the optimizer one update at a time and need its "
            "update(grads, params) (Adam, SGD); {} only offers run().".format(optimizer))
    clone = copy.deepcopy(optimizer)
    if getattr(clone, "needs_error", False) and hasattr(clone, "reset"):
        clone.reset()  # (LBFGS and its subclasses: every seed starts from fresh state)
    if hasattr(clone, "gradient_moment"):  # Adam.run(), adam.py:83-88 of the reference
        clone.iteration_count = 0
        clone.gradient_moment = np.zeros_like(flat_controls)
        clone.gradient_square_moment = np.zeros_like(flat_controls)
    return clone


# ---- the B optimizer states as [B, P] arrays ------------------------------------------------------
# The per-seed loop (one plugin object per seed: slap / clip / strip / update = ~60 small NumPy
# calls per seed and iteration) costs 13 ms of host time per iteration at B = 256, Nc = 1001,
# K = 2 - as long as the device evaluation it wraps. For the built-in Adam and
# SGD the same arithmetic runs on [rows, P] blocks: every operation is elementwise and in the
# reference's order (adam.py:110-165, sgd.py), so seed b still walks exactly its single-seed
# trajectory, bit for bit. Row blocks keep the temporaries cache resident.
_ROW_BLOCK = 16
_POOL = None


def _row_blocks(rows):
    """rows (sorted index array) as a list of slices where they are consecutive, index arrays
    otherwise, at most _ROW_BLOCK rows each."""
    out = []
    for lo in range(0, len(rows), _ROW_BLOCK):
        r = rows[lo:lo + _ROW_BLOCK]
        out.append(slice(int(r[0]), int(r[-1]) + 1) if r[-1] - r[0] + 1 == len(r) else r)
    return out


def _for_blocks(work, blocks):
    """work(block) for every block, on a small thread pool (NumPy releases the GIL inside its
    loops; the blocks are disjoint rows)."""
    global _POOL
    if len(blocks) < 4:
        for blk in blocks:
            work(blk)
        return
    if _POOL is None:
        import os
        from concurrent.futures import ThreadPoolExecutor
        _POOL = ThreadPoolExecutor(max_workers=max(1, min(8, (os.cpu_count() or 2) - 1)))
    list(_POOL.map(work, blocks))


_NATIVE_HOST = None


def _native_ok(*arrays):
    """The [B, P] host routines of libqocx (clip, Adam / SGD on host threads) can take these
    arrays. Without the library (a CPU box running the host logic against the oracle backend)
    the NumPy block path below each call site does the same arithmetic."""
    global _NATIVE_HOST
    if _NATIVE_HOST is None:
        from qoc_amd import engine
        try:
            engine.load_library()
            _NATIVE_HOST = True
        except ImportError:  # the library FILE is absent: a CPU box running the host logic only
            _NATIVE_HOST = False
        # (a library that is present but does not load, or lacks a declared symbol, is a broken
        # build: OSError / AttributeError propagate instead of silently taking the NumPy path)
    return _NATIVE_HOST and all(a.dtype == np.float64 and a.flags.c_contiguous for a in arrays)


class _BatchedSGD(object):
    def __init__(self, optimizer, params):
        self.learning_rate = optimizer.learning_rate

    def update(self, grads, params, rows):
        """params[rows] <- SGD.update(grads[rows], params[rows]), in place."""
        if _native_ok(grads, params):
            from qoc_amd import engine
            engine.host_optimizer_update(0, params, grads, None, None, rows, self.learning_rate)
            return

        def work(r):
            params[r] = params[r] - self.learning_rate * grads[r]
        _for_blocks(work, _row_blocks(rows))


class _BatchedAdam(object):
    def __init__(self, optimizer, params):
        self.o = optimizer
        self.m = np.zeros_like(params)
        self.v = np.zeros_like(params)
        self.count = np.zeros(params.shape[0], dtype=np.int64)

    def update(self, grads, params, rows):
        """params[rows] <- Adam.update(grads[rows], params[rows]) with every seed's own moments and
        step counter, in place: the operations of adam.py:110-165 in their order, element by
        element (a * x + b * y is formed as (a * x) + (b * y) there and here)."""
        o = self.o
        for count in np.unique(self.count[rows]):  # (seeds that stopped earlier keep their own)
            sel = rows[self.count[rows] == count]
            if o.apply_learning_rate_decay:
                learning_rate = (o.initial_learning_rate
                                 * np.exp(-np.divide(count, o.learning_rate_decay)))
            else:
                learning_rate = o.initial_learning_rate
            step = count + 1
            corr_1 = 1 - np.power(o.beta_1, step)
            corr_2 = 1 - np.power(o.beta_2, step)
            if not o.apply_scale_grads and _native_ok(grads, params, self.m, self.v):
                # the same operations on host threads of libqocx (qocx_host_optimizer_update)
                from qoc_amd import engine
                engine.host_optimizer_update(
                    1, params, grads, self.m, self.v, sel, learning_rate, o.beta_1, o.beta_2,
                    o.epsilon, corr_1, corr_2, o.clip_grads if o.apply_clip_grads else None)
                self.count[sel] = step
                continue

            def work(r):
                g = grads[r]
                if o.apply_scale_grads:
                    norms = np.array([np.linalg.norm(row) for row in g])
                    g = (g / norms[:, None]) * o.scale_grads
                if o.apply_clip_grads:
                    g = np.clip(g, -o.clip_grads, o.clip_grads)
                m, v = self.m[r], self.v[r]  # views for a slice, copies for an index array
                t = np.multiply(g, 1 - o.beta_1)
                np.multiply(m, o.beta_1, out=m)
                m += t                                    # gradient_moment
                np.square(g, out=t)
                t *= (1 - o.beta_2)
                np.multiply(v, o.beta_2, out=v)
                v += t                                    # gradient_square_moment
                if not isinstance(r, slice):
                    self.m[r] = m
                    self.v[r] = v
                u = np.divide(v, corr_2)                  # square_hat
                np.sqrt(u, out=u)
                u += o.epsilon
                np.divide(m, corr_1, out=t)               # moment_hat
                np.divide(t, u, out=t)
                t *= learning_rate
                if isinstance(r, slice):
                    p = params[r]
                    p -= t
                else:
                    params[r] = params[r] - t
            _for_blocks(work, _row_blocks(sel))
            self.count[sel] = step


class _BatchedLBFGS(object):
    """B per-seed LBFGS state machines (the arithmetic of a seed is not elementwise: each keeps its
    own history and line-search state); `finished` [B] is read by the loop after every update."""

    needs_error = True

    def __init__(self, optimizer, params):
        self.seeds = [_optimizer_clone(optimizer, p) for p in params]
        self.finished = np.zeros(params.shape[0], dtype=bool)

    def update(self, grads, params, rows, errors):
        """params[rows] <- the seeds' next trial points, in place."""
        for b in rows:
            params[b] = self.seeds[b].update(grads[b], params[b], errors[b])
            self.finished[b] = self.seeds[b].finished


def batched_stepper(optimizer, params):
    """The [B, P] form of the built-in step-wise optimizers; None for any other plugin (those keep
    one deep copy per seed and their own update()). The LBFGS stepper also takes the seeds' errors."""
    if type(optimizer) is LBFGS:
        return _BatchedLBFGS(optimizer, params)
    if type(optimizer) is Adam:
        return _BatchedAdam(optimizer, params)
    if type(optimizer) is SGD:
        return _BatchedSGD(optimizer, params)
    return None


def _coefficients_batch(params, pstate):
    """The rows of params [B, P] as coefficient arrays (B x P x control_count) of a ControlBasis."""
    shape = (params.shape[0],) + tuple(pstate.coefficients_shape)
    if pstate.complex_controls:
        half = params.shape[1] // 2
        return (params[:, :half] + 1j * params[:, half:]).reshape(shape)
    return params.reshape(shape)


def _cost_format_batch(params, pstate):
    """_cost_format on all rows of params [B, P] at once: (B x Nc x K) controls, clipped in place
    (a view of params for real controls, as in the single-seed driver), conditions per seed. With a
    ControlBasis the rows are coefficients: they stay as they are, their expansion is clipped."""
    B = params.shape[0]
    shape = (B,) + tuple(pstate.controls_shape)
    basis = getattr(pstate, "control_basis", None)
    if basis is not None:
        controls = basis.expand(_coefficients_batch(params, pstate))
    elif pstate.complex_controls:
        half = params.shape[1] // 2
        controls = (params[:, :half] + 1j * params[:, half:]).reshape(shape)
    else:
        controls = params.reshape(shape)
        if _native_ok(params) and controls.base is not None:
            from qoc_amd import engine
            engine.host_clip_controls(controls, pstate.max_control_norms)
            if pstate.impose_control_conditions is not None:
                controls = np.stack([pstate.impose_control_conditions(controls[b])
                                     for b in range(B)])
            return controls
    for i, max_norm in enumerate(pstate.max_control_norms):  # clip_control_norms, all seeds
        column = controls[:, :, i]
        moduli = np.abs(column)
        over = np.less(max_norm, moduli)
        if over.any():
            column[over] = (column[over] / moduli[over]) * max_norm
    if pstate.impose_control_conditions is not None:
        controls = np.stack([pstate.impose_control_conditions(controls[b]) for b in range(B)])
    return controls


def _strip_batch(complex_controls, arrays):
    """strip_controls on every row: (B x Nc x K) -> [B, P]."""
    flat = np.reshape(arrays, (arrays.shape[0], -1))
    if complex_controls:
        flat = np.hstack((np.real(flat), np.imag(flat)))
    return flat


def prepare_seeds(initial_controls, complex_controls, control_count, control_eval_count,
                  evolution_time, max_control_norms, impose_control_conditions, comm,
                  control_basis=None):
    """This rank's block of the seeds, checked as the single-seed drivers check one control array:
    (comm, pstate for _cost_format_batch, params [B, P] in the optimizer's format). With a
    control_basis the seeds are coefficient arrays (seed_count x P x control_count) and so are the
    parameters; their expansions are checked as start controls."""
    from qoc_amd import parallel
    if control_basis is not None and initial_controls is None:
        raise ValueError("with a control_basis, initial_controls must hold the initial "
                         "coefficients (seed_count x P x control_count)")
    initial_controls = np.asarray(initial_controls)
    if initial_controls.ndim != 3:
        raise ValueError("initial_controls must be (seed_count x {} x control_count), got shape {}"
                         "".format("control_eval_count" if control_basis is None else "P",
                                   initial_controls.shape))
    comm = comm if comm is not None else parallel.SingleComm()
    lo, hi = parallel.shard_bounds(initial_controls.shape[0], comm.rank, comm.world)
    if max_control_norms is None:  # the default of initialize_controls, also for a rank without seeds
        max_control_norms = np.ones(control_count)
    seeds = []
    for b in range(lo, hi):
        if control_basis is not None:
            controls_b, _, max_control_norms = initialize_coefficients(
                control_basis, complex_controls, control_count, control_eval_count,
                evolution_time, initial_controls[b], max_control_norms)
        else:
            controls_b, max_control_norms = initialize_controls(
                complex_controls, control_count, control_eval_count, evolution_time,
                initial_controls[b], max_control_norms)
        seeds.append(np.array(controls_b))
    pstate = Dummy()
    pstate.control_basis = control_basis
    knots = control_eval_count
    if control_basis is not None:
        if control_basis.knot_count != control_eval_count:  # (also for a rank without seeds)
            raise ValueError("control_basis maps to {} knots, control_eval_count is {}"
                             "".format(control_basis.knot_count, control_eval_count))
        knots = control_basis.coefficient_count
        pstate.coefficients_shape = (knots, control_count)
    pstate.complex_controls = complex_controls
    pstate.controls_shape = (control_eval_count, control_count)
    pstate.max_control_norms = max_control_norms
    pstate.impose_control_conditions = impose_control_conditions
    params = (np.stack([strip_controls(complex_controls, c) for c in seeds]) if seeds
              else np.zeros((0, knots * control_count)))
    return comm, pstate, np.array(params, dtype=np.float64)


def rank_sweep(sweep, seed_total, comm):
    """The block of a HamiltonianSweep that this rank's seeds (parallel.shard_bounds) belong to.
    The sweep must have one system per seed of the whole batch."""
    from qoc_amd import parallel
    if seed_total != sweep.seed_count:
        raise ValueError("a HamiltonianSweep of {} seeds needs initial_controls for exactly that "
                         "many seeds, got {}".format(sweep.seed_count, seed_total))
    comm = comm if comm is not None else parallel.SingleComm()
    lo, hi = parallel.shard_bounds(seed_total, comm.rank, comm.world)
    if hi == lo:  # (a rank without seeds sets up a problem that it never evaluates)
        return sweep.slice(0, 1)
    return sweep.slice(lo, hi)


def sweep_sensitivities(evaluator, result):
    """result.sweep_sensitivities: the sweep's sensitivities at every seed's best controls, from one
    evaluation with gradients of all seeds after the loop (a seed without best controls is
    evaluated at zero controls and its rows are NaN)."""
    B = len(result.best_controls)
    if B == 0:
        return
    have = np.array([c is not None for c in result.best_controls])
    if not have.any():
        return
    template = result.best_controls[int(np.nonzero(have)[0][0])]
    controls = np.stack([c if c is not None else np.zeros_like(template)
                         for c in result.best_controls])
    # (a duration search: at every seed's best duration too; a seed without one keeps its start)
    best_tau = getattr(result, "_best_tau", None)
    if best_tau is not None:
        evaluator.set_durations(np.where(have, best_tau, evaluator.durations()))
    # (the Lindblad path: rate sensitivities are asked for in this one evaluation only)
    want_rates = getattr(evaluator, "want_rate_sensitivities", None)
    if want_rates is not None:
        want_rates(True)
    try:
        evaluator.evaluate_batch(controls, want_grad=True)
        out = evaluator.sweep_sensitivities()
    finally:
        if want_rates is not None:
            want_rates(False)
    for value in out.values():
        if value is not None:
            value[~have] = np.nan
    result.sweep_sensitivities = out


def resident_route(stepper, optimizer, pstate, evaluator, batch):
    """The device-resident loop applies: built-in Adam / SGD without scale_grads or LBFGS, no control
    conditions, and an evaluator that can keep everything on the device (structured Hamiltonian,
    device costs and built-in costs of the controls; real or complex controls). LBFGS also needs
    the backend's L-BFGS calls: a stand-in backend without them takes the host loop."""
    if type(optimizer) is LBFGS and not (hasattr(evaluator, "resident_lbfgs_capable")
                                         and evaluator.resident_lbfgs_capable()):
        return False
    # (a duration search: the two-loop recursion needs tau inside the resident vector, which is
    # not laid out that way - LBFGS takes the host loop, where tau is the vector's last entry)
    if type(optimizer) is LBFGS and getattr(pstate, "duration_search", None) is not None:
        return False
    # (a ControlBasis needs the backend's basis calls in the same way)
    if getattr(pstate, "control_basis", None) is not None and not (
            hasattr(evaluator, "resident_basis_capable") and evaluator.resident_basis_capable()):
        return False
    return (batch > 0 and stepper is not None and pstate.impose_control_conditions is None
            and not getattr(optimizer, "apply_scale_grads", False)
            and hasattr(evaluator, "resident_capable") and evaluator.resident_capable())


def _log_header(log_iteration_step, comm):
    if log_iteration_step != 0 and comm.rank == 0:
        print("iter   |  summed error  |   min error    |  active seeds \n"
              "===========================================================")


def _finish(result, comm):
    best_local = float(np.min(result.best_error)) if len(result.best_error) else np.inf
    result.global_best_error = float(-comm.allreduce_max(np.array([-best_local]))[0])
    return result


class ResidentOps(object):
    """One path's resident driver of the engine as run_batch_resident calls it: the engine's bound
    methods of `path` under the loop's names upload_controls, opt_begin (the complex one for
    complex controls), opt_clip, eval_resident, download_costs, opt_step, opt_download_best, and
    for LBFGS opt_lbfgs_begin, opt_lbfgs_step (None on a backend without them). PATH_SCHROEDINGER
    has them under these names, PATH_LINDBLAD behind `lindblad_`.
    control_costs: the descriptors of the costs of the controls alone, which the engine then adds
    to every resident evaluation of `path` until finish(); complex_controls: the loop's complex
    arrays travel as two real channels per control and the engine clips a copy of the parameters.
    The Schroedinger path's final states come back as columns ([B, S, n, 1])."""

    def __init__(self, engine, path, control_costs=(), complex_controls=False):
        self.engine = engine
        self.path = path
        self.control_costs = list(control_costs)
        self.complex_controls = complex_controls
        lindblad = path == PATH_LINDBLAD
        self.column_states = not lindblad
        prefix = "lindblad_" if lindblad else ""
        self._upload_controls = getattr(engine, prefix + "upload_controls")
        self._opt_download_best = getattr(engine, prefix + "opt_download_best")
        self.opt_begin = getattr(engine, prefix + ("opt_begin_complex" if complex_controls
                                                   else "opt_begin"))
        self.eval_resident = engine.eval_lindblad_resident if lindblad else engine.eval_resident
        for name in ("opt_clip", "download_costs", "opt_step"):
            setattr(self, name, getattr(engine, prefix + name))
        for name in ("opt_lbfgs_begin", "opt_lbfgs_step"):
            setattr(self, name, getattr(engine, prefix + name, None))
        # a ControlBasis (None on a backend without the calls)
        self._opt_begin_basis = getattr(engine, prefix + "opt_begin_basis", None)
        self._opt_download_best_params = getattr(engine, prefix + "opt_download_best_params", None)
        # a duration search (None on a backend, or a path, without the call)
        self.opt_download_best_durations = getattr(engine, prefix + "opt_download_best_durations",
                                                   None)

    def upload_controls(self, controls):
        if self.control_costs:
            self.engine.set_control_costs(self.path, self.complex_controls, self.control_costs)
        self._upload_controls(structure.to_real_controls(controls, self.complex_controls))

    def opt_download_best(self):
        controls, finals = self._opt_download_best()
        return (structure.from_real_gradients(controls, self.complex_controls),
                finals[..., None] if self.column_states else finals)

    def opt_begin_basis(self, basis, coefficients):
        """Instead of opt_begin, after upload_controls of the expanded start pulses: the driver's
        parameters are `coefficients` (B x P x control_count, complex for complex controls)."""
        self._opt_begin_basis(self.complex_controls, basis.matrix,
                              structure.to_real_controls(coefficients, self.complex_controls))

    def opt_download_best_params(self):
        """The coefficients (B x P x control_count) behind the best controls."""
        return structure.from_real_gradients(self._opt_download_best_params(),
                                             self.complex_controls)

    def finish(self):
        if self.control_costs:  # evaluate_batch and the single-seed entry points keep them on the host
            self.engine.set_control_costs(self.path, self.complex_controls, [])


def run_batch_resident(ops, optimizer, params, pstate, iteration_count, log_iteration_step,
                       min_error, comm, result):
    """The loop with everything but the decisions on the device: ops.opt_clip -> ops.eval_resident
    -> B costs to the host -> ops.opt_step. `ops` is the engine's resident driver of one problem
    (upload_controls, opt_begin, opt_clip, eval_resident, download_costs, opt_step,
    opt_download_best -> (controls [B, Nc, K], finals in the result's shape); with a ControlBasis
    opt_begin_basis in the place of opt_begin and opt_download_best_params); controls go in and
    come back in the cost-function format (complex arrays for complex controls: ops holds them as
    two real channels each and keeps the optimizer's parameters unclipped, as _cost_format_batch
    does on the host). ops.finish(), if there is one, runs when the loop ends, however it ends.
    A duration search (pstate.duration_search, its evaluator): tau_b lives on the device beside the
    controls - ops.opt_clip clips it and rewrites the tables, ops.opt_step steps it - and the loop
    itself does nothing more per iteration; the device adds the price of time while it runs."""
    search = getattr(pstate, "duration_search", None)
    try:
        if search is not None:
            search.time_term_resident(True)
        return _run_batch_resident(ops, optimizer, params, pstate, iteration_count,
                                   log_iteration_step, min_error, comm, result)
    finally:
        getattr(ops, "finish", lambda: None)()
        if search is not None:
            search.time_term_resident(False)


def _run_batch_resident(ops, optimizer, params, pstate, iteration_count, log_iteration_step,
                        min_error, comm, result):
    B = params.shape[0]
    is_adam = type(optimizer) is Adam
    is_lbfgs = type(optimizer) is LBFGS
    _log_header(log_iteration_step, comm)
    shape = (B,) + tuple(pstate.controls_shape)
    basis = getattr(pstate, "control_basis", None)
    if basis is not None:
        # the start pulses expanded here; from opt_begin_basis on the coefficients are the driver's
        # parameters and every opt_clip expands them again on the device
        coefficients = _coefficients_batch(params, pstate)
        ops.upload_controls(basis.expand(coefficients))
        ops.opt_begin_basis(basis, coefficients)
    elif pstate.complex_controls:
        half = params.shape[1] // 2
        ops.upload_controls((params[:, :half] + 1j * params[:, half:]).reshape(shape))
        ops.opt_begin()
    else:
        ops.upload_controls(params.reshape(shape))
        ops.opt_begin()
    if is_lbfgs:
        ops.opt_lbfgs_begin(optimizer.history)
    active = np.ones(B, dtype=bool)
    count = 0  # optimizer steps taken so far (every active seed has taken all of them)
    should_log = log_iteration_step != 0
    for iteration in range(iteration_count):
        ops.opt_clip(pstate.max_control_norms)
        ops.eval_resident(True)
        errors = ops.download_costs()
        result.iterations_run[active] = iteration + 1
        improved = active & (errors < result.best_error)  # strict, as the reference
        result.best_error[improved] = errors[improved]
        result.best_iteration[improved] = iteration
        if should_log and (iteration % log_iteration_step == 0 or iteration == iteration_count - 1):
            total = comm.allreduce_sum(np.array([float(np.sum(errors[active]))]))[0]
            low = -comm.allreduce_max(np.array([-float(np.min(errors))]))[0]
            seeds = comm.allreduce_sum(np.array([float(np.sum(active))]))[0]
            if comm.rank == 0:
                print("{:^6d} | {:^1.8e} | {:^1.8e} | {:^6d}".format(iteration, total, low,
                                                                     int(seeds)))
        active &= ~(errors <= min_error)
        if is_lbfgs:
            o = optimizer
            finished = ops.opt_lbfgs_step(improved, active, o.first_step, o.armijo, o.shrink,
                                          o.max_backtracks)
            active &= ~finished  # (a finished seed is back at its accepted point and stays there)
        elif is_adam:
            o = optimizer
            if o.apply_learning_rate_decay:
                learning_rate = (o.initial_learning_rate
                                 * np.exp(-np.divide(count, o.learning_rate_decay)))
            else:
                learning_rate = o.initial_learning_rate
            step = count + 1
            ops.opt_step(1, improved, active, learning_rate, o.beta_1, o.beta_2, o.epsilon,
                         1 - np.power(o.beta_1, step), 1 - np.power(o.beta_2, step),
                         o.clip_grads if o.apply_clip_grads else None)
        else:
            ops.opt_step(0, improved, active, optimizer.learning_rate)
        count += 1
        still = comm.allreduce_sum(np.array([float(np.sum(active))]))[0]
        if still == 0:
            break
    best_controls, best_finals = ops.opt_download_best()
    best_coefficients = ops.opt_download_best_params() if basis is not None else None
    search = getattr(pstate, "duration_search", None)
    if search is not None:
        _keep_best_durations(result, search, ops.opt_download_best_durations())
    finals = getattr(result, result.final_field)
    for b in range(B):
        if result.best_iteration[b] >= 0:
            result.best_controls[b] = best_controls[b]
            finals[b] = best_finals[b]
            if basis is not None:
                result.best_coefficients[b] = np.array(best_coefficients[b])
    return _finish(result, comm)


def _keep_best_durations(result, evaluator, best_tau):
    """result.best_evolution_times (and the tau behind them) of a duration search."""
    have = result.best_iteration >= 0
    result._best_tau = np.where(have, best_tau, np.nan)
    result.best_evolution_times = result._best_tau * evaluator.sweep.reference_time


def run_batch_host(evaluator, stepper, optimizer, params, pstate, iteration_count,
                   log_iteration_step, min_error, comm, result):
    """The loop on the host: evaluator.evaluate_batch once per iteration, the [B, P] stepper of the
    built-in optimizers or one deep copy of any other step-wise plugin per seed.
    A duration search (pstate.duration_search, its evaluator): tau_b is the LAST entry of seed b's
    flat parameter vector - after the coefficients of a basis, after [Re..., Im...] of complex
    controls -, clipped in place to its box before every evaluation and stepped by the optimizer
    with the gradient the engine returns for it."""
    B = params.shape[0]
    shape = tuple(pstate.controls_shape)
    search = getattr(pstate, "duration_search", None) if B > 0 else None
    if search is not None:
        params = np.ascontiguousarray(np.hstack([params, search.durations()[:, None]]))
        tau_lo, tau_hi = search.sweep.tau_bounds
        best_tau = np.zeros(B)
        if stepper is not None:  # (its state is shaped like the parameters)
            stepper = batched_stepper(optimizer, params)
    own = params if search is None else params[:, :-1]  # the controls' own parameters (a view)
    optimizers = None if stepper is not None else [_optimizer_clone(optimizer, p) for p in params]
    needs_error = bool(getattr(stepper if stepper is not None else optimizer, "needs_error", False))
    _log_header(log_iteration_step, comm)
    active = np.ones(B, dtype=bool)
    best_controls = best_finals = None
    basis = getattr(pstate, "control_basis", None)
    best_params = np.zeros_like(own) if basis is not None else None
    should_log = log_iteration_step != 0
    for iteration in range(iteration_count):
        # cost-function format of every seed (clipping acts in place on the optimizer's params
        # for real controls, exactly as in the single-seed driver)
        if search is not None:
            tau = params[:, -1]
            np.minimum(np.maximum(tau, tau_lo, out=tau), tau_hi, out=tau)
            search.set_durations(tau)
        controls = _cost_format_batch(own, pstate)
        if B > 0:
            errors, grads, finals, _ = evaluator.evaluate_batch(controls, want_grad=True)
        else:
            errors, grads, finals = np.zeros(0), np.zeros((0,) + shape), np.zeros(0)
        errors = np.asarray(errors)
        result.iterations_run[active] = iteration + 1
        improved = active & (errors < result.best_error)  # strict, as the reference
        if improved.any():
            if best_controls is None:
                best_controls = np.zeros_like(controls)
                best_finals = np.zeros_like(finals)
            best_controls[improved] = controls[improved]
            best_finals[improved] = finals[improved]
            if basis is not None:
                best_params[improved] = own[improved]
            if search is not None:
                best_tau[improved] = params[improved, -1]
            result.best_error[improved] = errors[improved]
            result.best_iteration[improved] = iteration
        if should_log and (iteration % log_iteration_step == 0 or iteration == iteration_count - 1):
            local = np.array([float(np.sum(errors[active])) if B else 0.0])
            total = comm.allreduce_sum(local)[0]
            low = -comm.allreduce_max(np.array([-float(np.min(errors)) if B else -np.inf]))[0]
            count = comm.allreduce_sum(np.array([float(np.sum(active))]))[0]
            if comm.rank == 0:
                print("{:^6d} | {:^1.8e} | {:^1.8e} | {:^6d}".format(iteration, total, low,
                                                                     int(count)))
        # a seed at error <= min_error ends its optimizer loop (terminate = True): frozen from here
        active &= ~(errors <= min_error)
        rows = np.nonzero(active)[0]
        if len(rows):
            grads = np.asarray(grads)
            if basis is not None:  # d error / d coefficients (the derivative of the clip is ignored)
                grads = basis.project(grads)
            flat_grads = _strip_batch(pstate.complex_controls, grads)
            if search is not None:
                flat_grads = np.ascontiguousarray(
                    np.hstack([flat_grads, search.duration_gradients()[:, None]]))
            if stepper is not None and needs_error:
                stepper.update(flat_grads, params, rows, errors)
                active &= ~stepper.finished
            elif stepper is not None:
                stepper.update(flat_grads, params, rows)
            else:
                for b in rows:
                    if needs_error:
                        params[b] = optimizers[b].update(flat_grads[b], params[b], errors[b])
                        active[b] = not getattr(optimizers[b], "finished", False)
                    else:
                        params[b] = optimizers[b].update(flat_grads[b], params[b])
        still = comm.allreduce_sum(np.array([float(np.sum(active))]))[0]
        if still == 0:
            break
    if search is not None:
        _keep_best_durations(result, search, best_tau)
    finals = getattr(result, result.final_field)
    for b in range(B):
        if result.best_iteration[b] >= 0:
            result.best_controls[b] = best_controls[b]
            finals[b] = best_finals[b]
            if basis is not None:
                result.best_coefficients[b] = np.array(slap_controls(
                    pstate.complex_controls, best_params[b], pstate.coefficients_shape))
    return _finish(result, comm)
