"""
engine.py - thin ctypes binding of libqocx.so (include/qocx.h): NumPy in, NumPy out.

This is the only way the package reaches the hot path, and there is no CPU fallback: if the
HIP library is missing or no MI355X is visible, construction fails loudly.
"""

import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIBRARY_PATH = os.path.join(_HERE, "libqocx.so")
# the measurement build (make -C qoc_amd/csrc diag): loaded by the scripts under tools/ only
DIAG_LIBRARY_PATH = os.path.join(_HERE, "libqocx_diag.so")

COST_TARGET_COHERENT = 0
COST_TARGET_INCOHERENT = 1
COST_FORBID = 2
COST_TARGET_DENSITY = 3
COST_FORBID_DENSITY = 4

MAGNUS_CODES = {"M2": 2, "M4": 4, "M6": 6}
# QOCX_INTERP_* of include/qocx.h, by InterpolationPolicy.short
INTERPOLATION_CODES = {"linear": 1, "piecewise_constant": 2}

PATH_SCHROEDINGER = 0
PATH_LINDBLAD = 1
CONTROL_NORM = 0
CONTROL_VARIATION = 1
CONTROL_AREA = 2
CONTROL_BANDWIDTH_MAX = 3

ERR_STATE = -3
ERR_SINGULAR = -4

KERNEL_NAMES = ("pade_pq", "sweep", "krylov_grad", "scatter", "lu", "lindblad", "lindblad_combine")

_c_double_p = ctypes.POINTER(ctypes.c_double)
_c_int_p = ctypes.POINTER(ctypes.c_int32)


def host_clip_controls(controls, max_norms):
    """clip_control_norms (qoc/core/common.py:8-30) on a C-contiguous float64 (B x Nc x K) array,
    IN PLACE, on host threads (qocx_host_clip_controls; no GPU involved)."""
    lib = load_library()
    max_norms = np.ascontiguousarray(max_norms, dtype=np.float64)
    rc = lib.qocx_host_clip_controls(controls.ctypes.data_as(_c_double_p), controls.shape[0],
                                     controls.shape[1], controls.shape[2],
                                     max_norms.ctypes.data_as(_c_double_p))
    if rc != 0:
        raise QocxError(rc, "qocx_host_clip_controls")


def host_optimizer_update(kind, params, grads, moment, square_moment, rows, learning_rate,
                          beta_1=0.0, beta_2=0.0, epsilon=0.0, corr_1=1.0, corr_2=1.0,
                          clip_grads=None):
    """Adam (kind 1) / SGD (kind 0) update of the rows `rows` of C-contiguous float64 [B][P]
    arrays, in place, in the reference's operation order (qocx_host_optimizer_update)."""
    lib = load_library()
    rows = np.ascontiguousarray(rows, dtype=np.int64)
    none = ctypes.cast(None, _c_double_p)
    rc = lib.qocx_host_optimizer_update(
        kind, params.ctypes.data_as(_c_double_p), grads.ctypes.data_as(_c_double_p),
        moment.ctypes.data_as(_c_double_p) if moment is not None else none,
        square_moment.ctypes.data_as(_c_double_p) if square_moment is not None else none,
        params.shape[1], rows.ctypes.data_as(ctypes.POINTER(_I64)), len(rows),
        float(learning_rate), float(beta_1), float(beta_2), float(epsilon), float(corr_1),
        float(corr_2), 0 if clip_grads is None else 1, 0.0 if clip_grads is None else float(clip_grads))
    if rc != 0:
        raise QocxError(rc, "qocx_host_optimizer_update")


class QocxError(RuntimeError):
    def __init__(self, code, message):
        super().__init__("libqocx error {}: {}".format(code, message))
        self.code = code
        self.message = message


class _CostDesc(ctypes.Structure):
    _fields_ = [("kind", ctypes.c_int32), ("step_cost", ctypes.c_int32),
                ("scale", ctypes.c_double), ("vectors", _c_double_p), ("counts", _c_int_p)]


class _ControlCostDesc(ctypes.Structure):
    _fields_ = [("kind", ctypes.c_int32), ("order", ctypes.c_int32),
                ("multiplier", ctypes.c_double), ("max_norms", _c_double_p),
                ("weights", _c_double_p), ("bins", _c_int_p), ("bin_ptr", _c_int_p)]


class _SchroedingerProblem(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_int32),
                ("hilbert_size", ctypes.c_int32), ("state_count", ctypes.c_int32),
                ("control_count", ctypes.c_int32), ("control_eval_count", ctypes.c_int32),
                ("system_eval_count", ctypes.c_int32), ("cost_eval_step", ctypes.c_int32),
                ("magnus_policy", ctypes.c_int32), ("nt", ctypes.c_int32),
                ("evolution_time", ctypes.c_double), ("h0", _c_double_p), ("g", _c_double_p),
                ("initial_states", _c_double_p), ("cost_count", ctypes.c_int32),
                ("costs", ctypes.POINTER(_CostDesc))]


class _LindbladProblem(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_int32),
                ("hilbert_size", ctypes.c_int32), ("density_count", ctypes.c_int32),
                ("control_count", ctypes.c_int32), ("control_eval_count", ctypes.c_int32),
                ("system_eval_count", ctypes.c_int32), ("cost_eval_step", ctypes.c_int32),
                ("operator_count", ctypes.c_int32), ("evolution_time", ctypes.c_double),
                ("h0", _c_double_p), ("g", _c_double_p), ("dissipators", _c_double_p),
                ("operators", _c_double_p), ("initial_densities", _c_double_p),
                ("cost_count", ctypes.c_int32), ("costs", ctypes.POINTER(_CostDesc)),
                ("fixed_subdivision", ctypes.c_int32), ("h0_stages", _c_double_p),
                ("g_stages", _c_double_p), ("diss_stages", _c_double_p),
                ("op_stages", _c_double_p)]


class ActionFacts(ctypes.Structure):
    """qocx_action_facts of include/qocx.h: what qocx_debug_action_route decides on."""
    _fields_ = ([(name, ctypes.c_int32) for name in (
        "n", "S", "K", "nt", "nodes", "eff_kind", "Ke", "hermitian", "unit_ok", "has_step_costs",
        "cost_count", "inj_count", "keep_step_states", "explicit_gen", "dense", "one_wave_k1a",
        "latency", "have_norms", "have_eff_norms", "have_e_img")]
                + [(name, ctypes.c_double) for name in ("bound1", "bound1_mid", "bound2", "bound2_mid")]
                + [(name, ctypes.c_int32) for name in (
                    "action", "action_states", "action_costs", "action_small", "action_eff",
                    "action_eff_exact", "action_degree", "action_plan", "pade_order", "unit_adjoint",
                    "allow")])


class LindbladFacts(ctypes.Structure):
    """qocx_lindblad_facts of include/qocx.h: what qocx_debug_lindblad_route decides on."""
    _fields_ = [(name, ctypes.c_int32) for name in (
        "n", "S", "K", "nops", "stage_tables", "g_tables", "op_tables", "hermitian", "ops_real", "unit_ok",
        "inj_count", "want_grad", "rates", "sweep", "want_rate_sens", "side_streams", "cu_count",
        "dbg_wave_mode", "lindblad_4t", "lindblad_two_sided", "lindblad_hermitian", "lindblad_q2",
        "lindblad_chain", "lindblad_real_ops", "lindblad_pad_operator", "lindblad_side_limit",
        "lindblad_stamps", "single_wave")]


# name -> (restype, argtypes); every symbol declared in include/qocx.h
_VP = ctypes.c_void_p
_I32 = ctypes.c_int32
_I64 = ctypes.c_int64
_U8P = ctypes.POINTER(ctypes.c_uint8)
SIGNATURES = {
    "qocx_last_error": (ctypes.c_char_p, []),
    "qocx_version": (ctypes.c_int, []),
    "qocx_device_count": (ctypes.c_int, [ctypes.POINTER(ctypes.c_int)]),
    "qocx_create": (ctypes.c_int, [ctypes.c_int, ctypes.POINTER(_VP)]),
    "qocx_destroy": (ctypes.c_int, [_VP]),
    "qocx_synchronize": (ctypes.c_int, [_VP]),
    "qocx_set_schroedinger_problem": (ctypes.c_int, [_VP, ctypes.POINTER(_SchroedingerProblem)]),
    "qocx_set_interpolation_policy": (ctypes.c_int, [_VP, _I32]),
    "qocx_eval_schroedinger": (ctypes.c_int, [_VP, _I32, _c_double_p, _I32, _c_double_p,
                                              _c_double_p, _c_double_p]),
    "qocx_upload_controls": (ctypes.c_int, [_VP, _I32, _c_double_p]),
    "qocx_eval_resident": (ctypes.c_int, [_VP, _I32]),
    "qocx_download_results": (ctypes.c_int, [_VP, _c_double_p, _c_double_p, _c_double_p]),
    "qocx_upload_generators": (ctypes.c_int, [_VP, _I32, _c_double_p]),
    "qocx_download_generator_cotangents": (ctypes.c_int, [_VP, _c_double_p]),
    "qocx_set_quadratic_terms": (ctypes.c_int, [_VP, _I32, _c_int_p, _c_double_p]),
    "qocx_set_ensemble": (ctypes.c_int, [_VP, _I32, _I32, _c_double_p, _c_double_p, _c_double_p]),
    "qocx_ensemble_download_members": (ctypes.c_int, [_VP, _c_double_p]),
    "qocx_set_ensemble_quadratic_scales": (ctypes.c_int, [_VP, _I32, _I32, _c_double_p]),
    "qocx_set_sweep": (ctypes.c_int, [_VP, _I32, _I32, _c_double_p, _c_double_p]),
    "qocx_sweep_download_sensitivities": (ctypes.c_int, [_VP, _c_double_p, _c_double_p]),
    "qocx_sweep_set_durations": (ctypes.c_int, [_VP, _c_double_p, _c_double_p, _c_double_p,
                                                ctypes.c_double, ctypes.c_double, ctypes.c_double]),
    "qocx_sweep_download_durations": (ctypes.c_int, [_VP, _c_double_p, _c_double_p]),
    "qocx_opt_download_best_durations": (ctypes.c_int, [_VP, _c_double_p]),
    "qocx_set_keep_step_states": (ctypes.c_int, [_VP, _I32]),
    "qocx_download_step_states": (ctypes.c_int, [_VP, _c_double_p]),
    "qocx_set_lindblad_problem": (ctypes.c_int, [_VP, ctypes.POINTER(_LindbladProblem)]),
    "qocx_lindblad_stage_times": (ctypes.c_int, [ctypes.c_double, _I32, _I32, _I32, _I32,
                                                 _c_double_p, _I64, ctypes.POINTER(_I64)]),
    "qocx_eval_lindblad": (ctypes.c_int, [_VP, _I32, _c_double_p, _I32, _c_double_p,
                                          _c_double_p, _c_double_p]),
    "qocx_download_step_densities": (ctypes.c_int, [_VP, _c_double_p]),
    "qocx_lindblad_last_subintervals": (ctypes.c_int, [_VP, ctypes.POINTER(_I64)]),
    "qocx_set_density_cotangents": (ctypes.c_int, [_VP, _I32, _I32, _c_int_p, _c_double_p]),
    "qocx_set_state_cotangents": (ctypes.c_int, [_VP, _I32, _I32, _c_int_p, _c_double_p]),
    "qocx_lindblad_set_ensemble": (ctypes.c_int, [_VP, _I32, _I32, _c_double_p, _c_double_p,
                                                  _c_double_p]),
    "qocx_lindblad_ensemble_download_members": (ctypes.c_int, [_VP, _c_double_p]),
    "qocx_lindblad_set_ensemble_rates": (ctypes.c_int, [_VP, _I32, _I32, _c_double_p]),
    "qocx_lindblad_set_sweep": (ctypes.c_int, [_VP, _I32, _I32, _c_double_p, _c_double_p,
                                               _c_double_p]),
    "qocx_lindblad_sweep_want_rate_sensitivities": (ctypes.c_int, [_VP, _I32]),
    "qocx_lindblad_sweep_download_sensitivities": (ctypes.c_int, [_VP, _c_double_p, _c_double_p,
                                                                  _c_double_p]),
    "qocx_lindblad_sweep_set_durations": (ctypes.c_int, [_VP, _c_double_p, _c_double_p, _c_double_p,
                                                         _c_double_p, ctypes.c_double,
                                                         ctypes.c_double, ctypes.c_double]),
    "qocx_lindblad_sweep_download_durations": (ctypes.c_int, [_VP, _c_double_p, _c_double_p]),
    "qocx_lindblad_opt_download_best_durations": (ctypes.c_int, [_VP, _c_double_p]),
    "qocx_set_timing":(ctypes.c_int, [_VP, _I32]),
    "qocx_get_timing": (ctypes.c_int, [_VP, _I32, ctypes.POINTER(_I64), _c_double_p]),
    "qocx_reset_timing": (ctypes.c_int, [_VP]),
    "qocx_set_chunk": (ctypes.c_int, [_VP, _I32]),
    "qocx_set_pipeline": (ctypes.c_int, [_VP, _I32]),
    "qocx_comm_unique_id": (ctypes.c_int, [_U8P]),
    "qocx_comm_init": (ctypes.c_int, [_VP, _U8P, _I32, _I32]),
    "qocx_reduce_results": (ctypes.c_int, [_VP, _I32, _c_double_p, _I64]),
    "qocx_comm_allreduce_sum": (ctypes.c_int, [_VP, _c_double_p, _I64]),
    "qocx_comm_allreduce_max": (ctypes.c_int, [_VP, _c_double_p, _I64]),
    "qocx_comm_barrier": (ctypes.c_int, [_VP]),
    "qocx_comm_destroy": (ctypes.c_int, [_VP]),
    "qocx_debug_pade_factor": (ctypes.c_int, [_VP, _I32, _I32, _c_double_p, _c_double_p,
                                              _c_double_p, _c_int_p, _c_double_p, _c_int_p]),
    "qocx_debug_selftest": (ctypes.c_int, [_VP, _c_int_p, ctypes.c_char_p, _I32]),
    "qocx_debug_lindblad_knobs": (ctypes.c_int, [_VP, _I64, _I32, _I32]),
    "qocx_debug_set_knob": (ctypes.c_int, [_VP, ctypes.c_char_p, _I64]),
    "qocx_knob_kind": (ctypes.c_int, [ctypes.c_char_p]),
    "qocx_build_is_diag": (ctypes.c_int, []),
    "qocx_debug_read_stamps": (ctypes.c_int, [_VP, ctypes.POINTER(ctypes.c_uint64), _I64]),
    "qocx_debug_timeline": (ctypes.c_int, [_VP, _c_double_p, _I64, ctypes.POINTER(_I64)]),
    "qocx_pade_orders": (ctypes.c_int, [_VP, ctypes.POINTER(_I64)]),
    "qocx_lu_fallbacks": (ctypes.c_int, [_VP, ctypes.POINTER(_I64)]),
    "qocx_action_degrees": (ctypes.c_int, [_VP, ctypes.POINTER(_I64)]),
    "qocx_action_reruns": (ctypes.c_int, [_VP, ctypes.POINTER(_I64)]),
    "qocx_debug_spectral_bound": (ctypes.c_int, [_c_double_p, _I32, _c_double_p]),
    "qocx_debug_action_degree": (ctypes.c_int, [ctypes.c_double, ctypes.c_double, _I32, _c_int_p]),
    "qocx_debug_action_route": (ctypes.c_int, [ctypes.POINTER(ActionFacts), _c_int_p, _c_int_p, _c_int_p]),
    "qocx_debug_lindblad_route": (ctypes.c_int, [ctypes.POINTER(LindbladFacts), _c_int_p, _c_int_p, _c_int_p,
                                                 _c_int_p, _c_int_p]),
    "qocx_debug_lindblad_pieces": (ctypes.c_int, [_I32, _I32, _I64, _I64, _I32, _I32, _I32, _I32, _I64, _I32,
                                                  _c_int_p, _c_int_p, _c_int_p, _c_int_p,
                                                  ctypes.POINTER(_I64)]),
    "qocx_debug_mfma_peak": (ctypes.c_int, [_VP, _I32, _I32, _c_double_p]),
    "qocx_opt_begin": (ctypes.c_int, [_VP]),
    "qocx_opt_clip": (ctypes.c_int, [_VP, _c_double_p]),
    "qocx_download_costs": (ctypes.c_int, [_VP, _c_double_p]),
    "qocx_opt_step": (ctypes.c_int, [
        _VP, _I32, ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint8), ctypes.c_double,
        ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_double, _I32,
        ctypes.c_double]),
    "qocx_opt_download_best": (ctypes.c_int, [_VP, _c_double_p, _c_double_p]),
    "qocx_lindblad_upload_controls": (ctypes.c_int, [_VP, _I32, _c_double_p]),
    "qocx_eval_lindblad_resident": (ctypes.c_int, [_VP, _I32]),
    "qocx_lindblad_download_results": (ctypes.c_int, [_VP, _c_double_p, _c_double_p, _c_double_p]),
    "qocx_lindblad_download_costs": (ctypes.c_int, [_VP, _c_double_p]),
    "qocx_lindblad_opt_begin": (ctypes.c_int, [_VP]),
    "qocx_lindblad_opt_clip": (ctypes.c_int, [_VP, _c_double_p]),
    "qocx_lindblad_opt_step": (ctypes.c_int, [
        _VP, _I32, ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint8), ctypes.c_double,
        ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_double, _I32,
        ctypes.c_double]),
    "qocx_lindblad_opt_download_best": (ctypes.c_int, [_VP, _c_double_p, _c_double_p]),
    "qocx_set_control_costs": (ctypes.c_int, [_VP, _I32, _I32, _I32,
                                              ctypes.POINTER(_ControlCostDesc)]),
    "qocx_eval_control_costs": (ctypes.c_int, [_VP, _I32, _I32, _c_double_p, _c_double_p,
                                               _c_double_p]),
    "qocx_opt_begin_complex": (ctypes.c_int, [_VP]),
    "qocx_lindblad_opt_begin_complex": (ctypes.c_int, [_VP]),
    "qocx_opt_lbfgs_begin": (ctypes.c_int, [_VP, _I32]),
    "qocx_opt_lbfgs_step": (ctypes.c_int, [_VP, _U8P, _U8P, ctypes.c_double, ctypes.c_double,
                                           ctypes.c_double, _I32, _U8P]),
    "qocx_lindblad_opt_lbfgs_begin": (ctypes.c_int, [_VP, _I32]),
    "qocx_lindblad_opt_lbfgs_step": (ctypes.c_int, [_VP, _U8P, _U8P, ctypes.c_double,
                                                    ctypes.c_double, ctypes.c_double, _I32, _U8P]),
    "qocx_opt_begin_basis": (ctypes.c_int, [_VP, _I32, _I32, _c_double_p, _c_double_p]),
    "qocx_opt_download_best_params": (ctypes.c_int, [_VP, _c_double_p]),
    "qocx_lindblad_opt_begin_basis": (ctypes.c_int, [_VP, _I32, _I32, _c_double_p, _c_double_p]),
    "qocx_lindblad_opt_download_best_params": (ctypes.c_int, [_VP, _c_double_p]),
    "qocx_control_basis_apply": (ctypes.c_int, [_VP, _I32, _I32, _I32, _I32, _I32, _c_double_p,
                                                _c_double_p, _c_double_p]),
    "qocx_host_clip_controls": (ctypes.c_int, [_c_double_p, _I64, _I64, _I32, _c_double_p]),
    "qocx_host_optimizer_update": (ctypes.c_int, [
        _I32, _c_double_p, _c_double_p, _c_double_p, _c_double_p, _I64, ctypes.POINTER(_I64), _I64,
        ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_double,
        ctypes.c_double, _I32, ctypes.c_double]),
}

_lib = None


def load_library(path=None):
    """Load libqocx.so and bind every declared symbol. Raises if the library is absent."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    path = path or LIBRARY_PATH
    if not os.path.exists(path):
        raise ImportError(
            "qoc_amd: the HIP engine {} is missing. Build it with "
            "`python -c 'import __graft_entry__ as g; g.build()'` (hipcc --offload-arch=gfx950). "
            "There is no CPU fallback.".format(path))
    # Multi-process GPU work on this platform needs dmabuf IPC (RCCL between the ranks of a node
    # fails with hipIpcGetMemHandle: invalid argument otherwise). The HSA runtime reads
    # HSA_ENABLE_IPC_MODE_LEGACY when it initialises - which dlopen of libqocx does not trigger, the
    # first qocx_create does - so it is defaulted here, before any context exists: a value the user
    # (or the launcher, qoc_amd/parallel.py documents it) has set is kept, a process in which
    # another library initialised HSA earlier is not affected, and child processes inherit it.
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    lib = ctypes.CDLL(path)
    for name, (restype, argtypes) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the library lacks a declared symbol
        fn.restype = restype
        fn.argtypes = argtypes
    _lib = lib
    return lib


def _dp(array):
    return array.ctypes.data_as(_c_double_p)


def _as_complex(array, shape=None):
    out = np.ascontiguousarray(array, dtype=np.complex128)
    if shape is not None:
        out = out.reshape(shape)
    return out


class Engine(object):
    """One context on one MI355X."""

    @staticmethod
    def device_count():
        """HIP devices visible to this process (qocx_device_count)."""
        lib = load_library()
        count = ctypes.c_int(0)
        code = lib.qocx_device_count(ctypes.byref(count))
        if code != 0:
            raise QocxError(code, lib.qocx_last_error().decode("utf-8", "replace"))
        return int(count.value)

    def __init__(self, device=-1):
        self._lib = load_library()
        self._ctx = _VP()
        self._check(self._lib.qocx_create(int(device), ctypes.byref(self._ctx)))
        self._problem = None
        self._ensemble = None
        self._sweep = None
        self._lindblad_ensemble = None
        self._lindblad_sweep = None
        self._quadratic_count = 0
        self._keepalive = []
        self.batch = 0
        self._interpolation = INTERPOLATION_CODES["linear"]  # of the context (its default)
        self._basis_P = {}  # path -> coefficients per channel of the resident driver's basis

    # -- plumbing ----------------------------------------------------------------------------
    def _check(self, code):
        if code != 0:
            msg = self._lib.qocx_last_error().decode("utf-8", "replace")
            if code == ERR_SINGULAR:
                raise np.linalg.LinAlgError(msg)
            raise QocxError(code, msg)

    def close(self):
        if getattr(self, "_ctx", None) is not None and self._ctx.value is not None:
            self._lib.qocx_destroy(self._ctx)
            self._ctx = _VP()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def synchronize(self):
        self._check(self._lib.qocx_synchronize(self._ctx))

    # -- problem -------------------------------------------------------------------------------
    def set_interpolation_policy(self, interpolation):
        """How the NEXT problem set on this context reads the controls between their grid points
        (qocx_set_interpolation_policy, sticky): "linear", "piecewise_constant", a
        qoc_amd.models.InterpolationPolicy or one of the QOCX_INTERP_* codes."""
        name = getattr(interpolation, "short", interpolation)
        code = INTERPOLATION_CODES.get(name, name)
        if isinstance(code, str):
            raise ValueError("Unrecognized interpolation {!r}.".format(interpolation))
        # (the call is made only when the context's policy changes: a context that only ever
        # sets linear problems never makes it)
        if int(code) != self._interpolation:
            self._check(self._lib.qocx_set_interpolation_policy(self._ctx, int(code)))
            self._interpolation = int(code)

    def set_schroedinger_problem(self, hilbert_size, state_count, control_count,
                                 control_eval_count, system_eval_count, evolution_time,
                                 h0, g, initial_states, costs=(), cost_eval_step=1,
                                 magnus_policy="M2", interpolation="linear"):
        """
        h0 :: (nt, n, n) complex, g :: (nt, K, n, n) complex, initial_states :: (S, n) complex,
        costs :: iterable of dicts {kind, step_cost, scale, vectors, counts(optional)}.
        interpolation: as set_interpolation_policy; it is set on the context before the problem, so
        a later problem set without the argument is linear again.
        """
        self.set_interpolation_policy(interpolation)
        n, S, K = int(hilbert_size), int(state_count), int(control_count)
        h0 = _as_complex(h0)
        if h0.ndim == 2:
            h0 = h0[None]
        nt = h0.shape[0]
        h0 = _as_complex(h0, (nt, n, n))
        g = _as_complex(g if K > 0 else np.zeros((nt, 0, n, n)), (nt, K, n, n))
        psi = _as_complex(initial_states, (S, n))
        keep = [h0, g, psi]
        descs = (_CostDesc * max(1, len(costs)))()
        for i, c in enumerate(costs):
            vec = _as_complex(c["vectors"])
            vec = vec.reshape(-1, n)
            keep.append(vec)
            descs[i].kind = int(c["kind"])
            descs[i].step_cost = int(bool(c["step_cost"]))
            descs[i].scale = float(c["scale"])
            descs[i].vectors = _dp(vec)
            if c.get("counts") is not None:
                cnt = np.ascontiguousarray(c["counts"], dtype=np.int32)
                keep.append(cnt)
                descs[i].counts = cnt.ctypes.data_as(_c_int_p)
        p = _SchroedingerProblem()
        p.struct_size = ctypes.sizeof(_SchroedingerProblem)
        p.hilbert_size, p.state_count, p.control_count = n, S, K
        p.control_eval_count, p.system_eval_count = int(control_eval_count), int(system_eval_count)
        p.cost_eval_step = int(cost_eval_step)
        p.magnus_policy = MAGNUS_CODES[magnus_policy]
        p.nt = nt
        p.evolution_time = float(evolution_time)
        p.h0, p.g, p.initial_states = _dp(h0), _dp(g), _dp(psi)
        p.cost_count = len(costs)
        p.costs = descs
        self._check(self._lib.qocx_set_schroedinger_problem(self._ctx, ctypes.byref(p)))
        self._problem = dict(n=n, S=S, K=K, Nc=int(control_eval_count), N=int(system_eval_count))
        self._ensemble = None
        self._sweep = None
        self._quadratic_count = 0
        self.batch = 0

    def set_quadratic_terms(self, pairs, matrices):
        """+ sum_q r_k r_l Q_q on the current problem (qocx_set_quadratic_terms): pairs :: (count, 2)
        real-control indices k <= l, matrices :: (count, n, n) complex. An empty `pairs` clears them.
        Controls must be uploaded again afterwards."""
        n = self._problem["n"]
        pairs = np.ascontiguousarray(np.asarray(pairs, dtype=np.int32).reshape(-1, 2))
        count = pairs.shape[0]
        mats = _as_complex(matrices if count else np.zeros((0, n, n)), (count, n, n))
        self._check(self._lib.qocx_set_quadratic_terms(
            self._ctx, count, pairs.ctypes.data_as(_c_int_p), _dp(mats)))
        self._quadratic_count = count
        self.batch = 0

    def set_ensemble(self, scales, offsets, weights):
        """An ensemble of M members on the current problem (qocx_set_ensemble): the problem's last J
        control channels are the perturbation matrices D_j. scales :: (M, K - J) or None (all 1),
        offsets :: (M, J) or None (J = 0), weights :: (M,). From here on the seed-level calls
        (upload_controls, download_results, download_costs, reduce_results, opt_*) take and return
        the seeds' K - J channels, and final states carry a member axis: (B, M, S, n)."""
        weights = np.ascontiguousarray(weights, dtype=np.float64).reshape(-1)
        M = weights.shape[0]
        J = 0 if offsets is None else np.asarray(offsets).size // max(M, 1)
        kr = self._problem["K"] - J
        none = ctypes.cast(None, _c_double_p)
        sc = None if scales is None else np.ascontiguousarray(scales, dtype=np.float64).reshape(M, kr)
        off = None if offsets is None else np.ascontiguousarray(offsets, dtype=np.float64).reshape(M, J)
        self._check(self._lib.qocx_set_ensemble(
            self._ctx, M, J, none if sc is None else _dp(sc), none if off is None else _dp(off),
            _dp(weights)))
        self._ensemble = dict(M=M, J=J, Kr=kr)
        self.batch = 0

    def set_ensemble_quadratic_scales(self, scales):
        """c_mq of an ensemble with quadratic terms (qocx_set_ensemble_quadratic_scales): scales ::
        (M, count) real, member m's factor of term q; None clears them (all 1). Both set_ensemble
        and set_quadratic_terms come first. Controls must be uploaded again afterwards."""
        M = 0 if self._ensemble is None else self._ensemble["M"]
        if scales is None:
            self._check(self._lib.qocx_set_ensemble_quadratic_scales(
                self._ctx, M, self._quadratic_count, ctypes.cast(None, _c_double_p)))
        else:
            sc = np.ascontiguousarray(scales, dtype=np.float64)
            if sc.ndim != 2:
                raise ValueError("scales must be (M, count), got shape {}".format(sc.shape))
            self._check(self._lib.qocx_set_ensemble_quadratic_scales(
                self._ctx, sc.shape[0], sc.shape[1], _dp(sc)))
        self.batch = 0

    def ensemble_member_costs(self):
        """The unweighted cost of every member of every seed of the last evaluation, (B, M)
        (qocx_ensemble_download_members)."""
        out = np.empty((self.batch, self._ensemble["M"]), dtype=np.float64)
        self._check(self._lib.qocx_ensemble_download_members(self._ctx, _dp(out)))
        return out

    def set_sweep(self, scales, offsets):
        """A sweep of B seeds on the current problem (qocx_set_sweep): seed b is a system of its own,
        the problem on the controls [scales[b] * u_b, offsets[b]]; the problem's last J control
        channels are the fixed matrices D_j. scales :: (B, K - J) or None (all 1), offsets :: (B, J)
        or None (J = 0); one of them is needed (B is read from it). From here on the seed-level
        calls take and return the seeds' K - J channels and the batch is exactly B."""
        if scales is None and offsets is None:
            raise ValueError("a sweep needs scales or offsets (the seed count is read from them)")
        none = ctypes.cast(None, _c_double_p)
        off = None if offsets is None else np.ascontiguousarray(offsets, dtype=np.float64)
        if off is not None and off.ndim != 2:
            raise ValueError("offsets must be (B, J), got shape {}".format(off.shape))
        J = 0 if off is None else off.shape[1]
        kr = self._problem["K"] - J
        sc = None if scales is None else np.ascontiguousarray(scales, dtype=np.float64)
        B = off.shape[0] if sc is None else sc.shape[0]
        if sc is not None and sc.shape != (B, kr):
            raise ValueError("scales must be (B, K - J) = ({}, {}), got shape {}".format(B, kr, sc.shape))
        if off is not None and off.shape[0] != B:
            raise ValueError("scales and offsets disagree on the seed count")
        if J == 0:
            off = None
        self._check(self._lib.qocx_set_sweep(
            self._ctx, B, J, none if sc is None else _dp(sc), none if off is None else _dp(off)))
        self._sweep = dict(B=B, J=J, Kr=kr)
        self.batch = 0

    def sweep_sensitivities(self):
        """(dE_b / d scales [B, K - J], dE_b / d offsets [B, J]) of the last evaluation with
        gradients (qocx_sweep_download_sensitivities)."""
        sw = self._sweep
        if sw is None:
            raise ValueError("no sweep set (set_sweep)")
        scales = np.empty((sw["B"], sw["Kr"]), dtype=np.float64)
        offsets = np.empty((sw["B"], sw["J"]), dtype=np.float64)
        self._check(self._lib.qocx_sweep_download_sensitivities(self._ctx, _dp(scales), _dp(offsets)))
        return scales, offsets

    def sweep_set_durations(self, tau, base_scales, base_offsets, tau_min, tau_max,
                            time_weight=0.0):
        """The current sweep as a duration search (qocx_sweep_set_durations): tau :: (B,) the seeds'
        durations in units of the evolution time, clipped to [tau_min, tau_max] on the device;
        base_scales :: (B, K - J) or None (all 1) and base_offsets :: (B, J) the tables before the
        factor tau (the drift column of base_offsets is 1). The engine derives the sweep's tables
        from them; controls must be uploaded again afterwards."""
        sw = self._sweep
        if sw is None:  # (the engine's own refusal: QOCX_ERR_STATE)
            B, kr, J = len(np.atleast_1d(tau)), 0, 0
        else:
            B, kr, J = sw["B"], sw["Kr"], sw["J"]
        tau = np.ascontiguousarray(tau, dtype=np.float64).reshape(-1)
        if tau.shape[0] != B:
            raise ValueError("tau must be (B,) = ({},), got shape {}".format(B, tau.shape))
        none = ctypes.cast(None, _c_double_p)
        s0 = None if base_scales is None else np.ascontiguousarray(base_scales, dtype=np.float64)
        d0 = None if base_offsets is None else np.ascontiguousarray(base_offsets, dtype=np.float64)
        if sw is not None and s0 is not None and s0.shape != (B, kr):
            raise ValueError("base_scales must be (B, K - J) = ({}, {}), got shape {}".format(
                B, kr, s0.shape))
        if sw is not None and d0 is not None and d0.shape != (B, J):
            raise ValueError("base_offsets must be (B, J) = ({}, {}), got shape {}".format(
                B, J, d0.shape))
        self._check(self._lib.qocx_sweep_set_durations(
            self._ctx, _dp(tau), none if s0 is None else _dp(s0), none if d0 is None else _dp(d0),
            float(tau_min), float(tau_max), float(time_weight)))
        self.batch = 0

    def sweep_download_durations(self, want_grad=True):
        """(tau [B], d error_b / d tau_b + time_weight [B] or None) of a duration search
        (qocx_sweep_download_durations); the gradient is that of the last evaluation with
        gradients."""
        B = self._sweep["B"] if self._sweep is not None else 1
        tau = np.empty(B, dtype=np.float64)
        grad = np.empty(B, dtype=np.float64) if want_grad else None
        self._check(self._lib.qocx_sweep_download_durations(
            self._ctx, _dp(tau), _dp(grad) if want_grad else ctypes.cast(None, _c_double_p)))
        return tau, grad

    def opt_download_best_durations(self):
        """tau [B] at every seed's best evaluation of the resident driver
        (qocx_opt_download_best_durations)."""
        B = self._sweep["B"] if self._sweep is not None else 1
        tau = np.empty(B, dtype=np.float64)
        self._check(self._lib.qocx_opt_download_best_durations(self._ctx, _dp(tau)))
        return tau

    def _seed_channels(self):
        """Control channels of a seed: the problem's K, or K - J with an ensemble or a sweep set."""
        if self._sweep is not None:
            return self._sweep["Kr"]
        return self._problem["K"] if self._ensemble is None else self._ensemble["Kr"]

    def _final_shape(self, B, path=PATH_SCHROEDINGER):
        if path == PATH_LINDBLAD:
            pr = self._lindblad
            return (B,) + self._lindblad_members() + (pr["S"], pr["n"], pr["n"])
        pr = self._problem
        members = () if self._ensemble is None else (self._ensemble["M"],)
        return (B,) + members + (pr["S"], pr["n"])

    # -- evaluation ----------------------------------------------------------------------------
    def upload_controls(self, controls):
        pr = self._problem
        if pr["K"] > 0:
            controls = np.ascontiguousarray(controls, dtype=np.float64)
            controls = controls.reshape(-1, pr["Nc"], self._seed_channels())
            batch = controls.shape[0]
            self._check(self._lib.qocx_upload_controls(self._ctx, batch, _dp(controls)))
        else:
            batch = 1 if controls is None else int(controls)
            self._check(self._lib.qocx_upload_controls(self._ctx, batch, None))
        self.batch = batch

    def upload_generators(self, generators):
        """generators :: (B, N-1, n, n) complex step generators M_j = -i dt H (opaque Hamiltonians);
        the problem must have been set with control_count = 0 and magnus_policy M2."""
        pr = self._problem
        gens = _as_complex(generators).reshape(-1, pr["N"] - 1, pr["n"], pr["n"])
        self._check(self._lib.qocx_upload_generators(self._ctx, gens.shape[0], _dp(gens)))
        self.batch = gens.shape[0]

    def download_generator_cotangents(self):
        pr = self._problem
        out = np.empty((self.batch, pr["N"] - 1, pr["n"], pr["n"]), dtype=np.complex128)
        self._check(self._lib.qocx_download_generator_cotangents(self._ctx, _dp(out)))
        return out

    def eval_resident(self, want_grad=True):
        self._check(self._lib.qocx_eval_resident(self._ctx, int(bool(want_grad))))

    def download_results(self, want_grad=True, want_final=True):
        return self._download_results(self._lib.qocx_download_results, PATH_SCHROEDINGER,
                                      want_grad, want_final)

    def evaluate(self, controls, want_grad=True):
        """(cost[B], grads[B,Nc,K] or None, final_states[B,S,n]) for controls[B,Nc,K]."""
        self.upload_controls(controls)
        self.eval_resident(want_grad)
        return self.download_results(want_grad)

    def set_keep_step_states(self, keep):
        self._check(self._lib.qocx_set_keep_step_states(self._ctx, int(bool(keep))))

    def download_step_states(self):
        pr, B = self._problem, self.batch
        members = () if self._ensemble is None else (self._ensemble["M"],)
        out = np.empty((B,) + members + (pr["N"], pr["S"], pr["n"]), dtype=np.complex128)
        self._check(self._lib.qocx_download_step_states(self._ctx, _dp(out)))
        return out

    # -- Lindblad -------------------------------------------------------------------------------
    @staticmethod
    def lindblad_stage_times(evolution_time, system_eval_count, control_eval_count, control_count,
                             subdivision):
        """Times at which a time-dependent Hamiltonian is sampled for `subdivision` pieces per
        system step (no GPU needed)."""
        lib = load_library()
        count = _I64(0)
        args = (float(evolution_time), int(system_eval_count), int(control_eval_count),
                int(control_count), int(subdivision))
        code = lib.qocx_lindblad_stage_times(*args, None, 0, ctypes.byref(count))
        if code:
            raise QocxError(code, lib.qocx_last_error().decode("utf-8", "replace"))
        times = np.empty(count.value, dtype=np.float64)
        code = lib.qocx_lindblad_stage_times(*args, _dp(times), count.value, ctypes.byref(count))
        if code:
            raise QocxError(code, lib.qocx_last_error().decode("utf-8", "replace"))
        return times

    def set_lindblad_problem(self, hilbert_size, density_count, control_count,
                             control_eval_count, system_eval_count, evolution_time,
                             h0, g, dissipators, operators, initial_densities, costs=(),
                             cost_eval_step=1, fixed_subdivision=0, h0_stages=None,
                             g_stages=None, diss_stages=None, op_stages=None,
                             interpolation="linear"):
        """
        h0 :: (n, n), g :: (K, n, n), dissipators :: (L,), operators :: (L, n, n),
        initial_densities :: (S, n, n); costs :: dicts {kind (3|4), step_cost, scale,
        vectors (matrices), counts(optional)}.
        interpolation: as in set_schroedinger_problem. Piecewise constant, the stage tables are
        those of lindblad_stage_times(..., control_eval_count + 1, ...): the slice edges are the
        cut points of one knot more.
        """
        self.set_interpolation_policy(interpolation)
        n, S, K = int(hilbert_size), int(density_count), int(control_count)
        h0 = _as_complex(h0, (n, n))
        g = _as_complex(g if K > 0 else np.zeros((0, n, n)), (K, n, n))
        L = 0 if operators is None else len(operators)
        ops = _as_complex(operators if L > 0 else np.zeros((0, n, n)), (L, n, n))
        gam = np.ascontiguousarray(dissipators if L > 0 else np.zeros(0), dtype=np.float64)
        gam = gam.reshape(L)
        rho = _as_complex(initial_densities, (S, n, n))
        keep = [h0, g, ops, gam, rho]
        descs = (_CostDesc * max(1, len(costs)))()
        for i, c in enumerate(costs):
            mats = _as_complex(c["vectors"]).reshape(-1, n, n)
            keep.append(mats)
            descs[i].kind = int(c["kind"])
            descs[i].step_cost = int(bool(c["step_cost"]))
            descs[i].scale = float(c["scale"])
            descs[i].vectors = _dp(mats)
            if c.get("counts") is not None:
                cnt = np.ascontiguousarray(c["counts"], dtype=np.int32)
                keep.append(cnt)
                descs[i].counts = cnt.ctypes.data_as(_c_int_p)
        p = _LindbladProblem()
        p.struct_size = ctypes.sizeof(_LindbladProblem)
        p.hilbert_size, p.density_count, p.control_count = n, S, K
        p.control_eval_count, p.system_eval_count = int(control_eval_count), int(system_eval_count)
        p.cost_eval_step = int(cost_eval_step)
        p.operator_count = L
        p.evolution_time = float(evolution_time)
        p.h0, p.g, p.initial_densities = _dp(h0), _dp(g), _dp(rho)
        p.dissipators, p.operators = _dp(gam), _dp(ops)
        p.cost_count = len(costs)
        p.costs = descs
        p.fixed_subdivision = int(fixed_subdivision)
        if fixed_subdivision:
            hs = _as_complex(h0_stages).reshape(-1, n, n)
            keep.append(hs)
            p.h0_stages = _dp(hs)
            if g_stages is not None and K > 0:
                gs = _as_complex(g_stages).reshape(-1, K, n, n)
                keep.append(gs)
                p.g_stages = _dp(gs)
            if op_stages is not None and L > 0:  # time-dependent lindblad_data
                ds = np.ascontiguousarray(diss_stages, dtype=np.float64).reshape(-1, L)
                os_ = _as_complex(op_stages).reshape(-1, L, n, n)
                keep.extend([ds, os_])
                p.diss_stages, p.op_stages = _dp(ds), _dp(os_)
        self._check(self._lib.qocx_set_lindblad_problem(self._ctx, ctypes.byref(p)))
        self._lindblad = dict(n=n, S=S, K=K, Nc=int(control_eval_count),
                              N=int(system_eval_count), L=L)
        self._lindblad_batch = 0
        self._lindblad_resident_batch = 0
        self._lindblad_ensemble = None
        self._lindblad_sweep = None
        self._lindblad_seeds = 0

    def set_lindblad_ensemble(self, scales, offsets, weights):
        """An ensemble of M members on the current Lindblad problem (qocx_lindblad_set_ensemble): the
        problem's last J control channels are the perturbation matrices D_j. scales :: (M, K - J) or
        None (all 1), offsets :: (M, J) or None (J = 0), weights :: (M,). From here on
        evaluate_lindblad and the lindblad_* calls take and return the seeds' K - J channels, final
        densities carry a member axis (B, M, S, n, n) and step densities are (B, M, N, S, n, n)."""
        weights = np.ascontiguousarray(weights, dtype=np.float64).reshape(-1)
        M = weights.shape[0]
        J = 0 if offsets is None else np.asarray(offsets).size // max(M, 1)
        kr = self._lindblad["K"] - J
        none = ctypes.cast(None, _c_double_p)
        sc = None if scales is None else np.ascontiguousarray(scales, dtype=np.float64).reshape(M, kr)
        off = None if offsets is None else np.ascontiguousarray(offsets, dtype=np.float64).reshape(M, J)
        self._check(self._lib.qocx_lindblad_set_ensemble(
            self._ctx, M, J, none if sc is None else _dp(sc), none if off is None else _dp(off),
            _dp(weights)))
        self._lindblad_ensemble = dict(M=M, J=J, Kr=kr)
        self._lindblad_batch = self._lindblad_seeds = 0
        self._lindblad_resident_batch = 0

    def set_lindblad_ensemble_rates(self, rate_scales):
        """Per-member dissipation rates of the current Lindblad ensemble
        (qocx_lindblad_set_ensemble_rates): rate_scales :: (M, L) finite and >= 0, member m decays
        with the rates rate_scales[m] * dissipators; None clears them. After set_lindblad_ensemble;
        a new problem or a new ensemble clears the rates. Static problems only (no stage tables)."""
        if rate_scales is None:
            self._check(self._lib.qocx_lindblad_set_ensemble_rates(
                self._ctx, 0, 0, ctypes.cast(None, _c_double_p)))
        else:
            rates = np.ascontiguousarray(rate_scales, dtype=np.float64)
            if rates.ndim != 2:
                raise ValueError("rate_scales must be (M, L), got shape {}".format(rates.shape))
            keep = rates if rates.size else np.zeros(1)  # (L = 0: nothing is read)
            self._check(self._lib.qocx_lindblad_set_ensemble_rates(
                self._ctx, rates.shape[0], rates.shape[1], _dp(keep)))
        self._lindblad_batch = self._lindblad_seeds = 0
        self._lindblad_resident_batch = 0

    def lindblad_ensemble_member_costs(self):
        """The unweighted cost of every member of every seed of the last Lindblad evaluation, (B, M)
        (qocx_lindblad_ensemble_download_members)."""
        M = 1 if self._lindblad_ensemble is None else self._lindblad_ensemble["M"]
        out = np.empty((max(1, self._lindblad_seeds), M), dtype=np.float64)
        self._check(self._lib.qocx_lindblad_ensemble_download_members(self._ctx, _dp(out)))
        return out

    def _lindblad_members(self):
        return () if self._lindblad_ensemble is None else (self._lindblad_ensemble["M"],)

    def _lindblad_seed_channels(self):
        """Control channels of a Lindblad seed: the problem's K, or K - J with an ensemble or a sweep
        set."""
        ens = self._lindblad_ensemble if self._lindblad_sweep is None else self._lindblad_sweep
        return self._lindblad["K"] if ens is None else ens["Kr"]

    def set_lindblad_sweep(self, scales, offsets, rate_scales=None):
        """A sweep of B seeds on the current Lindblad problem (qocx_lindblad_set_sweep): seed b is an
        open system of its own, the problem on the controls [scales[b] * u_b, offsets[b]] with the
        rates rate_scales[b] * dissipators; the problem's last J control channels are the fixed
        matrices D_j. scales :: (B, K - J) or None (all 1), offsets :: (B, J) or None (J = 0),
        rate_scales :: (B, L) finite and >= 0 or None (the problem's rates); one of them is needed
        (B is read from it). From here on evaluate_lindblad and the lindblad_* calls take and return
        the seeds' K - J channels, the batch is exactly B and final densities are (B, S, n, n)."""
        if scales is None and offsets is None and rate_scales is None:
            raise ValueError("a sweep needs scales, offsets or rate_scales (the seed count is read "
                             "from them)")
        none = ctypes.cast(None, _c_double_p)
        off = None if offsets is None else np.ascontiguousarray(offsets, dtype=np.float64)
        if off is not None and off.ndim != 2:
            raise ValueError("offsets must be (B, J), got shape {}".format(off.shape))
        J = 0 if off is None else off.shape[1]
        kr = self._lindblad["K"] - J
        sc = None if scales is None else np.ascontiguousarray(scales, dtype=np.float64)
        rates = None if rate_scales is None else np.ascontiguousarray(rate_scales, dtype=np.float64)
        if rates is not None and (rates.ndim != 2 or rates.shape[1] != self._lindblad["L"]):
            raise ValueError("rate_scales must be (B, L) with L = {} operators, got shape {}".format(
                self._lindblad["L"], rates.shape))
        B = next(a.shape[0] for a in (sc, off, rates) if a is not None)
        if sc is not None and sc.shape != (B, kr):
            raise ValueError("scales must be (B, K - J) = ({}, {}), got shape {}".format(B, kr, sc.shape))
        if any(a is not None and a.shape[0] != B for a in (off, rates)):
            raise ValueError("scales, offsets and rate_scales disagree on the seed count")
        if J == 0:
            off = None
        if rates is not None and rates.size == 0:  # (L = 0: nothing to scale)
            rates = None
        self._check(self._lib.qocx_lindblad_set_sweep(
            self._ctx, B, J, none if sc is None else _dp(sc), none if off is None else _dp(off),
            none if rates is None else _dp(rates)))
        self._lindblad_ensemble = None
        self._lindblad_sweep = dict(B=B, J=J, Kr=kr, L=self._lindblad["L"])
        self._lindblad_batch = self._lindblad_seeds = 0
        self._lindblad_resident_batch = 0

    def lindblad_sweep_want_rate_sensitivities(self, on):
        """Ask the evaluations from here on for the rate sensitivities of the sweep
        (qocx_lindblad_sweep_want_rate_sensitivities): one more kernel launch per piece."""
        self._check(self._lib.qocx_lindblad_sweep_want_rate_sensitivities(self._ctx, int(bool(on))))

    def lindblad_sweep_sensitivities(self, want_rates=True):
        """(dE_b / d scales [B, K - J], dE_b / d offsets [B, J], dE_b / d rate_scales [B, L] or None)
        of the last evaluation with gradients (qocx_lindblad_sweep_download_sensitivities). The
        rate entry is None unless the evaluation was asked for it and every piece of it ran
        two-sided (the engine then answers QOCX_ERR_STATE for that output alone)."""
        sw = self._lindblad_sweep
        if sw is None:
            raise ValueError("no sweep set (set_lindblad_sweep)")
        none = ctypes.cast(None, _c_double_p)
        scales = np.empty((sw["B"], sw["Kr"]), dtype=np.float64)
        offsets = np.empty((sw["B"], sw["J"]), dtype=np.float64)
        self._check(self._lib.qocx_lindblad_sweep_download_sensitivities(
            self._ctx, _dp(scales), _dp(offsets), none))
        rates = None
        if want_rates and sw["L"] > 0:
            rates = np.empty((sw["B"], sw["L"]), dtype=np.float64)
            code = self._lib.qocx_lindblad_sweep_download_sensitivities(
                self._ctx, none, none, _dp(rates))
            if code == ERR_STATE:
                rates = None
            else:
                self._check(code)
        return scales, offsets, rates

    def lindblad_sweep_set_durations(self, tau, base_scales, base_offsets, base_rate_scales,
                                     tau_min, tau_max, time_weight=0.0):
        """The current Lindblad sweep as a duration search (qocx_lindblad_sweep_set_durations):
        tau :: (B,) the seeds' durations in units of the evolution time, clipped to
        [tau_min, tau_max] on the device; base_scales :: (B, K - J) or None (all 1), base_offsets ::
        (B, J) and base_rate_scales :: (B, L) or None (all 1) the tables before the factor tau (the
        drift column of base_offsets is 1). The engine derives the sweep's tables and the seeds'
        control-free generators from them; controls must be uploaded again afterwards."""
        sw = self._lindblad_sweep
        tau = np.ascontiguousarray(tau, dtype=np.float64).reshape(-1)
        none = ctypes.cast(None, _c_double_p)
        s0 = None if base_scales is None else np.ascontiguousarray(base_scales, dtype=np.float64)
        d0 = None if base_offsets is None else np.ascontiguousarray(base_offsets, dtype=np.float64)
        c0 = (None if base_rate_scales is None
              else np.ascontiguousarray(base_rate_scales, dtype=np.float64))
        if sw is not None:  # (without a sweep the engine refuses by itself: QOCX_ERR_STATE)
            B = sw["B"]
            if tau.shape[0] != B:
                raise ValueError("tau must be (B,) = ({},), got shape {}".format(B, tau.shape))
            for name, table, width in (("base_scales", s0, sw["Kr"]), ("base_offsets", d0, sw["J"]),
                                       ("base_rate_scales", c0, sw["L"])):
                if table is not None and table.shape != (B, width):
                    raise ValueError("{} must be ({}, {}), got shape {}".format(
                        name, B, width, table.shape))
        self._check(self._lib.qocx_lindblad_sweep_set_durations(
            self._ctx, _dp(tau), none if s0 is None else _dp(s0), none if d0 is None else _dp(d0),
            none if c0 is None else _dp(c0), float(tau_min), float(tau_max), float(time_weight)))
        self._lindblad_batch = self._lindblad_seeds = 0
        self._lindblad_resident_batch = 0

    def lindblad_sweep_download_durations(self, want_grad=True):
        """(tau [B], d error_b / d tau_b + time_weight [B] or None) of a duration search
        (qocx_lindblad_sweep_download_durations); the gradient is that of the last evaluation with
        gradients."""
        B = self._lindblad_sweep["B"] if self._lindblad_sweep is not None else 1
        tau = np.empty(B, dtype=np.float64)
        grad = np.empty(B, dtype=np.float64) if want_grad else None
        self._check(self._lib.qocx_lindblad_sweep_download_durations(
            self._ctx, _dp(tau), _dp(grad) if want_grad else ctypes.cast(None, _c_double_p)))
        return tau, grad

    def lindblad_opt_download_best_durations(self):
        """tau [B] at every seed's best evaluation of the resident driver
        (qocx_lindblad_opt_download_best_durations)."""
        B = self._lindblad_sweep["B"] if self._lindblad_sweep is not None else 1
        tau = np.empty(B, dtype=np.float64)
        self._check(self._lib.qocx_lindblad_opt_download_best_durations(self._ctx, _dp(tau)))
        return tau

    def evaluate_lindblad(self, controls, want_grad=True, want_final=True):
        """(cost[B], grads[B,Nc,K] or None, final_densities[B,S,n,n]) for controls[B,Nc,K]; with an
        ensemble K is the seeds' K - J channels and the final densities are [B,M,S,n,n]."""
        pr = self._lindblad
        K = self._lindblad_seed_channels()
        if pr["K"] > 0:
            controls = np.ascontiguousarray(controls, dtype=np.float64)
            controls = controls.reshape(-1, pr["Nc"], K)
            B = controls.shape[0]
        else:
            B = 1 if controls is None else int(controls)
            controls = None
        cost = np.empty(B, dtype=np.float64)
        want_grad = bool(want_grad) and pr["K"] > 0
        grads = np.empty((B, pr["Nc"], K), dtype=np.float64) if want_grad else None
        final = (np.empty(self._final_shape(B, PATH_LINDBLAD), dtype=np.complex128)
                 if want_final else None)
        self._check(self._lib.qocx_eval_lindblad(
            self._ctx, B, _dp(controls) if controls is not None else None, int(want_grad),
            _dp(cost), _dp(grads) if want_grad else None, _dp(final) if want_final else None))
        self._lindblad_batch = self._lindblad_seeds = B
        return cost, grads, final

    def lindblad_last_subintervals(self):
        """DOP853 sub-intervals of the last evaluate_lindblad, summed over its seeds."""
        total = _I64(0)
        self._check(self._lib.qocx_lindblad_last_subintervals(self._ctx, ctypes.byref(total)))
        return total.value

    def set_density_cotangents(self, steps, bars):
        """bars :: (B, len(steps), S, n, n) complex cotangents of the densities at `steps`."""
        if steps is None or len(steps) == 0:
            self._check(self._lib.qocx_set_density_cotangents(self._ctx, 0, 0, None, None))
            return
        pr = self._lindblad
        steps = np.ascontiguousarray(steps, dtype=np.int32)
        bars = _as_complex(bars).reshape(-1, len(steps), pr["S"], pr["n"], pr["n"])
        self._check(self._lib.qocx_set_density_cotangents(
            self._ctx, bars.shape[0], len(steps), steps.ctypes.data_as(_c_int_p), _dp(bars)))

    def download_step_densities(self):
        pr, B = self._lindblad, self._lindblad_batch
        out = np.empty((B,) + self._lindblad_members() + (pr["N"], pr["S"], pr["n"], pr["n"]),
                       dtype=np.complex128)
        self._check(self._lib.qocx_download_step_densities(self._ctx, _dp(out)))
        return out

    def set_state_cotangents(self, steps, bars):
        """bars :: (B, len(steps), S, n) complex cotangents of the states at system steps `steps`;
        steps = None or empty clears them."""
        if steps is None or len(steps) == 0:
            self._check(self._lib.qocx_set_state_cotangents(self._ctx, 0, 0, None, None))
            return
        pr = self._problem
        steps = np.ascontiguousarray(steps, dtype=np.int32)
        bars = _as_complex(bars).reshape(-1, len(steps), pr["S"], pr["n"])
        self._check(self._lib.qocx_set_state_cotangents(
            self._ctx, bars.shape[0], len(steps), steps.ctypes.data_as(_c_int_p), _dp(bars)))

    def set_chunk(self, seeds_per_chunk):
        self._check(self._lib.qocx_set_chunk(self._ctx, int(seeds_per_chunk)))

    def set_pipeline(self, time_segments):
        """Number of time segments the evaluation pipeline is cut into (0 = automatic)."""
        self._check(self._lib.qocx_set_pipeline(self._ctx, int(time_segments)))

    def pade_orders(self):
        """{order: propagator steps} of the last evaluation (include/qocx.h: qocx_pade_orders)."""
        counts = (_I64 * 5)()
        self._check(self._lib.qocx_pade_orders(self._ctx, counts))
        return {order: int(counts[i]) for i, order in enumerate((3, 5, 7, 9, 13))}

    def lu_fallbacks(self):
        """Matrices of the last evaluation / debug_pade_factor call whose factorisation left the
        diagonal-pivot MFMA form for the general elimination (include/qocx.h: qocx_lu_fallbacks)."""
        count = _I64(0)
        self._check(self._lib.qocx_lu_fallbacks(self._ctx, ctypes.byref(count)))
        return int(count.value)

    def action_degrees(self):
        """{degree: propagator steps} the last evaluation executed on the matrix-free route, degrees
        1 .. 18; every count is zero when it took the Pade route (include/qocx.h: qocx_action_degrees)."""
        counts = (_I64 * 19)()
        self._check(self._lib.qocx_action_degrees(self._ctx, counts))
        return {m: int(counts[m]) for m in range(1, 19)}

    def action_reruns(self):
        """Evaluations the matrix-free route handed back to the Pade route (qocx_action_reruns)."""
        count = _I64(0)
        self._check(self._lib.qocx_action_reruns(self._ctx, ctypes.byref(count)))
        return int(count.value)

    def timeline(self, capacity=4096):
        """(which, start_ms, end_ms) of the last evaluation's kernel launches (timing on)."""
        out = np.zeros((capacity, 3))
        count = _I64(0)
        self._check(self._lib.qocx_debug_timeline(
            self._ctx, out.ctypes.data_as(_c_double_p), capacity, ctypes.byref(count)))
        return out[:min(capacity, count.value)]

    # -- timing --------------------------------------------------------------------------------
    def set_timing(self, enable, only=None):
        """enable: every launch carries HIP events; only = a name of KERNEL_NAMES: that kernel only."""
        mode = (2 + KERNEL_NAMES.index(only)) if (enable and only) else int(bool(enable))
        self._check(self._lib.qocx_set_timing(self._ctx, mode))

    def reset_timing(self):
        self._check(self._lib.qocx_reset_timing(self._ctx))

    def timing(self):
        out = {}
        for which, name in enumerate(KERNEL_NAMES):
            launches, ms = _I64(0), ctypes.c_double(0)
            self._check(self._lib.qocx_get_timing(self._ctx, which, ctypes.byref(launches),
                                                  ctypes.byref(ms)))
            out[name] = (launches.value, ms.value)
        return out

    # -- RCCL ----------------------------------------------------------------------------------
    @staticmethod
    def comm_unique_id():
        lib = load_library()
        buf = (ctypes.c_uint8 * 128)()
        code = lib.qocx_comm_unique_id(buf)
        if code != 0:
            raise QocxError(code, lib.qocx_last_error().decode("utf-8", "replace"))
        return bytes(buf)

    def comm_init(self, unique_id, rank, world):
        buf = (ctypes.c_uint8 * 128).from_buffer_copy(unique_id)
        self._check(self._lib.qocx_comm_init(self._ctx, buf, int(rank), int(world)))

    # -- multi-start driver with the optimizer states on the device -----------------------------
    # The Schroedinger and the Lindblad problem have their own resident buffers and their own C
    # entry points with one signature; each public method below names its C function and, where
    # shapes are needed, its path.
    def _resident_batch(self, path):
        return self._lindblad_resident_batch if path == PATH_LINDBLAD else self.batch

    def _download_results(self, call, path, want_grad, want_final):
        B, (nc, channels) = self._resident_batch(path), self._control_channels(path)
        cost = np.empty(B, dtype=np.float64)
        want_grad = want_grad and channels > 0
        grads = np.empty((B, nc, channels), dtype=np.float64) if want_grad else None
        final = np.empty(self._final_shape(B, path), dtype=np.complex128) if want_final else None
        self._check(call(self._ctx, _dp(cost), _dp(grads) if want_grad else None,
                         _dp(final) if want_final else None))
        return cost, grads, final

    def _download_costs(self, call, path):
        cost = np.empty(self._resident_batch(path), dtype=np.float64)
        self._check(call(self._ctx, _dp(cost)))
        return cost

    def _opt_clip(self, call, max_norms):
        max_norms = np.ascontiguousarray(max_norms, dtype=np.float64)
        self._check(call(self._ctx, _dp(max_norms)))

    def _opt_step(self, call, kind, improved, update, learning_rate, beta_1, beta_2, epsilon,
                  corr_1, corr_2, clip_grads):
        improved = np.ascontiguousarray(improved, dtype=np.uint8)
        update = np.ascontiguousarray(update, dtype=np.uint8)
        self._check(call(
            self._ctx, int(kind), improved.ctypes.data_as(_U8P), update.ctypes.data_as(_U8P),
            float(learning_rate), float(beta_1), float(beta_2), float(epsilon), float(corr_1),
            float(corr_2), 0 if clip_grads is None else 1,
            0.0 if clip_grads is None else float(clip_grads)))

    def _lbfgs_step(self, call, improved, update, first_step, armijo, shrink, max_backtracks):
        improved = np.ascontiguousarray(improved, dtype=np.uint8)
        update = np.ascontiguousarray(update, dtype=np.uint8)
        finished = np.zeros(len(update), dtype=np.uint8)
        self._check(call(self._ctx, improved.ctypes.data_as(_U8P), update.ctypes.data_as(_U8P),
                         float(first_step), float(armijo), float(shrink), int(max_backtracks),
                         finished.ctypes.data_as(_U8P)))
        return finished.astype(bool)

    def _opt_download_best(self, call, path):
        B = self._resident_batch(path)
        controls = np.empty((B,) + self._control_channels(path), dtype=np.float64)
        final = np.empty(self._final_shape(B, path), dtype=np.complex128)
        self._check(call(self._ctx, _dp(controls), _dp(final)))
        return controls, final

    def _opt_begin_basis(self, call, path, complex_controls, matrix, coefficients):
        nc, channels = self._control_channels(path)
        matrix = np.ascontiguousarray(matrix, dtype=np.float64)
        if matrix.ndim != 2 or matrix.shape[0] != nc:
            raise ValueError("the basis matrix must be ({} x P), got shape {}".format(nc, matrix.shape))
        P = matrix.shape[1]
        coefficients = np.ascontiguousarray(coefficients, dtype=np.float64)
        if P > 0:
            coefficients = coefficients.reshape(-1, P, channels)
            if coefficients.shape[0] != self._resident_batch(path) > 0:
                raise ValueError("coefficients for {} seeds, {} are resident".format(
                    coefficients.shape[0], self._resident_batch(path)))
        self._basis_P[path] = 0
        self._check(call(self._ctx, int(bool(complex_controls)), P, _dp(matrix), _dp(coefficients)))
        self._basis_P[path] = P

    def _opt_download_best_params(self, call, path):
        _, channels = self._control_channels(path)
        params = np.empty((self._resident_batch(path), max(1, self._basis_P.get(path, 0)), channels),
                          dtype=np.float64)
        self._check(call(self._ctx, _dp(params)))
        return params

    def opt_begin(self):
        self._check(self._lib.qocx_opt_begin(self._ctx))

    def opt_begin_basis(self, complex_controls, matrix, coefficients):
        """In the place of opt_begin / opt_begin_complex, after upload_controls of the expanded start
        pulses: the optimizer's parameters are `coefficients` [B, P, channels] of the basis `matrix`
        [Nc, P]; opt_clip expands them into the evaluated controls and clips those, opt_step /
        opt_lbfgs_step work on the coefficients and the projected gradient (qocx_opt_begin_basis)."""
        self._opt_begin_basis(self._lib.qocx_opt_begin_basis, PATH_SCHROEDINGER, complex_controls,
                              matrix, coefficients)

    def opt_download_best_params(self):
        """The coefficients [B, P, channels] behind the best controls (qocx_opt_download_best_params)."""
        return self._opt_download_best_params(self._lib.qocx_opt_download_best_params,
                                              PATH_SCHROEDINGER)

    def opt_begin_complex(self):
        """opt_begin for complex controls (channels 2k, 2k+1): the optimizer's parameters stay
        unclipped, opt_clip takes one modulus bound per complex control (qocx_opt_begin_complex)."""
        self._check(self._lib.qocx_opt_begin_complex(self._ctx))

    def opt_clip(self, max_norms):
        self._opt_clip(self._lib.qocx_opt_clip, max_norms)

    def download_costs(self):
        return self._download_costs(self._lib.qocx_download_costs, PATH_SCHROEDINGER)

    def opt_step(self, kind, improved, update, learning_rate, beta_1=0.0, beta_2=0.0, epsilon=0.0,
                 corr_1=1.0, corr_2=1.0, clip_grads=None):
        self._opt_step(self._lib.qocx_opt_step, kind, improved, update, learning_rate, beta_1,
                       beta_2, epsilon, corr_1, corr_2, clip_grads)

    def opt_lbfgs_begin(self, history):
        """After opt_begin / opt_begin_complex: the seeds' L-BFGS state, zeroed (qocx_opt_lbfgs_begin)."""
        self._check(self._lib.qocx_opt_lbfgs_begin(self._ctx, int(history)))

    def opt_lbfgs_step(self, improved, update, first_step, armijo, shrink, max_backtracks):
        """The best-so-far bookkeeping of opt_step, then one LBFGS.update of the seeds flagged in
        `update` on the last evaluation's costs and gradients; returns finished [B] (bool)."""
        return self._lbfgs_step(self._lib.qocx_opt_lbfgs_step, improved, update, first_step, armijo,
                                shrink, max_backtracks)

    def opt_download_best(self):
        return self._opt_download_best(self._lib.qocx_opt_download_best, PATH_SCHROEDINGER)

    # -- the same for the Lindblad problem (its own resident buffers, seed order) -----------------
    def lindblad_upload_controls(self, controls):
        """controls :: (B, Nc, K) real, kept in HBM for eval_lindblad_resident / lindblad_opt_* (with
        an ensemble the seeds' K - J channels)."""
        pr = self._lindblad
        controls = np.ascontiguousarray(controls, dtype=np.float64).reshape(
            -1, pr["Nc"], self._lindblad_seed_channels())
        self._check(self._lib.qocx_lindblad_upload_controls(self._ctx, controls.shape[0],
                                                            _dp(controls)))
        self._lindblad_resident_batch = controls.shape[0]

    def eval_lindblad_resident(self, want_grad=True):
        self._check(self._lib.qocx_eval_lindblad_resident(self._ctx, int(bool(want_grad))))
        self._lindblad_batch = self._lindblad_seeds = self._lindblad_resident_batch

    def lindblad_download_results(self, want_grad=True, want_final=True):
        """(cost[B], grads[B,Nc,K] or None, final_densities[B,S,n,n] or None), seed order."""
        return self._download_results(self._lib.qocx_lindblad_download_results, PATH_LINDBLAD,
                                      want_grad, want_final)

    def lindblad_download_costs(self):
        return self._download_costs(self._lib.qocx_lindblad_download_costs, PATH_LINDBLAD)

    def lindblad_opt_begin(self):
        self._check(self._lib.qocx_lindblad_opt_begin(self._ctx))

    def lindblad_opt_begin_complex(self):
        self._check(self._lib.qocx_lindblad_opt_begin_complex(self._ctx))

    def lindblad_opt_begin_basis(self, complex_controls, matrix, coefficients):
        self._opt_begin_basis(self._lib.qocx_lindblad_opt_begin_basis, PATH_LINDBLAD,
                              complex_controls, matrix, coefficients)

    def lindblad_opt_download_best_params(self):
        return self._opt_download_best_params(self._lib.qocx_lindblad_opt_download_best_params,
                                              PATH_LINDBLAD)

    def lindblad_opt_clip(self, max_norms):
        self._opt_clip(self._lib.qocx_lindblad_opt_clip, max_norms)

    def lindblad_opt_step(self, kind, improved, update, learning_rate, beta_1=0.0, beta_2=0.0,
                          epsilon=0.0, corr_1=1.0, corr_2=1.0, clip_grads=None):
        self._opt_step(self._lib.qocx_lindblad_opt_step, kind, improved, update, learning_rate,
                       beta_1, beta_2, epsilon, corr_1, corr_2, clip_grads)

    def lindblad_opt_lbfgs_begin(self, history):
        self._check(self._lib.qocx_lindblad_opt_lbfgs_begin(self._ctx, int(history)))

    def lindblad_opt_lbfgs_step(self, improved, update, first_step, armijo, shrink, max_backtracks):
        return self._lbfgs_step(self._lib.qocx_lindblad_opt_lbfgs_step, improved, update, first_step,
                                armijo, shrink, max_backtracks)

    def lindblad_opt_download_best(self):
        return self._opt_download_best(self._lib.qocx_lindblad_opt_download_best, PATH_LINDBLAD)

    # -- costs of the controls alone on the device ------------------------------------------------
    def _control_channels(self, path):
        if path == PATH_LINDBLAD:
            return self._lindblad["Nc"], self._lindblad_seed_channels()
        return self._problem["Nc"], self._seed_channels()

    def set_control_costs(self, path, complex_controls, descriptors):
        """The costs of the controls alone of the problem `path` (PATH_SCHROEDINGER / PATH_LINDBLAD),
        added by eval_resident / eval_lindblad_resident from here on (qocx_set_control_costs); an
        empty list clears them. descriptors :: dicts {kind (CONTROL_*), multiplier, order (optional),
        max_norms / weights (per control, optional), bins (one ascending index array per control,
        bandwidth cost)} as the control_descriptor() of the cost classes returns them."""
        descriptors = list(descriptors)
        descs = (_ControlCostDesc * max(1, len(descriptors)))()
        keep = []

        def doubles(values):
            if values is None:
                return ctypes.cast(None, _c_double_p)
            array = np.ascontiguousarray(values, dtype=np.float64).reshape(-1)
            keep.append(array)
            return _dp(array)

        for i, d in enumerate(descriptors):
            descs[i].kind = int(d["kind"])
            descs[i].order = int(d.get("order", 0))
            descs[i].multiplier = float(d["multiplier"])
            descs[i].max_norms = doubles(d.get("max_norms"))
            descs[i].weights = doubles(d.get("weights"))
            if d.get("bins") is not None:
                sets = [np.asarray(b, dtype=np.int32).reshape(-1) for b in d["bins"]]
                ptr = np.ascontiguousarray(np.cumsum([0] + [len(b) for b in sets]), dtype=np.int32)
                bins = np.ascontiguousarray(np.concatenate(sets) if sets else np.zeros(0),
                                            dtype=np.int32)
                keep.extend([ptr, bins])
                descs[i].bins = bins.ctypes.data_as(_c_int_p)
                descs[i].bin_ptr = ptr.ctypes.data_as(_c_int_p)
        self._check(self._lib.qocx_set_control_costs(
            self._ctx, int(path), int(bool(complex_controls)), len(descriptors), descs))

    def eval_control_costs(self, path, controls, want_grad=True):
        """(cost [B], gradient [B, Nc, channels] or None) of the control costs alone for controls
        [B, Nc, channels] real (a complex control: channels 2k, 2k+1) (qocx_eval_control_costs)."""
        nc, channels = self._control_channels(path)
        controls = np.ascontiguousarray(controls, dtype=np.float64).reshape(-1, nc, channels)
        cost = np.empty(controls.shape[0], dtype=np.float64)
        grads = np.empty(controls.shape, dtype=np.float64) if want_grad else None
        self._check(self._lib.qocx_eval_control_costs(
            self._ctx, int(path), controls.shape[0], _dp(controls), _dp(cost),
            _dp(grads) if want_grad else None))
        return cost, grads

    def control_basis_apply(self, matrix, array, transpose=False):
        """The map of a control basis alone, host arrays in and out (qocx_control_basis_apply):
        matrix [Nc, P]; array [B, P, channels] -> [B, Nc, channels], or with transpose
        [B, Nc, channels] -> [B, P, channels]."""
        matrix = np.ascontiguousarray(matrix, dtype=np.float64)
        nc, P = matrix.shape
        array = np.ascontiguousarray(array, dtype=np.float64)
        rows_in, rows_out = (nc, P) if transpose else (P, nc)
        if array.ndim != 3 or array.shape[1] != rows_in:
            raise ValueError("array must be (B x {} x channels), got shape {}".format(rows_in,
                                                                                     array.shape))
        out = np.empty((array.shape[0], rows_out, array.shape[2]), dtype=np.float64)
        self._check(self._lib.qocx_control_basis_apply(
            self._ctx, int(bool(transpose)), array.shape[0], nc, P, array.shape[2], _dp(matrix),
            _dp(array), _dp(out)))
        return out

    def reduce_results(self, allreduce=False, want_grad=True):
        """(sum of the costs, sum of the gradients [Nc x K] or None) over the seeds of the last
        evaluation, summed on the device and - allreduce=True - over the ranks of the communicator
        by one ncclAllReduce on the device buffer (qocx_reduce_results)."""
        nc, k = self._problem["Nc"], self._seed_channels()
        want_grad = want_grad and k > 0
        count = 1 + (nc * k if want_grad else 0)
        out = np.zeros(count)
        self._check(self._lib.qocx_reduce_results(self._ctx, 1 if allreduce else 0, _dp(out), count))
        return float(out[0]), (out[1:].reshape(nc, k) if want_grad else None)

    def comm_allreduce_sum(self, array):
        array = np.ascontiguousarray(array, dtype=np.float64)
        self._check(self._lib.qocx_comm_allreduce_sum(self._ctx, _dp(array), array.size))
        return array

    def comm_allreduce_max(self, array):
        array = np.ascontiguousarray(array, dtype=np.float64)
        self._check(self._lib.qocx_comm_allreduce_max(self._ctx, _dp(array), array.size))
        return array

    def comm_barrier(self):
        self._check(self._lib.qocx_comm_barrier(self._ctx))

    def comm_destroy(self):
        self._check(self._lib.qocx_comm_destroy(self._ctx))

    # -- debug ---------------------------------------------------------------------------------
    def debug_pade_factor(self, a):
        a = _as_complex(a)
        if a.ndim == 2:
            a = a[None]
        count, n = a.shape[0], a.shape[1]
        q = np.empty((count, n, n), dtype=np.complex128)
        lu = np.empty((count, n, n), dtype=np.complex128)
        perm = np.empty((count, n), dtype=np.int32)
        dinv = np.empty((count, n), dtype=np.complex128)
        s = np.empty(count, dtype=np.int32)
        self._check(self._lib.qocx_debug_pade_factor(
            self._ctx, count, n, _dp(a), _dp(q), _dp(lu), perm.ctypes.data_as(_c_int_p),
            _dp(dinv), s.ctypes.data_as(_c_int_p)))
        # entry of the step table: squarings in bits 0..7, Pade order in bits 8..15 (0: 13)
        order = (s >> 8) & 0xff
        return dict(q=q, lu=lu, perm=perm, dinv=dinv, s=s & 0xff, order=np.where(order == 0, 13, order))

    def set_knob(self, name, value):
        """Kernel-variant switch (include/qocx.h: qocx_debug_set_knob)."""
        self._check(self._lib.qocx_debug_set_knob(self._ctx, name.encode(), int(value)))

    def read_stamps(self, batch, roles=4):
        """[batch][roles][8] cycle sums of a stamped diagnostic kernel build (knobs sweep3_stamps:
        4 roles; lindblad_stamps: 6 wavefronts)."""
        out = np.zeros((batch, roles, 8), dtype=np.uint64)
        self._check(self._lib.qocx_debug_read_stamps(
            self._ctx, out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), out.size))
        return out

    def debug_lindblad_knobs(self, stage_budget_seeds=0, min_piece=256, wave_mode=0):
        """Force the Lindblad launch variants (piece-wise, recompute, one / several waves per
        seed); see include/qocx.h. Defaults restore the automatic choice."""
        self._check(self._lib.qocx_debug_lindblad_knobs(
            self._ctx, int(stage_budget_seeds), int(min_piece), int(wave_mode)))

    def mfma_peak(self, waves_per_simd=1, iters=20000):
        """Sustained FP64 MFMA TFLOP/s of a register-only MFMA loop (roofline calibration)."""
        out = ctypes.c_double(0)
        self._check(self._lib.qocx_debug_mfma_peak(self._ctx, int(waves_per_simd), int(iters),
                                                   ctypes.byref(out)))
        return out.value

    def selftest(self):
        failures = ctypes.c_int32(0)
        report = ctypes.create_string_buffer(4096)
        self._check(self._lib.qocx_debug_selftest(self._ctx, ctypes.byref(failures), report, 4096))
        return failures.value, report.value.decode("utf-8", "replace")
