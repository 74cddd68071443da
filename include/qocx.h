/*
 * qocx.h - C ABI of the MI355X GRAPE propagation engine (libqocx.so).
 *
 * The reference (SchusterLab/qoc) is pure Python and has no FFI; the "interface" this
 * library replaces is the Python call pair
 *
 *     error        = _evaluate_schroedinger_discrete(controls, pstate, reporter)
 *                                   qoc/core/schroedingerdiscrete.py:356-438
 *     error, grads = ans_jacobian(_evaluate_schroedinger_discrete, 0)(controls, pstate, reporter)
 *                                   qoc/core/schroedingerdiscrete.py:318-319
 *                                   qoc/standard/utils/autogradutil.py:10-31
 *
 * i.e. "controls in -> total cost, d cost / d controls and final states out", batched here
 * over B independent control arrays (seeds).  Each entry point below cites the reference
 * code whose work it performs.  INTEGRATION.md shows the ctypes stub a maintainer of the
 * reference would add at those call sites.
 *
 * Conventions
 *   - every function returns 0 on success, <0 on error; qocx_last_error() gives the text;
 *   - the caller owns all host buffers (C-contiguous; complex = interleaved re,im float64);
 *   - the library owns all device memory inside the opaque context;
 *   - calls are blocking unless named *_async; one context per (host thread, device);
 *   - no global mutable state besides the per-thread error string.
 */
#ifndef QOCX_H
#define QOCX_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct qocx_ctx qocx_ctx;

#define QOCX_OK 0
#define QOCX_ERR_ARG -1       /* invalid argument / unsupported size        */
#define QOCX_ERR_HIP -2       /* HIP runtime error                          */
#define QOCX_ERR_STATE -3     /* call sequence error (no problem set, ...)  */
#define QOCX_ERR_SINGULAR -4  /* Pade denominator numerically singular (numpy.linalg.LinAlgError
                                 in the reference: expm.py:246)             */
#define QOCX_ERR_CAPACITY -5  /* squaring sub-step capacity exceeded        */
#define QOCX_ERR_RCCL -6      /* RCCL error / librccl not loadable          */

/* qoc.models.MagnusPolicy (qoc/models/magnuspolicy.py:8-26) */
#define QOCX_MAGNUS_M2 2
#define QOCX_MAGNUS_M4 4
#define QOCX_MAGNUS_M6 6

/* qoc_amd.models.InterpolationPolicy (qocx_set_interpolation_policy) */
#define QOCX_INTERP_LINEAR 1
#define QOCX_INTERP_PIECEWISE_CONSTANT 2

/* State-cost kinds evaluated on the device (qoc/standard/costs/). */
#define QOCX_COST_TARGET_COHERENT 0   /* TargetStateInfidelity[Time], neglect_relative_pahse=False:
                                         scale * (1 - |sum_s <t_s|psi_s>|^2 / S^2)
                                         targetstateinfidelity.py:52-56                            */
#define QOCX_COST_TARGET_INCOHERENT 1 /* ... neglect_relative_pahse=True:
                                         scale * (1 - sum_s |<t_s|psi_s>|^2 / S)   :58-61          */
#define QOCX_COST_FORBID 2            /* ForbidStates: scale * sum_s (1/F_s) sum_f |<f_sf|psi_s>|^2
                                         forbidstates.py:64-81 (scale = multiplier / (E * S))      */

#define QOCX_COST_TARGET_DENSITY 3    /* TargetDensityInfidelity[Time]:
                                         scale * (1 - sum_s |tr(T_s^H rho_s)| / (S n))
                                         targetdensityinfidelity.py:41-69; vectors = [S][n][n]      */
#define QOCX_COST_FORBID_DENSITY 4    /* ForbidDensities: scale * sum_s (1/F_s) sum_f |tr(F_sf^H rho_s)/n|^2
                                         forbiddensities.py:53-85; vectors = [sum_s F_s][n][n]       */

typedef struct qocx_cost_desc {
    int32_t kind;          /* QOCX_COST_*                                                         */
    int32_t step_cost;     /* 1: evaluated at system steps j*cost_eval_step, j>=1, before evolving
                              from that step (schroedingerdiscrete.py:412-416); 0: final states
                              only (:429-432)                                                      */
    double scale;          /* cost_multiplier (and 1/cost_eval_count etc.) folded in               */
    const double* vectors; /* TARGET_*: [S][n] complex target states (NOT conjugated)
                              FORBID  : [sum_s F_s][n] complex forbidden states, state-major       */
    const int32_t* counts; /* FORBID: [S] F_s ; TARGET_*: ignored (may be NULL)                    */
} qocx_cost_desc;

/*
 * Static data of one Schroedinger problem; mirrors the fields of
 * GrapeSchroedingerDiscreteState / ProgramState (qoc/models/programstate.py:33-61,
 * qoc/models/schroedingermodels.py:178-206) that the evolve loop reads.
 *
 * The Hamiltonian callable of the reference (schroedingerdiscrete.py:43-46, :485) is passed
 * in structured form   H(u, t) = h0(t) + sum_k u_k g[k](t),  u real (a complex control is two
 * real ones), sampled by the host at the quadrature times of the Magnus
 * policy: nt = 1 (time independent) or nt = (system_eval_count-1) * nodes.
 */
typedef struct qocx_schroedinger_problem {
    int32_t struct_size;         /* sizeof(qocx_schroedinger_problem) of the CALLER's header: a
                                    stale binding is rejected (QOCX_ERR_ARG) instead of over-read  */
    int32_t hilbert_size;        /* n, 1..1024 (65..1024: the general path, qocx_general.hip)              */
    int32_t state_count;         /* S >= 1                                                          */
    int32_t control_count;       /* K real controls, >= 0                                           */
    int32_t control_eval_count;  /* Nc (>= 2 when K > 0)                                            */
    int32_t system_eval_count;   /* N >= 2; N-1 propagator steps                                    */
    int32_t cost_eval_step;      /* >= 1                                                            */
    int32_t magnus_policy;       /* QOCX_MAGNUS_M2 / _M4 / _M6 (mathmethods.py:72-164)               */
    int32_t nt;                  /* time samples of h0/g: 1 or (N-1)*nodes, nodes = 1/2/3 for M2/4/6,
                                    ordered [step][node], t = step*dt + c_node*dt                   */
    double evolution_time;       /* T; dt = T/(N-1), control_eval_times = linspace(0,T,Nc)          */
    const double* h0;            /* [nt][n][n] complex                                              */
    const double* g;             /* [nt][K][n][n] complex                                           */
    const double* initial_states;/* [S][n] complex                                                  */
    int32_t cost_count;
    const qocx_cost_desc* costs; /* [cost_count]                                                    */
} qocx_schroedinger_problem;

/*
 * Static data of one Lindblad problem; mirrors the fields of GrapeLindbladDiscreteState
 * (qoc/models/lindbladmodels.py:125-203) that _evaluate_lindblad_discrete reads
 * (qoc/core/lindbladdiscrete.py:357-441). hamiltonian(u, t) = h0(t) + sum_k u_k g[k](t):
 * time independent (h0, g; fixed_subdivision = 0) or sampled at the integrator's stage times
 * (fixed_subdivision > 0, h0_stages, g_stages). lindblad_data(t) = (dissipators, operators) is
 * constant (dissipators, operators) or sampled the same way (diss_stages, op_stages; the reference
 * calls it at every right-hand side, lindbladdiscrete.py:486-492).
 */
typedef struct qocx_lindblad_problem {
    int32_t struct_size;          /* sizeof(qocx_lindblad_problem) of the CALLER's header         */
    int32_t hilbert_size;         /* n, 1..32 (n > 16: four tiles per matrix, HBM scratch); with the
                                     knob "lindblad_wide" at 1: 1..64 (33..64: static problems only,
                                     no stage tables; 65 and more are refused by name)             */
    int32_t density_count;        /* S >= 1                                                        */
    int32_t control_count;        /* K real controls, 0..8                                         */
    int32_t control_eval_count;   /* Nc                                                            */
    int32_t system_eval_count;    /* N >= 2                                                        */
    int32_t cost_eval_step;
    int32_t operator_count;       /* L Lindblad operators, 0..8 (17 <= n <= 32: as many as fit the LDS, 5) */
    double evolution_time;
    const double* h0;             /* [n][n] complex                                                */
    const double* g;              /* [K][n][n] complex                                             */
    const double* dissipators;    /* [L] float64 (gamma_i)                                         */
    const double* operators;      /* [L][n][n] complex                                             */
    const double* initial_densities; /* [S][n][n] complex                                          */
    int32_t cost_count;
    const qocx_cost_desc* costs;  /* kinds QOCX_COST_TARGET_DENSITY / QOCX_COST_FORBID_DENSITY     */
    /* Hamiltonian with explicit time dependence: every seed then uses `fixed_subdivision` pieces
     * per system step and h0 / g are given at the stage times of that grid
     * (qocx_lindblad_stage_times, same order). 0: time independent, sub-division chosen per seed. */
    int32_t fixed_subdivision;
    const double* h0_stages;      /* [count][n][n] complex                                         */
    const double* g_stages;       /* [count][K][n][n] complex, or NULL when g is constant          */
    /* time-dependent lindblad_data (needs fixed_subdivision > 0 and h0_stages): both or neither   */
    const double* diss_stages;    /* [count][L] float64 gamma_i(t), or NULL                        */
    const double* op_stages;      /* [count][L][n][n] complex L_i(t), or NULL                      */
} qocx_lindblad_problem;

const char* qocx_last_error(void);
int qocx_version(void);

/* Device discovery / context. device < 0: use LOCAL_RANK (or 0). */
int qocx_device_count(int* count);
int qocx_create(int device, qocx_ctx** out);
int qocx_destroy(qocx_ctx* ctx);
int qocx_synchronize(qocx_ctx* ctx);

/* Upload a problem (replaces any previous one). Performs what the construction of
 * GrapeSchroedingerDiscreteState does for the evolve loop: dt, control_eval_times,
 * step-cost selection (programstate.py:41-61). */
int qocx_set_schroedinger_problem(qocx_ctx* ctx, const qocx_schroedinger_problem* problem);

/*
 * How the controls are read between their grid points. Sticky on the context: the NEXT
 * qocx_set_schroedinger_problem / qocx_set_lindblad_problem reads it (a problem already set keeps
 * the policy it was set under); a context that never calls this interpolates linearly.
 *   QOCX_INTERP_LINEAR              controls[j] is the knot at t = j T / (Nc - 1), linear between
 *                                   knots (mathmethods.py:14-67).
 *   QOCX_INTERP_PIECEWISE_CONSTANT  controls[j] is the value on slice j of Nc equal slices:
 *                                   u(t) = controls[min(floor(t Nc / T), Nc - 1)]. Every quadrature
 *                                   node reads the slice it lies in; Lindblad sub-intervals are cut
 *                                   at the slice edges j T / Nc, which are the cut points
 *                                   qocx_lindblad_stage_times gives for control_eval_count = Nc + 1.
 * Array shapes, gradients, costs of the controls and the qocx_opt_* calls are the same under both.
 * QOCX_ERR_ARG for any other value.
 */
int qocx_set_interpolation_policy(qocx_ctx* ctx, int32_t policy);

/*
 * One batched evaluation == B calls of _evaluate_schroedinger_discrete (+ its reverse-mode
 * gradient when want_grad != 0), schroedingerdiscrete.py:318-324, :356-438.
 *   controls      [B][Nc][K] float64 (ignored when K == 0)
 *   cost_out      [B]
 *   grad_out      [B][Nc][K] float64   (d cost / d controls; NULL allowed when !want_grad)
 *   final_out     [B][S][n] complex    (reporter.final_states, :435-436; NULL allowed)
 * Host buffers in, host buffers out (H2D/D2H inside the call).
 */
int qocx_eval_schroedinger(qocx_ctx* ctx, int32_t batch, const double* controls,
                           int32_t want_grad, double* cost_out, double* grad_out,
                           double* final_out);

/* Same evaluation split so that inputs can be made resident first (bench.py times this). */
int qocx_upload_controls(qocx_ctx* ctx, int32_t batch, const double* controls);
int qocx_eval_resident(qocx_ctx* ctx, int32_t want_grad);
int qocx_download_results(qocx_ctx* ctx, double* cost_out, double* grad_out, double* final_out);

/*
 * Opaque Hamiltonians. The reference calls hamiltonian(controls, time) - arbitrary Python, not
 * necessarily linear in the controls (schroedingerdiscrete.py:483-486) - at every step. For a
 * callable the structured form above cannot represent, the host samples the step generators
 * itself, M_j = -i dt H(u(t_j + dt/2), t_j + dt/2) (mathmethods.py:90-93, magnus_m2), and the
 * engine takes them as they are (problem set with control_count = 0, magnus_policy M2):
 *   generators  [B][N-1][n][n] complex, row-major
 *   qocx_eval_resident / qocx_download_results as usual (cost_out, final_out);
 *   cotangents  [B][N-1][n][n] complex: Mbar_j = d cost / d Re(M_j) + i d cost / d Im(M_j), from
 *               which the host forms d cost / d u_k = Re sum_rc conj(Mbar_j[r][c]) (dM_j/du_k)[r][c]
 *               (what autograd's tape does at :318-319 through the user's callable).
 * qocx_upload_controls switches back to the structured form.
 */
int qocx_upload_generators(qocx_ctx* ctx, int32_t batch, const double* generators);
int qocx_download_generator_cotangents(qocx_ctx* ctx, double* cotangents_out);

/*
 * Hamiltonians quadratic in the real controls r (the reference's report names an epsilon^2
 * AC-Stark term, report.tex:22-32):
 *     H(r, t) = H0(t) + sum_k r_k G_k(t) + sum_q r_(k_q) r_(l_q) Q_q
 * with H0 / G_k from qocx_set_schroedinger_problem and constant Q_q. Call after that function
 * (which clears the terms); count = 0 clears them too. Real-control indices follow the problem's
 * layout (complex controls: Re u_j -> 2j, Im u_j -> 2j+1).
 *   pairs     [count][2] int32, 0 <= k_q <= l_q < control_count (repeated pairs add up)
 *   matrices  [count][n][n] complex, row-major
 * The engine evaluates H as linear in the K + count effective controls (r_k, r_k r_l) on both
 * evaluation routes, and folds their cotangents back to the real controls on the device; the
 * controls, the gradients and the qocx_opt_* state stay in the K real controls. QOCX_ERR_ARG for
 * indices out of range, magnus_policy M4 / M6, explicit generators, or control_count + count > 64;
 * QOCX_ERR_CAPACITY when a time-dependent problem's augmented tables (nt x (K + count) padded
 * matrices, three images below hilbert_size 65) would exceed 4 GiB. Controls must be uploaded
 * again afterwards.
 * With an ensemble (below; the two setters may come in either order) control_count is K_r + J: the
 * limit is K_r + J + count <= 64, the tables hold nt x (K_r + J + count) matrices, and the pairs
 * index the seeds' channels, l_q < K_r (QOCX_ERR_ARG otherwise, from whichever setter comes second).
 */
int qocx_set_quadratic_terms(qocx_ctx* ctx, int32_t count, const int32_t* pairs, const double* matrices);

/*
 * Hamiltonian ensembles (robust GRAPE): M members of the problem, all driven by the same seed
 * controls u. Call after qocx_set_schroedinger_problem, whose LAST `fixed` = J control channels
 * are the perturbation matrices D_j; K_r = control_count - J channels remain for the seeds.
 * Member m of seed b evaluates the problem on the K-channel controls
 *     r[j][k] = s_mk u_b[j][k] (k < K_r),   r[j][K_r + i] = delta_mi (every knot)
 * i.e. H_m(u, t) = H(s_m . u, t) + sum_i delta_mi D_i.
 *   scales  [M][K_r] (NULL: all 1)   offsets [M][J] (NULL exactly when J = 0)   weights [M] >= 0
 * QOCX_ERR_ARG unless 1 <= M <= 1024, 0 <= J < control_count and every input is finite. A new
 * problem clears the ensemble. Controls must be uploaded afterwards.
 * With quadratic terms (qocx_set_quadratic_terms, before or after this call) member m of seed b is
 *     H_(b,m)(t) = H_lin(s_m . u_b, t) + sum_i delta_mi D_i + sum_q c_mq (s_m,kq r_kq)(s_m,lq r_lq) Q_q
 * with r the seed's real channels and c_mq = 1 unless qocx_set_ensemble_quadratic_scales sets them.
 * An evaluation then runs: expansion of the seeds into the B x M items, the items' effective
 * controls (r_k, c_mq r_k r_l), the factor / sweep / gradient kernels of any batch, the chain rule
 * back to the items' real channels, the scatter to the knots, and the reduction below. The
 * squaring bound of the quadratic share is that of the expanded items,
 *     sum_q ||Q_q||_1 max_m |c_mq| (max_m |s_m,kq| max |r_kq|) (max_m |s_m,lq| max |r_lq|)
 * (the product of the members' maxima, not the maximum of the members' products), on an upload from
 * the uploaded controls and in qocx_opt_clip with max_norms in their place.
 * With an ensemble set:
 *   qocx_upload_controls(ctx, B, controls [B][Nc][K_r]) keeps the seed controls on the device and
 *     expands them into the B x M items (item b * M + m); the squaring bounds are those of the
 *     expanded array.
 *   qocx_eval_resident evaluates the items as any batch, then reduces them in member order:
 *     cost_b = sum_m w_m c_bm, grad_b[j][k] = sum_m w_m s_mk dc_bm / dr[j][k] (k < K_r; the
 *     gradients of the fixed channels are dropped).
 *   qocx_download_results (costs [B], gradients [B][Nc][K_r], final states [B][M][S][n]),
 *   qocx_download_costs, qocx_reduce_results and qocx_opt_* act on the B seeds and their K_r
 *     channels (qocx_opt_clip takes max_norms [K_r]; the best final states are [B][M][S][n]).
 *   qocx_download_step_states returns the items, [B][M][N][S][n].
 * qocx_ensemble_download_members: the unweighted cost of every item of the last evaluation, [B][M].
 */
int qocx_set_ensemble(qocx_ctx* ctx, int32_t members, int32_t fixed, const double* scales,
                      const double* offsets, const double* weights);
int qocx_ensemble_download_members(qocx_ctx* ctx, double* cost_out);

/*
 * Per-member scales of the quadratic terms of an ensemble (an uncertain Stark coefficient):
 *   scales [M][count] real, c_mq multiplying term q of member m; NULL clears them (all 1).
 * Needs qocx_set_ensemble with that M and qocx_set_quadratic_terms with that count, in either
 * order, before it; QOCX_ERR_ARG otherwise and for non-finite values. A new problem, a new
 * ensemble and new quadratic terms clear the scales. Controls must be uploaded again afterwards.
 */
int qocx_set_ensemble_quadratic_scales(qocx_ctx* ctx, int32_t members, int32_t count, const double* scales);

/*
 * Hamiltonian sweeps: B seeds, each a system of its own with a pulse of its own (gate-time sweeps,
 * calibration families) - the complement of an ensemble, which drives M systems with one pulse.
 * Call after qocx_set_schroedinger_problem, whose LAST `fixed` = J control channels are the fixed
 * matrices D_j; K_r = control_count - J channels remain for the seeds. Seed b evaluates the problem
 * on the K-channel controls
 *     r_b[j][k] = s_bk u_b[j][k] (k < K_r),   r_b[j][K_r + i] = delta_bi (every knot)
 * i.e. H_b(u, t) = H(s_b . u, t) + sum_i delta_bi D_i. A duration T_b = tau_b T is the case where the
 * drift is the fixed channel D_0 = H0 of a problem with H0 = 0: delta_b0 = tau_b, s_bk = tau_b s_k.
 *   scales  [seeds][K_r] (NULL: all 1)   offsets [seeds][J] (NULL exactly when J = 0)
 * QOCX_ERR_ARG unless seeds >= 1, 0 <= J < control_count and every entry is finite; QOCX_ERR_STATE
 * while an ensemble or quadratic terms are set, and qocx_set_ensemble / qocx_set_quadratic_terms
 * return QOCX_ERR_STATE while a sweep is set. A new problem clears the sweep. Controls must be
 * uploaded afterwards.
 * With a sweep set:
 *   qocx_upload_controls(ctx, seeds, controls [seeds][Nc][K_r]) keeps the seed controls on the device
 *     and expands them into the items; any other batch size is QOCX_ERR_ARG. The squaring bounds are
 *     those of the expanded array, bit for bit: item b is the plain K-channel problem on r_b.
 *   qocx_eval_resident evaluates the items as any batch; cost_b is the item's cost and
 *     grad_b[j][k] = s_bk dc_b / dr[j][k] (k < K_r, one rounding).
 *   qocx_download_results (costs [B], gradients [B][Nc][K_r], final states [B][S][n]),
 *   qocx_download_costs, qocx_reduce_results, qocx_set_control_costs and qocx_opt_* (the basis,
 *     complex and L-BFGS calls included) act on the B seeds and their K_r channels; qocx_opt_clip
 *     takes max_norms [K_r] and bounds the items with max_norms_k max_b |s_bk| and max_b |delta_bi|.
 * qocx_sweep_download_sensitivities, after an evaluation with gradients (QOCX_ERR_STATE otherwise):
 *     scales_out [B][K_r]  dE_b / ds_bk     = sum_j u_b[j][k] dc_b / dr[j][k]
 *     offsets_out [B][J]   dE_b / ddelta_bi = sum_j dc_b / dr[j][K_r + i]
 *   (either may be NULL), each sum in the fixed order stated in qocx_sweep.hip: 64 partial sums over
 *   the knots l, l + 64, ... ascending, then a halving tree - independent of the launch.
 */
int qocx_set_sweep(qocx_ctx* ctx, int32_t seeds, int32_t fixed, const double* scales, const double* offsets);
int qocx_sweep_download_sensitivities(qocx_ctx* ctx, double* scales_out, double* offsets_out);

/*
 * Duration search of a sweep (minimum-time GRAPE): tau_b = T_b / T, seed b's duration in units of the
 * problem's evolution time, becomes one more optimised parameter of the seed. Call after qocx_set_sweep
 * (QOCX_ERR_STATE without a sweep) of a problem whose first fixed channel is the drift (J >= 1).
 *   tau          [B]      the starting durations; clipped to [tau_min, tau_max] on the device
 *   base_scales  [B][K_r] s0, the control scales before the factor tau (NULL: all 1)
 *   base_offsets [B][J]   delta0, the offsets before the factor tau; column 0, the drift, is 1
 *   0 < tau_min <= tau_max finite; time_weight >= 0 finite (QOCX_ERR_ARG otherwise, or for a
 *   non-finite entry)
 * The engine keeps tau, s0 and delta0 on the device and derives the sweep's tables there,
 *     scales_bk = tau_b s0_bk      offsets_bj = tau_b delta0_bj     (one product, one rounding each)
 * replacing those of qocx_set_sweep; the bounds qocx_opt_clip commits are those of tau_max, so they hold
 * for every tau the optimizer can reach. A new problem or a new qocx_set_sweep clears the search.
 * Controls must be uploaded afterwards.
 * With durations set:
 *   every evaluation adds time_weight tau_b to the cost of seed b, after the costs of the controls
 *     (one product, one sum); one with gradients also produces dE_b/dtau_b + time_weight, the chain
 *     rule through the tables in the fixed order stated in qocx_duration.hip
 *   qocx_opt_begin* allocates the optimizer state of tau (moments, best tau)
 *   qocx_opt_clip clips tau in place to the box and rewrites the tables before the seeds are expanded
 *   qocx_opt_step keeps tau of the improved seeds as their best and steps tau of the flagged seeds
 *     with the rule and learning rate of the controls (Adam / SGD are element-wise)
 *   qocx_opt_lbfgs_begin returns QOCX_ERR_STATE (the resident L-BFGS vectors do not hold tau)
 * qocx_sweep_download_durations: tau_out [B] the current (clipped) durations, tau_grad_out [B] the
 *   gradient of the last evaluation with gradients (QOCX_ERR_STATE without one); either may be NULL.
 * qocx_opt_download_best_durations: tau_out [B], tau at every seed's best evaluation so far.
 */
int qocx_sweep_set_durations(qocx_ctx* ctx, const double* tau, const double* base_scales,
                             const double* base_offsets, double tau_min, double tau_max, double time_weight);
int qocx_sweep_download_durations(qocx_ctx* ctx, double* tau_out, double* tau_grad_out);
int qocx_opt_download_best_durations(qocx_ctx* ctx, double* tau_out);

/* Optional: all system-step states of the last evaluation, [B][N][S][n] complex
 * (what save_intermediate_states persists, schroedingerdiscrete.py:395-402). */
int qocx_set_keep_step_states(qocx_ctx* ctx, int32_t keep); /* before the evaluation */
int qocx_download_step_states(qocx_ctx* ctx, double* states_out);

/*
 * Cotangents of the states supplied by the host, for Cost plugins whose derivative the engine
 * does not know (the reference obtains it from autograd, schroedingerdiscrete.py:412-416,
 * :429-432): bars [B][count][S][n] complex = d cost / d Re(psi) + i d cost / d Im(psi) of the
 * states at system steps steps[c] (1..N-1; N-1 = final states). They are added to the adjoint
 * sweep of every following evaluation of the same batch size; count = 0 clears them.
 */
int qocx_set_state_cotangents(qocx_ctx* ctx, int32_t batch, int32_t count, const int32_t* steps,
                              const double* bars);

/*
 * Lindblad path: B calls of _evaluate_lindblad_discrete (+ gradient), lindbladdiscrete.py:321-322,
 * :357-441. The device integrates the same master equation with a fixed-step DOP853 scheme
 * and its exact discrete adjoint (parity tolerances there).
 *   controls [B][Nc][K]; cost_out [B]; grad_out [B][Nc][K]; final_out [B][S][n][n] complex.
 * qocx_download_step_densities: [B][N][S][n][n] complex after qocx_set_keep_step_states(ctx, 1).
 */
int qocx_set_lindblad_problem(qocx_ctx* ctx, const qocx_lindblad_problem* problem);
/* The times at which a time-dependent Hamiltonian must be sampled for `subdivision` pieces per
 * system step: for every sub-interval [t_a, t_b] (uniform pieces cut at the control knots) the 12
 * DOP853 stage times t_a + c_i (t_b - t_a). times_out may be NULL to query *count_out. */
int qocx_lindblad_stage_times(double evolution_time, int32_t system_eval_count,
                              int32_t control_eval_count, int32_t control_count,
                              int32_t subdivision, double* times_out, int64_t capacity,
                              int64_t* count_out);
int qocx_eval_lindblad(qocx_ctx* ctx, int32_t batch, const double* controls, int32_t want_grad,
                       double* cost_out, double* grad_out, double* final_out);
int qocx_download_step_densities(qocx_ctx* ctx, double* densities_out);
/* Sub-intervals (12-stage DOP853 steps) the last qocx_eval_lindblad integrated, summed over its
 * seeds: the unit of the Lindblad kernel's work (bench.py prices its roofline with it). */
int qocx_lindblad_last_subintervals(qocx_ctx* ctx, int64_t* total);
/* The Lindblad twin of qocx_set_state_cotangents: bars [B][count][S][n][n] complex. */
int qocx_set_density_cotangents(qocx_ctx* ctx, int32_t batch, int32_t count, const int32_t* steps,
                                const double* bars);

/*
 * Hamiltonian ensembles on the Lindblad path (robust GRAPE under decoherence): the twin of
 * qocx_set_ensemble with its argument rules. Call after qocx_set_lindblad_problem, whose LAST `fixed`
 * = J control channels are the perturbation matrices D_j; K_r = control_count - J channels remain for
 * the seeds, and control_count = K_r + J <= QOCX_LINDBLAD_MAX_K as for any Lindblad problem. Member m
 * of seed b is the Lindblad problem with the Hamiltonian H(s_m . u_b, t) + sum_i delta_mi D_i; the
 * lindblad_data, initial densities and costs are the problem's. It is, bit for bit, the plain
 * (K_r + J)-channel problem on the expanded controls
 *     r[j][k] = s_mk u_b[j][k] (k < K_r),   r[j][K_r + i] = delta_mi (every knot).
 *   scales  [M][K_r] (NULL: all 1)   offsets [M][J] (NULL exactly when J = 0)   weights [M] >= 0
 * QOCX_ERR_ARG unless 1 <= M <= 1024, 0 <= J < control_count and every input is finite. A new
 * Lindblad problem clears the ensemble; setting one clears the resident controls, the results and
 * the costs of the controls (qocx_set_control_costs comes after it, for K_r channels).
 * With an ensemble set:
 *   qocx_eval_lindblad, qocx_lindblad_upload_controls, qocx_lindblad_download_results,
 *     qocx_lindblad_download_costs and qocx_lindblad_opt_* take and return the seeds: controls and
 *     gradients [B][Nc][K_r], costs [B] (qocx_lindblad_opt_clip: max_norms [K_r]). Final densities are
 *     those of the items, [B][M][S][n][n]; qocx_download_step_densities returns [B][M][N][S][n][n].
 *   An evaluation expands the seeds into the B x M items (item b * M + m) on the device. EVERY ITEM
 *     picks its own sub-division count, from the maxima |s_mk| max|u_bk| (k < K_r) and |delta_mj| -
 *     those of the expanded array -, so the items of one seed may run in different groups and no
 *     result depends on the batch neighbours. The items are evaluated as any batch, go back to item
 *     order and are reduced in member order:
 *       cost_b = sum_m w_m c_bm, grad_b[j][k] = sum_m w_m s_mk dc_bm / dr[j][k] (k < K_r).
 *   Costs of the controls act once per seed on the seeds' controls, after the reduction.
 *   qocx_set_density_cotangents (count > 0) is QOCX_ERR_STATE, and so is this call while cotangents
 *     are set.
 * qocx_lindblad_ensemble_download_members: the unweighted cost of every item of the last evaluation
 * (qocx_eval_lindblad or qocx_eval_lindblad_resident), [B][M]; QOCX_ERR_STATE without an ensemble.
 * Not built: per-member operators or targets, gradients with respect to delta or to the rates below
 * (a sweep has them: qocx_lindblad_sweep_download_sensitivities).
 */
int qocx_lindblad_set_ensemble(qocx_ctx* ctx, int32_t members, int32_t fixed, const double* scales,
                               const double* offsets, const double* weights);
int qocx_lindblad_ensemble_download_members(qocx_ctx* ctx, double* cost_out);

/* Per-member dissipation rates of the ensemble (an uncertain T1 / T2): member m decays with
 *     gamma_mi = rate_scales[m][i] * dissipators[i]      (one product, one rounding)
 * under the problem's operators, and is otherwise the member of qocx_lindblad_set_ensemble. Its
 * control-free generators, its rates and its norm bound are, bit for bit, those of the plain problem set
 * with dissipators = rate_scales[m] . dissipators - so is its sub-division count (item (b, m) reads
 * member m's bound), and so are its cost, gradient and densities. The seeds' results are reduced as
 * before; the gradient is with respect to the seeds' controls only.
 *   after qocx_lindblad_set_ensemble; rate_scales [M][L], L = operator_count; NULL clears the rates
 *   (members and operators are then not read).
 * QOCX_ERR_STATE without an ensemble, or on a problem set with stage tables (fixed_subdivision > 0: the
 * control-free generator then lives in per-stage tables - one set, not M). QOCX_ERR_ARG if members != M,
 * operators != operator_count, or an entry is non-finite or negative. qocx_set_lindblad_problem and
 * qocx_lindblad_set_ensemble both clear the rates (as qocx_set_ensemble clears the quadratic scales);
 * this call may be repeated. It clears the resident controls and the results, not the costs of the
 * controls. */
int qocx_lindblad_set_ensemble_rates(qocx_ctx* ctx, int32_t members, int32_t operators,
                                     const double* rate_scales);

/*
 * Lindblad sweeps: the twin of qocx_set_sweep on the Lindblad path - B seeds, each an open system of its
 * own with a pulse of its own (a gate-time sweep under T1 / T2, a calibration family). Call after
 * qocx_set_lindblad_problem, whose LAST `fixed` = J control channels are the fixed matrices D_j;
 * K_r = control_count - J channels remain for the seeds. Item b IS seed b, the plain problem on
 *     r_b[j][k] = s_bk u_b[j][k] (k < K_r),   r_b[j][K_r + i] = delta_bi (every knot)
 * and, with rate_scales, with the rates gamma_bl = rate_scales[b][l] * dissipators[l] (one product, one
 * rounding): its control-free generators, rates and norm bound are built by the function that builds the
 * plain problem's, so seed b is bit for bit the plain (K_r + J)-channel problem set with dissipators =
 * rate_scales[b] . dissipators on [s_b . u_b, delta_b] - cost, gradient (after the one product with
 * s_bk), densities and the sub-division count, which seed b picks from its own control maxima and bound.
 * A duration T_b = tau_b T is delta_b0 = tau_b on D_0 = H0 (a problem with H0 = 0), s_bk = tau_b s_k and
 * rate_scales[b][l] = tau_b c_bl: scaling the whole Lindbladian is scaling time.
 *   scales [seeds][K_r] (NULL: all 1)   offsets [seeds][J] (NULL exactly when J = 0)
 *   rate_scales [seeds][L], L = operator_count (NULL: every seed takes the problem's rates, and the
 *   kernels of a run without rates are launched)
 * QOCX_ERR_ARG unless 1 <= seeds <= 1024 (the rates tables' member limit), 0 <= J < control_count, every
 * entry is finite and every rate factor >= 0. QOCX_ERR_STATE while an ensemble is set (and
 * qocx_lindblad_set_ensemble / _set_ensemble_rates while a sweep is set), for rate_scales on a problem
 * with stage tables (fixed_subdivision > 0), and while density cotangents are set (they are refused with
 * a sweep set). A new problem clears the sweep; setting one clears the resident controls, the results
 * and the costs of the controls (qocx_set_control_costs comes after it, for K_r channels).
 * With a sweep set qocx_eval_lindblad, qocx_lindblad_upload_controls, qocx_eval_lindblad_resident,
 * qocx_lindblad_download_results / _costs, qocx_lindblad_opt_* (the basis, complex and L-BFGS calls
 * included) and qocx_set_control_costs act on the B seeds and their K_r channels; any other batch size
 * is QOCX_ERR_ARG. Final densities are [B][S][n][n], without a member axis.
 *
 * qocx_lindblad_sweep_download_sensitivities, after an evaluation with gradients whose seed controls
 * still stand (QOCX_ERR_STATE otherwise); each output may be NULL:
 *     scales_out [B][K_r]  dE_b / ds_bk     = sum_j u_b[j][k] dc_b / dr[j][k]
 *     offsets_out [B][J]   dE_b / ddelta_bi = sum_j dc_b / dr[j][K_r + i]
 *   in the summation order of qocx_sweep.hip (its kernels run here as they are), and
 *     rates_out [B][L]     dE_b / dc_bl, c_bl the factor of seed b's l-th rate (1 without rate_scales):
 *   the exact derivative of the discrete scheme on its frozen grid (qocx_lindblad_ratesens.hip, which
 *   states its summation order). rates_out is QOCX_ERR_STATE unless the evaluation was asked for them -
 *   qocx_lindblad_sweep_want_rate_sensitivities(ctx, 1) before it; the flag is cleared by a new problem
 *   or sweep - and EVERY piece of it ran two-sided: one final target-density cost and no step cost, 1 to 4
 *   operators, no stage tables, stage values that fit the memory (a piece that recomputes them has no
 *   stage cotangents to contract), and the knobs lindblad_two_sided (and lindblad_4t for n > 16) on.
 * Not built: rate sensitivities on the classic one-launch adjoint; per-seed operators, targets or
 * densities; optimising the duration itself.
 */
int qocx_lindblad_set_sweep(qocx_ctx* ctx, int32_t seeds, int32_t fixed, const double* scales,
                            const double* offsets, const double* rate_scales);
int qocx_lindblad_sweep_want_rate_sensitivities(qocx_ctx* ctx, int32_t on);
int qocx_lindblad_sweep_download_sensitivities(qocx_ctx* ctx, double* scales_out, double* offsets_out,
                                               double* rates_out);

/*
 * Duration search of a Lindblad sweep (minimum-time GRAPE under T1 / T2): tau_b = T_b / T becomes one
 * more optimised parameter of seed b, and seed b is tau_b times the WHOLE Lindbladian - Hamiltonian,
 * fixed channels and rates. Call after qocx_lindblad_set_sweep with per-seed rates. QOCX_ERR_STATE:
 * no sweep, no rates tables, a problem with stage tables (fixed_subdivision > 0), or a problem whose
 * own h0 is not zero - in a duration sweep the drift is the first fixed channel, so the control-free
 * part is the dissipator alone and scales with tau as a whole.
 *   tau              [B]      the starting durations; clipped to [tau_min, tau_max] on the device
 *   base_scales      [B][K_r] s0, the control scales before the factor tau (NULL: all 1)
 *   base_offsets     [B][J]   delta0, the offsets before the factor tau; column 0, the drift, is 1
 *   base_rate_scales [B][L]   c0, the rate factors before the factor tau (NULL: all 1); finite, >= 0
 *   0 < tau_min <= tau_max finite; time_weight >= 0 finite; J >= 1; L in 1 .. 4 (QOCX_ERR_ARG
 *   otherwise, or for a non-finite entry)
 * Once, on the host, the engine builds every seed's control-free generators, rates and norm bound at
 * tau = 1 (rates c0_bl gamma_l) as the plain setter builds its own, and keeps them on the device
 * beside tau, s0, delta0 and c0. From them it derives on the device
 *     scales_bk = tau_b s0_bk    offsets_bj = tau_b delta0_bj
 *     A0_b = tau_b A0_b(tau = 1)  gamma_bl = tau_b (c0_bl gamma_l)       (one product, one rounding each)
 * and on the host, from the tau that comes back with the control maxima, the same scales and offsets
 * and the bound tau_b ||L0_b(tau = 1)|| from which seed b's sub-division count follows. Against a
 * fixed-duration sweep at the same tau the search agrees to rounding, not bit for bit: there the rates
 * are (tau_b c0_bl) gamma_l and the generators are summed from them.
 * A new problem or a new qocx_lindblad_set_sweep clears the search; controls must be uploaded afterwards.
 * With durations set:
 *   every evaluation adds time_weight tau_b to the cost of seed b, after the costs of the controls
 *     (one product, one sum); one with gradients runs the rate sensitivities as well and produces
 *     dE_b/dtau_b + time_weight, the chain rule through scales, offsets and rate factors in the fixed
 *     order stated in qocx_lindblad_duration.hip. Where a piece of it cannot run two-sided (more
 *     than one cost, a step cost, stage values that do not fit) the evaluation fails with
 *     QOCX_ERR_STATE and leaves no gradient
 *   qocx_lindblad_opt_begin* allocates the optimizer state of tau (moments, best tau)
 *   qocx_lindblad_opt_clip clips tau in place to the box and rewrites the tables
 *   qocx_lindblad_opt_step keeps tau of the improved seeds as their best and steps tau of the flagged
 *     seeds with the rule and learning rate of the controls
 *   qocx_lindblad_opt_lbfgs_begin returns QOCX_ERR_STATE (the resident L-BFGS vectors do not hold tau)
 * qocx_lindblad_sweep_download_durations: tau_out [B] the current durations, tau_grad_out [B] the
 *   gradient of the last evaluation with gradients (QOCX_ERR_STATE without one); either may be NULL.
 * qocx_lindblad_opt_download_best_durations: tau_out [B], tau at every seed's best evaluation so far.
 */
int qocx_lindblad_sweep_set_durations(qocx_ctx* ctx, const double* tau, const double* base_scales,
                                      const double* base_offsets, const double* base_rate_scales,
                                      double tau_min, double tau_max, double time_weight);
int qocx_lindblad_sweep_download_durations(qocx_ctx* ctx, double* tau_out, double* tau_grad_out);
int qocx_lindblad_opt_download_best_durations(qocx_ctx* ctx, double* tau_out);

/* Per-kernel timing, measured with HIP events on the launch streams.
 * enable: 0 off, 1 every launch, 2 + k the launches of kernel k only (two events per timed launch
 * cost the evaluation 2-3 % when all ~45 launches of it carry them; bench.py times its roofline
 * kernel only inside the timed region). After evaluations, qocx_get_timing returns for kernel `which`
 * (0 pade_pq, 1 sweep, 2 krylov_grad, 3 scatter, 4 lu, 5 lindblad, 6 lindblad_combine) the launch
 * count and total ms
 * since the last reset. */
int qocx_set_timing(qocx_ctx* ctx, int32_t enable);
int qocx_get_timing(qocx_ctx* ctx, int32_t which, int64_t* launches, double* total_ms);
int qocx_reset_timing(qocx_ctx* ctx);

/* Seeds per memory chunk (0 = auto from free HBM) and number of time segments of the pipeline
 * (0 = auto: 8 for large evaluations; 1 = no overlap of the sweep with the other kernels). Results
 * do not depend on either. */
int qocx_set_chunk(qocx_ctx* ctx, int32_t seeds_per_chunk);
int qocx_set_pipeline(qocx_ctx* ctx, int32_t time_segments);

/*
 * Multi-GPU: one process per GPU; the seed axis is sharded by the caller, the summed
 * cost/gradient is one RCCL all-reduce (no reference counterpart: the reference is single
 * process).  unique_id is ncclUniqueId bytes (128) produced by rank 0.
 */
int qocx_comm_unique_id(uint8_t* id128);
int qocx_comm_init(qocx_ctx* ctx, const uint8_t* id128, int32_t rank, int32_t world);
int qocx_comm_allreduce_sum(qocx_ctx* ctx, double* buf_host, int64_t count);
/* The path's single collective, device resident: out[0] = sum over the seeds of the last
 * evaluation of the cost, out[1 ..] = sum over the seeds of the gradient ([nc][K]); the sums are
 * formed on the device (fixed order: deterministic), all-reduced over the ranks of the
 * communicator with ONE ncclAllReduce on the device buffer when allreduce != 0 (qocx_comm_init
 * must have run), and only 8 (1 + nc K) bytes travel to the host. count = 1 + nc * K, or 1 for
 * the cost alone. */
int qocx_reduce_results(qocx_ctx* ctx, int32_t allreduce, double* out, int64_t count);
int qocx_comm_allreduce_max(qocx_ctx* ctx, double* buf_host, int64_t count);
int qocx_comm_barrier(qocx_ctx* ctx);
int qocx_comm_destroy(qocx_ctx* ctx);

/*
 * Debug / unit-test entry points (used by tests/, not by the host package).
 *   qocx_debug_pade_factor: K1 on explicit generator matrices a [count][n][n] complex:
 *     q_out, lu_out [count][n][n] complex (row-major, lu = L\U of the row-permuted P),
 *     perm_out [count][n], dinv_out [count][n] complex (1/U_kk), s_out [count].
 *   qocx_debug_selftest: wave-level primitives (DPP reductions, MFMA layout); returns the
 *     number of failed checks in *failures.
 */
int qocx_debug_pade_factor(qocx_ctx* ctx, int32_t count, int32_t n, const double* a,
                           double* q_out, double* lu_out, int32_t* perm_out,
                           double* dinv_out, int32_t* s_out);
int qocx_debug_selftest(qocx_ctx* ctx, int32_t* failures, char* report, int32_t report_len);
/* Kernel-variant switches for A/B measurements in one process and for tests that pin a variant.
 * Every knob libqocx.so accepts selects between paths that give the same numbers to rounding;
 * no environment variable changes which kernels the product library runs. Known names:
 *   "sweep_impl"    1 (default): column-chain sweep (one wavefront per seed; best inside the
 *                   segmented pipeline of large batches); 3: blocked-inverse sweep (four wavefronts
 *                   per seed: compute | inverter L | loader | inverter U'; qocx_sweep3.hip), 1.5x
 *                   faster per step when the sweep has the chip to itself (<= 128 seeds). One
 *                   implementation serves all batch sizes of a context, so results stay bit
 *                   identical across batching.
 *   "sweep_one"     one state, n <= 32: the dedicated one-state kernel of qocx_sweep1.hip (0: the
 *                   one-state form of the column-chain sweep).
 *   "pade_order"    0 (default): Pade order 3 / 5 / 7 / 9 / 13 by the 1-norm of the step generator;
 *                   13: always [13/13], as the reference executes it (qocx_pade_orders).
 *   "action"        1 (default): one state, Hermitian H, 17 <= n <= 32, one final TargetStateInfidelity,
 *                   "pade_order" 0: matrix-free sweeps - exp(a) psi by the truncated Taylor series, no
 *                   factorisation (qocx_action.hip, qocx_action_degrees); 0: the Pade route;
 *                   2: as 1, and the same problems at 33 <= n <= 64 too (qocx_action4.hip: workgroups
 *                   of three / four waves). Opt-in: above n = 32 the values 0 and 1 launch exactly
 *                   what they always launched.
 *   "action_states" 0 (default): the matrix-free route takes one state per seed only. 2 .. 4
 *                   (QOCX_ACTION_MAX_STATES): the most states per seed that take it at 17 <= n <= 32,
 *                   where "action" admits the problem and the one cost is a COHERENT final
 *                   TargetStateInfidelity (one scalar for every state): a wave per state, the states'
 *                   generator cotangents summed before one contraction (qocx_action_states.hip). Any
 *                   other value is QOCX_ERR_ARG. Opt-in: at 0 every problem launches what it always
 *                   launched. n <= 16 and the wide route of "action" = 2 stay one-state.
 *   "action_costs"  0 (default): the matrix-free route needs the one final TargetStateInfidelity. 1: one
 *                   state, 17 <= n <= 32, where "action" admits the problem in every respect but the cost
 *                   set: any set of device descriptors (COHERENT, INCOHERENT, FORBID; final or step; one
 *                   or several) - the adjoint sweep carries the true cotangent, forward sweep first, then
 *                   the adjoint sweep (qocx_action_costs.hip). Any other value is QOCX_ERR_ARG. Opt-in: at
 *                   0 every problem launches what it always launched, and the single final target keeps
 *                   its kernels at 1 too. Several states, n <= 16 and n > 32 stay on the Pade route.
 *   "action_degree" 1 (default): the Taylor degree of a step of the matrix-free route (every kernel file of
 *                   it) is the lesser of the Al-Mohy-Higham degree of the 1-norm bound |dt| (||H0||_1 +
 *                   sum |u_k| ||G_k||_1) and the degree at which the Lagrange remainder beta^(m+1) / (m+1)!
 *                   of a NORMAL generator is below 2^-53, beta = |dt| (rho(H0) + sum |u_k| rho(G_k)) from
 *                   upper bounds of the spectral radii (qocx_debug_spectral_bound, qocx_debug_action_degree)
 *                   - never more terms than the 1-norm alone asks for; the headline runs degree 8 instead
 *                   of 11. 0: the 1-norm alone, bit for bit what the route computed before the knob
 *                   existed. Any other value is QOCX_ERR_ARG. Pade orders and squarings stay on the 1-norm.
 *   "action_plan"   1 (default): in the two-sided pipeline each sweep of the matrix-free route runs to the
 *                   crossing of the two as ONE launch (nothing is factored on this route, so its segment
 *                   boundaries there buy nothing) and in pieces from there on; 0: one launch per piece, as
 *                   before the knob existed. The same bits. Any other value is QOCX_ERR_ARG.
 *   "action_small"  0 (default): n <= 16 stays on the Pade route. 1: one state, Hermitian H, n <= 16, every
 *                   other condition of "action" (one final TargetStateInfidelity, "pade_order" 0, not latency
 *                   mode, bound <= theta_18): matrix-free sweeps there too (qocx_action16.hip: one wave per
 *                   seed, its four rows of 16 lanes the four real products of a complex one), decided before
 *                   and independent of "sweep_inverse_small", "pack8" and "sweep_umode". Any other value is
 *                   QOCX_ERR_ARG. Opt-in: at 0 every problem launches what it always launched; no effect
 *                   above n = 16; "action_states" and "action_costs" stay at 17 <= n <= 32.
 *   "action_eff"    0 (default): a problem on EFFECTIVE controls - MAGNUS_M4 on a time-independent system, or
 *                   quadratic terms (qocx_set_quadratic_terms) under M2 - stays on the Pade route. 1: one
 *                   state, every operator Hermitian (the Q_q included), every other condition of "action" (one
 *                   final TargetStateInfidelity, "pade_order" 0, not latency mode, bound <= theta_18): the
 *                   matrix-free sweeps run on its Ke effective controls over the augmented operators
 *                   (qocx_action_eff.hip: one kernel writes them and the Taylor degree of every step, from the
 *                   norms of the augmented operators), on the kernels its size selects - 17 <= n <= 32 where
 *                   "action" is not 0, n <= 16 only with "action_small" = 1, 33 <= n <= 64 only with "action" =
 *                   2 -, and the chain kernel folds the Ke step cotangents back. Any other value is
 *                   QOCX_ERR_ARG. Opt-in: at 0 every problem launches what it always launched. Several states,
 *                   step costs or several costs ("action_states", "action_costs" do not combine with it), M6, M4
 *                   on a time-dependent system and explicit generators keep their routes.
 *   "action_eff_exact" 1 (default): with "action_eff", 17 <= n <= 32 and Ke = 5 (M4 with two controls) the
 *                   sweep holds all five operator images in registers; 0: the build that streams every image
 *                   past the second from memory at every step, as every other Ke > 2 does. The same numbers to
 *                   rounding; kept for the measurement (tools/bench_action_effective.py). 0 or 1.
 *   "unit_adjoint"  one final TargetStateInfidelity: the adjoint sweep back-propagates the targets.
 *   "bidir"         with it: forward and adjoint sweep side by side, factorisation from both ends.
 *   "fuse_lu"       17 <= n <= 32: the LU factorisation runs inside the Pade kernel;
 *   "lu_mfma"       (round 4) ... and takes its Schur updates to the matrix cores (qocx_lu4.h).
 *   "lu_dpp"        diagonally dominant Pade denominators (every step of the evaluation): the
 *                   factorisations without pivot search (qocx_lu5.h).
 *   "k1a_three"     17 <= n <= 32, orders 3 and 5: the three-wave K1a (qocx_pade3.hip); "k1a_share":
 *                   which generator tiles it takes from LDS; "k1a_four" (default 0): the second
 *                   halves of its factorisations four to a wave behind it (1) or on a side stream (2).
 *   "k1a_herm4": four-wave K1a, Hermitian generators, orders 3..9: two thirds of the tiles (0: all tiles).
 *   "latency"       0 (default; the host sets 1 for entry points that evaluate ONE control set):
 *                   two time segments, the inverse-image sweep.
 *   "sweep_inverse" latency mode: sub-steps as two matrix-vector products with P^-1 (qocx_sweepi.hip);
 *   "sweep_inverse_small": the same sweep for every batch at n <= 16; "pack8": n <= 8, two steps
 *                   of a seed as the diagonal blocks of one 16 x 16 tile through K1a and K1b;
 *   "sweep_umode": latency mode, the propagator U = P^-1 Q in the Q image, one product per sub-step.
 *   "sweep_dense"   8 <= S <= 32 states at 17 <= n <= 32 as MFMA GEMM columns (qocx_sweepd.hip);
 *                   "lu_inverse": the debug factor entry point returns P^-1.
 *   "m4_linear"     MagnusPolicy.M4 with time-independent H0, G_k on the M2 kernels (commutators
 *                   hoisted into constant matrices); "magnus_4w": four-wave LDS-resident Magnus
 *                   kernels at 17 <= n <= 32.
 *   "general_split", "general_skew": n > 64 (qocx_general.hip): the many-state sweep in groups of
 *                   rows on several workgroups; the Krylov chains of Hermitian generators.
 *   "lindblad_two_sided", "lindblad_side_limit": forward and unit-adjoint Lindblad passes side by side.
 *   "lindblad_q2": their stage loop with 18 of the 72 MFMAs of a right-hand side per wave (0: the quarter-split loops);
 *   "lindblad_chain", "lindblad_real_ops": the chained stage loop of several jump operators; real operators
 *                   as two real products per complex one.
 *   "lindblad_4t": Lindblad at 17 <= n <= 32 on the tile-per-wave kernel where it applies (0: one wave per seed).
 *   "lindblad_hermitian": that kernel's shorter stages for Hermitian problems (Y A_R = (A_L Y)^H; 0: the general stages).
 *   "lindblad_pad_operator": Lindblad with ONE operator at n <= 16 on the four-wave launches of two (the second zero);
 *                   read when the problem is set (0: the three-wave form).
 *   "lindblad_wide": 1: qocx_set_lindblad_problem takes 33 <= hilbert_size <= 64 (the sixteen-wave kernel of
 *                   qocx_lindblad16t.hip: one workgroup per seed, the classic launch, 0..8 operators); read when the
 *                   problem is set. Default 0: hilbert_size > 32 is refused as ever. Above 32 stage tables
 *                   (fixed_subdivision > 0, h0_stages, g_stages, op_stages), per-member and per-seed rates
 *                   (qocx_lindblad_set_ensemble_rates, rate_scales of qocx_lindblad_set_sweep), per-seed durations
 *                   (qocx_lindblad_sweep_set_durations) and rate sensitivities are refused by name: each has kernels
 *                   of its own at n <= 32, and nothing runs two-sided. Ensembles and sweeps without rates, density
 *                   cotangents, step densities and the qocx_lindblad_opt_* family work as at n <= 32.
 * Diagnostic knobs - libqocx_diag.so only (make diag, -DQOCX_DIAG; the product library answers
 * QOCX_ERR_ARG): "dbg_skip", "sweep3_dbg", "k1a_dbg" switch parts of an evaluation off for timing
 * (results are garbage); "sweep3_stamps", "lindblad_stamps", "k1a_stamps" run kernel builds that
 * execute in-kernel clock stamps (qocx_debug_read_stamps). The diagnostic library also reads the
 * QOCX_* environment switches of earlier experiments (qoc_amd/csrc/qocx_diag.h). */
int qocx_debug_set_knob(qocx_ctx* ctx, const char* name, int64_t value);
/* 1: a variant knob (every build), 2: a diagnostic knob this library accepts, -2: a diagnostic
 * knob this (product) library rejects, 0: unknown. No context, no GPU needed. */
int qocx_knob_kind(const char* name);
/* 1 for libqocx_diag.so, 0 for the product library. */
int qocx_build_is_diag(void);
/* After evaluations with the knob "sweep3_stamps" = 1 (a diagnostic build of the sweep that
 * executes in-kernel clock stamps; never the product kernel): per seed, per role (compute |
 * inverter L | loader | inverter U'), 8 sums - shader-clock cycles per phase of the role's step loop, [7] = the
 * 100 MHz real-time counter over the role's life. out: [batch][4][8]. */
int qocx_debug_read_stamps(qocx_ctx* ctx, uint64_t* out, int64_t count);
/* Pade orders of the last Schroedinger evaluation (its last memory chunk): counts[0..4] = number of
 * propagator steps evaluated with the [3/3], [5/5], [7/7], [9/9], [13/13] approximant. The engine
 * takes the order from the 1-norm of the step generator by the thresholds of Higham 2005,
 * Algorithm 2.3 - the table /root/reference/qoc/standard/functions/expm.py:194-209 carries; the
 * reference itself always evaluates [13/13] (expm.py:230-233: its selection loop has no break),
 * which the knob "pade_order" = 13 reproduces. Same matrix and same derivative to rounding.
 * These are bits 8..15 of the step table's entries: the table's classification of the steps, and
 * what the Pade route executes. An evaluation on the matrix-free route (qocx_action_degrees) forms
 * no approximant; the counts then say what the Pade route would have taken. */
int qocx_pade_orders(qocx_ctx* ctx, int64_t* counts);
/* Taylor degrees the last Schroedinger evaluation executed on the matrix-free route (one state,
 * Hermitian H, 17 <= n <= 32 - with knob "action" = 2 up to n = 64 -, one final TargetStateInfidelity;
 * qoc_amd/csrc/qocx_action.hip, qocx_action4.hip): counts[m], m = 1 .. 18, = propagator steps whose exp(a) psi was the degree-m
 * truncated Taylor series (Al-Mohy & Higham 2011: the least m with ||a||_1 <= theta_m; with knob
 * "action_degree" = 1, the default, no more than the normal generator's remainder needs), summed over
 * every seed of the evaluation. All 19 entries are zero when the evaluation took the Pade route. */
int qocx_action_degrees(qocx_ctx* ctx, int64_t* counts);
/* Evaluations of this context the matrix-free route handed back to the Pade route because a step's
 * degree, decided on the device, was beyond the buffers the host had sized from its norm bound
 * (stale after qocx_opt_step). The results are those of the Pade route. */
int qocx_action_reruns(qocx_ctx* ctx, int64_t* count);
/* The two host functions behind the degrees of the matrix-free route; no context, no GPU call.
 * qocx_debug_spectral_bound: m is a HERMITIAN n x n matrix (complex row-major, 1 <= n <= 64); *bound is an
 * upper bound of its spectral radius rho (= ||m||_2), rho <= *bound <= 1.01 rho, by eight normalised
 * squarings (rho <= ||m^256||_F^(1/256) <= n^(1/512) rho); 0 for the zero matrix, NaN where an entry is
 * not finite. The engine takes it of H0 and every G_k when a problem is set.
 * qocx_debug_action_degree: the degree of a step whose generator a has ||a||_1 <= bound1 and
 * ||a||_2 <= bound2. rule 0: the least m in 1 .. 18 with bound1 <= theta_m (Al-Mohy & Higham 2011), 19
 * above theta_18 and for NaN. rule 1 (knob "action_degree", the default): the lesser of that and the least
 * m with bound2^(m+1) / (m+1)! <= 2^-53 - the Lagrange remainder of e^(i lambda), which bounds the
 * truncation error of T_m(a) psi for a NORMAL a (a = -i dt H, H Hermitian) - 19 above theta'_18 and for NaN. */
int qocx_debug_spectral_bound(const double* m, int32_t n, double* bound);
int qocx_debug_action_degree(double bound1, double bound2, int32_t rule, int32_t* degree);
/* What decides whether an evaluation takes the matrix-free route, and on which kernels
 * (qoc_amd/csrc/qocx_action_route.h: action_plan - the engine fills these from its context once per
 * evaluation): the problem, what the problem setter left on the device, the host's norm bounds and the
 * knobs above, by their names. Flags are 0 / 1. */
typedef struct qocx_action_facts {
    int32_t n, S, K;           /* Hilbert size, states per seed, real controls */
    int32_t nt;                /* time samples of the operators (1: a time-independent system) */
    int32_t nodes;             /* nodes of the generator kernels (1: M2, and M4 on effective controls) */
    int32_t eff_kind;          /* effective controls: 0 none, 1 M4-linear, 2 quadratic ... */
    int32_t Ke;                /* ... and how many per step */
    int32_t hermitian;         /* every operator is exactly Hermitian */
    int32_t unit_ok;           /* the cost set is one final TargetStateInfidelity with one scalar for all states */
    int32_t has_step_costs, cost_count;
    int32_t inj_count;         /* externally supplied state cotangents (qocx_set_state_cotangents) */
    int32_t keep_step_states;  /* qocx_set_keep_step_states */
    int32_t explicit_gen;      /* generators sampled by the host (qocx_upload_generators) */
    int32_t dense;             /* the dense-state sweep serves the problem ("sweep_dense") */
    int32_t one_wave_k1a;      /* diagnostic library only: the one-wave K1a, which knows no step table */
    int32_t latency;           /* knob "latency" */
    int32_t have_norms;        /* ||G_k||_1 of the operators are on the device */
    int32_t have_eff_norms;    /* both norms of the augmented operators of effective controls are */
    int32_t have_e_img;        /* the images E = -i dt G of the operators the gradient contracts with are */
    double bound1, bound1_mid; /* the host's bounds of ||a||_1 of a step: over the knots, at the step midpoints */
    double bound2, bound2_mid; /* ... and of ||a||_2 */
    int32_t action, action_states, action_costs, action_small, action_eff, action_eff_exact;
    int32_t action_degree, action_plan, pade_order, unit_adjoint;  /* the knobs' values */
    int32_t allow;             /* 0: the evaluation is the rerun after a step's degree was beyond the buffers */
} qocx_action_facts;
/* qocx_debug_action_route: the route decision itself; no context, no GPU call. *kernel: 0 the Pade route,
 * 1 qocx_action.hip, 2 the Ke = 5 sweep of qocx_action_eff.hip (gradient: qocx_action.hip), 3
 * qocx_action_states.hip, 4 qocx_action_costs.hip, 5 qocx_action16.hip, 6 qocx_action4.hip. *table: 0
 * launch_step_table, 1 the table of qocx_action_eff.hip. *m_max: the Taylor terms per step the buffers
 * hold (0 on the Pade route). */
int qocx_debug_action_route(const qocx_action_facts* facts, int32_t* kernel, int32_t* table, int32_t* m_max);
/* What decides the kernels of a Lindblad evaluation and whether it runs two-sided
 * (qoc_amd/csrc/qocx_lindblad_route.h: lindblad_form when a problem is set, lindblad_route once per
 * evaluation - the engine fills these from its context): the problem, the evaluation, and the knobs above by
 * their names. Flags are 0 / 1. */
typedef struct qocx_lindblad_facts {
    int32_t n, S, K, nops;         /* Hilbert size, densities per seed, real controls, Lindblad operators */
    int32_t stage_tables;          /* the problem was set with stage tables (fixed_subdivision > 0) ... */
    int32_t g_tables, op_tables;   /* ... among them time-dependent G_k (g_stages), operators (op_stages) */
    int32_t hermitian;             /* H0, G_k, sum gamma L^H L, initial densities and cost matrices are Hermitian */
    int32_t ops_real;              /* every Lindblad operator has a zero imaginary part */
    int32_t unit_ok;               /* the cost set is one final target-density infidelity */
    int32_t inj_count;             /* host-supplied density cotangents (qocx_set_density_cotangents) */
    int32_t want_grad;
    int32_t rates;                 /* per-member or per-seed rates (rate_scales) */
    int32_t sweep;                 /* a sweep is set (qocx_lindblad_set_sweep) ... */
    int32_t want_rate_sens;        /* ... which asked for rate sensitivities, or searches its durations */
    int32_t side_streams;          /* streams beside the context's own */
    int32_t cu_count;
    int32_t dbg_wave_mode;         /* qocx_debug_lindblad_knobs */
    int32_t lindblad_4t, lindblad_two_sided, lindblad_hermitian, lindblad_q2, lindblad_chain;
    int32_t lindblad_real_ops, lindblad_pad_operator, lindblad_side_limit, lindblad_stamps;  /* the knobs' values */
    int32_t single_wave;           /* diagnostic library only: the environment switch QOCX_LINDBLAD_SINGLE_WAVE */
} qocx_lindblad_facts;
/* qocx_debug_lindblad_route: the form and the route of these facts; no context, no GPU call. kernels[3]: the
 * kernel of the classic launch, of the forward and of the adjoint launch of a two-sided piece - 0 none, 1 one
 * wave in LDS, 2 one wave with scratch, 3 one wave at 17 <= n <= 32, 4 nops + 2 waves, 5 four waves, 6 four
 * waves q2, 7 four waves chain, 8 tile-per-wave, 9 its Hermitian build, 10 the sixteen-wave kernel of
 * 33 <= n <= 64. *multi_wave: pieces run several waves per seed; *two_sided: a piece that keeps its stage
 * values runs as forward launch, adjoint launch and combine; *rate_sens: such an evaluation delivers rate
 * sensitivities. form[4]: scratch, pad_op, multi_wave, cache_gen as the problem setter stores them. */
int qocx_debug_lindblad_route(const qocx_lindblad_facts* facts, int32_t* kernels, int32_t* multi_wave,
                              int32_t* two_sided, int32_t* rate_sens, int32_t* form);
/* qocx_debug_lindblad_pieces: the piece schedule of one group of `seeds` seeds with `per_seed` stage elements
 * each (lindblad_group_pieces of the same header) under a stage budget in elements, the values of
 * qocx_debug_lindblad_knobs and the CU count; no context, no GPU call. counts / keep_stages / multi_wave
 * receive up to `capacity` pieces in launch order, *pieces how many there are, *sized_for the seeds the stage
 * buffers are sized for (0: no piece keeps its stage values). */
int qocx_debug_lindblad_pieces(int32_t want_grad, int32_t multi_wave, int64_t stage_budget,
                               int64_t stage_budget_seeds, int32_t min_piece, int32_t wave_mode, int32_t cu_count,
                               int32_t seeds, int64_t per_seed, int32_t capacity, int32_t* counts,
                               int32_t* keep_stages, int32_t* piece_multi_wave, int32_t* pieces, int64_t* sized_for);
/* Matrices of the last Schroedinger evaluation (or qocx_debug_pade_factor call) whose LU factorisation
 * left the diagonal-pivot form with MFMA Schur updates (knob "lu_mfma"; qoc_amd/csrc/qocx_lu4.h,
 * qocx_lu4m.hip) for the general partial-pivoting elimination: LAPACK's pivot rule asked for a row
 * interchange somewhere. 0 for the Pade denominators of well-scaled generators. */
int qocx_lu_fallbacks(qocx_ctx* ctx, int64_t* count);
/* With qocx_set_timing on: the kernel launches of the LAST evaluation as (which, start_ms, end_ms)
 * triples relative to its first launch (HIP events on the launch streams; which = the index of
 * qocx_get_timing: 0 K1a, 1 sweep, 2 K3, 3 scatter, 4 K1b, 5 Lindblad, 6 its combine kernel). out
 * holds up to `capacity`
 * triples, *count receives how many there were. A view of how the pipeline overlaps. */
int qocx_debug_timeline(qocx_ctx* ctx, double* out, int64_t capacity, int64_t* count);
/* Force the variants of the Lindblad launch that large batches / little free HBM select:
 *   stage_budget_seeds  seeds whose forward stage values may be kept for the adjoint (0: as many
 *                       as fit 45 % of free HBM); a larger group is launched in pieces;
 *   min_piece           below this many seeds per piece the adjoint recomputes the stage values
 *                       from the checkpoints instead (default 256);
 *   wave_mode           0 auto (several waves per seed, batches beyond the CU count in rounds of
 *                       one seed per CU), 1 one wave per seed, 2 several waves per seed in ONE
 *                       launch whatever the batch size.
 * Results do not depend on any of them (tests/test_gpu_lindblad.py). */
int qocx_debug_lindblad_knobs(qocx_ctx* ctx, int64_t stage_budget_seeds, int32_t min_piece,
                              int32_t wave_mode);
/* Sustained FP64 MFMA rate of the device: waves_per_simd x 4 x CUs waves issue `iters` rounds of
 * 8 independent v_mfma_f64_16x16x4_f64 from registers (no memory traffic). bench.py reports it
 * next to the spec peak. */
int qocx_debug_mfma_peak(qocx_ctx* ctx, int32_t waves_per_simd, int32_t iters, double* tflops);

/* ---- multi-start GRAPE with the optimizer states resident on the device ------------------------
 * The reference's driver iteration - clip the controls, evaluate, keep the best so far, apply the
 * optimizer (qoc/core/schroedingerdiscrete.py:293-353, common.py:8-30, optimizers/adam.py:110-165,
 * sgd.py) - for the B control sets that qocx_upload_controls left in HBM, without a trip to the host:
 * per iteration 8 B bytes of costs come back, B flags go in. Real controls, built-in Adam / SGD
 * (no scale_grads). IEEE operations in the reference's order, no contraction: every seed walks its
 * single-seed trajectory bit for bit.
 *   qocx_opt_begin          after qocx_upload_controls: zero the Adam moments, allocate the
 *                           best-so-far buffers for the current batch.
 *   qocx_opt_clip           clip_control_norms on the resident controls, in place; the squaring
 *                           capacity of the next evaluation is re-derived from max_norms [K].
 *   qocx_download_costs     the B costs of the last evaluation.
 *   qocx_opt_step           improved[b] != 0: best controls / final states of seed b := those of the
 *                           last evaluation; then update[b] != 0: seed b takes the optimizer step
 *                           (kind 0 SGD, 1 Adam) with the gradients of the last evaluation;
 *                           corr_i = 1 - beta_i^step and the learning rate are the caller's scalars.
 *   qocx_opt_download_best  best controls [B][Nc][K] and best final states [B][S][n] complex. */
int qocx_opt_begin(qocx_ctx* ctx);
int qocx_opt_clip(qocx_ctx* ctx, const double* max_norms);
int qocx_download_costs(qocx_ctx* ctx, double* cost_out);
int qocx_opt_step(qocx_ctx* ctx, int32_t kind, const uint8_t* improved, const uint8_t* update,
                  double learning_rate, double beta_1, double beta_2, double epsilon, double corr_1,
                  double corr_2, int32_t apply_clip_grads, double clip_grads);
int qocx_opt_download_best(qocx_ctx* ctx, double* controls_out, double* final_out);

/* ---- the same driver for the Lindblad problem --------------------------------------------------
 * Multi-start Lindblad GRAPE (qoc/core/lindbladdiscrete.py:297-352 per seed) with controls, results,
 * Adam moments and the best so far in HBM, apart from the Schroedinger state of the qocx_opt_* family
 * (a context may hold both problems). The contract is that of qocx_opt_*; every array is in seed
 * order. An evaluation is that of qocx_eval_lindblad on the same controls, bit for bit: each seed
 * takes its sub-division count from the maxima |u_k| of ITS controls, seeds with equal counts run as
 * one group, and the results go back to seed order on the device.
 *   qocx_lindblad_upload_controls    controls [B][Nc][K] real into HBM (a problem with K >= 1).
 *   qocx_eval_lindblad_resident      evaluate the resident controls (cost, gradients if want_grad,
 *                                    final densities); no wait for the device.
 *   qocx_lindblad_download_results   cost [B], gradients [B][Nc][K], final densities [B][S][n][n]
 *                                    complex of the last resident evaluation; any pointer may be NULL.
 *   qocx_lindblad_download_costs     the B costs alone (what the driver polls).
 *   qocx_lindblad_opt_begin          zero the Adam moments, allocate the best-so-far buffers.
 *   qocx_lindblad_opt_clip           clip_control_norms on the resident controls, in place; the
 *                                    per-seed control maxima of the next evaluation's sub-division
 *                                    come back with it (B K doubles; none on a fixed grid).
 *   qocx_lindblad_opt_step           as qocx_opt_step: best controls / final densities of the flagged
 *                                    seeds, then the SGD (kind 0) / Adam (kind 1) update.
 *   qocx_lindblad_opt_download_best  best controls [B][Nc][K] and best final densities [B][S][n][n]
 *                                    complex. */
int qocx_lindblad_upload_controls(qocx_ctx* ctx, int32_t batch, const double* controls);
int qocx_eval_lindblad_resident(qocx_ctx* ctx, int32_t want_grad);
int qocx_lindblad_download_results(qocx_ctx* ctx, double* cost_out, double* grad_out,
                                   double* final_out);
int qocx_lindblad_download_costs(qocx_ctx* ctx, double* cost_out);
int qocx_lindblad_opt_begin(qocx_ctx* ctx);
int qocx_lindblad_opt_clip(qocx_ctx* ctx, const double* max_norms);
int qocx_lindblad_opt_step(qocx_ctx* ctx, int32_t kind, const uint8_t* improved,
                           const uint8_t* update, double learning_rate, double beta_1,
                           double beta_2, double epsilon, double corr_1, double corr_2,
                           int32_t apply_clip_grads, double clip_grads);
int qocx_lindblad_opt_download_best(qocx_ctx* ctx, double* controls_out, double* final_out);

/* ---- costs of the controls alone, on the device ------------------------------------------------
 * The reference's ControlNorm, ControlVariation, ControlArea and ControlBandwidthMax
 * (qoc/standard/costs/controlnorm.py:48-73, controlvariation.py:47-75, controlarea.py:43-67,
 * controlbandwidthmax.py:52-77) and their gradients for the control sets resident in HBM, so that the
 * multi-start drivers above keep pulse-shaping penalties off the host. `path` names the problem of
 * the context they belong to. K controls; with complex_controls != 0 control k is the real channels
 * 2k (Re) and 2k + 1 (Im) of the problem, K = channels / 2, and gradients are d/dRe, d/dIm in those
 * channels. With an ensemble set the channels are the seeds' K_r. */
#define QOCX_PATH_SCHROEDINGER 0
#define QOCX_PATH_LINDBLAD 1
#define QOCX_CONTROL_NORM 0          /* multiplier * sum |u_jk / max_k * w_k|^2                      */
#define QOCX_CONTROL_VARIATION 1     /* multiplier * sum |order-th forward difference of u_k / max_k|^2 */
#define QOCX_CONTROL_AREA 2          /* multiplier * sum_k |sum_j u_jk / max_k|                      */
#define QOCX_CONTROL_BANDWIDTH_MAX 3 /* multiplier * sum_k sum_P |X_f| / (|P_k| max_P |X_f|), X = DFT(u_k) */

typedef struct qocx_control_cost_desc {
    int32_t kind;            /* QOCX_CONTROL_*                                                      */
    int32_t order;           /* VARIATION: 1 <= order < Nc                                          */
    double multiplier;       /* cost_multiplier with the normalisation constant of the cost folded in:
                                / (Nc K), / (K (Nc - order) 2^order), / (Nc K), / K                  */
    const double* max_norms; /* [K] max_control_norms, or NULL (none; AREA needs them)              */
    const double* weights;   /* NORM: [K] control_weights, or NULL                                  */
    const int32_t* bins;     /* BANDWIDTH_MAX: the DFT bins f with fftfreq(Nc, dt)[f] >= max_bandwidths[k], */
    const int32_t* bin_ptr;  /*   ascending per control: P_k = bins[bin_ptr[k] .. bin_ptr[k + 1]), [K + 1]  */
} qocx_control_cost_desc;

/* Set (count > 0) or clear (count = 0) the control costs of a path. Call after the qocx_set_*_problem
 * of that path (and after qocx_set_ensemble), which clear them. QOCX_ERR_ARG for a problem without
 * controls, an odd channel count with complex_controls, an unknown kind, `order` out of range, an
 * empty or out-of-range P_k, AREA without max_norms, or non-finite inputs.
 * With control costs set, qocx_eval_resident (after the ensemble reduction: once per seed, on the
 * seed's unscaled controls) and qocx_eval_lindblad_resident add their sum to every seed's cost and
 * - with gradients - its gradient to the seed's gradient, one addition per entry; what
 * qocx_download_costs / _results, qocx_reduce_results, qocx_opt_step and the Lindblad twins see are
 * the totals. qocx_eval_schroedinger and qocx_eval_lindblad (host buffers in and out) do not add them. */
int qocx_set_control_costs(qocx_ctx* ctx, int32_t path, int32_t complex_controls, int32_t count,
                           const qocx_control_cost_desc* descs);
/* The control costs alone: controls [batch][Nc][channels] on the host in, their sum cost_out [batch]
 * and its gradient grad_out [batch][Nc][channels] (NULL: none) out. A seed's numbers do not depend on
 * the batch it is part of. */
int qocx_eval_control_costs(qocx_ctx* ctx, int32_t path, int32_t batch, const double* controls,
                            double* cost_out, double* grad_out);
/* Complex controls in the resident drivers. The reference clips a COPY of complex controls
 * (common.py:8-30 on the array slap_controls builds, :201-223) and its optimizer keeps the unclipped parameters. Begun
 * with these instead of qocx_opt_begin / qocx_lindblad_opt_begin, the driver keeps the parameters
 * apart from the evaluated controls: *_opt_clip takes max_norms [K = channels / 2] and writes the
 * parameters, clipped by modulus hypot(Re, Im), into the evaluation buffer; *_opt_step updates the
 * parameters; the best so far are the clipped controls that were evaluated. */
int qocx_opt_begin_complex(qocx_ctx* ctx);
int qocx_lindblad_opt_begin_complex(qocx_ctx* ctx);

/* ---- L-BFGS in the resident drivers -------------------------------------------------------------
 * Limited-memory BFGS with an Armijo backtracking line search for every seed of the resident batch,
 * its state in HBM (qocx_lbfgs.hip). qoc_amd/standard/optimizers/lbfgs.py states the algorithm as a
 * per-seed state machine that consumes one (parameters, error, gradients) triple per evaluation and
 * gives the next trial point; the kernel does the same arithmetic - every product and sum rounded on
 * its own, IEEE division and square root, every inner product in that file's one defined order - so a
 * seed walks the host loop's trajectory bit for bit, whatever the batch.
 *   *_opt_lbfgs_begin  after *_opt_begin / *_opt_begin_complex: allocate and zero the state of the
 *                      current batch with P = Nc * channels parameters per seed: accepted point,
 *                      its gradient, the direction, `history` pairs (s, y, rho) and the scalars.
 *                      QOCX_ERR_ARG for history outside 1..64, QOCX_ERR_CAPACITY if the state does
 *                      not fit the free device memory.
 *   *_opt_lbfgs_step   improved[b] != 0: best controls / final states of seed b := those of the last
 *                      evaluation (as *_opt_step). Then, for update[b] != 0, seed b's state machine
 *                      takes the last evaluation's total cost and gradient (with an ensemble the
 *                      reduced ones; control costs included) and the trial point goes into the
 *                      resident parameters. finished_out [B]: 1 for a seed whose steepest-descent
 *                      direction has run out of backtracks - its parameters are back at its last
 *                      accepted point and it takes no further steps. */
int qocx_opt_lbfgs_begin(qocx_ctx* ctx, int32_t history);
int qocx_opt_lbfgs_step(qocx_ctx* ctx, const uint8_t* improved, const uint8_t* update,
                        double first_step, double armijo, double shrink, int32_t max_backtracks,
                        uint8_t* finished_out);
int qocx_lindblad_opt_lbfgs_begin(qocx_ctx* ctx, int32_t history);
int qocx_lindblad_opt_lbfgs_step(qocx_ctx* ctx, const uint8_t* improved, const uint8_t* update,
                                 double first_step, double armijo, double shrink,
                                 int32_t max_backtracks, uint8_t* finished_out);

/* ---- a control basis in the resident drivers ------------------------------------------------------
 * The optimizer's parameters are P coefficients per control channel, the evaluated pulse is their image
 * under a real matrix M [Nc][P]: u[b][j][c] = sum_p M[j][p] coef[b][p][c] (qocx_ctrlbasis.hip;
 * qoc_amd/standard/controlbasis.py states the arithmetic). Both directions run in one defined order -
 * the expansion over p = 0 .. P-1, the projection h[b][p][c] = sum_j M[j][p] g[b][j][c] over
 * j = 0 .. Nc-1, acc = acc + M * x from +0.0, the product and the sum each rounded on its own - so a
 * seed walks the host loop's trajectory bit for bit. The clip follows the complex-controls precedent
 * above: the coefficients are never clipped, the expanded copy is.
 *   *_opt_begin_basis  in the place of *_opt_begin / *_opt_begin_complex, after *_upload_controls of
 *                      the start pulses (expanded by the caller): the driver keeps `coefficients`
 *                      [B][P][channels] as its parameters, apart from the evaluation buffer, and M on
 *                      the device in both orientations. The optimizer state (Adam moments, and what
 *                      *_opt_lbfgs_begin allocates and checks against the free memory) is sized by
 *                      P * channels per seed. complex_controls: channels 2k, 2k+1 are one control
 *                      (the clip by modulus, the parameter order of L-BFGS), mapped channel by channel.
 *                      QOCX_ERR_ARG for P < 1, a non-finite matrix, odd channels with
 *                      complex_controls; QOCX_ERR_STATE without uploaded controls. A later
 *                      *_opt_begin / *_opt_begin_complex clears the basis.
 *   *_opt_clip         expands the coefficients into the evaluation buffer, then clips that buffer
 *                      (per channel, or by modulus) as without a basis; the squaring capacity and the
 *                      Lindblad sub-divisions follow from the clipped buffer as before.
 *   *_opt_step, *_opt_lbfgs_step   keep the coefficients of the improved seeds beside their controls,
 *                      project the last evaluation's gradients (control costs included) to
 *                      [B][P][channels] and run the optimizer on the coefficients and that gradient.
 *   *_opt_download_best_params   the coefficients [B][P][channels] behind the best controls;
 *                      QOCX_ERR_STATE without a basis. */
int qocx_opt_begin_basis(qocx_ctx* ctx, int32_t complex_controls, int32_t p, const double* matrix,
                         const double* coefficients);
int qocx_opt_download_best_params(qocx_ctx* ctx, double* params_out);
int qocx_lindblad_opt_begin_basis(qocx_ctx* ctx, int32_t complex_controls, int32_t p,
                                  const double* matrix, const double* coefficients);
int qocx_lindblad_opt_download_best_params(qocx_ctx* ctx, double* params_out);
/* The two maps alone, host arrays in and out, no state kept: matrix [nc][p];
 * transpose = 0: in [batch][p][channels] -> out [batch][nc][channels] (expansion),
 * transpose != 0: in [batch][nc][channels] -> out [batch][p][channels] (projection).
 * A seed's numbers do not depend on the batch it is part of. */
int qocx_control_basis_apply(qocx_ctx* ctx, int32_t transpose, int32_t batch, int32_t nc, int32_t p,
                             int32_t channels, const double* matrix, const double* in, double* out);

/* ---- host-side helpers of the multi-start GRAPE driver (no GPU work, no context) --------------
 * The reference's driver loop clips the controls and applies its optimizer plugin to ONE control
 * set per process (qoc/core/common.py:8-30, qoc/standard/optimizers/adam.py:110-165, sgd.py). The
 * batched driver holds B optimizer states as [B][P] arrays; these two functions are that loop's
 * arithmetic over the rows `rows[0..row_count)` on a few host threads - IEEE double operations in
 * the reference's order (no contraction), so every seed walks its single-seed trajectory bit for
 * bit. */
/* controls [B][Nc][K] real, in place: an entry whose modulus exceeds max_norms[k] becomes
 * (entry / modulus) * max_norms[k] (clip_control_norms). */
int qocx_host_clip_controls(double* controls, int64_t batch, int64_t nc, int32_t k,
                            const double* max_norms);
/* Adam.update on rows of params / grads / moment / square_moment (all [B][P]):
 *   g' = clip(g, -clip_grads, clip_grads) if apply_clip_grads
 *   m = beta_1 m + (1 - beta_1) g' ; v = beta_2 v + (1 - beta_2) g'^2
 *   params -= learning_rate * ((m / corr_1) / (sqrt(v / corr_2) + epsilon))
 * corr_i = 1 - beta_i^step and the (possibly decayed) learning rate are the caller's scalars.
 * kind 0 = SGD (params -= learning_rate * g; the other arguments are ignored). */
int qocx_host_optimizer_update(int32_t kind, double* params, const double* grads, double* moment,
                               double* square_moment, int64_t p, const int64_t* rows,
                               int64_t row_count, double learning_rate, double beta_1,
                               double beta_2, double epsilon, double corr_1, double corr_2,
                               int32_t apply_clip_grads, double clip_grads);

#ifdef __cplusplus
}
#endif
#endif /* QOCX_H */
