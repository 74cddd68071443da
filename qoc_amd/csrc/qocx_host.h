// qocx_host.h - what the host translation units of the C ABI (include/qocx.h) share: the error
// string, device buffers, the context and the helpers more than one of the files uses. Internal:
// not installed with include/qocx.h. The host files hold no device code; the kernels and their
// launch_* functions are declared in qocx_device.h.
#ifndef QOCX_HOST_H
#define QOCX_HOST_H

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <string>
#include <vector>

#include "../../include/qocx.h"
#include "qocx_device.h"
#include "qocx_diag.h"
#include "qocx_lindblad_route.h"

namespace qocx::host {

// records msg as the calling thread's last error (qocx_last_error) and returns code
int fail(int code, const std::string& msg);

#define HIP_TRY(expr)                                                                      \
    do {                                                                                   \
        hipError_t e_ = (expr);                                                            \
        if (e_ != hipSuccess)                                                              \
            return fail(QOCX_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

// A device allocation and its owner: freed with the buffer's owner (the context, a ControlCosts, a
// local), or early by release().
template <class T>
struct DevBuf {
    T* p = nullptr;
    size_t count = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { release(); }
    int ensure(size_t n) {
        if (n <= count && p != nullptr) return 0;
        if (p) (void)hipFree(p);
        p = nullptr;
        count = 0;
        if (n == 0) return 0;
        hipError_t e = hipMalloc((void**)&p, n * sizeof(T));
        if (e != hipSuccess) {
            return fail(QOCX_ERR_HIP, std::string("hipMalloc(") + std::to_string(n * sizeof(T)) +
                                          " bytes): " + hipGetErrorString(e));
        }
        count = n;
        return 0;
    }
    int upload(const std::vector<T>& v, hipStream_t st) {
        int rc = ensure(v.size());
        if (rc) return rc;
        if (v.empty()) return 0;
        hipError_t e = hipMemcpyAsync(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, st);
        if (e != hipSuccess) return fail(QOCX_ERR_HIP, hipGetErrorString(e));
        e = hipStreamSynchronize(st);  // v may be a temporary
        if (e != hipSuccess) return fail(QOCX_ERR_HIP, hipGetErrorString(e));
        return 0;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        count = 0;
    }
};

struct TimingRec {
    int which;
    hipEvent_t a, b;
};

// RCCL entry points, resolved lazily so that single-GPU use never loads librccl.
struct Rccl {
    void* lib = nullptr;
    int (*GetUniqueId)(void*) = nullptr;
    int (*AllReduce)(const void*, void*, size_t, int, int, void*, hipStream_t) = nullptr;
    int (*CommDestroy)(void*) = nullptr;
    const char* (*GetErrorString)(int) = nullptr;
};

// The costs of the controls alone of one path (qocx_set_control_costs, qocx_ctrlcost.hip)
struct ControlCosts {
    int count = 0;        // 0: none set
    int cplx = 0, K = 0;  // complex controls; controls (channels / 2 when complex)
    int Kr = 0, nc = 0;   // the channels and knots they were set for
    int elementwise = 0;  // descriptors of the kernel of NORM / VARIATION / AREA
    bool variation = false;
    struct Bandwidth {
        double multiplier;
        int pmax;
        size_t bins, bin_ptr;  // offsets into `ints`
    };
    std::vector<Bandwidth> bandwidth;
    DevBuf<qocx::CtrlCostDev> descs;
    DevBuf<double> arrays;  // the per-control arrays of the descriptors
    DevBuf<int> ints;       // bins and bin_ptr of the bandwidth costs
    DevBuf<double2> twiddle;
    // per evaluation
    DevBuf<double> cost, grad, work0, work1, stage;
    DevBuf<double2> spectrum, ybar;
    void clear() {
        count = 0;
        bandwidth.clear();
    }
};

// The device-resident state of one path's multi-start optimizer driver (qocx_opt_* /
// qocx_lindblad_opt_*, qocx_api_multistart.hip)
struct MultiStart {
    DevBuf<double> opt_m, opt_v, opt_best_controls, opt_max_norms;
    DevBuf<double2> opt_best_final;
    DevBuf<unsigned char> opt_flags;  // [2][B]: improved | update
    DevBuf<double> opt_params;        // complex controls: the optimizer's parameters - the seed controls
                                      // are then the copy clipped by modulus that is evaluated
    // L-BFGS (qocx_opt_lbfgs_begin): accepted point, its gradient, direction, the rings of pairs
    DevBuf<double> lb_x, lb_g, lb_d, lb_s, lb_y, lb_rho;
    DevBuf<qocx::LbfgsSeed> lb_seed;
    DevBuf<unsigned char> lb_finished;
    // a control basis (qocx_opt_begin_basis): opt_params are then the coefficients [B][P][channels],
    // the seed controls their expanded, clipped image
    DevBuf<double> basis_matrix, basis_matrix_t;  // M [Nc][P] (projection), its transpose [P][Nc] (expansion)
    DevBuf<double> basis_grads;                   // [B][P][channels]: the projected gradients
    DevBuf<double> opt_best_params;               // [B][P][channels]: the coefficients of the best so far
    int basis_P = 0;                  // 0: no basis
    int lbfgs_history = 0;            // 0: no L-BFGS state for this batch
    int batch = 0;                    // the path's batch the states were set up for (0: none)
    bool complex_controls = false;    // qocx_opt_begin_complex / qocx_lindblad_opt_begin_complex
};

// Padded device images of operators (h0, g, an augmented set): the MFMA tile layout of K1a and the
// Magnus kernels; column-major and its transpose for K3 (`t` is the general path's row-major matrix)
struct OperatorImages {
    DevBuf<double2> c, r, t;
    DevBuf<double2>& layout(int i) { return i == 0 ? c : (i == 1 ? r : t); }
    // from `count` row-major complex n x n matrices (every operator of every time sample)
    int build(const double* m, size_t count, int n, int nb, hipStream_t st, bool t_only = false);
};

// What a problem that runs on the M2 kernels through Ke effective controls keeps (EffCtlArgs): M4
// on a time-independent system, or H quadratic in the real controls (qocx_set_quadratic_terms),
// which needs M2 - the two never coexist.
struct EffectiveControls {
    enum Kind { NONE, M4_LINEAR, QUADRATIC };
    Kind kind = NONE;                    // what the problem offers (qocx_ctx::effctl_kind: what an evaluation uses)
    int Ke = 0;                          // effective controls per step
    OperatorImages images;               // the augmented set: G_k, A_k, B_kl | [nt][G_k(t), Q_q]
    DevBuf<qocx::StepInterp> interp_id;  // row j of veff for step j
    DevBuf<double> veff, gchain;         // per evaluation: EffCtlArgs::veff, ::gchain
    std::vector<int> pairs;              // quadratic terms: [count][2]
    std::vector<double> norm;            // ||Q_q||_1
    DevBuf<int> pairs_dev;
    // The matrix-free route on effective controls (qocx_action_eff.hip, knob "action_eff"): ||G^_e||_1 of each
    // of the Ke augmented operators and the bound of its spectral norm (spectral_bound where the problem is
    // Hermitian and constant in time, never above the 1-norm), on the host and on the device; and at n <= 32
    // the image of E_e = -i dt G^_e the gradient kernels contract with, in the layout of qocx_ctx::g_eimg
    // (released where it cannot be formed: a time-dependent system, n > 32).
    std::vector<double> op_norm1, op_norm2;
    DevBuf<double> op_norm1_dev, op_norm2_dev;
    DevBuf<double2> eimg;
    int quad_count() const { return kind == QUADRATIC ? (int)pairs.size() / 2 : 0; }
};

// Per-seed or per-member tables of the controls' channels, held by value by both paths (ctx->seeds,
// ctx->lb.seeds): the last J of the problem's K channels are fixed channels, the first Kr = K - J
// those of the seeds, and row r of the tables scales the seed channels (s_rk u_k) and sets the fixed
// ones (delta_rj).
//  - Hamiltonian ensemble (qocx_set_ensemble / qocx_lindblad_set_ensemble, EnsembleArgs): M member
//    rows; every seed is evaluated as its M member items, item b * M + m, whose results are folded
//    with `weights` into the seed's. The seed-level calls take and return the seeds' Kr channels.
//  - Hamiltonian sweep (qocx_set_sweep / qocx_lindblad_set_sweep, SystemSweepArgs): seed b is a
//    system of its own, item b, with row b: swp_B rows and M = 1, ONE item per seed, so every
//    seed-level call (the optimizer drivers, control costs, downloads) serves it as it serves an
//    ensemble; swp_B is also the only batch size the sweep takes.
// A problem takes one or the other (the setters refuse the second kind, and a new problem clears
// both), so the tables in these buffers are those of the last setter that succeeded and no launch
// reads another kind's: rows() of them stand.
struct SeedTables {
    int M = 0;           // 0: neither; items per seed
    int J = 0, Kr = 0;   // fixed channels, seed channels (K = Kr + J)
    int swp_B = 0;       // 0: no sweep
    std::vector<double> scales_h, offsets_h;  // [rows][Kr], [rows][J]: what the staging bounds read
    DevBuf<double> scales, offsets, weights;  // ... on the device; [M] (an ensemble's only)
    DevBuf<double> scale_sens, offset_sens;   // a sweep: dE_b/ds_bk [B][Kr], dE_b/ddelta_bj [B][J]
    // Duration search of a sweep (qocx_sweep_set_durations / qocx_lindblad_sweep_set_durations): tau_b
    // is a parameter of seed b on the device and the sweep's tables are derived there, tau_b times the
    // base tables. The optimizer's clip and step move tau without telling the host: mirror_stale
    // until the path has re-formed scales_h / offsets_h (which the next upload or sub-division reads).
    struct Durations {
        bool set = false, mirror_stale = false;
        bool have_grad = false;  // `grad` is that of the standing evaluation
        double tau_min = 0, tau_max = 0, weight = 0;
        DevBuf<double> tau, base_scales, base_offsets, grad;  // [B], [B][Kr], [B][J], [B]
        DevBuf<double> m, v, best;  // [B] each: Adam moments of tau, best tau (the drivers' *_opt_begin)
        void clear() { set = mirror_stale = have_grad = false; }
    } dur;
    bool sweep() const { return swp_B > 0; }
    int rows() const { return swp_B > 0 ? swp_B : M; }
    void clear() {  // a new problem
        M = J = Kr = swp_B = 0;
        dur.clear();
    }
};

}  // namespace qocx::host

// (the host files name the shared helpers as the single file they were cut from did)
using namespace qocx::host;

struct qocx_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    // ---- problem ----
    bool has_problem = false;
    int n = 0, nb = 0, np = 0, S = 0, K = 0, nc = 0, N = 0, nsteps = 0, ces = 1, nt = 1;
    double T = 0, dt = 0;
    int interp_policy = QOCX_INTERP_LINEAR;  // qocx_set_interpolation_policy: read by the next problem setter
    bool pwc = false;                        // the Schroedinger problem was set piecewise constant
    int has_step_costs = 0, cost_count = 0;
    double h0_norm_max = 0;
    std::vector<double> g_norm_max;
    // upper bounds of the SPECTRAL norms of the same operators (spectral_bound; the 1-norms above where it
    // does not apply): they decide the Taylor degrees of the matrix-free route and nothing else
    double h0_norm2_max = 0;
    std::vector<double> g_norm2_max;
    OperatorImages h0, g;  // [nt], [nt][K]
    // [K] E_k = -i dt G_k in the order of g.r (ActionGradArgs::e_img), where the matrix-free route of
    // 17 <= n <= 32 can run (nt == 1); upload_operators writes it with g and dt, and nothing else writes those
    DevBuf<double2> g_eimg;
    DevBuf<double2> psi0, cost_vectors;
    DevBuf<qocx::StepInterp> interp;
    DevBuf<qocx::DevCost> costs;
    DevBuf<int> cost_counts, row_ptr, col_step;
    DevBuf<double> weight;
    // ---- evaluation state ----
    int B = 0;
    int sbound = 0;
    int last_chunk = 0;         // seeds of the last memory chunk of the last evaluation (its step table is in s_arr)
    double norm_bound = 1e300;  // host bound of ||step generator||_1 of the uploaded controls / generators
    // M2, control knots at the system times (Nc = N): a bound of the step generators at their MIDPOINTS,
    // where u is the mean of two knots - what the step table's per-step bound can reach at most; 1e300 when
    // it does not apply. Decides only whether the two-wave K1a is launched beside the three-wave one.
    double norm_bound_mid = 1e300;
    // the same two bounds of ||step generator||_2, from h0_norm2_max / g_norm2_max: they size the Taylor
    // buffers of the matrix-free route (ResidentRoute::m_max); 1e300 where no such bound was formed
    double norm2_bound = 1e300, norm2_bound_mid = 1e300;
    size_t slot_cap = 0;
    int chunk_user = 0;
    int pipe_user = 0;
    std::vector<hipStream_t> sweep_streams;
    hipStream_t lu_stream = nullptr;       // K1b of a segment beside K1a of the next one (n > 32)
    std::vector<hipEvent_t> ev_pq;         // K1a of segment i has finished
    std::vector<hipEvent_t> ev_factored, ev_swept, ev_fwd;
    bool unit_ok = false;          // the only cost is one separable final cost (qocx_sweep_common.h)
    MultiStart ms;  // multi-start driver on the device (qocx_opt_*)
    ControlCosts control_costs;  // qocx_set_control_costs(QOCX_PATH_SCHROEDINGER)
    DevBuf<double2> lam_scale;     // unit adjoint: [B][S]
    DevBuf<int> offs_x;            // unit adjoint: [chunk][nsteps + 1]
    int keep_step_states = 0;
    bool have_results = false, have_grads = false, have_step_states = false;
    DevBuf<double> controls, cost_out, grads, gstep;
    double* pin_controls = nullptr;  // pinned staging of the controls (qocx_upload_controls)
    size_t pin_controls_cap = 0;
    DevBuf<double2> final_out, step_states;
    DevBuf<double2> q_img, lu_img, dinv, states, xs;
    DevBuf<double2> qt_img;  // one control set (sweep_umode): the transposed propagator images
    DevBuf<int> perm, iperm, s_arr, offs, status;
    DevBuf<int> lu_fallbacks;  // [1] matrices that left the diagonal-pivot MFMA factorisation (qocx_lu_fallbacks)
    DevBuf<int> lu_redo;  // 33 <= n <= 64: matrices the MFMA factorisation hands to the general one (LuArgs::redo)
    // matrix-free route (qocx_action.hip): the Taylor terms of every step of a chunk, the forward sweep's
    // state between launches, the degrees the last evaluation executed (qocx_action_degrees) and the
    // evaluations run again on the Pade route because a step's degree was beyond the buffers (qocx_action_reruns)
    DevBuf<double2> kry_f, kry_b, action_carry;
    DevBuf<int> action_counts;
    int64_t action_reruns = 0;
    // ---- Magnus M4/M6 ----
    int nodes = 1;
    int cu_count = 256;
    int hermitian = 0;  // every h0[t], g[t][k] equals its conjugate transpose bit for bit
    bool general_path = false;  // the evaluation runs on qocx_general.hip (n > 64, or S beyond the sweep's LDS)
    DevBuf<double2> m_rm, mbar_rm, magnus_scratch, lam_buf;
    EffectiveControls eff;
    // Which effective-control route an evaluation takes. The knob "m4_linear" switches M4-linear off
    // on the resident route only: the general route (eval_general) has never consulted it.
    EffectiveControls::Kind effctl_kind(bool resident) const {
        using E = EffectiveControls;
        if (explicit_mode) return E::NONE;
        if (eff.kind == E::M4_LINEAR && nodes == 2 && (!resident || knob("m4_linear", 1))) return E::M4_LINEAR;
        return eff.kind == E::QUADRATIC && nodes == 1 ? E::QUADRATIC : E::NONE;
    }
    int hermitian_linear = 0;  // `hermitian` of H0 / G_k alone (qocx_set_quadratic_terms folds in the Q_q)
    // Hamiltonian ensemble or sweep (SeedTables). The seeds' controls, costs and gradients live in ens_*
    // and the evaluation buffers (controls, cost_out, grads, final_out) hold the items; a sweep keeps
    // the maxima over its seeds in ens_scale_max / ens_offset_max, and its expansion, reduction and
    // staging are its own.
    SeedTables seeds;
    int ens_B = 0;                       // seeds of the last upload (ctx->B = ens_B * seeds.M)
    bool ens_stale = false;              // ens_controls moved (qocx_opt_clip / _step) since the expansion
    std::vector<double> ens_scale_max, ens_offset_max;  // max_r |s_rk|, max_r |delta_rj| (a duration search: at tau_max)
    DevBuf<double> ens_controls, ens_cost, ens_grads;   // [B][nc][Kr], [B], [B][nc][Kr]
    // ... with quadratic terms: the members' scales c_mq of the terms (qocx_set_ensemble_quadratic_scales)
    bool ens_qscales_set = false;
    std::vector<double> ens_qscale_max;                 // max_m |c_mq|
    DevBuf<double> ens_qscales;                         // [M][count]
    DevBuf<double> ustep, g_norm_dev;  // step table (launch_step_table): u_k(t_mid) per step; ||G_k||_1
    DevBuf<double> g_norm2_dev;        // ... and the bounds of ||G_k||_2
    // explicit-generator mode (qocx_upload_generators): opaque Hamiltonians sampled by the host
    bool explicit_mode = false;
    int explicit_hermitian = 0;
    DevBuf<double2> gen_rm, genbar_rm;  // [B][nsteps] row-major padded generators / cotangents
    // ---- host-supplied state cotangents ----
    int inj_count = 0, inj_batch = 0;
    DevBuf<int> inj_index;
    DevBuf<double2> inj_bars;
    struct Lindblad {
        bool has_problem = false;
        int n = 0, S = 0, K = 0, nc = 0, N = 0, nsteps = 0, ces = 1, nops = 0;
        double T = 0, dt = 0, h0_norm = 0, diss_norm = 0, l0_norm = 0;
        bool pwc = false;  // set piecewise constant: nc slices, sub-intervals cut at j T / nc
        std::vector<double> g_norm;
        int has_step_costs = 0, cost_count = 0;
        DevBuf<double2> a0l, a0r, a0ld, a0rd, gp, gpd, gpt, ops, rho0, cost_matrices;
        DevBuf<double> gammas;
        DevBuf<qocx::DevCost> costs;
        DevBuf<int> cost_counts;
        // sub-interval tables, by sub-division count
        struct Grid {
            int nsub = 0;
            DevBuf<qocx::SubStep> substeps;
            DevBuf<int> row_ptr, col;
            DevBuf<double> weight;
        };
        std::map<int, Grid> grids;
        // per evaluation
        int B = 0;
        std::vector<int> order;  // device position -> seed
        // What stands of the last evaluation: set where a result comes about, cleared by these functions alone.
        bool have_results = false, have_steps = false;
        void results_stand(int items, bool kept_steps) { B = items; have_results = true; have_steps = kept_steps; }
        // the resident controls moved (clip, step, upload): only the resident results are no longer theirs
        void resident_controls_moved(bool maxima_known) { res_have_results = false; umax_valid = maxima_known; }
        // a setter changed what an evaluation means: nothing of the last one stands
        void drop_results() {
            have_results = have_steps = res_have_results = res_have_grads = swp_have_grads = swp_rates_ok = false;
            swp_seed_controls = nullptr; ens_members_B = 0;
        }
        // ... nor does the resident batch: controls must be uploaded again, and the driver begun again
        void drop_resident() { drop_results(); res_B = ms.batch = 0; umax_valid = false; }
        // host-supplied density cotangents
        int inj_count = 0, inj_batch = 0;
        std::vector<int> inj_steps;
        std::vector<double> inj_host;  // [B][count][S][n][n] complex
        DevBuf<int> inj_index;
        DevBuf<double2> inj_bars;
        DevBuf<double> gsub, cost_out, grads, controls;
        DevBuf<double2> checkpoints, final_out, step_densities, ystages, scratch;
        DevBuf<double2> kbstages, lam_scale;  // two-sided evaluation (LindbladArgs::phase)
        bool unit_ok = false;                 // one final TargetDensityInfidelity, one density
        bool hermitian = false;               // H0, G_k, sum gamma L^H L, initial densities and cost matrices
                                              // are Hermitian: so is every density and every cotangent
        bool ops_real = false;                // every Lindblad operator has a zero imaginary part
        qocx::LindbladForm form;         // where the densities live, how many waves work on a seed (set time)
        int fixed_ksub = 0;              // > 0: time-dependent Hamiltonian sampled for this grid
        // qocx_debug_lindblad_knobs (tests force the kernel variants large batches / little HBM use)
        int64_t last_subintervals = 0;   // sum over the seeds of the last evaluation
        int64_t dbg_stage_seeds = 0;     // seeds whose stage values may be kept; 0: 45 % of free HBM
        int dbg_min_piece = 256;         // below this many seeds per piece the adjoint recomputes
        int dbg_wave_mode = 0;           // 0 auto, 1 one wave per seed, 2 several whenever built for
        DevBuf<double2> a0_tab, gp_tab, op_tab;
        DevBuf<double> gamma_tab;
        // multi-start driver on the device (qocx_lindblad_upload_controls / _opt_*): controls and
        // results in seed order, apart from the evaluation's buffers above (group order)
        int res_B = 0;
        bool res_have_results = false, res_have_grads = false;
        bool umax_valid = false;          // umax_host holds the control maxima of res_controls
        std::vector<double> umax_host;    // [B][K]
        DevBuf<double> res_controls, res_cost, res_grads, umax;
        DevBuf<double2> res_final;        // [B][S] dumps
        DevBuf<int> order_dev;            // lb.order on the device
        MultiStart ms;                    // qocx_lindblad_opt_*
        ControlCosts control_costs;       // qocx_set_control_costs(QOCX_PATH_LINDBLAD)
        // Hamiltonian ensemble or sweep (SeedTables). An evaluation runs on the items, each with its own
        // sub-division count, and the buffers above (controls, cost_out, grads, final_out, order, B) are
        // then those of the items.
        SeedTables seeds;
        DevBuf<double> ens_seed_controls;  // [B][nc][Kr]: the seeds of qocx_eval_lindblad
        DevBuf<double> ens_seed_cost, ens_seed_grads;  // ... and their reduced results
        DevBuf<double> ens_items;          // [B][M][nc][K]: the expanded controls, item order
        DevBuf<double> ens_cost, ens_grads;  // [B][M], [B][M][nc][K]: the items' results, item order
        DevBuf<double2> ens_final;         // [B][M][S] dumps, item order (qocx_eval_lindblad)
        int ens_members_B = 0;             // seeds whose member costs ens_cost holds (0: none)
        // ... with per-member dissipation rates gamma_mi = c_mi gamma_i (qocx_lindblad_set_ensemble_rates):
        // every member has its own control-free generators, rates and sub-division bound, built from the
        // problem's host copies below as the plain setter builds its own
        bool ens_rates = false;
        std::vector<double> h0_h, gammas_h, op_norms_h;  // H0; gamma_i [L'] (L' with pad_op's zero); ||L_i||_2 [L]
        std::vector<std::vector<double>> ops_h;          // L_i [L']
        std::vector<double> rate_l0_norm;                // [M]: l0_norm of the members
        DevBuf<double2> rate_a0;                         // [M][4] dumps A0L, A0R, A0L^H, A0R^H
        DevBuf<double> rate_gammas;                      // [M][L']
        // A sweep's expansion, reduction and channel sensitivities are the kernels of qocx_sweep.hip. With
        // rate factors the rates tables above hold one entry per seed (ens_rates, rate_a0, rate_gammas,
        // rate_l0_norm [B]) and item_member is the launched seed's own index.
        const double* swp_seed_controls = nullptr;          // the seed controls of the last evaluation (device)
        bool swp_have_grads = false;                        // ... which had gradients, and whose results stand
        // rate sensitivities (qocx_lindblad_ratesens.hip): asked for, and whether every piece of the last
        // evaluation ran two-sided with 1 .. 4 operators
        bool swp_want_rates = false, swp_rates_ok = false;
        DevBuf<double2> swp_ldl;                            // [L] dumps of L_l^H L_l
        DevBuf<double> swp_rate_partials, swp_rate_sens;    // [sub-intervals of the evaluation][L]; [B][L], launch order
        // A duration search (qocx_lindblad_duration.hip) also derives the rates tables (rate_a0, rate_gammas)
        // on the device, tau_b times the base tables below. The host mirrors - seeds.scales_h, seeds.offsets_h
        // and rate_l0_norm, which decide the sub-division counts - are re-formed from tau by the same single
        // products once it has come back (lindblad_duration_mirror).
        DevBuf<double> dur_base_rates;                      // [B][L]
        DevBuf<double2> dur_base_a0;                        // [B][4] dumps at tau = 1 (rates c0_b gamma)
        DevBuf<double> dur_base_gammas;                     // [B][L'] at tau = 1
        std::vector<double> dur_tau_h, dur_base_scales_h, dur_base_offsets_h, dur_base_rates_h;  // host copies
        std::vector<double> dur_l0_norm0;                   // [B]: the seeds' l0_norm at tau = 1
        int seed_channels() const { return seeds.M > 0 ? seeds.Kr : K; }
        size_t seed_items() const { return seeds.M > 0 ? (size_t)seeds.M : 1; }
    } lb;
    // ---- qocx_debug_set_knob: kernel-variant switches for A/B measurements and tests ----
    std::map<std::string, int64_t, std::less<>> knobs;  // (std::less<>: a lookup by const char* builds no string)
    DevBuf<unsigned long long> stamps;  // sweep3 diagnostic build
    int64_t knob(const char* name, int64_t dflt) const {
        auto it = knobs.find(name);
        return it == knobs.end() ? dflt : it->second;
    }
    // ---- timing ----
    int timing = 0;            // 0 off, 1 every launch, 2 + k the launches of kernel k only
    bool time_active = false;  // the launch between the last time_begin / time_end is being timed
    std::vector<TimingRec> pending;
    std::vector<double> timeline;  // (which, start, end) of the last evaluation's launches
    std::vector<hipEvent_t> ev_pool;
    size_t ev_used = 0;
    int64_t t_launch[7] = {0, 0, 0, 0, 0, 0, 0};
    double t_ms[7] = {0, 0, 0, 0, 0, 0, 0};
    // ---- comm ----
    Rccl rccl;
    void* comm = nullptr;
    DevBuf<double> comm_buf;
};

namespace qocx::host {

// ---- qocx_api.hip: kernel timing (qocx_set_timing) ----
void time_begin(qocx_ctx* ctx, int which, hipStream_t st);
void time_end(qocx_ctx* ctx, hipStream_t st);
void time_collect(qocx_ctx* ctx);

// ---- qocx_api.hip: norm bounds of the step generators; the seed-level view ----
int pade_scale_count(double norm1);
// sbound, norm_bound and slot_cap from a bound of ||step generator||_1; `needs`: the caller's wording
// bound2: the same of ||step generator||_2 into norm2_bound (1e300: none formed; norm2_bound_mid is reset
// with norm_bound_mid - qocx_upload_controls sets both after the call)
int commit_step_bound(qocx_ctx* ctx, double bound, bool keep_larger, const char* needs, double bound2 = 1e300);
double one_norm(const double* m, int n);  // complex row-major
// Hermitian m, n <= 64: a value in [rho(m), 1.01 rho(m)] - never below the spectral radius (= ||m||_2)
double spectral_bound(const double* m, int n);
double pade_eps_max(double theta);
double magnus_norm_bound(int nodes, double bound);
double quad_bound(const qocx_ctx* ctx, const double* umax);
int seed_count(const qocx_ctx* ctx);
int seed_channels(const qocx_ctx* ctx);
double* seed_controls(qocx_ctx* ctx);
double* seed_costs(qocx_ctx* ctx);
double* seed_grads(qocx_ctx* ctx);
// ---- qocx_api.hip: what both paths do with a SeedTables ----
// The setters' shared part: checks members / seeds (`rows`), `fixed` of the problem's K channels and the
// three pointers (weights: an ensemble's), fills the tables with the defaults (scales 1), uploads them and
// commits the shape; synchronises. The caller has made its own state checks and set the device.
int set_seed_tables(SeedTables& s, bool sweep, int K, int rows, int fixed, const double* scales,
                    const double* offsets, const double* weights, hipStream_t st);
// ... of the duration setters: the box and weight checks, tau and the base tables s0 / d0 (returned: the
// paths take their own maxima and mirrors from them) checked and uploaded, the sweep's tables ensured
int set_seed_durations(SeedTables& s, const double* tau, const double* base_scales, const double* base_offsets,
                       double tau_min, double tau_max, double time_weight, hipStream_t st, std::vector<double>& s0,
                       std::vector<double>& d0);
// tau and, where the caller says its gradient stands, dE/dtau of a duration search
int download_seed_durations(const SeedTables& s, hipStream_t st, bool gradient_stands, double* tau_out,
                            double* tau_grad_out);
// The kernels' arguments from the tables and the buffers of a path they expand and reduce on
struct SeedBuffers {
    const double* seed_controls;   // [B][nc][Kr]
    double* items;                 // the expanded controls [B][M][nc][K]
    double *item_cost, *item_grads;  // the items' results, item order
    double *cost, *grads;          // the seeds' reduced results (grads nullptr: none)
};
qocx::EnsembleArgs ensemble_args(const SeedTables& s, int seeds, int nc, const SeedBuffers& b);
qocx::SystemSweepArgs sweep_args(const SeedTables& s, int nc, const SeedBuffers& b);
qocx::DurationArgs duration_args(const SeedTables& s, double* tau_grad, double* cost);

// ---- qocx_api_lindblad.hip: duration search of a Lindblad sweep (qocx_lindblad_sweep_set_durations) ----
// clips tau and rewrites the sweep's tables and the seeds' generator tables from it (enqueued)
void lindblad_duration_tables(qocx_ctx* ctx);
// enqueues the copy of tau to the host; after the caller's synchronisation lindblad_duration_mirror()
// re-forms the host mirrors from it
int lindblad_duration_fetch(qocx_ctx* ctx);
void lindblad_duration_mirror(qocx_ctx* ctx);

// ---- qocx_host_resident.hip ----
int eval_items(qocx_ctx* ctx, int32_t want_grad);

// ---- qocx_api_lindblad.hip: the C-layout dumps of the densities ----
int dump_elems(int n);
void from_c_dump(const double2* d, int n, double* out);

// ---- qocx_api_multistart.hip ----
int run_control_costs(qocx_ctx* ctx, ControlCosts& cc, int B, int nc, int Kr, const double* controls,
                      bool want_grad);

}  // namespace qocx::host

#endif
