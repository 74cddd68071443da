// qocx_device.h - argument blocks shared by the kernels (qocx_kernels.hip) and the host side of
// the C ABI (qocx_api*.hip, qocx_host_resident.hip). Plain structs of device pointers and sizes.
#ifndef QOCX_DEVICE_H
#define QOCX_DEVICE_H

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace qocx {

#define QOCX_DEV_COST_COHERENT 0
#define QOCX_DEV_COST_INCOHERENT 1
#define QOCX_DEV_COST_FORBID 2
#define QOCX_DEV_COST_TARGET_DENSITY 3
#define QOCX_DEV_COST_FORBID_DENSITY 4
#define QOCX_LINDBLAD_MAX_K 8

// Linear interpolation of the controls at the quadrature time of one propagator step
// (qoc/core/mathmethods.py:33, :54-65): u = y[i1] + ((y[i2] - y[i1]) / dx) * off.
struct StepInterp {
    int i1, i2;
    double dx, off;
};

struct DevCost {
    int kind;
    int step_cost;
    double scale;
    int vec_offset;  // first vector of this cost in the pooled cost_vectors, in units of vectors
    int cnt_offset;  // FORBID: first entry in cost_counts
};

struct FactorArgs {
    // inputs
    const double* controls;    // [B][nc][K]
    const StepInterp* interp;  // [nsteps]
    const double2* h0_cimg;    // [nt] C-images
    const double2* g_cimg;     // [nt][K] C-images
    int K, nc, nsteps, nt;
    int step0, seg_len;        // this launch covers steps [step0, step0 + seg_len) of every seed
    int hermitian;             // every h0[t], g[t][k] is exactly Hermitian
    int n;                     // Hilbert size (used by the sixteen-tile K1a: <= 48 -> nine tiles); 0: unknown
    int pade_policy = 0;       // 0: Pade order by norm (qocx_wave.h), 13: always [13/13]
    int prefer_low = 0;        // the host's bound of ||dt a||_1 is below theta_9 (1) or theta_5 (2): which
                               // paths the four-wave K1a inlines (qocx_pade4.hip)
    int skip_q = 0;            // timing experiment: the two-wave K1a does not store Q
    int herm_tiles = 1;        // four-wave K1a, Hermitian generators, orders 3 / 5: two thirds of the tiles (knob "k1a_herm4")
    // diagnostic build only (qocx_diag.h; knobs "k1a_dbg", "k1a_stamps"): bits 0-1 s_setprio level of
    // the fused factorisation, bit 2 no factorisation at all (garbage), and the cycle sums of the
    // stamped build, [2 waves][8]
    int dbg = 0;
    unsigned long long* stamps = nullptr;
    int lu_mfma = 0;           // fused K1b with its Schur updates on the matrix cores (qocx_lu4.h)
    int lu_dpp = 0;            // fused K1b on the vector unit for provably diagonal pivots (qocx_lu5.h)
    int three_wave = 0;        // orders 3 / 5, Hermitian, step table: one tile per wave on three waves (qocx_pade3.hip)
    int four_steps = 0;     // three-wave K1a: the second halves of the factorisations four to a wave in a kernel of their own (knob "k1a_four"; 1: launch_pq launches it, 2: the caller)
    int pack8 = 0;          // n <= 8, one-wave K1a: two consecutive steps of a seed as the diagonal blocks of ONE 16 x 16 tile (pade_pq8_kernel)
    int gen_share = 2;      // three-wave K1a: which tiles of the generator come from the LDS slot instead of the images (knob "k1a_share")
    // Step table (round 4, launch_step_table): `controls` is [B][nsteps][K] = the interpolated
    // controls u_k(t_mid) of every step (interp unused), and s_arr already holds every step's Pade
    // order and squaring count, taken from the bound dt (||H0||_1 + sum |u_k| ||G_k||_1): the kernel
    // neither interpolates nor forms a norm.
    int direct = 0;
    int* lu_fallbacks = nullptr;  // LuArgs::fallbacks of the fused factorisation
    // two-wave K1a (17 <= n <= 32) with K1b fused in: P stays in LDS, wave 0 factors it, only the
    // factors (and 1/U_kk, the permutation) go to HBM; launch_lu is then not called
    int fuse_lu = 0;
    double2* dinv = nullptr;
    int* perm = nullptr;
    int* iperm = nullptr;
    double dt;
    // outputs, indexed by (b * nsteps + step); column-major NP x NP images
    double2* q_img;
    double2* lu_img;  // receives P; lu_kernel factors it in place
    int* s_arr;
    int* status;
};

// u_k(t_mid) of every (seed, step) by the reference's interpolation formula, and the step's entry
// of s_arr (Pade order, squarings: qocx_wave.h) from the norm bound of that step's generator.
struct StepTableArgs {
    const double* controls;    // [B][nc][K]
    const StepInterp* interp;  // [nsteps]
    int K, nc, nsteps, batch;
    double dt;                 // the bound is |dt| (h0_norm + sum_k |u_k| g_norm[k])
    double h0_norm;            // max over time of ||H0(t)||_1
    const double* g_norm;      // [K] max over time of ||G_k(t)||_1 (device memory)
    int pade_policy;           // 0: order by norm, 13: always [13/13]
    int sq_max = 30;           // the squaring count the host sized the sub-step slots for
    int order_max = 13;        // 5: the three-wave K1a of qocx_pade3.hip runs the evaluation (host bound below theta_5)
    int action = 0;            // the entries also carry the Taylor degree of the step (qocx_action.h)
    // ... by action_degree_rule from the bound above and |dt| (h0_norm2 + sum_k |u_k| g_norm2[k]) >= ||a||_2
    double h0_norm2 = 0;       // max over time of an upper bound of ||H0(t)||_2 (Hermitian H: its spectral radius)
    const double* g_norm2 = nullptr;  // [K] the same of G_k(t) (device memory; read where action and degree_rule are set)
    int degree_rule = 0;       // knob "action_degree": 1 the lesser of the two criteria, 0 the 1-norm alone
    double* ustep;            // out: [B][nsteps][K]
    int* s_arr;                // out: [B][nsteps]
    int* status;               // bit 1: non-finite controls
};
void launch_step_table(const StepTableArgs& a, hipStream_t st);

struct LuArgs {
    double2* lu_img;  // in: P, out: L\\U of the row-permuted P (column-major)
    double2* dinv;    // [NP] 1/U_kk
    int* perm;        // [NP] perm[pos] = original row
    int* iperm;       // [NP] iperm[row] = pos
    int* status;
    int nsteps, step0, seg_len;  // work item w -> matrix (w / seg_len) * nsteps + step0 + w % seg_len
    int n;                       // Hilbert size (sixteen-tile K1b: <= 48 -> 48 elimination steps); 0: unknown
    int dbg = 0;                 // timing experiment (dbg_skip bit 4): loads and stores only
    int inverse = 0;             // lu_img receives P^-1 instead of the factors (n <= 32; qocx_lu.h inv_body)
    int all_dominant = 0;        // every matrix of the launch is diagonally dominant by the margin of qocx_lu5.h
    int pack8 = 0;         // inv16: the image of every EVEN step of the launch holds two steps (FactorArgs::pack8); the inverses go out unpacked
                                 // (the host's bound of the step norm says so): n <= 16 inverses four to a wave
    // 33 <= n <= 64, round 4: [matrices] flags of the MFMA factorisation (qocx_lu4m.hip) - 1: its
    // diagonal-pivot attempt was abandoned, lu4_kernel factors the matrix; nullptr: lu4_kernel factors
    // every matrix
    int* redo = nullptr;
    // how many matrices left the diagonal-pivot MFMA factorisation for the general one (qocx_lu4.h,
    // qocx_lu4m.hip); a device counter the host zeroes per evaluation (qocx_lu_fallbacks), or nullptr
    int* fallbacks = nullptr;
};

struct SweepArgs {
    const double2* q_img;
    const double2* lu_img;
    const double2* dinv;
    const int* perm;
    const int* iperm;
    const int* s_arr;
    const double2* psi0;  // [S][NP]
    int S, nsteps, cost_eval_step, want_grad, has_step_costs;
    int n = 0;  // Hilbert size (sixteen-tile sweep: <= 48 -> nine-tile images in LDS); 0: unknown
    // Time segmentation: one launch runs the forward sweep over steps [j_begin, j_end) (phase
    // bit 0) and / or the adjoint sweep from j_end back to j_begin (phase bit 1); state is carried
    // between launches in states/offs/cost_out (forward) and lam_buf (adjoint).
    int phase, j_begin, j_end;
    int unit_adjoint = 0; // separable final cost: the adjoint runs on lam = targets (qocx_sweep_common.h)
    double2* lam_scale = nullptr;   // [B][S] scalars c_s, written at the end of the forward sweep, read by K3
    int* offs_x = nullptr;  // unit adjoint: [B][nsteps+1] first xs slot of each step, written by the ADJOINT
                          // sweep (it may run before the forward sweep has numbered the sub-steps)
    int batch = 0;        // seeds of the launch (set by the launchers of the one-state forms)
    int one_state = 0;    // one state, n <= 32: the dedicated kernel of qocx_sweep1.hip (knob "sweep_one")
    const double2* qt_img = nullptr;  // umode: U^T images (launch_umul) - the adjoint sweep copies them straight instead of gathering
    int umode = 0;        // sweepi: q_img holds the propagator U = P^-1 Q (launch_umul): ONE product per sub-step;
                          // the adjoint leaves lambda' in `xs` and K3 forms x = P^-H lambda' (KrylovArgs::umode)
    int dbg;              // sweep3 timing diagnostics (results are garbage): bit 0 no inversion,
                          // bit 1 no solves, bit 2 no LU fetch, bit 3 no Q fetch, bit 4 no Q touch
    unsigned long long* stamps;  // sweep3 diagnostic build: [B][4 roles][8] cycle sums, or nullptr
    double2* lam_buf;     // [B][S][NP]
    // Externally supplied state cotangents (user Cost plugins whose derivative the host
    // provides): inj_index[step] = row of inj_bars or -1; added to lambda at system step `step`
    // (the states before evolving from it; step N-1 = the final states).
    const int* inj_index;     // [nsteps + 1] or nullptr
    const double2* inj_bars;  // [B][inj_count][S][NP]
    int inj_count;
    size_t slot_cap;      // sub-step slots per seed
    // costs
    int cost_count;
    const DevCost* costs;
    const double2* cost_vectors;  // pooled, padded to NP
    const int* cost_counts;
    // outputs
    double2* states;       // [B][slot_cap][S][NP]  state before sub-step t
    double2* xs;           // [B][slot_cap][S][NP]  x = P^-H lambda' of sub-step t
    int* offs;             // [B][nsteps+1] first sub-step slot of each step
    double* cost_out;      // [B]
    double2* final_out;    // [B][S][NP]
    double2* step_states;  // [B][nsteps+1][S][NP] or nullptr
    int* status;
};

struct KrylovArgs {
    int umode = 0;                       // `xs` holds lambda' (SweepArgs::umode): x = P^-H lambda' is formed here from pinv_img
    const double2* pinv_img = nullptr;   // [B][nsteps] column-major P^-1 images (the LU buffer in inverse mode)
    const double* controls;
    const StepInterp* interp;
    const double2* h0_rimg;  // column-major h0
    const double2* h0_timg;  // column-major h0^T
    const double2* g_rimg;
    const double2* g_timg;
    int K, nc, nsteps, nt, S;
    int direct = 0;  // controls is the step table [B][nsteps][K] (FactorArgs::direct)
    int n = 0;  // Hilbert size (four-wave K3: <= 48 -> the zero pad columns are skipped); 0: unknown
    int step0;  // grid.x covers steps [step0, step0 + gridDim.x)
    int skew;   // 1: every H0(t), G_k(t) is exactly Hermitian (a^H = -a)
    double dt;
    const int* s_arr;
    const int* offs;
    const double2* states;
    const double2* xs;
    size_t slot_cap;
    double* gstep;  // [B][nsteps][K]
    // unit adjoint (qocx_sweep_common.h): x sits at slots of its own (offs_x: first xs slot of each
    // step) and is the back-propagated TARGET; gstep then receives the complex number
    // gamma = sum conj(abar_1) E_k per (step, k) - [B][nsteps][K][2] - and the scatter kernel forms
    // Re(conj(c) gamma) with the cost's scalar c. nullptr: x is the true cotangent, gstep is real.
    const int* offs_x = nullptr;
    // Magnus M4/M6: the generator is read from m_rm (row-major padded NP x NP, unscaled) and the
    // cotangent of M is written to mbar_rm instead of the contraction with G_k. nullptr for M2.
    const double2* m_rm;
    double2* mbar_rm;
};

// Matrix-free route of one-state Hermitian problems at 17 <= n <= 32 (qocx_action.hip; 33 <= n <= 64:
// qocx_action4.hip, NP = 64 in the buffer shapes below): the sweeps
// apply exp(a_j) to their vector by the truncated Taylor series and leave its terms behind
// (which problems take it, and on which of the kernel families below: qocx_action_route.h, action_plan;
// who fills these blocks and launches them: qocx_host_action.h)
struct ActionArgs {
    SweepArgs sw;              // phase, j_begin / j_end, psi0, costs, cost_out, final_out, lam_scale, lam_buf, s_arr, status
    const double* ustep;       // [B][nsteps][K] the step table's u_k(t_mid)
    const double2* h0_rimg;    // column-major H0
    const double2* g_rimg;     // [K] column-major G_k
    int K, m_max;              // controls; Taylor terms a step of the Krylov buffers holds
    double dt;
    double2* kv_f;             // [B][nsteps][m_max][NP] v_0 .. v_(m-1) of every step, or nullptr (no gradient wanted)
    double2* kv_b;             // [B][nsteps][m_max][NP] w_0 .. w_(m-1)
    double2* carry_f;          // [B][NP] the state between two forward launches
    int* degree_counts;        // [QOCX_ACTION_MAX_DEGREE + 1] steps of the forward sweep per degree
};
struct ActionGradArgs {
    const double2* kv_f;
    const double2* kv_b;
    const int* s_arr;
    const double2* g_rimg;
    int K, m_max, nsteps;
    int step0;                 // grid.x covers steps [step0, step0 + gridDim.x), grid.y the seeds
    double dt;
    double* gstep;             // [B][nsteps][K][2]: gamma_k as KrylovArgs::gstep under the unit adjoint
    // [K] E_k = -i dt G_k in the order of g_rimg, (re, im) = (dt G.y, -dt G.x): what action_grad_kernel
    // contracts with (qocx_action.hip). The problem setter builds it, where dt and the G_k are set.
    const double2* e_img = nullptr;
};
void launch_action_sweep(const ActionArgs& a, int batch, hipStream_t st);
void launch_action_grad(const ActionGradArgs& a, int nsteps, int batch, hipStream_t st);
int action_grad_lds_bytes(int m_max);
// ... with two to four states per seed at 17 <= n <= 32 (qocx_action_states.hip, knob "action_states"): a
// workgroup of sw.S waves per (seed, direction), wave s the state s. The same arguments with the state
// between the terms' step and degree: kv_f / kv_b [B][nsteps][S][m_max][NP], carry_f [B][S][NP]. The
// gradient kernel adds the states' cotangents of the generator and contracts once with the G_k.
struct ActionStatesGradArgs {
    ActionGradArgs g;
    int S;
};
void launch_action_states_sweep(const ActionArgs& a, int batch, hipStream_t st);
void launch_action_states_grad(const ActionStatesGradArgs& a, int nsteps, int batch, hipStream_t st);
// ... at 33 <= n <= 64 (qocx_action4.hip, knob "action" = 2; images and vectors padded to 64): workgroups
// of three (n <= 48) or four waves, each wave 16 columns of the generator; the same arguments, buffers
// and contract
void launch_action4_sweep(int n, const ActionArgs& a, int batch, hipStream_t st);
void launch_action4_grad(int n, const ActionGradArgs& a, int nsteps, int batch, hipStream_t st);
int action4_grad_lds_bytes(int n, int m_max, int K);
// ... at n <= 16 (qocx_action16.hip, knob "action_small" = 1; NP = 16 in the buffer shapes): one wave per
// seed whose four rows of 16 lanes do the four real products of a complex one; the same arguments,
// buffers and contract
void launch_action16_sweep(const ActionArgs& a, int batch, hipStream_t st);
void launch_action16_grad(const ActionGradArgs& a, int nsteps, int batch, hipStream_t st);
// ... one state at 17 <= n <= 32 under any set of device cost descriptors (qocx_action_costs.hip, knob
// "action_costs"): the same arguments and buffers; sw.unit_adjoint is 0, the forward launches carry the
// partial cost in sw.cost_out, the adjoint sweep carries the true cotangent and reads psi_j from kv_f,
// and gstep receives ONE real per (step, k) - [B][nsteps][K], KrylovArgs::gstep without the unit adjoint
void launch_action_costs_sweep(const ActionArgs& a, int batch, hipStream_t st);
void launch_action_costs_grad(const ActionGradArgs& a, int nsteps, int batch, hipStream_t st);

// Magnus M4 / M6 generator kernels (qocx_magnus.hip)
struct MagnusArgs {
    const double* controls;    // [B][nc][K]
    const StepInterp* interp;  // [nsteps * nodes]
    const double2* h0_cimg;    // [nt] C-images, nt = 1 or nsteps * nodes
    const double2* g_cimg;     // [nt][K]
    int K, nc, nsteps, nt, nodes;
    int step0, seg_len;        // work item w -> (seed w / seg_len, step step0 + w % seg_len)
    int skew;                  // every H0(t), G_k(t) Hermitian: one product per commutator
    double dt;
    double2* m_rm;             // fwd out: [B][nsteps] row-major padded generators
    const double2* mbar_rm;    // vjp in : cotangents of the generators
    double* gstep;             // vjp out: [B][nsteps * nodes][K]
    double2* scratch;          // [blocks][11] lane-linear matrix dumps
    size_t total;              // B * seg_len work items
    int n = 0;                 // Hilbert size (qocx_magnus4w.hip: 33..48 -> the three-wave form)
};

// Effective controls (qocx_effctl.hip): a step generator that is LINEAR in Ke effective controls
// over an augmented operator set runs on the M2 kernels unchanged. What the two routes share:
struct EffCtlArgs {
    const double* controls;    // [B][nc][K]
    const StepInterp* interp;  // the problem's table: [nsteps * 2] (M4-linear), [nsteps] (quadratic)
    int K, Ke, nc, nsteps, S;
    double* veff;              // controls kernel out: [B][nsteps][Ke]
    const double* gstep;       // chain kernel in: [B][nsteps][Ke] (x 2: complex, unit adjoint)
    const double2* lam_scale;  // unit adjoint: [B][S] (see ScatterArgs), or nullptr
    double* gchain;            // chain kernel out, read by scatter_kernel (real, lam_scale applied):
                               // [B][nsteps * 2][K] (M4-linear), [B][nsteps][K] (quadratic)
    size_t total;              // B * nsteps
};

// Magnus M4 with time-independent H0, G_k ("commutator-free" form):
//   m4 = -i dt (H0 + sum_k v_k G_k + sum_k w_k A_k + sum_{k<l} z_kl B_kl),
//   A_k = -i [G_k, H0], B_kl = -i [G_k, G_l],
//   v_k = (u1_k + u2_k) / 2, w_k = F0 dt (u2_k - u1_k), z_kl = F0 dt (u2_k u1_l - u2_l u1_k)
// with u1, u2 the controls at the two quadrature nodes: Ke = 2 K + K (K - 1) / 2.
#define QOCX_M4LIN_MAX_K 8
struct M4LinArgs : EffCtlArgs {
    double f0dt;               // F0 * dt
};

// Hamiltonian quadratic in the real controls: Ke = K + count effective controls
struct QuadArgs : EffCtlArgs {
    const int* pairs;          // [count][2], k <= l
    int count;
    // Per-member scales of the terms (qocx_set_ensemble_quadratic_scales): item i of the evaluation
    // is member i % M of its seed, and its term q is c_(m,q) r_k r_l Q_q. nullptr: no scales - the
    // launch then takes the kernels without them.
    const double* term_scales = nullptr;  // [M][count]
    int M = 1;
    size_t item0 = 0;          // evaluation index of the chunk's first item (B above is the chunk's)
};

// Hamiltonian ensemble (qocx_ensemble.hip): B seeds x M members, K = Kr + J channels per member
struct EnsembleArgs {
    const double* seed_controls;  // expand in: [B][nc][Kr]
    const double* scales;         // [M][Kr]
    const double* offsets;        // [M][J] (J > 0)
    const double* weights;        // [M]
    double* controls;             // expand out: [B][M][nc][K]
    const double* member_cost;    // reduce in: [B][M]
    const double* member_grads;   // reduce in: [B][M][nc][K]
    double* cost;                 // reduce out: [B]
    double* grads;                // reduce out: [B][nc][Kr], or nullptr (no gradients)
    int B, M, nc, K, Kr, J;
};

// Hamiltonian sweep (qocx_sweep.hip): B seeds, each its own item on K = Kr + J channels
#define QOCX_SWEEP_LANES 64     // partial sums of a sensitivity (the summation order: qocx_sweep.hip)
struct SystemSweepArgs {
    const double* seed_controls;  // expand / sensitivity in: [B][nc][Kr]
    const double* scales;         // [B][Kr]
    const double* offsets;        // [B][J] (J > 0)
    double* controls;             // expand out: [B][nc][K]
    const double* item_cost;      // reduce in: [B]
    const double* item_grads;     // reduce / sensitivity in: [B][nc][K]
    double* cost;                 // reduce out: [B]
    double* grads;                // reduce out: [B][nc][Kr], or nullptr (no gradients)
    double* scale_sens;           // sensitivity out: [B][Kr]
    double* offset_sens;          // sensitivity out: [B][J] (J > 0)
    int B, nc, K, Kr, J;
};

struct ScatterArgs {
    const double* gstep;
    const int* row_ptr;   // [nc+1]
    const int* col_step;  // [nnz]
    const double* weight; // [nnz]
    double* grads;        // [B][nc][K]
    int B, nc, K, nsteps;
    const double2* lam_scale = nullptr;  // unit adjoint: [B][S] (entry of state 0 is used), gstep holds
    int S = 1;                           // complex numbers (see KrylovArgs); nullptr: gstep is real
};

// One sub-interval of the fixed-step Lindblad integrator: [t_a, t_b] inside system step `step`,
// never straddling a control knot; u(t_a), u(t_b) by linear interpolation on the control grid.
struct SubStep {
    double h;
    int ia1, ia2, ib1, ib2;
    double wa1, wa2, wb1, wb2;
    int step;
    int first_of_step;
};

struct LindbladArgs {
    const double* controls;    // [B][nc][K]
    const SubStep* substeps;   // [nsub]
    const double2* a0l_cimg;   // C-dumps (256 complex): A0L, A0R and their conjugate transposes
    const double2* a0r_cimg;
    const double2* a0ld_cimg;
    const double2* a0rd_cimg;
    const double2* gp_cimg;    // [K] Gp_k = -i G_k
    const double2* gpd_cimg;   // [K] Gp_k^H
    const double2* gpt_cimg;   // [K] Gp_k^T
    const double2* a0_tab;     // time-dependent H: [nsub * 12][4] dumps A0L, A0R, A0L^H, A0R^H at the
                               // stage times, or nullptr
    const double2* gp_tab;     // time-dependent G: [nsub * 12][K][3] dumps Gp, Gp^H, Gp^T, or nullptr
    const double2* op_tab;     // time-dependent lindblad_data: [nsub * 12][nops] dumps of L_i at the
                               // stage times (+ gamma_tab [nsub * 12][nops]), or nullptr
    const double* gamma_tab;
    const double2* op_cimg;    // [nops] L_i (n > 32: then [nops] L_i^H)
    const double* gammas;      // [nops]
    const double2* rho0_cimg;  // [S]
    int n, S, K, nc, nops, nsub, nsteps, cost_eval_step, want_grad, has_step_costs;
    int cost_count;
    const DevCost* costs;
    const double2* cost_matrices;  // pooled C-dumps
    const int* cost_counts;
    double2* checkpoints;      // [B][nsub][S] C-dumps: densities at the start of each sub-interval
    int multi_wave;            // 1: nops + 2 wavefronts per seed (n <= 16, everything in LDS)
    int cache_gen;             // multi_wave: constant generator dumps copied to LDS
    double2* scratch;          // [B][2 S + 12] (n > 16: [B][2 S + 36], n > 32: [B][2 S + 31]) dumps when densities / cotangents / stage
                               // derivatives do not live in LDS (always for n > 16), else nullptr
    double2* ystages;          // [B][nsub][S][12] C-dumps of the stage values, or nullptr: the
                               // adjoint then recomputes them from the checkpoints
    double* gsub;              // [B][nsub][2][K] control cotangents at t_a / t_b
    double* cost_out;          // [B]
    double2* final_out;        // [B][S] C-dumps
    double2* step_densities;   // [B][nsteps+1][S] C-dumps or nullptr
    const int* inj_index;      // host-supplied density cotangents (see SweepArgs): [nsteps + 1]
    const double2* inj_bars;   // [B][inj_count][S] C-dumps
    int inj_count;
    unsigned long long* stamps;  // diagnostic build: [B][6 waves][8] cycle sums, or nullptr
    // Two-sided evaluation (several waves per seed, ONE final TargetDensityInfidelity): the
    // cotangent of a final density is a scalar times its target, and the adjoint of the discrete
    // scheme is linear in it, so it runs on the TARGET beside the forward pass (phase 2 beside
    // phase 1, two launches on two streams) and stores its stage cotangents kbar_i; a third kernel
    // (lindblad_combine) contracts them with the forward stage values and the scalars into the
    // control cotangents. phase 0: the classic forward-then-adjoint launch.
    int phase = 0;
    int hermitian = 0;             // every density and cotangent is Hermitian, A_R = A_L^H, Gp_k^H = -Gp_k (host-checked)
    int tile4 = 1;                 // 17 <= n <= 32: the tile-per-wave kernel (qocx_lindblad4t.hip) where it applies
    int q2 = 0;                    // phases 1 / 2, four waves: the stage loop with 18 MFMAs per wave (substep_q2)
    int chain = 0;                 // with q2, 2 <= nops <= 4: the stage loop with one barrier per stage (substep_chain)
    int ops_real = 0;              // every Lindblad operator has a zero imaginary part (host-checked): chain form only
    double2* kbstages = nullptr;   // [B][nsub][S][12] C-dumps of kbar_i (phase 2 out, combine in)
    double2* lam_scale = nullptr;  // [B][S]: phase 1 out
};

// Per-member dissipation rates (qocx_lindblad_set_ensemble_rates), the second argument of the kernels of
// qocx_lindblad_rates.hip / qocx_lindblad4t_rates.hip: workgroup b of the launch belongs to ensemble member
// item_member[b], and a0l / a0r / a0ld / a0rd_cimg and gammas of the LindbladArgs are the tables of member 0
// with these strides (in elements) to the next member. An argument of its own: LindbladArgs, and with it
// every kernel that runs without rates, is what it was without them.
struct LindbladMembers {
    const int* item_member = nullptr;  // [B], launch order
    size_t a0_stride = 0, gamma_stride = 0;
    // Called once at the top of a kernel, on its by-value copy of the arguments: folds the workgroup's member
    // into the base pointers, so no read site below knows about members. The index is uniform over the
    // workgroup (one scalar load of item_member[blockIdx.x]); nothing is added inside a stage.
    __device__ __forceinline__ void select(LindbladArgs& a) const {
        const size_t m = (size_t)item_member[blockIdx.x];
        a.a0l_cimg += m * a0_stride;
        a.a0r_cimg += m * a0_stride;
        a.a0ld_cimg += m * a0_stride;
        a.a0rd_cimg += m * a0_stride;
        a.gammas += m * gamma_stride;
    }
};

// Rate sensitivities of a two-sided evaluation (qocx_lindblad_ratesens.hip), the second argument of its
// kernels beside the LindbladArgs of the piece's combine launch (ystages, kbstages, lam_scale, op_cimg).
struct RateSensArgs {
    const double2* ldl_cimg = nullptr;  // [L] C-dumps of L_l^H L_l
    const double* gammas = nullptr;     // [L] the problem's own rates gamma_l (never a member's)
    double* partials = nullptr;         // kernel out: [Bp][nsub][L], one per (item, sub-interval, l)
    double* out = nullptr;              // reduce out: [Bp][L], launch order
    int nops = 0;                       // L: the problem's operators (without the zero one of pad_op)
};

// ---- Hilbert sizes above 64 (qocx_general.hip): row-major padded np x np matrices in HBM, np = 16 ceil(n / 16) ----
struct GeneralArgs {  // K1a + K1b: one work item per (seed, step), `total` = seeds * nsteps
    int np, K, nc, nsteps, nt;
    double dt;
    const double* controls;    // [B][nc][K]
    const StepInterp* interp;  // [nsteps]
    const double2* h0_rm;      // [nt] row-major
    const double2* g_rm;       // [nt][K]
    const double2* gen_rm;     // explicit mode: [B][nsteps] generators sampled by the host, else nullptr
    int pade_policy, sq_max;
    double2* q_img;            // out: Q, row-major
    double2* pinv_img;         // out: P^-1, row-major
    int* s_arr;
    int* status;
    double2* scratch;          // [blocks][7] matrices
    size_t total;
};
struct GeneralSweepArgs {  // K2: one workgroup per seed
    int np, S, nsteps, cost_eval_step, has_step_costs, phase;  // phase bit 0 forward, bit 1 adjoint
    const double2* q_img;
    const double2* pinv_img;
    const int* s_arr;
    const double2* psi0;       // [S][np]
    size_t slot_cap;
    double2* states;           // [B][slot_cap][S][np]
    double2* xs;
    int* offs;                 // [B][nsteps + 1]
    double2* lam_buf;          // [B][S][np]
    int cost_count;
    const DevCost* costs;
    const double2* cost_vectors;
    const int* cost_counts;
    const int* inj_index;
    const double2* inj_bars;
    int inj_count;
    double* cost_out;
    double2* final_out;
    double2* step_states;
    int* status;
};
struct GeneralKrylovArgs {  // K3: one work item per (seed, step)
    int np, S, K, nc, nsteps, nt;
    double dt;
    const double* controls;
    const StepInterp* interp;
    const double2* h0_rm;
    const double2* g_rm;
    const double2* gen_rm;     // explicit mode (then mbar_rm receives the generator cotangents)
    double2* mbar_rm;
    const int* s_arr;
    const int* offs;
    const double2* states;
    const double2* xs;
    size_t slot_cap;
    double* gstep;             // [B][nsteps][K]
    double2* scratch;          // [blocks][3] matrices
    size_t total;
    int skew = 0;              // the generator is skew-Hermitian bit for bit (Hermitian H): both chains run on a^H, one pass each
};
int general_factor_lds(int np);
int general_sweep_lds(int np);
int general_krylov_lds(int np);
int launch_general_factor(const GeneralArgs& a, int blocks, hipStream_t st);
void launch_general_sweep(const GeneralSweepArgs& a, int batch, hipStream_t st);
int launch_general_krylov(const GeneralKrylovArgs& a, int blocks, hipStream_t st);

// Multi-start driver on the device (qocx_optim.hip)
struct OptimArgs {
    int kind;  // 0 SGD, 1 Adam
    double* params;              // [B][per_seed] = the resident controls
    const double* grads;         // [B][per_seed]
    double* moment;              // Adam: [B][per_seed]
    double* square_moment;
    const unsigned char* update; // [B]: seeds that take the step
    size_t per_seed;
    double learning_rate, beta_1, beta_2, one_m_b1, one_m_b2, epsilon, corr_1, corr_2, clip;
    int apply_clip;
};
// One element of Adam.update / SGD.update (adam.py:110-165, sgd.py): the arithmetic of
// optimizer_update_kernel and of duration_step_kernel, one definition. Every product and sum is
// rounded on its own; division and square root are the IEEE ones.
__device__ __forceinline__ void optimizer_update_element(const OptimArgs& a, size_t e) {
#pragma clang fp contract(off)
    double g = a.grads[e];
    if (a.kind == 0) {  // SGD: params - learning_rate * grads
        const double s = a.learning_rate * g;
        a.params[e] = a.params[e] - s;
        return;
    }
    if (a.apply_clip) g = g < -a.clip ? -a.clip : (g > a.clip ? a.clip : g);
    const double m0 = a.beta_1 * a.moment[e], m1 = a.one_m_b1 * g;
    const double m = m0 + m1;
    const double sq = g * g;
    const double v0 = a.beta_2 * a.square_moment[e], v1 = a.one_m_b2 * sq;
    const double v = v0 + v1;
    a.moment[e] = m;
    a.square_moment[e] = v;
    const double mh = m / a.corr_1, vh = v / a.corr_2;
    const double den = sqrt(vh) + a.epsilon;
    const double q = mh / den;
    const double s = a.learning_rate * q;
    a.params[e] = a.params[e] - s;
}
// Duration search of a sweep (qocx_duration.hip, qocx_sweep_set_durations): tau_b = T_b / T is one
// more parameter of seed b; the sweep's tables are tau_b times the base tables s0, delta0
struct DurationArgs {
    double* tau;                  // [B]: read, clipped to [tau_min, tau_max], written back
    const double* base_scales;    // s0 [B][Kr]
    const double* base_offsets;   // delta0 [B][J] (column 0, the drift, is 1)
    double* scales;               // tables out: [B][Kr] = tau_b s0_bk
    double* offsets;              // tables out: [B][J] = tau_b delta0_bj
    const double* scale_sens;     // gradient in: [B][Kr] (sweep_sensitivity_kernel)
    const double* offset_sens;    // gradient in: [B][J]
    double* tau_grad;             // gradient out: [B] dE_b/dtau_b + time_weight, or nullptr (none wanted)
    double* cost;                 // [B] seed costs: cost_b + time_weight tau_b
    double tau_min, tau_max, time_weight;
    int B, Kr, J;
};
struct DurationStepArgs {
    OptimArgs rule;               // params = tau, grads = tau_grad, the moments [B]; per_seed = 1
    double* best_tau;             // [B]
    const unsigned char* improved;  // [B]: seeds whose tau is kept as the best so far
    int B;
};
// Duration search of a Lindblad sweep (qocx_lindblad_duration.hip, qocx_lindblad_sweep_set_durations):
// the per-seed control-free generators and rates are tau_b times base tables built at tau = 1, and the
// chain rule runs through the scales, the offsets and the rate factors c_bl = tau_b c0_bl
struct LindbladDurationArgs {
    const double* tau;            // [B], clipped by duration_tables_kernel
    const double2* base_a0;       // [B][4] dumps A0L, A0R, A0L^H, A0R^H of the rates c0_b gamma
    double2* a0;                  // tables out: [B][4] dumps = tau_b base_a0
    const double* base_gammas;    // [B][Lp]: c0_bl gamma_l
    double* gammas;               // tables out: [B][Lp] = tau_b base_gammas
    const double* base_scales;    // s0 [B][Kr]
    const double* base_offsets;   // delta0 [B][J]
    const double* base_rates;     // c0 [B][L]
    const double* scale_sens;     // gradient in: [B][Kr], seed order (sweep_sensitivity_kernel)
    const double* offset_sens;    // gradient in: [B][J], seed order
    const double* rate_sens;      // gradient in: [B][L], LAUNCH order (qocx_lindblad_ratesens.hip)
    const int* order;             // [B]: the seed launched at position p
    double* tau_grad;             // gradient out: [B] dE_b/dtau_b + time_weight, or nullptr (none wanted)
    double* cost;                 // [B] seed costs: cost_b + time_weight tau_b
    double time_weight;
    size_t a0_per_seed;           // 4 md double2
    int B, Kr, J, L, Lp;
};

void launch_clip_controls(double* controls, size_t total, int k, const double* max_norms, hipStream_t st);
void launch_keep_best(const double* controls, double* best_controls, size_t per_seed,
                      const double2* final_states, double2* best_final, size_t final_per_seed,
                      const unsigned char* improved, int batch, hipStream_t st);
void launch_optimizer_update(const OptimArgs& a, int batch, hipStream_t st);
// complex controls: controls[b][j][2k .. 2k+1] = params clipped by modulus to max_norms[k]; params stay
void launch_clip_complex(const double* params, double* controls, size_t pairs, int k,
                         const double* max_norms, hipStream_t st);

// The linear map of a control basis (qocx_ctrlbasis.hip; qoc_amd/standard/controlbasis.py): each
// output summed in increasing index, acc = acc + M * x from +0.0, product and sum rounded on their own
// matrix_t [P][Nc], coef [B][P][C] -> out [B][Nc][C]
void launch_basis_expand(const double* matrix_t, const double* coef, double* out, int batch, int nc,
                         int p_count, int channels, hipStream_t st);
// matrix [Nc][P], grads [B][Nc][C] -> out [B][P][C]
void launch_basis_project(const double* matrix, const double* grads, double* out, int batch, int nc,
                          int p_count, int channels, hipStream_t st);

// L-BFGS with Armijo backtracking for the seeds of the multi-start driver (qocx_lbfgs.hip;
// qoc_amd/standard/optimizers/lbfgs.py is the statement of the algorithm)
enum { LBFGS_MAX_HISTORY = 64 };
struct LbfgsSeed {  // the scalars of one seed
    double f, t, gamma;  // accepted error; step along d; s.y / y.y of the newest pair
    int bt, steepest, started, finished;
    int head, count;     // ring of pairs: slot of the oldest, pairs stored
};
struct LbfgsArgs {
    double* params;              // [B][per_seed]: the evaluated point in, the next trial point out
    const double* grads;         // [B][per_seed] gradients of the last evaluation
    const double* cost;          // [B] its total costs
    double* x;                   // [B][per_seed] accepted point
    double* g;                   // [B][per_seed] its gradient
    double* d;                   // [B][per_seed] direction (the two-loop recursion's q on the way)
    double* s;                   // [B][history][per_seed] ring of steps
    double* y;                   // [B][history][per_seed] ring of gradient differences
    double* rho;                 // [B][history] 1 / s.y
    LbfgsSeed* seed;             // [B]
    const unsigned char* update; // [B]: seeds that take the step
    unsigned char* finished;     // [B] out
    size_t per_seed;
    // complex controls: element i of the host's parameter vector (all real parts, then all imaginary
    // parts) lives at 2 i / 2 (i - per_seed / 2) + 1 in the device's interleaved channels; inner
    // products run in the host's element order
    int interleaved;
    int history;
    double first_step, armijo, shrink;
    int max_backtracks;
};
void launch_lbfgs_step(const LbfgsArgs& a, int batch, hipStream_t st);

// Costs of the controls alone (qocx_ctrlcost.hip; qoc/standard/costs/control*.py)
struct CtrlCostDev {
    int kind, order;    // QOCX_CONTROL_*; ControlVariation: order of the difference
    double multiplier;  // cost_multiplier with the cost's normalisation constant folded in
    const double* max_norms;  // [K] per control (ones when the cost has none)
    const double* weights;    // [K] ControlNorm (ones when it has none)
};
struct CtrlCostArgs {
    const double* controls;  // [B][nc][Kr]; a complex control k is the channels 2k, 2k+1
    double* cost;            // out [B]: the sum of the control costs
    double* grad;            // out [B][nc][Kr]: its gradient, or nullptr
    double* work0;           // [B][nc][Kr] each: the difference passes of ControlVariation
    double* work1;
    const CtrlCostDev* descs;  // the costs that are not bandwidth costs, in the caller's order
    int count;
    int B, nc, Kr, cplx;
};
// one ControlBandwidthMax: the bins P_k of control k are bins[bin_ptr[k] .. bin_ptr[k + 1])
struct BandwidthArgs {
    const double* controls;  // [B][nc][Kr]
    const double2* twiddle;  // [nc]: exp(-2 pi i m / nc)
    const int* bins;
    const int* bin_ptr;      // [K + 1]
    double2* spectrum;       // [B][Kr][pmax]: the DFT of every real channel at the bins of its control
    double2* ybar;           // [B][K][pmax]: the cotangents of the bins
    double* cost;            // [B], added to
    double* grad;            // [B][nc][Kr], added to, or nullptr
    double multiplier;       // cost_multiplier / control_count
    int B, nc, Kr, K, cplx, pmax;
};
void launch_control_costs(const CtrlCostArgs& a, hipStream_t st);
void launch_bandwidth_cost(const BandwidthArgs& a, hipStream_t st);
// cost[b] += add_cost[b]; grads[e] += add_grad[e] (grads may be nullptr): one addition per entry
void launch_add_control_costs(double* cost, const double* add_cost, double* grads, const double* add_grad,
                              int batch, size_t per_seed, hipStream_t st);
// the Lindblad multi-start driver: per-seed control maxima, seed order <-> sub-division group order
void launch_control_maxima(const double* controls, int batch, int nc, int k, double* umax, hipStream_t st);
void launch_gather_seeds(const double* src, double* dst, size_t per_seed, const int* order, int batch,
                         hipStream_t st);
void launch_scatter_seeds(const double* cost, double* cost_out, const double* grads, double* grads_out,
                          size_t grad_per_seed, const double2* final_states, double2* final_out,
                          size_t final_per_seed, const int* order, int batch, hipStream_t st);

// The kernel of a launch is the host's to name (qocx_lindblad_route.h: lindblad_route); the launchers decide
// nothing. `stamped`: the four-wave kernels in their stamped builds (diagnostic library only). Nonzero: the
// launcher has no such kernel, and nothing was launched.
enum class LindbladKernel : int;
int launch_lindblad(LindbladKernel kernel, bool stamped, const LindbladArgs& a, int batch, hipStream_t st);
void launch_lindblad_combine(const LindbladArgs& a, int batch, hipStream_t st);
void launch_lindblad4t(bool hermitian, const LindbladArgs& a, int batch, hipStream_t st);
void launch_lindblad4t_combine(const LindbladArgs& a, int batch, hipStream_t st);
int launch_lindblad_rates(LindbladKernel kernel, bool stamped, const LindbladArgs& a, const LindbladMembers& mem,
                          int batch, hipStream_t st);
void launch_lindblad4t_rates(bool hermitian, const LindbladArgs& a, const LindbladMembers& mem, int batch,
                             hipStream_t st);
void launch_lindblad_ratesens(const LindbladArgs& a, const RateSensArgs& r, int batch, hipStream_t st);
int lindblad_lds_size(int n, int S, int nops, int mode, int K);
size_t lindblad_scratch_elems(int n, int S);
// 33 <= n <= 64 (qocx_lindblad16t.hip; the host accepts such problems under the knob lindblad_wide)
void launch_lindblad16t(const LindbladArgs& a, int batch, hipStream_t st);
int lindblad16t_lds_bytes();
size_t lindblad16t_scratch_elems(int S);

void launch_pq(int nb, const FactorArgs& a, int nsteps, int batch, hipStream_t st);
void launch_pq_explicit(int nb, const double2* a_in, int n, const FactorArgs& a, int count,
                        hipStream_t st);
// two-wave K1a for nb == 2 (qocx_pade2.hip)
void launch_pq2(const FactorArgs& a, int nsteps, int batch, hipStream_t st);
bool pq3_supports(const FactorArgs& a);
void launch_pq3(const FactorArgs& a, int nsteps, int batch, hipStream_t st);
// q_img := P^-1 Q of `count` steps (work item w -> seed w / seg_len, step step0 + w % seg_len), n <= 32
// (qt_img: where the transposed images go, for the adjoint sweep)
void launch_umul(int nb, const LuArgs& a, double2* q_img, double2* qt_img, size_t count, hipStream_t st);
bool pq3_parks(const FactorArgs& a, int nsteps);
void launch_pq3_second(const FactorArgs& a, int nsteps, int batch, hipStream_t st);
// true: launch_pq left the second halves of the factorisations to launch_pq3_second (FactorArgs::four_steps == 2)
bool pq_second_pending(int nb, const FactorArgs& a, int nsteps);
void launch_pq2_explicit(const double2* a_in, int n, const FactorArgs& a, int count, hipStream_t st);
// 33 <= n <= 64: four-wave workgroups (qocx_pade4.hip)
void launch_pq4(const FactorArgs& a, int nsteps, int batch, hipStream_t st);
void launch_pq4_explicit(const double2* a_in, int n, const FactorArgs& a, int count, hipStream_t st);
// ... and the four-wave K1b / K3 of qocx_big.hip
void launch_lu4(const LuArgs& a, size_t count, hipStream_t st);
void launch_lu4m(const LuArgs& a, size_t count, int* redo, hipStream_t st);  // qocx_lu4m.hip
void launch_krylov4(const KrylovArgs& a, int nsteps, int batch, hipStream_t st);
void launch_lu(int nb, const LuArgs& a, size_t count, hipStream_t st);
void launch_sweep(int nb, const SweepArgs& a, int batch, hipStream_t st);
int sweep_lds_bytes(int nb, int S);
// blocked-inverse sweep (qocx_sweep3.hip): three wavefronts per seed
void launch_sweep3(int nb, const SweepArgs& a, int batch, hipStream_t st);
// dense-state sweep (qocx_sweepd.hip): the states of a seed as GEMM columns; lu_img holds P^-1
bool sweepd_supports(int nb, int S);
void launch_sweepd(const SweepArgs& a, int batch, hipStream_t st);
// inverse-image sweep of latency mode (qocx_sweepi.hip): two matrix-vector products per sub-step
bool sweepi_supports(int nb, int S);
bool sweep1_supports(int nb, int S);
void launch_sweep1(int nb, const SweepArgs& a, int batch, hipStream_t st);
void launch_sweepi(int nb, const SweepArgs& a, int batch, hipStream_t st);
int sweep3_max_states(int nb);
void launch_krylov(int nb, const KrylovArgs& a, int nsteps, int batch, hipStream_t st);
void launch_scatter(const ScatterArgs& a, hipStream_t st);
// out[0] = sum_b cost[b]; out[1 + j] = sum_b grads[b][j], j < per_seed (seeds in index order)
void launch_reduce_results(const double* cost, const double* grads, int batch, int per_seed,
                           double* out, hipStream_t st);
void launch_mfma_peak(double* out, int blocks, int iters, hipStream_t st);
#ifdef QOCX_DIAG
void launch_pipe_mix(double* out, int blocks, int iters, int mode, hipStream_t st);
#endif
void launch_magnus_fwd(int nb, const MagnusArgs& a, int blocks, hipStream_t st);
void launch_magnus_vjp(int nb, const MagnusArgs& a, int blocks, hipStream_t st);
size_t magnus_scratch_elems(int nb, int blocks);
// multi-wave, LDS-resident forms for 17 <= n <= 48 (qocx_magnus4w.hip); grid = (a.seg_len, batch)
bool magnus4w_supports(int nb, int K, int n);
void launch_magnus4w_fwd(const MagnusArgs& a, int batch, hipStream_t st);
void launch_magnus4w_vjp(const MagnusArgs& a, int batch, hipStream_t st);
void launch_m4lin_controls(const M4LinArgs& a, hipStream_t st);
void launch_m4lin_chain(const M4LinArgs& a, hipStream_t st);
void launch_quad_controls(const QuadArgs& a, hipStream_t st);
void launch_quad_chain(const QuadArgs& a, hipStream_t st);
void launch_ensemble_expand(const EnsembleArgs& a, hipStream_t st);
void launch_ensemble_reduce(const EnsembleArgs& a, hipStream_t st);
void launch_sweep_expand(const SystemSweepArgs& a, hipStream_t st);
void launch_sweep_reduce(const SystemSweepArgs& a, hipStream_t st);
void launch_sweep_sensitivity(const SystemSweepArgs& a, hipStream_t st);
void launch_duration_tables(const DurationArgs& a, hipStream_t st);
void launch_duration_gradient(const DurationArgs& a, hipStream_t st);
void launch_duration_step(const DurationStepArgs& a, hipStream_t st);
void launch_lindblad_duration_generators(const LindbladDurationArgs& a, hipStream_t st);
void launch_lindblad_duration_gradient(const LindbladDurationArgs& a, hipStream_t st);
void launch_selftest(double* out, hipStream_t st);

}  // namespace qocx

#endif
