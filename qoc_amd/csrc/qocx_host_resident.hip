// qocx_host_resident.hip - the evaluation of the uploaded items of a Schroedinger problem
// (eval_items, behind qocx_eval_resident): the general path for Hilbert sizes above 64 and the
// resident pipeline of the wavefront kernels - route, buffers, chunks, schedules.
#include "qocx_host.h"
#include "qocx_effctl.h"

// Evaluation for Hilbert sizes above 64 (qocx_general.hip): classic order, one stream - factor every step,
// forward sweep, adjoint sweep, K3, scatter - per memory chunk of seeds.
namespace qocx {
size_t general_krylov_scratch(int np, int S);
void launch_general_magnus(const MagnusArgs& a, bool vjp, int blocks, hipStream_t st);
}
// the end of an evaluation of the uploaded items: waits for it and reads the kernels' status word
// (finish_items: a step of the matrix-free route asked for a degree beyond its buffers)
static constexpr int kActionRefused = -0x7a11;
static int finish_items(qocx_ctx* ctx, int want_grad) {
    HIP_TRY(hipGetLastError());
    int status = 0;
    HIP_TRY(hipMemcpyAsync(&status, ctx->status.p, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    time_collect(ctx);
    if (status & 8) return kActionRefused;  // eval_items runs the evaluation again on the Pade route
    if (status & 2) return fail(QOCX_ERR_ARG, "non-finite generator norm");
    if (status & 1) return fail(QOCX_ERR_SINGULAR, "Singular matrix");
    if (status & 4) return fail(QOCX_ERR_CAPACITY, "squaring sub-step capacity exceeded");
    ctx->have_results = true;
    ctx->have_grads = want_grad != 0;
    ctx->have_step_states = ctx->keep_step_states != 0;
    return 0;
}

using EffKind = EffectiveControls::Kind;

// The effective-control route of a chunk of `bc` seeds from item `b0` of the evaluation
// (qocx_effctl.hip): the controls kernel in front of K1a, the argument blocks of K1a and K3
// redirected to what it wrote, the chain kernel in front of scatter_kernel. With an ensemble the
// items are its members; its term scales, if set, go along (qocx_set_ensemble_quadratic_scales).
struct EffCtlChunk {
    qocx_ctx* ctx = nullptr;
    EffKind kind = EffectiveControls::NONE;
    hipStream_t st = nullptr;
    qocx::M4LinArgs m4;
    qocx::QuadArgs qa;

    static int channels(const qocx_ctx* ctx, EffKind kind) { return kind ? ctx->eff.Ke : ctx->K; }  // as K1a / K3 see them
    // veff and the chain output of chunks of `cm` (seed, step) pairs
    static int reserve(qocx_ctx* ctx, EffKind kind, size_t cm, int want_grad) {
        if (!kind) return 0;
        const size_t per_step = kind == EffectiveControls::M4_LINEAR ? 2 * ctx->K : ctx->K;
        return ctx->eff.veff.ensure(cm * ctx->eff.Ke) || ctx->eff.gchain.ensure(want_grad ? cm * per_step : 1);
    }

    // fills the args; lam_scale: the chunk's scalars under the unit adjoint, which the chain kernel then applies
    void set(qocx_ctx* c, EffKind k, const double* controls, const double2* lam_scale, int b0, int bc,
             hipStream_t stream) {
        ctx = c; kind = k; st = stream;
        if (!kind) return;
        qocx::EffCtlArgs& a = kind == EffectiveControls::M4_LINEAR ? (qocx::EffCtlArgs&)m4 : qa;
        a.controls = controls; a.interp = ctx->interp.p;
        a.K = ctx->K; a.Ke = ctx->eff.Ke; a.nc = ctx->nc; a.nsteps = ctx->nsteps; a.S = ctx->S;
        a.veff = ctx->eff.veff.p; a.gstep = ctx->gstep.p; a.lam_scale = lam_scale; a.gchain = ctx->eff.gchain.p;
        a.total = (size_t)bc * ctx->nsteps;
        if (kind == EffectiveControls::M4_LINEAR) {
            m4.f0dt = (std::sqrt(3.0) / 12) * ctx->dt;
        } else {
            qa.pairs = ctx->eff.pairs_dev.p; qa.count = ctx->eff.quad_count();
            if (ctx->seeds.M > 0 && ctx->ens_qscales_set) {
                qa.term_scales = ctx->ens_qscales.p; qa.M = ctx->seeds.M; qa.item0 = (size_t)b0;
            }
        }
    }

    // ... and launches the controls kernel (`timed`: as a launch of K1a)
    void begin(qocx_ctx* c, EffKind k, const double* controls, const double2* lam_scale, int b0, int bc,
               hipStream_t stream, bool timed) {
        set(c, k, controls, lam_scale, b0, bc, stream);
        if (!kind) return;
        if (timed) time_begin(ctx, 0, st);
        if (kind == EffectiveControls::M4_LINEAR) qocx::launch_m4lin_controls(m4, st);
        else qocx::launch_quad_controls(qa, st);
        if (timed) time_end(ctx, st);
    }

    // ... or, on the matrix-free route, the step table of qocx_action_eff.hip in place of the controls kernel:
    // the same veff, and the step words with the Taylor degrees (degree_rule: qocx_action.h)
    void table(qocx_ctx* c, EffKind k, const double* controls, const double2* lam_scale, int b0, int bc,
               hipStream_t stream, int degree_rule) {
        set(c, k, controls, lam_scale, b0, bc, stream);
        if (!kind) return;
        qocx::EffTableArgs ta;
        ta.dt = ctx->dt; ta.h0_norm = ctx->h0_norm_max; ta.h0_norm2 = ctx->h0_norm2_max;
        ta.norm1 = ctx->eff.op_norm1_dev.p; ta.norm2 = ctx->eff.op_norm2_dev.p;
        ta.degree_rule = degree_rule;
        ta.s_arr = ctx->s_arr.p; ta.status = ctx->status.p;
        time_begin(ctx, 0, st);
        if (kind == EffectiveControls::M4_LINEAR) qocx::launch_m4lin_table(m4, ta, st);
        else qocx::launch_quad_table(qa, ta, st);
        time_end(ctx, st);
    }

    // K1a: a row of Ke effective controls per step through the identity table; `g`: its operator images
    template <class Args>
    void redirect(Args& a, const double2*& g, const DevBuf<double2>& image) const {
        if (!kind) return;
        a.controls = ctx->eff.veff.p; a.interp = ctx->eff.interp_id.p; g = image.p;
        a.K = ctx->eff.Ke; a.nc = ctx->nsteps;
    }
    void redirect(qocx::KrylovArgs& ka) const {  // (K3's controls follow FactorArgs)
        if (kind) { ka.g_rimg = ctx->eff.images.r.p; ka.g_timg = ctx->eff.images.t.p; }
    }

    // launches the chain kernel; returns the buffer scatter_kernel must read
    const double* chain(const double* gstep) const {
        if (!kind) return gstep;
        if (kind == EffectiveControls::M4_LINEAR) qocx::launch_m4lin_chain(m4, st);
        else qocx::launch_quad_chain(qa, st);
        return ctx->eff.gchain.p;
    }
};

// per-step control cotangents -> the control gradients of the chunk [b0, b0 + bc); lam_scale: the
// chunk's scalars under the unit adjoint (the chain kernel, where there is one, has applied them)
static void scatter_gradients(qocx_ctx* ctx, const EffCtlChunk& eff, const double* gstep, const double2* lam_scale,
                              int b0, int bc, hipStream_t cs) {
    qocx::ScatterArgs sc;
    sc.row_ptr = ctx->row_ptr.p; sc.col_step = ctx->col_step.p; sc.weight = ctx->weight.p;
    sc.grads = ctx->grads.p + (size_t)b0 * ctx->nc * ctx->K;
    sc.B = bc; sc.nc = ctx->nc; sc.K = ctx->K; sc.nsteps = ctx->nsteps * ctx->nodes;
    sc.lam_scale = eff.kind ? nullptr : lam_scale;
    sc.S = ctx->S;
    time_begin(ctx, 3, cs);
    sc.gstep = eff.chain(gstep);
    qocx::launch_scatter(sc, cs);
    time_end(ctx, cs);
}

static int eval_general(qocx_ctx* ctx, int want_grad) {
    const int B = ctx->B, np = ctx->np, S = ctx->S, K = ctx->K, nsteps = ctx->nsteps;
    const size_t mat = (size_t)np * np;
    const bool explicit_gen = ctx->explicit_mode;
    // M4 with a time-independent system, or M2 with H quadratic in the real controls: linear in
    // effective controls over constant / augmented matrices (EffCtlChunk)
    const EffKind effk = ctx->effctl_kind(false);
    // M6, and M4 on a time-dependent system: generators and reverse rules by qocx_general.hip's magnus_kernel
    const bool magnus = ctx->nodes > 1 && effk != EffectiveControls::M4_LINEAR && !explicit_gen;
    const int nodes = magnus ? ctx->nodes : 1;
    const int Kk = EffCtlChunk::channels(ctx, effk);
    const size_t per_seed = (size_t)nsteps * (mat * 32 + 4) + ctx->slot_cap * S * np * 32 +
                            (size_t)(nsteps + 1) * 4 + (size_t)nsteps * std::max(Kk, 1) * 40;
    // (persistent workgroups with 7 scratch matrices each: as many as 16 GB hold, two per CU at most)
    const int max_blocks = (int)std::max<size_t>(1, std::min<size_t>((size_t)2 * ctx->cu_count, ((size_t)16 << 30) / (7 * mat * 16)));
    int chunk = ctx->chunk_user;
    if (chunk <= 0) {
        size_t free_b = 0, total_b = 0;
        HIP_TRY(hipMemGetInfo(&free_b, &total_b));
        const size_t have = ctx->q_img.count * 16 + ctx->lu_img.count * 16 + ctx->states.count * 16 +
                            ctx->xs.count * 16 + ctx->magnus_scratch.count * 16;
        const size_t fixed = (size_t)max_blocks * 7 * mat * 16;
        const size_t budget = (size_t)((double)(free_b + have) * 0.6);
        chunk = (int)std::min<size_t>((size_t)B, std::max<size_t>(1, (budget > fixed ? budget - fixed : 0) / per_seed));
    }
    chunk = std::min(chunk, B);
    const size_t cm = (size_t)chunk * nsteps;
    const int blocks = (int)std::min<size_t>(cm, (size_t)max_blocks);
    if (ctx->q_img.ensure(cm * mat) || ctx->lu_img.ensure(cm * mat) || ctx->s_arr.ensure(cm) ||
        ctx->states.ensure((size_t)chunk * ctx->slot_cap * S * np) ||
        ctx->xs.ensure(want_grad ? (size_t)chunk * ctx->slot_cap * S * np : 1) ||
        ctx->offs.ensure((size_t)chunk * (nsteps + 1)) || ctx->gstep.ensure(cm * std::max(Kk, 1)) ||
        EffCtlChunk::reserve(ctx, effk, cm, want_grad) ||
        ctx->cost_out.ensure(B) || ctx->grads.ensure((size_t)B * ctx->nc * std::max(K, 1)) ||
        ctx->final_out.ensure((size_t)B * S * np) || ctx->lam_buf.ensure((size_t)chunk * S * np) ||
        ctx->magnus_scratch.ensure((size_t)blocks * 7 * mat))
        return QOCX_ERR_HIP;
    // K3 of many states keeps the chains of every state in scratch: as many workgroups as 8 GB hold
    const size_t k3_elems = qocx::general_krylov_scratch(np, S);
    const int k3_blocks = (int)std::max<size_t>(1, std::min<size_t>((size_t)blocks, ((size_t)8 << 30) / (k3_elems * 16)));
    if (want_grad && ctx->magnus_scratch.ensure((size_t)k3_blocks * k3_elems)) return QOCX_ERR_HIP;
    const int mg_blocks = (int)std::max<size_t>(1, std::min<size_t>((size_t)blocks, ((size_t)8 << 30) / (24 * mat * 16)));
    if (magnus && (ctx->magnus_scratch.ensure((size_t)mg_blocks * 24 * mat) || ctx->m_rm.ensure(cm * mat) ||
                   ctx->mbar_rm.ensure(want_grad ? cm * mat : 1) || ctx->gstep.ensure(cm * nodes * std::max(K, 1))))
        return QOCX_ERR_HIP;
    if (ctx->keep_step_states)
        if (ctx->step_states.ensure((size_t)B * (nsteps + 1) * S * np)) return QOCX_ERR_HIP;
    HIP_TRY(hipMemsetAsync(ctx->status.p, 0, sizeof(int), ctx->stream));
    hipStream_t cs = ctx->stream;
    for (int b0 = 0; b0 < B; b0 += chunk) {
        const int bc = std::min(chunk, B - b0);
        ctx->last_chunk = bc;
        qocx::GeneralArgs fa;
        fa.np = np; fa.K = K; fa.nc = ctx->nc; fa.nsteps = nsteps; fa.nt = ctx->nt; fa.dt = ctx->dt;
        fa.controls = ctx->controls.p ? ctx->controls.p + (size_t)b0 * ctx->nc * K : nullptr;
        fa.interp = ctx->interp.p;
        fa.h0_rm = ctx->h0.t.p; fa.g_rm = ctx->g.t.p;
        fa.gen_rm = explicit_gen ? ctx->gen_rm.p + (size_t)b0 * nsteps * mat : nullptr;
        fa.pade_policy = (int)ctx->knob("pade_order", 0);
        fa.sq_max = std::min(30, ctx->sbound);
        fa.q_img = ctx->q_img.p; fa.pinv_img = ctx->lu_img.p; fa.s_arr = ctx->s_arr.p; fa.status = ctx->status.p;
        fa.scratch = ctx->magnus_scratch.p;
        fa.total = (size_t)bc * nsteps;
        EffCtlChunk eff;
        eff.begin(ctx, effk, fa.controls, nullptr, b0, bc, cs, false);
        eff.redirect(fa, fa.g_rm, ctx->eff.images.t);
        const int fblocks = (int)std::min<size_t>(fa.total, (size_t)blocks);
        qocx::MagnusArgs ma;
        if (magnus) {
            ma.controls = fa.controls; ma.interp = ctx->interp.p;
            ma.h0_cimg = ctx->h0.t.p; ma.g_cimg = ctx->g.t.p;  // (row-major padded matrices here)
            ma.K = K; ma.nc = ctx->nc; ma.nsteps = nsteps; ma.nt = ctx->nt; ma.nodes = nodes;
            ma.step0 = 0; ma.seg_len = nsteps; ma.skew = 0; ma.dt = ctx->dt;
            ma.m_rm = ctx->m_rm.p; ma.mbar_rm = nullptr; ma.gstep = nullptr;
            ma.scratch = ctx->magnus_scratch.p; ma.total = fa.total; ma.n = np;
            time_begin(ctx, 0, cs);
            qocx::launch_general_magnus(ma, false, std::min(fblocks, mg_blocks), cs);
            time_end(ctx, cs);
            fa.gen_rm = ctx->m_rm.p;  // the factor kernel and K3 take the step generators as they are
        }
        time_begin(ctx, 0, cs);
        if (qocx::launch_general_factor(fa, fblocks, cs)) return fail(QOCX_ERR_HIP, "K1a (general): LDS size refused");
        time_end(ctx, cs);

        qocx::GeneralSweepArgs sa;
        sa.np = np; sa.S = S; sa.nsteps = nsteps; sa.cost_eval_step = ctx->ces;
        sa.has_step_costs = ctx->has_step_costs; sa.phase = want_grad ? 3 : 1;
        sa.q_img = fa.q_img; sa.pinv_img = fa.pinv_img; sa.s_arr = fa.s_arr; sa.psi0 = ctx->psi0.p;
        sa.slot_cap = ctx->slot_cap; sa.states = ctx->states.p; sa.xs = ctx->xs.p; sa.offs = ctx->offs.p;
        sa.lam_buf = ctx->lam_buf.p;
        sa.cost_count = ctx->cost_count; sa.costs = ctx->costs.p; sa.cost_vectors = ctx->cost_vectors.p;
        sa.cost_counts = ctx->cost_counts.p;
        sa.inj_count = ctx->inj_count;
        sa.inj_index = ctx->inj_count > 0 ? ctx->inj_index.p : nullptr;
        sa.inj_bars = ctx->inj_count > 0 ? ctx->inj_bars.p + (size_t)b0 * ctx->inj_count * S * np : nullptr;
        sa.cost_out = ctx->cost_out.p + b0;
        sa.final_out = ctx->final_out.p + (size_t)b0 * S * np;
        sa.step_states = ctx->keep_step_states ? ctx->step_states.p + (size_t)b0 * (nsteps + 1) * S * np : nullptr;
        sa.status = ctx->status.p;
        // Many states, final costs only, few seeds (a full propagator of one control set): the states of a seed
        // in groups of rows on several workgroups (qocx_general.hip, split mode) - knob "general_split" 0: off
        int groups = 1;
        if (S >= 16 && !ctx->has_step_costs && ctx->inj_count == 0 && !ctx->keep_step_states &&
            ctx->knob("general_split", 1) != 0)
            groups = std::min((S + 7) / 8, std::max(1, 2 * ctx->cu_count / bc));
        time_begin(ctx, 1, cs);
        if (groups >= 2) {
            sa.phase = 1 | 8 | (groups << 8);
            qocx::launch_general_sweep(sa, bc, cs);
            sa.phase = 4 | 8 | (want_grad ? 16 : 0);
            qocx::launch_general_sweep(sa, bc, cs);
            if (want_grad) {
                sa.phase = 2 | 8 | (groups << 8);
                qocx::launch_general_sweep(sa, bc, cs);
            }
        } else {
            qocx::launch_general_sweep(sa, bc, cs);
        }
        time_end(ctx, cs);

        if (want_grad) {
            qocx::GeneralKrylovArgs ka;
            ka.np = np; ka.S = S; ka.K = fa.K; ka.nc = fa.nc; ka.nsteps = nsteps; ka.nt = ctx->nt; ka.dt = ctx->dt;
            ka.controls = fa.controls; ka.interp = fa.interp; ka.h0_rm = fa.h0_rm; ka.g_rm = fa.g_rm;
            ka.gen_rm = fa.gen_rm;
            ka.mbar_rm = explicit_gen ? ctx->genbar_rm.p + (size_t)b0 * nsteps * mat : (magnus ? ctx->mbar_rm.p : nullptr);
            ka.s_arr = fa.s_arr; ka.offs = ctx->offs.p; ka.states = ctx->states.p; ka.xs = ctx->xs.p;
            ka.slot_cap = ctx->slot_cap; ka.gstep = ctx->gstep.p; ka.scratch = ctx->magnus_scratch.p;
            ka.total = fa.total;
            // (Magnus generators are skew only to rounding: the general chains there)
            ka.skew = (magnus ? 0 : (explicit_gen ? ctx->explicit_hermitian : ctx->hermitian)) &&
                      ctx->knob("general_skew", 1) != 0;
            time_begin(ctx, 2, cs);
            if (qocx::launch_general_krylov(ka, std::min(fblocks, k3_blocks), cs))
                return fail(QOCX_ERR_HIP, "K3 (general): LDS size refused");
            time_end(ctx, cs);
            if (magnus) {
                ma.m_rm = nullptr; ma.mbar_rm = ctx->mbar_rm.p; ma.gstep = ctx->gstep.p;
                time_begin(ctx, 2, cs);
                qocx::launch_general_magnus(ma, true, std::min(fblocks, mg_blocks), cs);
                time_end(ctx, cs);
            }
            if (!explicit_gen) scatter_gradients(ctx, eff, ka.gstep, nullptr, b0, bc, cs);
        }
    }
    return finish_items(ctx, want_grad);
}

// ---- the resident Schroedinger evaluation (n <= 64): route, buffers, chunks, schedules ----------
#include "qocx_host_action.h"  // the matrix-free route: its buffers, argument blocks and launches (needs EffCtlChunk)

namespace {

// Which kernels serve the evaluation: a property of the PROBLEM, the context's knobs and the host's
// norm bound, never of the batch size, chunking or segmentation - results stay bit-identical
// across those (tests/test_gpu_engine.py::test_chunked_equals_unchunked, test_gpu_fullsize.py).
struct ResidentRoute {
    bool latency;        // one control set at a time (the host's single-evaluation entry points)
    EffKind eff;         // effective controls on the M2 kernels: M4-linear (one node) or quadratic
    int Kk;              // controls as K1a / K3 see them
    int nodes;           // nodes of the generator kernels
    bool dense;          // dense-state sweep (qocx_sweepd.hip)
    bool inverse_sweep;  // inverse-image sweep (qocx_sweepi.hip)
    bool unit;           // unit adjoint (qocx_sweep_common.h)
    bool sweep3;         // blocked sweep (qocx_sweep3.hip)
    bool magnus4w;       // Magnus kernels as four-wave workgroups (qocx_magnus4w.hip)
    bool one_wave_k1a;   // (experiments: the one-wave K1a)
    bool fused_lu;       // K1b fused into the two-wave K1a
    bool step_table;     // launch_step_table in front of K1a (or, where it is action.table, for the sweeps alone)
    bool all_dominant;   // every Pade denominator diagonally dominant
    bool pack8;          // n <= 8: two steps per 16 x 16 tile through K1a and K1b
    bool umode;          // the propagator itself in the Q image, one product per sweep sub-step
    qocx::ActionPlan action;  // matrix-free Taylor sweeps, nothing factored: whether, and on which kernels (qocx_action_route.h)
};

ResidentRoute resident_route(const qocx_ctx* ctx, int want_grad, bool allow_action) {
    ResidentRoute r;
    const int nb = ctx->nb, S = ctx->S;
    const bool explicit_gen = ctx->explicit_mode;
    // "latency": where the unit adjoint applies, the two-sided pipeline on few time segments is the
    // lowest latency there is - one seed, n = 32, 1000 steps, forward + gradient: 3.6 ms against 4.15 ms
    // with the blocked sweep and 6.4 ms with one launch of the column-chain sweep; n = 8, 500
    // steps: 1.1 against 2.1 / 1.8 ms (profiles/r03_latency.jsonl) - so it takes precedence
    // over "sweep_impl" = 3 there.
    r.latency = ctx->knob("latency", 0) != 0;
    // Both effective-control routes: one control row per step read through interp_id (nodes 1), the
    // unit adjoint with the scalar applied by the chain kernel, no step table (it interpolates the K
    // real controls at the knots and bounds with ||G_k||_1 alone, blind to the augmented operators),
    // no pack8 (kept to the plain structured problem). (The matrix-free route, below, runs on
    // the same effective controls where its plan says so, with a table of its own.)
    r.eff = ctx->effctl_kind(true);
    r.Kk = EffCtlChunk::channels(ctx, r.eff);
    r.nodes = r.eff == EffectiveControls::M4_LINEAR ? 1 : ctx->nodes;
    // 8..32 states of a seed as the columns of MFMA GEMMs, with P^-1 in place of the LU factors
    r.dense = qocx::sweepd_supports(nb, S) && ctx->knob("sweep_dense", 1) != 0;
    // a sub-step is two matrix-vector products with P^-1 from inv_kernel instead of two triangular
    // solves. In latency mode (the sweep chain is all there is), and always at n <= 16, where
    // Gauss-Jordan on a 16 x 16 matrix costs what its LU costs (0.10 against 0.085 ms per 32 000)
    // and the evaluation is bound by the sweeps: 256 seeds x 1000 steps at n = 8: 3.65 -> 2.79 ms.
    r.inverse_sweep = (r.latency || (nb == 1 && ctx->knob("sweep_inverse_small", 1))) && !r.dense &&
                      qocx::sweepi_supports(nb, S) && ctx->knob("sweep_inverse", 1) != 0;
    r.unit = ctx->unit_ok && want_grad && ctx->inj_count == 0 && !explicit_gen && !r.dense &&
             (ctx->nodes == 1 || r.eff == EffectiveControls::M4_LINEAR) && ctx->knob("unit_adjoint", 1);
    // "sweep_impl": 1 (default) column-chain sweep, 3 blocked sweep. Measured
    // (profiles/r02_sweep_ab.jsonl): the blocked sweep takes 2.1 us per step against 3.2 us when it
    // has the chip to itself, but inside the segmented pipeline at 256 seeds it loses (14.3 against
    // 13.4 ms): its workgroup owns the CU's LDS, so K1a / K1b / K3 cannot run beside it.
    // (latency mode, n <= 16: the column-chain sweep is the faster one there - 1.8 against 2.2 us
    // per step - so the two-sided pipeline keeps it; 17 <= n <= 32: two-sided on the blocked sweep)
    r.sweep3 = ctx->knob("sweep_impl", 1) == 3 && nb <= 2 && !r.dense && !r.inverse_sweep &&
               S <= qocx::sweep3_max_states(nb) && !(r.latency && r.unit && nb == 1);
    r.magnus4w = r.nodes > 1 && qocx::magnus4w_supports(nb, ctx->K, ctx->n) && ctx->knob("magnus_4w", 1) != 0;
    r.one_wave_k1a = qocx::diag_getenv("QOCX_PQ1") != nullptr;
    // K1b fused into the two-wave K1a (17 <= n <= 32; knob "fuse_lu" 0 restores the two kernels)
    r.fused_lu = nb == 2 && !r.one_wave_k1a && !r.dense && !r.inverse_sweep && ctx->knob("fuse_lu", 1) != 0;
    // Step table (two-wave K1a, structured M2 problem): one small kernel interpolates the controls of
    // every step and decides its Pade order and squaring count from the bound dt (||H0||_1 + sum |u_k|
    // ||G_k||_1); K1a and K3 then read both instead of interpolating and (K1a) reducing a norm behind
    // a barrier.
    r.step_table = nb == 2 && !r.one_wave_k1a && !explicit_gen && r.nodes == 1 && !r.eff && !r.dense &&
                   ctx->K > 0 && ctx->g_norm_dev.p != nullptr;
    // every Pade denominator of the evaluation diagonally dominant by the margin of qocx_lu5.h
    // (eps_m(theta) <= 0.40 for every order m at the host's bound theta of the step norm)
    r.all_dominant = pade_eps_max(ctx->norm_bound) <= 0.40 && ctx->knob("lu_dpp", 1) != 0;
    // n <= 8: two consecutive steps of a seed as the diagonal blocks of one 16 x 16 tile through K1a
    // and K1b (pade_pq8_kernel, inv16_dpp_kernel<1, true>); the sweeps and K3 see the usual images
    r.pack8 = nb == 1 && ctx->n <= 8 && r.inverse_sweep && !r.dense && r.all_dominant && !explicit_gen &&
              r.nodes == 1 && !r.eff && ctx->knob("pack8", 1) != 0;
    // One control set at a time, inverse-image sweep: K1b's sibling umul_kernel leaves the propagator
    // itself in the Q image; the sweeps apply ONE matrix per sub-step, the adjoint sweep hands lambda'
    // to K3, which forms x = P^-H lambda' from the P^-1 image (knob "sweep_umode").
    r.umode = r.latency && r.inverse_sweep && !r.dense && nb <= 2 && ctx->knob("sweep_umode", 1) != 0;
    // The matrix-free route: the facts its decision reads (plain values, no allocation), the decision itself
    // and the knobs' commentary in qocx_action_route.h. It is taken without the inverse-image sweep, pack8
    // or umode, so that no buffer or launch follows them; its plain step table is launch_step_table, which
    // above n = 32 and at n <= 16 no K1a reads.
    qocx::ActionFacts f{};
    f.n = ctx->n; f.S = S; f.K = ctx->K; f.nt = ctx->nt; f.nodes = r.nodes;
    f.eff_kind = (int)r.eff; f.Ke = ctx->eff.Ke;
    f.hermitian = ctx->hermitian; f.unit_ok = ctx->unit_ok; f.has_step_costs = ctx->has_step_costs;
    f.cost_count = ctx->cost_count; f.inj_count = ctx->inj_count; f.keep_step_states = ctx->keep_step_states;
    f.explicit_gen = explicit_gen; f.dense = r.dense; f.one_wave_k1a = r.one_wave_k1a; f.latency = r.latency;
    f.have_norms = ctx->g_norm_dev.p != nullptr;
    f.have_eff_norms = ctx->eff.op_norm1_dev.p != nullptr && ctx->eff.op_norm2_dev.p != nullptr;
    f.have_e_img = (r.eff ? ctx->eff.eimg.p : ctx->g_eimg.p) != nullptr;
    f.bound1 = ctx->norm_bound; f.bound1_mid = ctx->norm_bound_mid;
    f.bound2 = ctx->norm2_bound; f.bound2_mid = ctx->norm2_bound_mid;
    // (a knob is an int64 and "action" takes any: saturated, no comparison of the decision changes)
    const auto knob = [ctx](const char* name, int dflt) {
        return (int)std::min<int64_t>(std::max<int64_t>(ctx->knob(name, dflt), INT32_MIN), INT32_MAX);
    };
    f.action = knob("action", 1); f.action_states = knob("action_states", 0);
    f.action_costs = knob("action_costs", 0); f.action_small = knob("action_small", 0);
    f.action_eff = knob("action_eff", 0); f.action_eff_exact = knob("action_eff_exact", 1);
    f.action_degree = knob("action_degree", 1); f.action_plan = knob("action_plan", 1);
    f.pade_order = knob("pade_order", 0); f.unit_adjoint = knob("unit_adjoint", 1);
    f.allow = allow_action;
    r.action = qocx::action_plan(f);
    if (r.action.on()) {
        r.inverse_sweep = r.pack8 = r.umode = false;
        r.step_table = r.action.table == qocx::ActionPlan::PLAIN;
    }
    return r;
}

// Seeds per chunk from the memory budget (or the user's chunk), and the device buffers of a chunk.
int reserve_resident(qocx_ctx* ctx, const ResidentRoute& r, int want_grad, int& chunk) {
    const int B = ctx->B, np = ctx->np, mat = np * np, S = ctx->S, K = ctx->K, nsteps = ctx->nsteps;
    if (r.unit && ctx->lam_scale.ensure((size_t)B * S)) return QOCX_ERR_HIP;
    if (ctx->action_counts.ensure(QOCX_ACTION_MAX_DEGREE + 1)) return QOCX_ERR_HIP;
    if (r.action.on()) return reserve_action(ctx, r.action, r.eff, want_grad, chunk);
    const size_t per_seed = (size_t)nsteps * ((size_t)mat * 32 + (size_t)np * 20 + 4) +
                            ctx->slot_cap * S * np * 32 + (size_t)(nsteps + 1) * 4 +
                            (size_t)nsteps * ctx->nodes * std::max(r.Kk, 1) * 24 +
                            (ctx->nodes > 1 ? (size_t)nsteps * mat * 32 : 0);
    chunk = ctx->chunk_user;
    if (chunk <= 0) {
        size_t free_b = 0, total_b = 0;
        HIP_TRY(hipMemGetInfo(&free_b, &total_b));
        size_t have = ctx->q_img.count * 16 + ctx->lu_img.count * 16 + ctx->states.count * 16 +
                      ctx->xs.count * 16;
        size_t budget = (size_t)((double)(free_b + have) * 0.6);
        chunk = (int)std::min<size_t>((size_t)B, std::max<size_t>(1, budget / per_seed));
    }
    chunk = std::min(chunk, B);
    const size_t cm = (size_t)chunk * nsteps;
    if (ctx->q_img.ensure(cm * mat) || ctx->lu_img.ensure(cm * mat) || ctx->dinv.ensure(cm * np) ||
        ctx->perm.ensure(cm * np) || ctx->iperm.ensure(cm * np) || ctx->s_arr.ensure(cm) ||
        ctx->states.ensure((size_t)chunk * ctx->slot_cap * S * np) ||
        ctx->xs.ensure(want_grad ? (size_t)chunk * ctx->slot_cap * S * np : 1) ||
        ctx->offs.ensure((size_t)chunk * (nsteps + 1)) ||
        ctx->gstep.ensure(cm * r.nodes * std::max(r.Kk, 1) * (r.unit ? 2 : 1)) || ctx->cost_out.ensure(B) ||
        EffCtlChunk::reserve(ctx, r.eff, cm, want_grad) ||
        (r.unit && ctx->offs_x.ensure((size_t)chunk * (nsteps + 1))) ||
        ctx->grads.ensure((size_t)B * ctx->nc * std::max(K, 1)) ||
        ctx->final_out.ensure((size_t)B * S * np) ||
        (ctx->keep_step_states && ctx->step_states.ensure((size_t)B * (nsteps + 1) * S * np)) ||
        (r.nodes > 1 && (ctx->m_rm.ensure(cm * mat) || ctx->mbar_rm.ensure(want_grad ? cm * mat : 1) ||
                         ctx->magnus_scratch.ensure(qocx::magnus_scratch_elems(ctx->nb, (int)std::min<size_t>(cm, 1024))))) ||
        (r.umode && ctx->qt_img.ensure(cm * mat)) ||
        ctx->lam_buf.ensure((size_t)chunk * S * np) || ctx->lu_fallbacks.ensure(1))
        return QOCX_ERR_HIP;
    return 0;
}

// Steps [lo[i], lo[i + 1]) of time segment i. The segments the sweeps reach last are the short
// ones, because what they still have to do once those are factored is exposed: the last two
// (one-sided), the two in the middle (two-sided).
std::vector<int> segment_bounds(int nsteps, int nseg, bool two_sided) {
    std::vector<double> wgt(nseg, 1.0);
    if (two_sided) {
        wgt[nseg / 2 - 1] = 0.5;
        wgt[nseg / 2] = 0.5;
    } else if (nseg >= 4) {
        wgt[nseg - 2] = 0.6;
        wgt[nseg - 1] = 0.35;
    }
    double tot = 0, run = 0;
    for (double w : wgt) tot += w;
    std::vector<int> lo(nseg + 1);
    lo[0] = 0;
    for (int i = 0; i < nseg; ++i) {
        run += wgt[i];
        lo[i + 1] = std::max(lo[i] + 1, (int)llround(nsteps * run / tot));
    }
    lo[nseg] = nsteps;
    for (int i = nseg - 1; i > 0; --i) lo[i] = std::min(lo[i], lo[i + 1] - 1);
    return lo;
}

// One chunk of seeds [b0, b0 + bc): its time segments, the argument blocks of its kernels (built
// once by init) and the launches the two schedules are made of.
//
// Time-segmented pipeline. The serial sweep of a seed is latency bound (one wave, 2(N-1) dependent
// steps, <= B waves on the whole chip), the other kernels are throughput bound. The steps are
// therefore cut into `nseg` time segments: the compute stream `cs` factors segment after segment
// (Magnus, K1a, K1b), the high-priority sweep stream follows one segment behind with the forward
// sweep, then walks back with the adjoint sweep while the compute stream runs K3 on the segments
// the adjoint sweep has already left.
struct ResidentChunk {
    qocx_ctx* ctx;
    const ResidentRoute& r;
    int want_grad, b0, bc, nseg;
    bool two_sided;
    hipStream_t cs, ss;  // compute stream, sweep stream of the one-sided pipeline
    std::vector<int> lo;
    int dbg_skip;  // "dbg_skip" (timing experiments only, results are garbage): bit 0 no forward
                   // sweep, bit 1 no adjoint sweep, bit 2 no K3, bit 3 K1a stores no Q
    qocx::FactorArgs fa;
    EffCtlChunk eff;
    qocx::LuArgs la;
    qocx::MagnusArgs ma;
    qocx::SweepArgs sa;
    qocx::KrylovArgs ka;
    ActionChunk act;  // the matrix-free route (r.action)

    ResidentChunk(qocx_ctx* c, const ResidentRoute& route, int grad, int first, int count)
        : ctx(c), r(route), want_grad(grad), b0(first), bc(count), cs(c->stream) {
        const int nsteps = ctx->nsteps;
        nseg = ctx->pipe_user > 0 ? ctx->pipe_user : ((size_t)bc * nsteps >= 16384 && nsteps >= 64 ? 8 : 1);
        // (one control set, two-sided: TWO segments - the forward sweep takes the first as soon as it is
        // factored, the adjoint sweep the second, then they swap; every further segment is two more launch
        // latencies on the chain: configs[1] 0.535 -> 0.505 ms, dim 32 x 1000 steps 1.54 -> 1.50)
        if (ctx->pipe_user <= 0 && nseg == 1 && r.latency && r.unit && nsteps >= 64) nseg = 2;
        nseg = std::max(1, std::min(std::min(nseg, (int)ctx->ev_factored.size()), nsteps));
        ss = (nseg == 1) ? cs : ctx->sweep_streams[0];
        // Two-sided pipeline (unit adjoint): the adjoint sweep back-propagates the
        // targets from the LAST segment while the forward sweep propagates the states from the
        // FIRST one; the compute stream factors the segments from both ends towards the middle,
        // and K3 follows from the middle outwards once both sweeps have crossed a segment.
        two_sided = r.unit && nseg >= 2 && ctx->knob("bidir", 1) && (int)ctx->sweep_streams.size() >= 2;
        lo = segment_bounds(nsteps, nseg, two_sided);
        dbg_skip = (int)ctx->knob("dbg_skip", 0);
    }

    // the chunk's scalars of the unit adjoint
    double2* lam_scale() const { return r.unit ? ctx->lam_scale.p + (size_t)b0 * ctx->S : nullptr; }

    // the argument blocks; launches the step table and the effective-controls kernel. On the matrix-free
    // route nothing is factored: no LuArgs, and of FactorArgs what the step table reads
    int init() {
        if (int rc = init_table()) return rc;
        if (int rc = init_sweep_args()) return rc;
        if (r.action.on())
            return act.init(ctx, r.action, eff, r.eff, fa.controls, lam_scale(), want_grad, b0, bc, cs);
        if (int rc = init_factor()) return rc;
        return init_krylov();
    }

    // the chunk's controls and, where the route has one (r.step_table), the step table - with the part of
    // FactorArgs that the table and its question to K1a (pq3_supports) read
    int init_table() {
        const int K = ctx->K, nsteps = ctx->nsteps;
        fa.controls = ctx->controls.p ? ctx->controls.p + (size_t)b0 * ctx->nc * K : nullptr;
        fa.interp = ctx->interp.p;
        fa.K = K; fa.nc = ctx->nc; fa.nsteps = nsteps; fa.nt = ctx->nt; fa.dt = ctx->dt;
        fa.hermitian = ctx->explicit_mode ? ctx->explicit_hermitian : ctx->hermitian;
        fa.lu_dpp = (int)ctx->knob("lu_dpp", 1);
        fa.pade_policy = (int)ctx->knob("pade_order", 0);  // 0: by norm (qocx_wave.h), 13: always 13
        fa.prefer_low = ctx->norm_bound < 2.539398330063230e-01 ? 2 : ctx->norm_bound < 2.097847961257068 ? 1 : 0;  // theta_5, theta_9
        fa.s_arr = ctx->s_arr.p; fa.status = ctx->status.p;
        fa.fuse_lu = r.fused_lu ? 1 : 0;
        if (b0 == 0) HIP_TRY(hipMemsetAsync(ctx->lu_fallbacks.p, 0, sizeof(int), cs));
        if (!r.step_table) return 0;
        if (ctx->ustep.ensure((size_t)bc * nsteps * K)) return QOCX_ERR_HIP;
        qocx::StepTableArgs ta;
        ta.controls = fa.controls; ta.interp = fa.interp; ta.K = K; ta.nc = ctx->nc;
        ta.nsteps = nsteps; ta.batch = bc; ta.dt = ctx->dt; ta.h0_norm = ctx->h0_norm_max;
        ta.g_norm = ctx->g_norm_dev.p; ta.pade_policy = fa.pade_policy;
        ta.action = r.action.on() ? 1 : 0;
        ta.h0_norm2 = ctx->h0_norm2_max; ta.g_norm2 = ctx->g_norm2_dev.p;
        ta.degree_rule = r.action.degree_rule && ta.g_norm2 != nullptr ? 1 : 0;
        ta.sq_max = std::min(30, ctx->sbound);
        fa.direct = 1;  // (K1a and K3 read the table: fa.controls, below)
        fa.three_wave = (int)ctx->knob("k1a_three", 1);
        // (1: the second halves of the factorisations four to a wave in a kernel of their own behind K1a,
        // 2: on the factor side stream, beside the next segment's K1a. Measured, profiles/r05_k1a_four.txt:
        // K1a 0.650 -> 0.587 ms, the second kernel 0.061 ms - it moves 4 KB per step in and out, 262 MB
        // per segment -, the evaluation 8.05 -> 8.05 (1) / 7.93 ms (2). Off: 1.3 % for a kernel and a
        // stream more and 2 GB more traffic per evaluation.)
        fa.four_steps = (int)ctx->knob("k1a_four", 0);
        fa.gen_share = (int)ctx->knob("k1a_share", 2);
        if (fa.four_steps == 2 && ctx->lu_stream == nullptr) fa.four_steps = 1;
        // (the bound at the step midpoints, where it applies, speaks for the two-wave K1a only: the
        // four-wave kernels and the slot capacity keep the bound over the knots)
        // only the three-wave K1a (orders 3 and 5) will be launched: no step above order 5
        if (fa.three_wave && qocx::pq3_supports(fa) &&
            std::min(ctx->norm_bound, ctx->norm_bound_mid) < 2.539398330063230e-01) {
            fa.prefer_low = 2;
            ta.order_max = 5;
        }
        ta.ustep = ctx->ustep.p; ta.s_arr = fa.s_arr; ta.status = fa.status;
        qocx::launch_step_table(ta, cs);
        fa.controls = ctx->ustep.p; fa.nc = nsteps;
        return 0;
    }

    // the rest of FactorArgs, LuArgs; launches the effective-controls kernel
    int init_factor() {
        const int nsteps = ctx->nsteps;
        fa.h0_cimg = ctx->h0.c.p;
        fa.g_cimg = ctx->g.c.p;
        eff.begin(ctx, r.eff, fa.controls, lam_scale(), b0, bc, cs, true);
        eff.redirect(fa, fa.g_cimg, ctx->eff.images.c);
        fa.n = ctx->n;
        fa.skip_q = (dbg_skip & 8) ? 1 : 0;
        fa.dbg = (int)ctx->knob("k1a_dbg", 0);  // (diagnostic build: qocx_device.h)
        fa.stamps = nullptr;
        if (qocx::kDiagBuild && ctx->knob("k1a_stamps", 0)) {
            if (ctx->stamps.ensure(1024 * 16)) return QOCX_ERR_HIP;
            HIP_TRY(hipMemsetAsync(ctx->stamps.p, 0, 1024 * 16 * sizeof(unsigned long long), cs));
            HIP_TRY(hipStreamSynchronize(cs));
            fa.stamps = ctx->stamps.p;
        }
        fa.lu_mfma = (int)ctx->knob("lu_mfma", 1);
        fa.herm_tiles = (int)ctx->knob("k1a_herm4", 1);
        fa.lu_fallbacks = ctx->lu_fallbacks.p;
        fa.q_img = ctx->q_img.p; fa.lu_img = ctx->lu_img.p;
        fa.dinv = ctx->dinv.p; fa.perm = ctx->perm.p; fa.iperm = ctx->iperm.p;
        const int k1a_dbg = (int)ctx->knob("k1a_dbg", 0);
        la.lu_img = fa.lu_img; la.dinv = ctx->dinv.p; la.perm = ctx->perm.p;
        la.iperm = ctx->iperm.p; la.status = ctx->status.p; la.nsteps = nsteps; la.n = ctx->n;
        la.dbg = ((dbg_skip & 16) ? 1 : 0) | ((k1a_dbg & 8) ? 2 : 0) | ((k1a_dbg & 16) ? 4 : 0) |
                 ((k1a_dbg & 32) ? 8 : 0);
        la.inverse = (r.dense || r.inverse_sweep) ? 1 : 0;
        la.all_dominant = r.all_dominant ? 1 : 0;
        fa.pack8 = la.pack8 = r.pack8 ? 1 : 0;
        la.redo = nullptr;
        la.fallbacks = ctx->lu_fallbacks.p;
        if (ctx->nb == 4 && ctx->knob("lu_mfma", 1) != 0) {  // qocx_lu4m.hip in front of lu4_kernel
            if (ctx->lu_redo.ensure((size_t)bc * nsteps)) return QOCX_ERR_HIP;
            la.redo = ctx->lu_redo.p;
            // (Measured and not kept: the nine-tile factorisation INSIDE the nine-tile K1a, P through an
            // LDS image as at n <= 32 - 3.81 ms per launch against 2.48 + 0.78 apart: wave 0 factors for
            // 60 000 cycles while the workgroup's 46 KiB of LDS stay allocated.)
        }
        return 0;
    }

    // SweepArgs: the chunk's states, costs and carries (the matrix-free sweeps take them too, ActionArgs::sw)
    int init_sweep_args() {
        const int S = ctx->S, np = ctx->np, nsteps = ctx->nsteps;
        sa.q_img = ctx->q_img.p; sa.lu_img = ctx->lu_img.p; sa.dinv = ctx->dinv.p;
        sa.perm = ctx->perm.p; sa.iperm = ctx->iperm.p; sa.s_arr = ctx->s_arr.p;
        sa.psi0 = ctx->psi0.p;
        sa.umode = r.umode ? 1 : 0;
        sa.qt_img = r.umode ? ctx->qt_img.p : nullptr;
        sa.S = S; sa.nsteps = nsteps; sa.cost_eval_step = ctx->ces; sa.want_grad = want_grad;
        sa.n = ctx->n;
        sa.has_step_costs = ctx->has_step_costs; sa.slot_cap = ctx->slot_cap;
        sa.cost_count = ctx->cost_count; sa.costs = ctx->costs.p;
        sa.cost_vectors = ctx->cost_vectors.p; sa.cost_counts = ctx->cost_counts.p;
        sa.states = ctx->states.p;
        sa.xs = ctx->xs.p;
        sa.offs = ctx->offs.p;
        sa.cost_out = ctx->cost_out.p + b0;
        sa.final_out = ctx->final_out.p + (size_t)b0 * S * np;
        sa.step_states = ctx->keep_step_states
                             ? ctx->step_states.p + (size_t)b0 * (nsteps + 1) * S * np : nullptr;
        sa.status = ctx->status.p;
        sa.lam_buf = ctx->lam_buf.p;
        sa.batch = bc;
        sa.one_state = (int)ctx->knob("sweep_one", 1);
        sa.dbg = (int)ctx->knob("sweep3_dbg", 0);  // (bits 8, 9: the column-chain sweep fetches nothing)
        sa.stamps = nullptr;
        if (ctx->knob("sweep3_stamps", 0)) {
            if (ctx->stamps.ensure((size_t)ctx->B * 32)) return QOCX_ERR_HIP;
            HIP_TRY(hipMemsetAsync(ctx->stamps.p, 0, (size_t)ctx->B * 32 * sizeof(unsigned long long), cs));
            HIP_TRY(hipStreamSynchronize(cs));
            sa.stamps = ctx->stamps.p + (size_t)b0 * 32;
        }
        sa.unit_adjoint = r.unit ? 1 : 0;
        sa.lam_scale = lam_scale();
        sa.offs_x = r.unit ? ctx->offs_x.p : nullptr;
        sa.inj_count = ctx->inj_count;
        sa.inj_index = ctx->inj_count > 0 ? ctx->inj_index.p : nullptr;
        sa.inj_bars = ctx->inj_count > 0
                          ? ctx->inj_bars.p + (size_t)b0 * ctx->inj_count * S * np : nullptr;
        return 0;
    }

    // MagnusArgs, KrylovArgs
    int init_krylov() {
        const int S = ctx->S, np = ctx->np, nsteps = ctx->nsteps;
        const size_t mat = (size_t)np * np;
        const bool explicit_gen = ctx->explicit_mode;
        ma.controls = fa.controls; ma.interp = ctx->interp.p;
        ma.h0_cimg = ctx->h0.c.p; ma.g_cimg = ctx->g.c.p;
        ma.K = ctx->K; ma.nc = ctx->nc; ma.nsteps = nsteps; ma.nt = ctx->nt; ma.nodes = r.nodes;
        ma.dt = ctx->dt; ma.scratch = ctx->magnus_scratch.p; ma.n = ctx->n;
        ma.skew = ctx->hermitian;
        ka.controls = fa.controls;
        ka.interp = fa.interp;
        ka.h0_rimg = ctx->h0.r.p; ka.h0_timg = ctx->h0.t.p;
        ka.g_rimg = ctx->g.r.p; ka.g_timg = ctx->g.t.p;
        eff.redirect(ka);
        ka.K = fa.K; ka.nc = fa.nc; ka.nsteps = nsteps; ka.nt = ctx->nt; ka.S = S;
        ka.umode = r.umode ? 1 : 0;
        ka.pinv_img = fa.lu_img;
        ka.direct = fa.direct;
        ka.n = ctx->n;
        ka.dt = ctx->dt; ka.s_arr = ctx->s_arr.p;
        ka.offs = ctx->offs.p;
        ka.offs_x = r.unit ? ctx->offs_x.p : nullptr;
        ka.states = ctx->states.p;
        ka.xs = ctx->xs.p;
        ka.slot_cap = ctx->slot_cap;
        ka.gstep = ctx->gstep.p;
        ka.m_rm = r.nodes > 1 ? ctx->m_rm.p : nullptr;
        ka.mbar_rm = r.nodes > 1 ? ctx->mbar_rm.p : nullptr;
        if (explicit_gen) {
            ka.m_rm = ctx->gen_rm.p + (size_t)b0 * nsteps * mat;
            ka.mbar_rm = want_grad ? ctx->genbar_rm.p + (size_t)b0 * nsteps * mat : nullptr;
        }
        ka.skew = explicit_gen ? ctx->explicit_hermitian : ctx->hermitian;
        return 0;
    }

    // Magnus, K1a and K1b of segment i on the compute stream; ev_factored[i] once it is factored
    // (nseg > 1)
    int factor_segment(int i) {
        // (Measured and dropped: K1a / K1b of a segment as 2, 4 or 8 pairs of sub-launches, so
        // that K1b might find P in the last-level cache: 13.1 / 13.8 / 15.5 ms against 12.7 -
        // the launch tails cost more than any cache hit returns.)
        const int nb = ctx->nb, np = ctx->np, plo = lo[i], len = lo[i + 1] - lo[i];
        if (r.action.on()) {  // nothing to factor: the sweeps wait for the step table only
            if (nseg > 1) HIP_TRY(hipEventRecord(ctx->ev_factored[i], cs));
            return 0;
        }
        fa.step0 = plo; fa.seg_len = len;
        time_begin(ctx, 0, cs);
        if (ctx->explicit_mode) {
            // generators sampled by the host (opaque Hamiltonian): [seed][step] row-major
            qocx::launch_pq_explicit(nb, ctx->gen_rm.p + (size_t)b0 * ctx->nsteps * np * np, np, fa,
                                     bc * len, cs);
        } else if (r.nodes > 1) {
            ma.step0 = plo; ma.seg_len = len; ma.total = (size_t)bc * len;
            ma.m_rm = ctx->m_rm.p; ma.mbar_rm = nullptr; ma.gstep = nullptr;
            if (r.magnus4w) qocx::launch_magnus4w_fwd(ma, bc, cs);
            else qocx::launch_magnus_fwd(nb, ma, (int)std::min<size_t>(ma.total, 1024), cs);
            qocx::launch_pq_explicit(nb, ma.m_rm, np, fa, bc * len, cs);
        } else {
            qocx::launch_pq(nb, fa, len, bc, cs);
        }
        time_end(ctx, cs);
        if (!ctx->explicit_mode && r.nodes == 1 && qocx::pq_second_pending(nb, fa, len)) {
            // the second halves of the segment's factorisations (memory-bound: 4 KB in and out per
            // step) on the side stream, beside the K1a launch of the next segment
            HIP_TRY(hipEventRecord(ctx->ev_pq[i], cs));
            HIP_TRY(hipStreamWaitEvent(ctx->lu_stream, ctx->ev_pq[i], 0));
            time_begin(ctx, 4, ctx->lu_stream);
            qocx::launch_pq3_second(fa, len, bc, ctx->lu_stream);
            time_end(ctx, ctx->lu_stream);
            HIP_TRY(hipEventRecord(ctx->ev_factored[i], ctx->lu_stream));
            if (nseg <= 1) HIP_TRY(hipStreamWaitEvent(cs, ctx->ev_factored[i], 0));
            return 0;
        }
        la.step0 = plo; la.seg_len = len;
        // n > 32: K1b of this segment on a stream of its own, beside K1a of the next segment - the
        // four-wave K1a is bound by the matrix pipe, the two-wave / one-wave MFMA factorisation by
        // its pivot chains, and both fit a CU (n = 48: 34.2 -> 32.6 ms).
        // (At n <= 32 no gain: K1a then takes 1.08 ms per launch beside K1b instead of 0.80 + 0.32 ms
        // in sequence.)
        if (!r.fused_lu && nb == 4 && nseg > 1 && ctx->lu_stream != nullptr) {
            HIP_TRY(hipEventRecord(ctx->ev_pq[i], cs));
            HIP_TRY(hipStreamWaitEvent(ctx->lu_stream, ctx->ev_pq[i], 0));
            time_begin(ctx, 4, ctx->lu_stream);
            qocx::launch_lu(nb, la, (size_t)bc * len, ctx->lu_stream);
            time_end(ctx, ctx->lu_stream);
            HIP_TRY(hipEventRecord(ctx->ev_factored[i], ctx->lu_stream));
            return 0;
        }
        if (!r.fused_lu) {
            time_begin(ctx, 4, cs);
            qocx::launch_lu(nb, la, la.pack8 ? (size_t)bc * ((len + 1) / 2) : (size_t)bc * len, cs);
            // one control set: the propagator U = P^-1 Q in place of Q, one product per sweep sub-step
            if (r.umode) qocx::launch_umul(nb, la, fa.q_img, ctx->qt_img.p, (size_t)bc * len, cs);
            time_end(ctx, cs);
        }
        if (nseg > 1) HIP_TRY(hipEventRecord(ctx->ev_factored[i], cs));
        return 0;
    }

    // the sweep over steps [jb, je) on stream st: phase bit 0 forward, bit 1 adjoint
    void sweep(int jb, int je, int phase, hipStream_t st) {
        sa.j_begin = jb; sa.j_end = je; sa.phase = phase;
        time_begin(ctx, 1, st);
        if (!((dbg_skip & 1) && (phase & 1)) && !((dbg_skip & 2) && (phase & 2))) {
            if (r.action.on()) act.sweep(sa, st);
            else if (r.dense) qocx::launch_sweepd(sa, bc, st);
            else if (r.inverse_sweep) qocx::launch_sweepi(ctx->nb, sa, bc, st);
            else if (r.sweep3) qocx::launch_sweep3(ctx->nb, sa, bc, st);
            else qocx::launch_sweep(ctx->nb, sa, bc, st);
        }
        time_end(ctx, st);
    }

    // K3 (and the Magnus reverse rules) over steps [jb, je) on the compute stream
    void krylov(int jb, int je) {
        const int len = je - jb;
        ka.step0 = jb;
        time_begin(ctx, 2, cs);
        if (dbg_skip & 4) {
        } else if (r.action.on()) act.grad(jb, len, cs);
        else qocx::launch_krylov(ctx->nb, ka, len, bc, cs);
        if (r.nodes > 1) {
            ma.step0 = jb; ma.seg_len = len; ma.total = (size_t)bc * len;
            ma.m_rm = nullptr; ma.mbar_rm = ka.mbar_rm; ma.gstep = ka.gstep;
            if (r.magnus4w) qocx::launch_magnus4w_vjp(ma, bc, cs);
            else qocx::launch_magnus_vjp(ctx->nb, ma, (int)std::min<size_t>(ma.total, 1024), cs);
        }
        time_end(ctx, cs);
    }
};

// Factor + forward sweep segment by segment, then the adjoint sweep walks back with K3 behind it.
int run_one_sided(ResidentChunk& c) {
    qocx_ctx* ctx = c.ctx;
    const int nseg = c.nseg;
    for (int i = 0; i < nseg; ++i) {
        if (int rc = c.factor_segment(i)) return rc;
        if (nseg > 1) HIP_TRY(hipStreamWaitEvent(c.ss, ctx->ev_factored[i], 0));
        // (While the sweep needed a whole SIMD - 366 registers - the compute stream also waited here
        // until the sweep stream had passed its wait, or the next K1a grid starved the sweep. At 272
        // registers the sweep fits beside one K1a or K3 wave and the hand-shake only cost time.)
        c.sweep(c.lo[i], c.lo[i + 1], (nseg == 1 && c.want_grad) ? 3 : 1, c.ss);
    }
    // (Measured and dropped: evaluating a chunk as two seed halves with sweep streams of their own,
    // so that the first half's adjoint sweep runs under the second half's factorisation: 16.6 ms
    // against 14.6 ms.)
    if (nseg > 1 && c.want_grad) {
        for (int i = nseg - 1; i >= 0; --i) {
            c.sweep(c.lo[i], c.lo[i + 1], 2, c.ss);
            HIP_TRY(hipEventRecord(ctx->ev_swept[i], c.ss));
        }
    } else if (nseg > 1) {
        HIP_TRY(hipEventRecord(ctx->ev_swept[0], c.ss));
        HIP_TRY(hipStreamWaitEvent(c.cs, ctx->ev_swept[0], 0));
    }
    if (c.want_grad)
        for (int i = nseg - 1; i >= 0; --i) {
            if (nseg > 1) HIP_TRY(hipStreamWaitEvent(c.cs, ctx->ev_swept[i], 0));
            c.krylov(c.lo[i], c.lo[i + 1]);
        }
    return 0;
}

// The compute stream factors from both ends towards the middle; each sweep takes a segment as soon
// as it is factored AND the sweep has finished the one before it (stream order); K3 follows from
// the middle outwards.
// On the matrix-free route there is nothing to factor: each sweep runs to the crossing of the two as ONE
// launch and in pieces from there on (ActionPlan::fuse, below).
int run_two_sided(ResidentChunk& c) {
    qocx_ctx* ctx = c.ctx;
    const int nseg = c.nseg;
    const std::vector<int>& lo = c.lo;
    hipStream_t sf = ctx->sweep_streams[0], sb = ctx->sweep_streams[1];
    // The sweeps and K3 work in PIECES of the first and the last segment - the two whose sweeps
    // finish last: with them in pieces, all that is left of K3 once the sweeps have ended is a piece
    // of a segment (-0.05 ms, profiles/r05_k3_split_outer.jsonl). Every other segment is one piece:
    // at configs[1] 1 piece 12.86 ms, 2 -> 13.00, 3 -> 13.19, 4 -> 13.55 (every launch refills its
    // pipeline). (A small launch - one control set - is a chain of launch latencies: whole segments
    // there, configs[1] 0.57 -> 0.53 ms.)
    const bool small_launch = (size_t)c.bc * ctx->nsteps < 16384;
    int parts_out = small_launch ? 1 : 3;
    if ((nseg - 2) + 2 * parts_out > (int)ctx->ev_fwd.size()) parts_out = 1;
    struct Piece { int lo, hi; };
    std::vector<Piece> piece;
    std::vector<int> first(nseg + 1, 0);
    for (int i = 0; i < nseg; ++i) {
        const int np_i = (i == 0 || i == nseg - 1) ? parts_out : 1;
        first[i] = (int)piece.size();
        for (int part = 0; part < np_i; ++part)
            piece.push_back({lo[i] + (int)((int64_t)(lo[i + 1] - lo[i]) * part / np_i),
                             lo[i] + (int)((int64_t)(lo[i + 1] - lo[i]) * (part + 1) / np_i)});
    }
    first[nseg] = (int)piece.size();
    const int P = (int)piece.size();
    const int mid = first[nseg / 2];  // the piece at which the sweeps cross
    // The matrix-free route factors nothing (factor_segment only records its event), and no gradient launch
    // can begin before the sweeps have crossed: the launch boundaries of a sweep's way TO the crossing buy
    // nothing and each costs a launch gap and a start-up on the serial chain. So that way is ONE launch
    // (ActionPlan::fuse, the default), with the events of all its pieces recorded behind it; from the
    // crossing outwards the pieces stay, for the gradient to follow closely. A step's arithmetic does not
    // depend on where a launch begins: the same bits. Headline: the sweeps reach the crossing at 1.19 /
    // 1.30 ms instead of 1.64 / 1.67 (profiles/action_spread_timeline.txt).
    // (Measured and not kept, DESIGN.md 6: the pieces mid + d and mid - 1 - d as the two step ranges of ONE
    // gradient launch - the forward sweep is the faster of the two, so such a launch waits 0.1 ms for a
    // partner that the single piece does not need: 0.06-0.1 ms slower per evaluation.)
    const bool fuse_inward = c.r.action.on() && c.r.action.fuse;
    std::vector<char> factored(nseg, 0);
    int next_f = 0, next_b = nseg - 1;
    // (the adjoint sweep is the slower of the two - it gathers its images transposed -: with one control
    // set ITS side is factored first: 0.478 -> 0.456 ms at configs[1], 1.10 -> 1.05 ms at dim 32 x 1000
    // steps; the 256-seed evaluation, whose factor launches are what it waits for: 7.87 -> 8.00 ms)
    const bool adj_first = small_launch;
    for (int t = 0; t < nseg; ++t) {
        const bool back = adj_first ? (t % 2 == 0) : (t % 2 == 1);
        const int i = back ? nseg - 1 - t / 2 : t / 2;
        if (int rc = c.factor_segment(i)) return rc;
        factored[i] = 1;
        while (next_f < nseg && factored[next_f]) {
            HIP_TRY(hipStreamWaitEvent(sf, ctx->ev_factored[next_f], 0));
            // (every ev_factored of this route follows the step table on the compute stream, which is all a
            // sweep waits for: the first of them stands for the segments behind it)
            if (fuse_inward && next_f == 0) {  // the segments below the crossing in one launch
                if (piece[mid - 1].hi > piece[0].lo) c.sweep(piece[0].lo, piece[mid - 1].hi, 1, sf);
                for (int p = 0; p < mid; ++p) HIP_TRY(hipEventRecord(ctx->ev_fwd[p], sf));
                next_f = nseg / 2;
                continue;
            }
            for (int p = first[next_f]; p < first[next_f + 1]; ++p) {
                if (piece[p].hi > piece[p].lo) c.sweep(piece[p].lo, piece[p].hi, 1, sf);
                HIP_TRY(hipEventRecord(ctx->ev_fwd[p], sf));
            }
            ++next_f;
        }
        while (next_b >= 0 && factored[next_b]) {
            HIP_TRY(hipStreamWaitEvent(sb, ctx->ev_factored[next_b], 0));
            if (fuse_inward && next_b == nseg - 1) {  // the segments from the crossing up in one launch
                if (piece[P - 1].hi > piece[mid].lo) c.sweep(piece[mid].lo, piece[P - 1].hi, 2, sb);
                for (int p = P - 1; p >= mid; --p) HIP_TRY(hipEventRecord(ctx->ev_swept[p], sb));
                next_b = nseg / 2 - 1;
                continue;
            }
            for (int p = first[next_b + 1] - 1; p >= first[next_b]; --p) {
                if (piece[p].hi > piece[p].lo) c.sweep(piece[p].lo, piece[p].hi, 2, sb);
                HIP_TRY(hipEventRecord(ctx->ev_swept[p], sb));
            }
            --next_b;
        }
    }
    // K3 from the middle outwards: a piece is complete once the forward sweep (going up) and the
    // adjoint sweep (going down) have both crossed it
    for (int d = 0; d < P; ++d)
        for (int p : {mid + d, mid - 1 - d}) {
            if (p < 0 || p >= P || piece[p].hi <= piece[p].lo) continue;
            HIP_TRY(hipStreamWaitEvent(c.cs, ctx->ev_fwd[p], 0));
            HIP_TRY(hipStreamWaitEvent(c.cs, ctx->ev_swept[p], 0));
            c.krylov(piece[p].lo, piece[p].hi);
        }
    return 0;
}

}  // namespace

namespace qocx::host {

static int eval_resident(qocx_ctx* ctx, int32_t want_grad, bool allow_action);

// The evaluation of the ctx->B items of the uploaded controls (qocx_eval_resident)
int eval_items(qocx_ctx* ctx, int32_t want_grad) {
    if (!ctx->has_problem || ctx->B < 1) return fail(QOCX_ERR_STATE, "no problem / controls");
    HIP_TRY(hipSetDevice(ctx->device));
    const int B = ctx->B;
    const bool explicit_gen = ctx->explicit_mode;
    want_grad = (want_grad && (ctx->K > 0 || explicit_gen)) ? 1 : 0;
    if (explicit_gen && want_grad)
        if (ctx->genbar_rm.ensure((size_t)B * ctx->nsteps * ctx->np * ctx->np)) return QOCX_ERR_HIP;
    if (ctx->inj_count > 0 && ctx->inj_batch != B)
        return fail(QOCX_ERR_STATE, "state cotangents were set for a different batch size");
    // (the degrees of the matrix-free route: none executed unless its forward sweep says so)
    if (ctx->action_counts.p != nullptr)
        HIP_TRY(hipMemsetAsync(ctx->action_counts.p, 0, ctx->action_counts.count * sizeof(int), ctx->stream));
    if (ctx->general_path) return eval_general(ctx, want_grad);  // n > 64, or more states than the sweep's LDS (qocx_general.hip)
    int rc = eval_resident(ctx, want_grad, true);
    if (rc == kActionRefused) {
        // The host's bound was stale (qocx_opt_step moves the controls on the device): a step
        // asked for a Taylor degree beyond the buffers. Never clamped - the Pade route evaluates instead.
        ctx->action_reruns += 1;
        rc = eval_resident(ctx, want_grad, false);
    }
    return rc;
}

// ... on the resident pipeline, with or without the matrix-free route
int eval_resident(qocx_ctx* ctx, int32_t want_grad, bool allow_action) {
    const int B = ctx->B;
    const ResidentRoute route = resident_route(ctx, want_grad, allow_action);
    int chunk = 0;
    if (int rc = reserve_resident(ctx, route, want_grad, chunk)) return rc;
    HIP_TRY(hipMemsetAsync(ctx->status.p, 0, sizeof(int), ctx->stream));
    HIP_TRY(hipMemsetAsync(ctx->action_counts.p, 0, ctx->action_counts.count * sizeof(int), ctx->stream));
    for (int b0 = 0; b0 < B; b0 += chunk) {
        ResidentChunk c(ctx, route, want_grad, b0, std::min(chunk, B - b0));
        ctx->last_chunk = c.bc;
        if (int rc = c.init()) return rc;
        if (int rc = c.two_sided ? run_two_sided(c) : run_one_sided(c)) return rc;
        if (want_grad) scatter_gradients(ctx, c.eff, ctx->gstep.p, c.lam_scale(), b0, c.bc, c.cs);
    }
    return finish_items(ctx, want_grad);
}

}  // namespace qocx::host
