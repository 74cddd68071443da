// qocx_host_action.h - the host side of the matrix-free route (ActionPlan, qocx_action_route.h): its
// buffers, the argument blocks of a chunk and every launch of its kernel families. Part of
// qocx_host_resident.hip, which includes it behind EffCtlChunk and nowhere else; the plain step table
// (ActionPlan::PLAIN) is the resident pipeline's own launch there.
#ifndef QOCX_HOST_ACTION_H
#define QOCX_HOST_ACTION_H

#include "qocx_action_route.h"

namespace {

using qocx::ActionPlan;

// Seeds per chunk from the memory budget (or the user's chunk), and the device buffers of a chunk:
// no Q / LU images, 1 / U_kk, permutations or sub-step slots - the Taylor terms of both sweeps
// (gradient wanted) of every state, the step table and the step cotangents
// (on effective controls: Ke channels per step in veff and gstep, and the chain kernel's output)
int reserve_action(qocx_ctx* ctx, const ActionPlan& plan, EffKind eff, int want_grad, int& chunk) {
    const int B = ctx->B, np = ctx->np, S = ctx->S, K = ctx->K, nsteps = ctx->nsteps;
    const bool on_eff = plan.table == ActionPlan::EFF;
    const size_t Kc = (size_t)plan.channels;
    const size_t terms = want_grad ? (size_t)S * plan.m_max * np : 0;
    const size_t seed_bytes = (size_t)nsteps * (2 * terms * 16 + 4 + Kc * 8 + Kc * 16 + (on_eff ? (size_t)K * 16 : 0)) +
                              (size_t)S * np * 64;
    chunk = ctx->chunk_user;
    if (chunk <= 0) {
        size_t free_b = 0, total_b = 0;
        HIP_TRY(hipMemGetInfo(&free_b, &total_b));
        const size_t have = (ctx->kry_f.count + ctx->kry_b.count) * 16;
        const size_t budget = (size_t)((double)(free_b + have) * 0.6);
        chunk = (int)std::min<size_t>((size_t)B, std::max<size_t>(1, budget / seed_bytes));
    }
    chunk = std::min(chunk, B);
    const size_t cm = (size_t)chunk * nsteps;
    if (ctx->s_arr.ensure(cm) || ctx->kry_f.ensure(std::max<size_t>(1, cm * terms)) ||
        ctx->kry_b.ensure(std::max<size_t>(1, cm * terms)) || ctx->action_carry.ensure((size_t)chunk * S * np) ||
        ctx->gstep.ensure(cm * std::max<size_t>(Kc, 1) * 2) || ctx->cost_out.ensure(B) ||
        (on_eff && EffCtlChunk::reserve(ctx, eff, cm, want_grad)) ||
        ctx->grads.ensure((size_t)B * ctx->nc * std::max(K, 1)) || ctx->final_out.ensure((size_t)B * S * np) ||
        ctx->lam_buf.ensure((size_t)chunk * S * np) || ctx->lu_fallbacks.ensure(1))
        return QOCX_ERR_HIP;
    return 0;
}

// The route's argument blocks of one chunk of `bc` seeds and its launches: one switch over the plan's
// kernel for the sweeps, one for the gradient.
struct ActionChunk {
    qocx_ctx* ctx = nullptr;
    ActionPlan plan;
    int bc = 0;
    qocx::ActionArgs aa;
    qocx::ActionGradArgs ga;
    qocx::ActionStatesGradArgs sga;  // ... with several states per seed (qocx_action_states.hip)

    // ActionPlan::EFF: launches the table of qocx_action_eff.hip through `eff`, in place of its controls
    // kernel - the same veff, and the step words with the Taylor degrees (PLAIN: the caller has launched
    // launch_step_table). Then the argument blocks; fails where the gradient kernel would miss its E images.
    int init(qocx_ctx* c, const ActionPlan& p, EffCtlChunk& eff, EffKind kind, const double* controls,
             const double2* lam_scale, int want_grad, int b0, int count, hipStream_t cs) {
        ctx = c; plan = p; bc = count;
        const bool on_eff = plan.table == ActionPlan::EFF;
        if (on_eff) eff.table(ctx, kind, controls, lam_scale, b0, bc, cs, plan.degree_rule);
        aa.ustep = ctx->ustep.p; aa.h0_rimg = ctx->h0.r.p; aa.g_rimg = ctx->g.r.p;
        aa.K = ctx->K; aa.m_max = plan.m_max; aa.dt = ctx->dt;
        aa.kv_f = want_grad ? ctx->kry_f.p : nullptr;
        aa.kv_b = want_grad ? ctx->kry_b.p : nullptr;
        aa.carry_f = ctx->action_carry.p;
        aa.degree_counts = ctx->action_counts.p;
        ga.kv_f = ctx->kry_f.p; ga.kv_b = ctx->kry_b.p; ga.s_arr = ctx->s_arr.p; ga.g_rimg = ctx->g.r.p;
        ga.K = ctx->K; ga.m_max = plan.m_max; ga.nsteps = ctx->nsteps; ga.dt = ctx->dt; ga.gstep = ctx->gstep.p;
        ga.e_img = ctx->g_eimg.p;
        if (on_eff) {  // one row of Ke effective controls per step over the augmented operators
            aa.ustep = ctx->eff.veff.p; aa.g_rimg = ga.g_rimg = ctx->eff.images.r.p;
            aa.K = ga.K = plan.channels; ga.e_img = ctx->eff.eimg.p;
        }
        if (want_grad && ctx->nb <= 2 && ctx->S == 1 && plan.kernel != ActionPlan::COSTS && ga.e_img == nullptr)
            return fail(QOCX_ERR_STATE, "the matrix-free gradient has no image of -i dt G_k (upload_operators)");
        sga.S = ctx->S;
        return 0;
    }

    // the sweep `sw` describes (steps, phase, and the chunk's state and cost arguments) on stream st
    void sweep(const qocx::SweepArgs& sw, hipStream_t st) {
        aa.sw = sw;
        switch (plan.kernel) {
            case ActionPlan::N32: qocx::launch_action_sweep(aa, bc, st); break;
            case ActionPlan::N32_EFF_EXACT: qocx::launch_action_eff_sweep(aa, bc, st); break;
            case ActionPlan::STATES: qocx::launch_action_states_sweep(aa, bc, st); break;
            case ActionPlan::COSTS: qocx::launch_action_costs_sweep(aa, bc, st); break;
            case ActionPlan::N16: qocx::launch_action16_sweep(aa, bc, st); break;
            case ActionPlan::N64: qocx::launch_action4_sweep(ctx->n, aa, bc, st); break;
            case ActionPlan::NONE: break;
        }
    }

    // the step cotangents of steps [jb, jb + len) from the terms the two sweeps left, on stream cs
    void grad(int jb, int len, hipStream_t cs) {
        ga.step0 = jb;
        switch (plan.kernel) {
            case ActionPlan::N32:
            case ActionPlan::N32_EFF_EXACT: qocx::launch_action_grad(ga, len, bc, cs); break;
            case ActionPlan::STATES:
                sga.g = ga;
                qocx::launch_action_states_grad(sga, len, bc, cs);
                break;
            case ActionPlan::COSTS: qocx::launch_action_costs_grad(ga, len, bc, cs); break;
            case ActionPlan::N16: qocx::launch_action16_grad(ga, len, bc, cs); break;
            case ActionPlan::N64: qocx::launch_action4_grad(ctx->n, ga, len, bc, cs); break;
            case ActionPlan::NONE: break;
        }
    }
};

}  // namespace

#endif
