// qocx_api_multistart.hip - the multi-start GRAPE driver of the C ABI (include/qocx.h): one
// device-resident optimizer driver for both paths (qocx_opt_* / qocx_lindblad_opt_*), the costs of the
// controls alone (qocx_set_control_costs) and the host-side helpers of the driver.
#include <thread>

#include "qocx_host.h"

// ---- host-side helpers of the multi-start GRAPE driver (include/qocx.h) ---------------------------
namespace {
template <class F>
void host_parallel_rows(int64_t count, F f) {
    const unsigned hw = std::max(1u, std::min(8u, std::thread::hardware_concurrency()));
    const int64_t nthreads = std::max<int64_t>(1, std::min<int64_t>((int64_t)hw, count / 8));
    if (nthreads <= 1) {
        f(0, count);
        return;
    }
    std::vector<std::thread> pool;
    const int64_t per = (count + nthreads - 1) / nthreads;
    for (int64_t t = 1; t < nthreads; ++t) {
        const int64_t lo = t * per, hi = std::min(count, lo + per);
        if (lo < hi) pool.emplace_back([=] { f(lo, hi); });
    }
    f(0, std::min(count, per));  // the calling thread takes the first share
    for (auto& th : pool) th.join();
}

// One row of Adam.update. Every product and sum is rounded on its own, as NumPy's array
// operations are (no contraction into fused multiply-adds); division and square root are the
// IEEE ones in scalar and in vector form alike, so the AVX2 clone gives the same bits.
#if defined(__x86_64__) && !defined(__HIP_DEVICE_COMPILE__)
__attribute__((target_clones("avx2", "default")))
#endif
void adam_row(double* __restrict x, const double* __restrict g, double* __restrict m,
              double* __restrict v, int64_t p, double learning_rate, double beta_1, double beta_2,
              double one_m_b1, double one_m_b2, double epsilon, double corr_1, double corr_2,
              int apply_clip, double clip) {
#pragma clang fp contract(off)
    for (int64_t i = 0; i < p; ++i) {
        double gi = g[i];
        if (apply_clip) gi = gi < -clip ? -clip : (gi > clip ? clip : gi);
        const double a = beta_1 * m[i], b = one_m_b1 * gi;
        const double mi = a + b;
        const double sq = gi * gi;
        const double c = beta_2 * v[i], d = one_m_b2 * sq;
        const double vi = c + d;
        m[i] = mi;
        v[i] = vi;
        const double mh = mi / corr_1, vh = vi / corr_2;
        const double den = sqrt(vh) + epsilon;
        const double q = mh / den;
        const double s = learning_rate * q;
        x[i] = x[i] - s;
    }
}
}  // namespace

namespace qocx::host {

// ---- costs of the controls alone (qocx_set_control_costs) -----------------------------------------

// cc.cost [B] and, if want_grad, cc.grad [B][nc][Kr] of the control sets `controls` on the device
int run_control_costs(qocx_ctx* ctx, ControlCosts& cc, int B, int nc, int Kr, const double* controls,
                      bool want_grad) {
    if (cc.Kr != Kr || cc.nc != nc)
        return fail(QOCX_ERR_STATE, "the control costs were set for another control layout "
                                    "(qocx_set_control_costs after qocx_set_ensemble)");
    const size_t total = (size_t)B * nc * Kr;
    if ((size_t)nc * Kr > 0x7fffffffu) return fail(QOCX_ERR_ARG, "control arrays too large for the control-cost kernels");
    if (cc.cost.ensure((size_t)B) || (want_grad && cc.grad.ensure(total)) ||
        (cc.variation && (cc.work0.ensure(total) || cc.work1.ensure(total))))
        return QOCX_ERR_HIP;
    qocx::CtrlCostArgs a;
    a.controls = controls; a.cost = cc.cost.p; a.grad = want_grad ? cc.grad.p : nullptr;
    a.work0 = cc.work0.p; a.work1 = cc.work1.p;
    a.descs = cc.descs.p; a.count = cc.elementwise;
    a.B = B; a.nc = nc; a.Kr = Kr; a.cplx = cc.cplx;
    qocx::launch_control_costs(a, ctx->stream);
    int pmax = 0;  // (one allocation for all bandwidth costs: none while a kernel is in flight)
    for (const auto& bw : cc.bandwidth) pmax = std::max(pmax, bw.pmax);
    if (pmax > 0) {
        if (cc.spectrum.ensure((size_t)B * Kr * pmax) || (want_grad && cc.ybar.ensure((size_t)B * cc.K * pmax)))
            return QOCX_ERR_HIP;
        if ((size_t)B * (1 + cc.cplx) / 8 + 1 > 65535u)
            return fail(QOCX_ERR_ARG, "batch too large for the bandwidth kernels' grids");
    }
    for (const auto& bw : cc.bandwidth) {
        qocx::BandwidthArgs w;
        w.controls = controls; w.twiddle = cc.twiddle.p;
        w.bins = cc.ints.p + bw.bins; w.bin_ptr = cc.ints.p + bw.bin_ptr;
        w.spectrum = cc.spectrum.p; w.ybar = cc.ybar.p;
        w.cost = cc.cost.p; w.grad = want_grad ? cc.grad.p : nullptr;
        w.multiplier = bw.multiplier;
        w.B = B; w.nc = nc; w.Kr = Kr; w.K = cc.K; w.cplx = cc.cplx; w.pmax = bw.pmax;
        qocx::launch_bandwidth_cost(w, ctx->stream);
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // namespace qocx::host

// ---- the multi-start driver: resident optimizer states of the seeds of one path -------------------
namespace {

// What the driver needs of a path: its seeds' resident controls and results. Built by value from
// the path's own state at every call (an evaluation may have moved the buffers since).
struct SeedView {
    int seeds, channels, nc;  // seeds; control channels per seed; control knots
    double* controls;         // [seeds][nc][channels]
    double* grads;            // [seeds][nc][channels]
    double* cost;             // [seeds] total costs of the last resident evaluation
    double2* finals;          // [seeds][final_elems]
    size_t final_elems;       // elements of final state per seed
    size_t per_seed() const { return (size_t)nc * channels; }
    size_t total() const { return (size_t)seeds * nc * channels; }
};

// (ensemble: a seed's K_r channels, and the final states of its M items)
SeedView schroedinger_seeds(qocx_ctx* ctx) {
    const size_t items = ctx->seeds.M > 0 ? (size_t)ctx->seeds.M : 1;
    return SeedView{seed_count(ctx), seed_channels(ctx), ctx->nc, seed_controls(ctx), seed_grads(ctx),
                    seed_costs(ctx), ctx->final_out.p, items * ctx->S * ctx->np};
}

// (ensemble: a seed's K_r channels, and the final densities of its M items)
SeedView lindblad_seeds(qocx_ctx* ctx) {
    auto& lb = ctx->lb;
    return SeedView{lb.res_B, lb.seed_channels(), lb.nc, lb.res_controls.p, lb.res_grads.p, lb.res_cost.p,
                    lb.res_final.p, lb.seed_items() * lb.S * dump_elems(lb.n)};
}

// What the optimizer works on, as distinct from what is evaluated (the SeedView): the seeds' controls
// and their gradients themselves, the unclipped copy of complex controls, or - with a control basis -
// the coefficients and the projected gradients, P * channels per seed. Every optimizer state (Adam
// moments, the L-BFGS vectors, ring and capacity check) is sized by it.
struct ParamView {
    double* params;       // [seeds][per_seed]
    const double* grads;  // [seeds][per_seed]
    size_t per_seed, total;
};

// (the sizes alone are valid from the top of multistart_begin on: they follow from ms.basis_P)
ParamView optimizer_params(MultiStart& ms, const SeedView& v) {
    if (ms.basis_P > 0) {
        const size_t per = (size_t)ms.basis_P * v.channels;
        return ParamView{ms.opt_params.p, ms.basis_grads.p, per, (size_t)v.seeds * per};
    }
    return ParamView{ms.complex_controls ? ms.opt_params.p : v.controls, v.grads, v.per_seed(), v.total()};
}

// A control basis for multistart_begin: M [nc][P] and the seeds' coefficients [seeds][P][channels] on
// the host (P = 0: none)
struct BasisStart {
    int P = 0;
    const double* matrix = nullptr;
    const double* coefficients = nullptr;
};

// the seeds' optimizer states, zeroed; complex controls: the parameters start as the seeds' controls;
// a control basis: the parameters are its coefficients
int multistart_begin(qocx_ctx* ctx, MultiStart& ms, const SeedView& v, int batch, bool complex_controls,
                     const BasisStart& basis = BasisStart()) {
    ms.basis_P = 0;
    std::vector<double> transposed;
    if (basis.P > 0) {
        ms.batch = 0;  // (until the basis stands)
        if (complex_controls && v.channels % 2)
            return fail(QOCX_ERR_ARG, "complex controls need an even number of channels");
        const size_t entries = (size_t)v.nc * basis.P;
        for (size_t i = 0; i < entries; ++i)
            if (!std::isfinite(basis.matrix[i])) return fail(QOCX_ERR_ARG, "non-finite basis matrix");
        if ((size_t)basis.P * v.channels > 65535u * 256u)
            return fail(QOCX_ERR_ARG, "coefficient arrays too large for the optimizer kernels' grids");
        transposed.resize(entries);
        for (int j = 0; j < v.nc; ++j)
            for (int p = 0; p < basis.P; ++p) transposed[(size_t)p * v.nc + j] = basis.matrix[(size_t)j * basis.P + p];
        ms.basis_P = basis.P;
    }
    const size_t total = v.total(), ptotal = optimizer_params(ms, v).total;
    if (ms.opt_m.ensure(ptotal) || ms.opt_v.ensure(ptotal) || ms.opt_best_controls.ensure(total) ||
        ms.opt_best_final.ensure((size_t)v.seeds * v.final_elems) ||
        ms.opt_flags.ensure(2 * (size_t)v.seeds) || ms.opt_max_norms.ensure((size_t)v.channels)) {
        ms.basis_P = 0;
        return QOCX_ERR_HIP;
    }
    HIP_TRY(hipMemsetAsync(ms.opt_m.p, 0, ptotal * sizeof(double), ctx->stream));
    HIP_TRY(hipMemsetAsync(ms.opt_v.p, 0, ptotal * sizeof(double), ctx->stream));
    ms.lbfgs_history = 0;  // (L-BFGS state is set up per batch: qocx_opt_lbfgs_begin)
    ms.complex_controls = false;
    if (basis.P > 0) {
        const size_t entries = (size_t)v.nc * basis.P;
        if (ms.opt_params.ensure(ptotal) || ms.opt_best_params.ensure(ptotal) || ms.basis_grads.ensure(ptotal) ||
            ms.basis_matrix.ensure(entries) || ms.basis_matrix_t.ensure(entries)) {
            ms.basis_P = 0;
            return QOCX_ERR_HIP;
        }
        hipError_t e = hipMemcpyAsync(ms.basis_matrix.p, basis.matrix, entries * sizeof(double),
                                      hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess)
            e = hipMemcpyAsync(ms.basis_matrix_t.p, transposed.data(), entries * sizeof(double),
                               hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess)
            e = hipMemcpyAsync(ms.opt_params.p, basis.coefficients, ptotal * sizeof(double),
                               hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess) e = hipMemsetAsync(ms.opt_best_params.p, 0, ptotal * sizeof(double), ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);  // the arrays are the caller's (and local) memory
        if (e != hipSuccess) {
            ms.basis_P = 0;
            return fail(QOCX_ERR_HIP, std::string("control basis upload: ") + hipGetErrorString(e));
        }
        ms.complex_controls = complex_controls;
        ms.batch = batch;
        return 0;
    }
    ms.batch = batch;
    if (!complex_controls) return 0;
    if (v.channels % 2) return fail(QOCX_ERR_ARG, "complex controls need an even number of channels");
    if (ms.opt_params.ensure(total)) return QOCX_ERR_HIP;
    HIP_TRY(hipMemcpyAsync(ms.opt_params.p, v.controls, total * sizeof(double), hipMemcpyDeviceToDevice,
                           ctx->stream));
    ms.complex_controls = true;
    return 0;
}

// max_norms to the device and the clip of the seeds' controls, enqueued: the caller synchronises
// (max_norms is its caller's memory). Complex controls: max_norms [channels / 2] bound the moduli.
int multistart_clip(qocx_ctx* ctx, MultiStart& ms, const SeedView& v, const double* max_norms) {
    const int Kn = ms.complex_controls ? v.channels / 2 : v.channels;
    HIP_TRY(hipMemcpyAsync(ms.opt_max_norms.p, max_norms, Kn * sizeof(double), hipMemcpyHostToDevice,
                           ctx->stream));
    if (ms.basis_P > 0) {  // the coefficients expanded into the evaluation buffer, which is then clipped
        qocx::launch_basis_expand(ms.basis_matrix_t.p, ms.opt_params.p, v.controls, v.seeds, v.nc, ms.basis_P,
                                  v.channels, ctx->stream);
        if (ms.complex_controls)  // (in place: every thread reads its pair before it writes it)
            qocx::launch_clip_complex(v.controls, v.controls, v.total() / 2, Kn, ms.opt_max_norms.p, ctx->stream);
        else
            qocx::launch_clip_controls(v.controls, v.total(), v.channels, ms.opt_max_norms.p, ctx->stream);
    } else if (ms.complex_controls)
        qocx::launch_clip_complex(ms.opt_params.p, v.controls, v.total() / 2, Kn, ms.opt_max_norms.p,
                                  ctx->stream);
    else
        qocx::launch_clip_controls(v.controls, v.total(), v.channels, ms.opt_max_norms.p, ctx->stream);
    return 0;
}

// the update rule of one optimizer step (Adam.update / SGD.update of the host loop)
struct StepRule {
    int32_t kind;  // 0 SGD, 1 Adam
    double learning_rate, beta_1, beta_2, epsilon, corr_1, corr_2;
    int32_t apply_clip_grads;
    double clip_grads;
};

// The head of every optimizer step: the flags to the device, the controls and final states of the
// improved seeds kept; with a control basis their coefficients too, and the evaluation's gradients
// projected onto the coefficients. Returns what the optimizer kernel then works on.
int multistart_keep_best(qocx_ctx* ctx, MultiStart& ms, const SeedView& v, const uint8_t* improved,
                         const uint8_t* update, ParamView& pv) {
    const int B = v.seeds;
    HIP_TRY(hipMemcpyAsync(ms.opt_flags.p, improved, B, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(ms.opt_flags.p + B, update, B, hipMemcpyHostToDevice, ctx->stream));
    qocx::launch_keep_best(v.controls, ms.opt_best_controls.p, v.per_seed(), v.finals, ms.opt_best_final.p,
                           v.final_elems, ms.opt_flags.p, B, ctx->stream);
    pv = optimizer_params(ms, v);
    if (ms.basis_P > 0) {
        qocx::launch_keep_best(ms.opt_params.p, ms.opt_best_params.p, pv.per_seed, nullptr, nullptr, 0,
                               ms.opt_flags.p, B, ctx->stream);
        qocx::launch_basis_project(ms.basis_matrix.p, v.grads, ms.basis_grads.p, B, v.nc, ms.basis_P, v.channels,
                                   ctx->stream);
    }
    return 0;
}

// keeps the controls and final states of the improved seeds, then steps the seeds flagged in `update`;
// `durations` (a duration search: tau, its gradient, moments and best): the same for the seeds' tau
int multistart_step(qocx_ctx* ctx, MultiStart& ms, const SeedView& v, const StepRule& rule,
                    const uint8_t* improved, const uint8_t* update,
                    const qocx::DurationStepArgs* durations = nullptr) {
    const int B = v.seeds;
    ParamView pv;
    if (int rc = multistart_keep_best(ctx, ms, v, improved, update, pv)) return rc;
    qocx::OptimArgs a;
    a.kind = rule.kind;
    a.params = pv.params; a.grads = pv.grads;
    a.moment = ms.opt_m.p; a.square_moment = ms.opt_v.p;
    a.update = ms.opt_flags.p + B;
    a.per_seed = pv.per_seed;
    a.learning_rate = rule.learning_rate; a.beta_1 = rule.beta_1; a.beta_2 = rule.beta_2;
    a.one_m_b1 = 1 - rule.beta_1; a.one_m_b2 = 1 - rule.beta_2;
    a.epsilon = rule.epsilon; a.corr_1 = rule.corr_1; a.corr_2 = rule.corr_2;
    a.clip = rule.clip_grads; a.apply_clip = rule.apply_clip_grads ? 1 : 0;
    qocx::launch_optimizer_update(a, B, ctx->stream);
    if (durations) {  // one more element per seed, the same rule: one thread each (qocx_duration.hip)
        qocx::DurationStepArgs d = *durations;
        const qocx::OptimArgs tau = d.rule;
        d.rule = a;
        d.rule.params = tau.params; d.rule.grads = tau.grads;
        d.rule.moment = tau.moment; d.rule.square_moment = tau.square_moment;
        d.rule.per_seed = 1;
        d.improved = ms.opt_flags.p;
        d.B = B;
        qocx::launch_duration_step(d, ctx->stream);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(ctx->stream));  // the flag arrays are the caller's memory
    return 0;
}

// the L-BFGS state of the seeds, zeroed: accepted point, its gradient, direction, `history` pairs
int multistart_lbfgs_begin(qocx_ctx* ctx, MultiStart& ms, const SeedView& v, int history) {
    if (history < 1 || history > qocx::LBFGS_MAX_HISTORY)
        return fail(QOCX_ERR_ARG, "history must be in 1..64");
    ms.lbfgs_history = 0;
    const size_t total = optimizer_params(ms, v).total, ring = total * (size_t)history;
    const size_t bytes = (3 * total + 2 * ring + (size_t)v.seeds * history) * sizeof(double) +
                         (size_t)v.seeds * (sizeof(qocx::LbfgsSeed) + 1);
    size_t held = 0;  // (what a previous run of the same size left allocated is taken again)
    for (const DevBuf<double>* buf : {&ms.lb_x, &ms.lb_g, &ms.lb_d, &ms.lb_s, &ms.lb_y, &ms.lb_rho})
        held += buf->count * sizeof(double);
    size_t free_bytes = 0, device_bytes = 0;
    HIP_TRY(hipMemGetInfo(&free_bytes, &device_bytes));
    if (bytes > held && bytes - held > free_bytes)
        return fail(QOCX_ERR_CAPACITY, "the L-BFGS state of " + std::to_string(v.seeds) + " seeds (" +
                                           std::to_string(bytes) + " bytes) does not fit the free device memory");
    if (ms.lb_x.ensure(total) || ms.lb_g.ensure(total) || ms.lb_d.ensure(total) || ms.lb_s.ensure(ring) ||
        ms.lb_y.ensure(ring) || ms.lb_rho.ensure((size_t)v.seeds * history) ||
        ms.lb_seed.ensure((size_t)v.seeds) || ms.lb_finished.ensure((size_t)v.seeds))
        return QOCX_ERR_HIP;
    HIP_TRY(hipMemsetAsync(ms.lb_x.p, 0, total * sizeof(double), ctx->stream));
    HIP_TRY(hipMemsetAsync(ms.lb_g.p, 0, total * sizeof(double), ctx->stream));
    HIP_TRY(hipMemsetAsync(ms.lb_d.p, 0, total * sizeof(double), ctx->stream));
    HIP_TRY(hipMemsetAsync(ms.lb_s.p, 0, ring * sizeof(double), ctx->stream));
    HIP_TRY(hipMemsetAsync(ms.lb_y.p, 0, ring * sizeof(double), ctx->stream));
    HIP_TRY(hipMemsetAsync(ms.lb_rho.p, 0, (size_t)v.seeds * history * sizeof(double), ctx->stream));
    HIP_TRY(hipMemsetAsync(ms.lb_seed.p, 0, (size_t)v.seeds * sizeof(qocx::LbfgsSeed), ctx->stream));
    HIP_TRY(hipMemsetAsync(ms.lb_finished.p, 0, (size_t)v.seeds, ctx->stream));
    ms.lbfgs_history = history;
    return 0;
}

// the step rule of LBFGS.update (qoc_amd/standard/optimizers/lbfgs.py)
struct LbfgsRule {
    double first_step, armijo, shrink;
    int32_t max_backtracks;
};

// keeps the controls and final states of the improved seeds, then runs the L-BFGS state machine of the
// seeds flagged in `update` on the last evaluation's costs and gradients; finished_out [seeds]
int multistart_lbfgs_step(qocx_ctx* ctx, MultiStart& ms, const SeedView& v, const LbfgsRule& rule,
                          const uint8_t* improved, const uint8_t* update, uint8_t* finished_out) {
    const int B = v.seeds;
    ParamView pv;
    if (int rc = multistart_keep_best(ctx, ms, v, improved, update, pv)) return rc;
    qocx::LbfgsArgs a;
    a.params = pv.params;
    a.grads = pv.grads; a.cost = v.cost;
    a.x = ms.lb_x.p; a.g = ms.lb_g.p; a.d = ms.lb_d.p; a.s = ms.lb_s.p; a.y = ms.lb_y.p;
    a.rho = ms.lb_rho.p; a.seed = ms.lb_seed.p;
    a.update = ms.opt_flags.p + B; a.finished = ms.lb_finished.p;
    a.per_seed = pv.per_seed;
    a.interleaved = ms.complex_controls ? 1 : 0;
    a.history = ms.lbfgs_history;
    a.first_step = rule.first_step; a.armijo = rule.armijo; a.shrink = rule.shrink;
    a.max_backtracks = rule.max_backtracks;
    qocx::launch_lbfgs_step(a, B, ctx->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(finished_out, ms.lb_finished.p, B, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));  // the flag arrays are the caller's memory
    return 0;
}

// the best controls as they are and the best final states in the device's layout (`fin`, where wanted)
int multistart_download_best(qocx_ctx* ctx, MultiStart& ms, const SeedView& v, double* controls_out,
                             std::vector<double2>* fin) {
    if (controls_out)
        HIP_TRY(hipMemcpyAsync(controls_out, ms.opt_best_controls.p, v.total() * sizeof(double),
                               hipMemcpyDeviceToHost, ctx->stream));
    if (fin) {
        fin->resize((size_t)v.seeds * v.final_elems);
        HIP_TRY(hipMemcpyAsync(fin->data(), ms.opt_best_final.p, fin->size() * sizeof(double2),
                               hipMemcpyDeviceToHost, ctx->stream));
    }
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return 0;
}

// the coefficients [seeds][P][channels] of the best so far (a driver begun with a control basis)
int multistart_download_best_params(qocx_ctx* ctx, MultiStart& ms, const SeedView& v, double* params_out) {
    if (!params_out) return fail(QOCX_ERR_ARG, "NULL argument");
    if (ms.basis_P < 1) return fail(QOCX_ERR_STATE, "the driver was not begun with a control basis");
    HIP_TRY(hipMemcpyAsync(params_out, ms.opt_best_params.p, optimizer_params(ms, v).total * sizeof(double),
                           hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return 0;
}

// a duration search: the optimizer state of the seeds' tau - moments and best, zeroed
int durations_begin(qocx_ctx* ctx, SeedTables::Durations& dur, size_t B, MultiStart& ms) {
    if (!dur.set) return 0;
    if (dur.m.ensure(B) || dur.v.ensure(B) || dur.best.ensure(B)) {
        ms.batch = 0;
        return QOCX_ERR_HIP;
    }
    for (DevBuf<double>* buf : {&dur.m, &dur.v, &dur.best})
        HIP_TRY(hipMemsetAsync(buf->p, 0, B * sizeof(double), ctx->stream));
    return 0;
}

// ... its part of an optimizer step: tau, its gradient (which must stand), the moments and the best
int durations_rule(SeedTables::Durations& dur, qocx::DurationStepArgs& step) {
    if (!dur.have_grad) return fail(QOCX_ERR_STATE, "no duration gradients to step with");
    step.rule.params = dur.tau.p; step.rule.grads = dur.grad.p;
    step.rule.moment = dur.m.p; step.rule.square_moment = dur.v.p;
    step.best_tau = dur.best.p;
    return 0;
}

// ... and the tau of the best so far [B]; `set_by`: the path's setter, for the message
int durations_download_best(qocx_ctx* ctx, SeedTables::Durations& dur, size_t B, const char* set_by, double* tau_out) {
    if (!dur.set) return fail(QOCX_ERR_STATE, std::string("no durations set (") + set_by + ")");
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipMemcpyAsync(tau_out, dur.best.p, B * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return 0;
}

int schroedinger_opt_begin(qocx_ctx* ctx, bool complex_controls, const BasisStart& basis = BasisStart()) {
    if (!ctx) return fail(QOCX_ERR_ARG, "ctx is NULL");
    if (!ctx->has_problem || ctx->B < 1 || ctx->K < 1 || ctx->explicit_mode)
        return fail(QOCX_ERR_STATE, "qocx_opt_begin needs uploaded controls of a structured problem");
    HIP_TRY(hipSetDevice(ctx->device));
    // (the seeds' optimizer states; the best final states of every item)
    if (int rc = multistart_begin(ctx, ctx->ms, schroedinger_seeds(ctx), ctx->B, complex_controls, basis)) return rc;
    return durations_begin(ctx, ctx->seeds.dur, (size_t)ctx->seeds.swp_B, ctx->ms);
}

int lindblad_opt_begin(qocx_ctx* ctx, bool complex_controls, const BasisStart& basis = BasisStart()) {
    if (!ctx) return fail(QOCX_ERR_ARG, "ctx is NULL");
    auto& lb = ctx->lb;
    if (!lb.has_problem || lb.res_B < 1)
        return fail(QOCX_ERR_STATE, "qocx_lindblad_opt_begin needs resident Lindblad controls");
    HIP_TRY(hipSetDevice(ctx->device));
    if (int rc = multistart_begin(ctx, lb.ms, lindblad_seeds(ctx), lb.res_B, complex_controls, basis)) return rc;
    return durations_begin(ctx, lb.seeds.dur, (size_t)lb.seeds.swp_B, lb.ms);
}

// the arguments of *_opt_begin_basis, checked
int basis_start(int32_t p, const double* matrix, const double* coefficients, BasisStart& out) {
    if (p < 1) return fail(QOCX_ERR_ARG, "a control basis needs P >= 1 coefficients");
    if (!matrix || !coefficients) return fail(QOCX_ERR_ARG, "NULL argument");
    out.P = p;
    out.matrix = matrix;
    out.coefficients = coefficients;
    return 0;
}

}  // namespace

extern "C" {

// ---- the Schroedinger path: the seeds of qocx_upload_controls ---------------------------------------

int qocx_opt_begin(qocx_ctx* ctx) { return schroedinger_opt_begin(ctx, false); }

int qocx_opt_begin_complex(qocx_ctx* ctx) { return schroedinger_opt_begin(ctx, true); }

int qocx_opt_begin_basis(qocx_ctx* ctx, int32_t complex_controls, int32_t p, const double* matrix,
                         const double* coefficients) {
    BasisStart basis;
    if (int rc = basis_start(p, matrix, coefficients, basis)) return rc;
    return schroedinger_opt_begin(ctx, complex_controls != 0, basis);
}

int qocx_opt_download_best_params(qocx_ctx* ctx, double* params_out) {
    if (!ctx) return fail(QOCX_ERR_ARG, "ctx is NULL");
    if (ctx->ms.batch != ctx->B || ctx->B < 1) return fail(QOCX_ERR_STATE, "qocx_opt_begin has not run for this batch");
    HIP_TRY(hipSetDevice(ctx->device));
    return multistart_download_best_params(ctx, ctx->ms, schroedinger_seeds(ctx), params_out);
}

int qocx_opt_clip(qocx_ctx* ctx, const double* max_norms) {
    if (!ctx || !max_norms) return fail(QOCX_ERR_ARG, "NULL argument");
    if (ctx->ms.batch != ctx->B || ctx->B < 1) return fail(QOCX_ERR_STATE, "qocx_opt_begin has not run for this batch");
    HIP_TRY(hipSetDevice(ctx->device));
    // after the clip |u_k| <= max_norms[k]: the squaring capacity follows from that bound
    // (ensemble: |s_mk u_k| <= max_norms[k] max_m |s_mk| on the K_r seed channels, |delta_mj| beyond;
    // a sweep keeps max_b |s_bk| and max_b |delta_bj| in the same two vectors)
    const bool ens = ctx->seeds.M > 0;
    const SeedView v = schroedinger_seeds(ctx);
    const int Ks = v.channels;
    // (complex controls: max_norms [Ks / 2] bound the moduli, hence both channels of a control)
    std::vector<double> channel_norms((size_t)Ks);
    for (int k = 0; k < Ks; ++k) channel_norms[k] = max_norms[ctx->ms.complex_controls ? k / 2 : k];
    double bound = ctx->h0_norm_max;
    for (int k = 0; k < Ks; ++k) {
        if (!(channel_norms[k] >= 0)) return fail(QOCX_ERR_ARG, "max_norms must be non-negative");
        bound += (ens ? channel_norms[k] * ctx->ens_scale_max[k] : channel_norms[k]) * ctx->g_norm_max[k];
    }
    for (int j = 0; ens && j < ctx->seeds.J; ++j) bound += ctx->ens_offset_max[j] * ctx->g_norm_max[Ks + j];
    // (quadratic terms: ||Q_q||_1 max_norms_k max_norms_l, with an ensemble times its members' largest
    // scales as in qocx_upload_controls)
    bound += quad_bound(ctx, channel_norms.data());
    bound = magnus_norm_bound(ctx->nodes, bound * fabs(ctx->dt));
    if (!(bound < 1e300)) return fail(QOCX_ERR_ARG, "non-finite bound");
    // (the plain M2 problem: the same bound with the spectral norms, for the Taylor buffers of the
    // matrix-free route - qocx_upload_controls; M4 and quadratic terms, knob "action_eff": none, the
    // buffers follow the 1-norm bound above)
    double bound2 = 1e300;
    if (!ens && ctx->nodes == 1 && ctx->eff.quad_count() == 0 && (int)ctx->g_norm2_max.size() >= Ks) {
        bound2 = ctx->h0_norm2_max;
        for (int k = 0; k < Ks; ++k) bound2 += channel_norms[k] * ctx->g_norm2_max[k];
        bound2 *= fabs(ctx->dt);
        if (!(bound2 < 1e300)) bound2 = 1e300;
    }
    if (int rc = commit_step_bound(ctx, bound, true, "bound needs", bound2)) return rc;
    // (the Lindblad path checks the second of these grid limits in qocx_lindblad_upload_controls and has
    // no check of the first: to be revisited)
    if ((v.total() + 255) / 256 > 0x7fffffffu || v.per_seed() > 65535u * 256u)
        return fail(QOCX_ERR_ARG, "control arrays too large for the optimizer kernels' grids");
    if (ctx->seeds.dur.set) {
        // a duration search: tau clipped in place to its box and the sweep's tables rewritten from it,
        // before the next evaluation expands the seeds (ens_scale_max / ens_offset_max above are those
        // of tau_max: the bound holds wherever the step has taken tau)
        qocx::launch_duration_tables(duration_args(ctx->seeds, nullptr, nullptr), ctx->stream);
        ctx->seeds.dur.mirror_stale = true;
    }
    if (int rc = multistart_clip(ctx, ctx->ms, v, max_norms)) return rc;
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(ctx->stream));  // max_norms is the caller's memory
    ctx->have_results = false;
    ctx->ens_stale = ens;  // (the next evaluation expands the clipped seed controls)
    return 0;
}

int qocx_opt_step(qocx_ctx* ctx, int32_t kind, const uint8_t* improved, const uint8_t* update,
                  double learning_rate, double beta_1, double beta_2, double epsilon, double corr_1,
                  double corr_2, int32_t apply_clip_grads, double clip_grads) {
    if (!ctx || !improved || !update) return fail(QOCX_ERR_ARG, "NULL argument");
    if (kind != 0 && kind != 1) return fail(QOCX_ERR_ARG, "kind must be 0 (SGD) or 1 (Adam)");
    if (ctx->ms.batch != ctx->B || ctx->B < 1) return fail(QOCX_ERR_STATE, "qocx_opt_begin has not run for this batch");
    if (!ctx->have_results || !ctx->have_grads) return fail(QOCX_ERR_STATE, "no gradients to step with");
    HIP_TRY(hipSetDevice(ctx->device));
    const StepRule rule{kind, learning_rate, beta_1, beta_2, epsilon, corr_1, corr_2, apply_clip_grads, clip_grads};
    qocx::DurationStepArgs durations;
    if (ctx->seeds.dur.set)
        if (int rc = durations_rule(ctx->seeds.dur, durations)) return rc;
    if (int rc = multistart_step(ctx, ctx->ms, schroedinger_seeds(ctx), rule, improved, update,
                                 ctx->seeds.dur.set ? &durations : nullptr))
        return rc;
    ctx->seeds.dur.have_grad = false;
    ctx->have_results = false;  // the resident controls are no longer those of the last evaluation
    ctx->ens_stale = ctx->seeds.M > 0;
    return 0;
}

int qocx_opt_lbfgs_begin(qocx_ctx* ctx, int32_t history) {
    if (!ctx) return fail(QOCX_ERR_ARG, "ctx is NULL");
    if (ctx->ms.batch != ctx->B || ctx->B < 1) return fail(QOCX_ERR_STATE, "qocx_opt_begin has not run for this batch");
    if (ctx->seeds.dur.set)
        return fail(QOCX_ERR_STATE, "a duration search (qocx_sweep_set_durations) steps with Adam or SGD: the "
                                    "resident L-BFGS vectors do not hold tau");
    HIP_TRY(hipSetDevice(ctx->device));
    return multistart_lbfgs_begin(ctx, ctx->ms, schroedinger_seeds(ctx), history);
}

int qocx_opt_lbfgs_step(qocx_ctx* ctx, const uint8_t* improved, const uint8_t* update, double first_step,
                        double armijo, double shrink, int32_t max_backtracks, uint8_t* finished_out) {
    if (!ctx || !improved || !update || !finished_out) return fail(QOCX_ERR_ARG, "NULL argument");
    if (ctx->ms.batch != ctx->B || ctx->B < 1) return fail(QOCX_ERR_STATE, "qocx_opt_begin has not run for this batch");
    if (ctx->ms.lbfgs_history < 1) return fail(QOCX_ERR_STATE, "qocx_opt_lbfgs_begin has not run for this batch");
    if (!ctx->have_results || !ctx->have_grads) return fail(QOCX_ERR_STATE, "no gradients to step with");
    HIP_TRY(hipSetDevice(ctx->device));
    const LbfgsRule rule{first_step, armijo, shrink, max_backtracks};
    if (int rc = multistart_lbfgs_step(ctx, ctx->ms, schroedinger_seeds(ctx), rule, improved, update, finished_out))
        return rc;
    ctx->have_results = false;  // the resident controls are no longer those of the last evaluation
    ctx->ens_stale = ctx->seeds.M > 0;
    return 0;
}

int qocx_opt_download_best(qocx_ctx* ctx, double* controls_out, double* final_out) {
    if (!ctx) return fail(QOCX_ERR_ARG, "ctx is NULL");
    if (ctx->ms.batch != ctx->B || ctx->B < 1) return fail(QOCX_ERR_STATE, "qocx_opt_begin has not run for this batch");
    HIP_TRY(hipSetDevice(ctx->device));
    std::vector<double2> fin;
    if (int rc = multistart_download_best(ctx, ctx->ms, schroedinger_seeds(ctx), controls_out,
                                          final_out ? &fin : nullptr))
        return rc;
    const int np = ctx->np, n = ctx->n;
    if (final_out)
        for (size_t v = 0; v < (size_t)ctx->B * ctx->S; ++v)
            for (int i = 0; i < n; ++i) {
                final_out[2 * (v * n + i)] = fin[v * np + i].x;
                final_out[2 * (v * n + i) + 1] = fin[v * np + i].y;
            }
    return 0;
}

int qocx_opt_download_best_durations(qocx_ctx* ctx, double* tau_out) {
    if (!ctx || !tau_out) return fail(QOCX_ERR_ARG, "NULL argument");
    if (ctx->ms.batch != ctx->B || ctx->B < 1) return fail(QOCX_ERR_STATE, "qocx_opt_begin has not run for this batch");
    return durations_download_best(ctx, ctx->seeds.dur, (size_t)ctx->seeds.swp_B, "qocx_sweep_set_durations", tau_out);
}

// ---- the Lindblad path: the seeds of qocx_lindblad_upload_controls ----------------------------------

int qocx_lindblad_opt_begin(qocx_ctx* ctx) { return lindblad_opt_begin(ctx, false); }

int qocx_lindblad_opt_begin_complex(qocx_ctx* ctx) { return lindblad_opt_begin(ctx, true); }

int qocx_lindblad_opt_begin_basis(qocx_ctx* ctx, int32_t complex_controls, int32_t p, const double* matrix,
                                  const double* coefficients) {
    BasisStart basis;
    if (int rc = basis_start(p, matrix, coefficients, basis)) return rc;
    return lindblad_opt_begin(ctx, complex_controls != 0, basis);
}

int qocx_lindblad_opt_download_best_params(qocx_ctx* ctx, double* params_out) {
    if (!ctx) return fail(QOCX_ERR_ARG, "ctx is NULL");
    auto& lb = ctx->lb;
    if (lb.ms.batch != lb.res_B || lb.res_B < 1)
        return fail(QOCX_ERR_STATE, "qocx_lindblad_opt_begin has not run for this batch");
    HIP_TRY(hipSetDevice(ctx->device));
    return multistart_download_best_params(ctx, lb.ms, lindblad_seeds(ctx), params_out);
}

int qocx_lindblad_opt_clip(qocx_ctx* ctx, const double* max_norms) {
    if (!ctx || !max_norms) return fail(QOCX_ERR_ARG, "NULL argument");
    auto& lb = ctx->lb;
    if (lb.ms.batch != lb.res_B || lb.res_B < 1)
        return fail(QOCX_ERR_STATE, "qocx_lindblad_opt_begin has not run for this batch");
    // (with an ensemble the seeds' K_r channels: the next evaluation expands the clipped seeds anew)
    const int B = lb.res_B, K = lb.seed_channels();
    const int Kn = lb.ms.complex_controls ? K / 2 : K;  // (complex controls: one modulus bound per control)
    for (int k = 0; k < Kn; ++k)
        if (!(max_norms[k] >= 0)) return fail(QOCX_ERR_ARG, "max_norms must be non-negative");
    HIP_TRY(hipSetDevice(ctx->device));
    if (lb.seeds.dur.set) {
        // a duration search: tau clipped in place to its box, the sweep's tables and the seeds' generator
        // tables rewritten from it before the next evaluation expands the seeds; tau comes back to the
        // host in the synchronisation below, for the mirrors the sub-division decision reads
        lindblad_duration_tables(ctx);
        lb.seeds.dur.mirror_stale = true;
        if (int rc = lindblad_duration_fetch(ctx)) return rc;
    }
    if (int rc = multistart_clip(ctx, lb.ms, lindblad_seeds(ctx), max_norms)) return rc;
    // the maxima of the clipped controls decide the next evaluation's sub-divisions: they come back
    // with the synchronisation the clip needs anyway (none on a fixed grid)
    const bool maxima = lb.fixed_ksub == 0;
    if (maxima) {
        if (lb.umax.ensure((size_t)B * K)) return QOCX_ERR_HIP;
        lb.umax_host.resize((size_t)B * K);
        qocx::launch_control_maxima(lb.res_controls.p, B, lb.nc, K, lb.umax.p, ctx->stream);
        HIP_TRY(hipMemcpyAsync(lb.umax_host.data(), lb.umax.p, (size_t)B * K * sizeof(double),
                               hipMemcpyDeviceToHost, ctx->stream));
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(ctx->stream));  // max_norms is the caller's memory
    lb.resident_controls_moved(maxima);
    if (lb.seeds.dur.set) lindblad_duration_mirror(ctx);
    return 0;
}

int qocx_lindblad_opt_step(qocx_ctx* ctx, int32_t kind, const uint8_t* improved, const uint8_t* update,
                           double learning_rate, double beta_1, double beta_2, double epsilon,
                           double corr_1, double corr_2, int32_t apply_clip_grads, double clip_grads) {
    if (!ctx || !improved || !update) return fail(QOCX_ERR_ARG, "NULL argument");
    if (kind != 0 && kind != 1) return fail(QOCX_ERR_ARG, "kind must be 0 (SGD) or 1 (Adam)");
    auto& lb = ctx->lb;
    if (lb.ms.batch != lb.res_B || lb.res_B < 1)
        return fail(QOCX_ERR_STATE, "qocx_lindblad_opt_begin has not run for this batch");
    if (!lb.res_have_results || !lb.res_have_grads) return fail(QOCX_ERR_STATE, "no gradients to step with");
    HIP_TRY(hipSetDevice(ctx->device));
    const StepRule rule{kind, learning_rate, beta_1, beta_2, epsilon, corr_1, corr_2, apply_clip_grads, clip_grads};
    qocx::DurationStepArgs durations;
    if (lb.seeds.dur.set)
        if (int rc = durations_rule(lb.seeds.dur, durations)) return rc;
    if (int rc = multistart_step(ctx, lb.ms, lindblad_seeds(ctx), rule, improved, update,
                                 lb.seeds.dur.set ? &durations : nullptr))
        return rc;
    lb.seeds.dur.have_grad = false;
    // (tau has moved: the tables are rewritten by the clip, or before the next evaluation)
    lb.seeds.dur.mirror_stale = lb.seeds.dur.set;
    lb.resident_controls_moved(false);  // ... and are no longer those of the last evaluation
    return 0;
}

int qocx_lindblad_opt_lbfgs_begin(qocx_ctx* ctx, int32_t history) {
    if (!ctx) return fail(QOCX_ERR_ARG, "ctx is NULL");
    auto& lb = ctx->lb;
    if (lb.ms.batch != lb.res_B || lb.res_B < 1)
        return fail(QOCX_ERR_STATE, "qocx_lindblad_opt_begin has not run for this batch");
    if (lb.seeds.dur.set)
        return fail(QOCX_ERR_STATE, "a duration search (qocx_lindblad_sweep_set_durations) steps with Adam or SGD: "
                                    "the resident L-BFGS vectors do not hold tau");
    HIP_TRY(hipSetDevice(ctx->device));
    return multistart_lbfgs_begin(ctx, lb.ms, lindblad_seeds(ctx), history);
}

int qocx_lindblad_opt_lbfgs_step(qocx_ctx* ctx, const uint8_t* improved, const uint8_t* update,
                                 double first_step, double armijo, double shrink, int32_t max_backtracks,
                                 uint8_t* finished_out) {
    if (!ctx || !improved || !update || !finished_out) return fail(QOCX_ERR_ARG, "NULL argument");
    auto& lb = ctx->lb;
    if (lb.ms.batch != lb.res_B || lb.res_B < 1)
        return fail(QOCX_ERR_STATE, "qocx_lindblad_opt_begin has not run for this batch");
    if (lb.ms.lbfgs_history < 1)
        return fail(QOCX_ERR_STATE, "qocx_lindblad_opt_lbfgs_begin has not run for this batch");
    if (!lb.res_have_results || !lb.res_have_grads) return fail(QOCX_ERR_STATE, "no gradients to step with");
    HIP_TRY(hipSetDevice(ctx->device));
    const LbfgsRule rule{first_step, armijo, shrink, max_backtracks};
    if (int rc = multistart_lbfgs_step(ctx, lb.ms, lindblad_seeds(ctx), rule, improved, update, finished_out))
        return rc;
    lb.resident_controls_moved(false);  // ... and are no longer those of the last evaluation
    return 0;
}

int qocx_lindblad_opt_download_best(qocx_ctx* ctx, double* controls_out, double* final_out) {
    if (!ctx) return fail(QOCX_ERR_ARG, "ctx is NULL");
    auto& lb = ctx->lb;
    if (lb.ms.batch != lb.res_B || lb.res_B < 1)
        return fail(QOCX_ERR_STATE, "qocx_lindblad_opt_begin has not run for this batch");
    HIP_TRY(hipSetDevice(ctx->device));
    const int B = lb.res_B, S = lb.S * (int)lb.seed_items(), n = lb.n;  // (ensemble: every item's densities)
    const size_t md = dump_elems(n);
    std::vector<double2> fin;
    if (int rc = multistart_download_best(ctx, lb.ms, lindblad_seeds(ctx), controls_out,
                                          final_out ? &fin : nullptr))
        return rc;
    if (final_out)
        for (size_t v = 0; v < (size_t)B * S; ++v) from_c_dump(fin.data() + v * md, n, final_out + v * n * n * 2);
    return 0;
}

int qocx_lindblad_opt_download_best_durations(qocx_ctx* ctx, double* tau_out) {
    if (!ctx || !tau_out) return fail(QOCX_ERR_ARG, "NULL argument");
    auto& lb = ctx->lb;
    if (lb.ms.batch != lb.res_B || lb.res_B < 1)
        return fail(QOCX_ERR_STATE, "qocx_lindblad_opt_begin has not run for this batch");
    return durations_download_best(ctx, lb.seeds.dur, (size_t)lb.seeds.swp_B, "qocx_lindblad_sweep_set_durations", tau_out);
}

// ---- costs of the controls alone; complex controls in the resident drivers -------------------------

static ControlCosts* control_costs_of(qocx_ctx* ctx, int32_t path, int& nc, int& Kr) {
    if (path == QOCX_PATH_SCHROEDINGER && ctx->has_problem) {
        nc = ctx->nc;
        Kr = ctx->seeds.M > 0 ? ctx->seeds.Kr : ctx->K;
        return &ctx->control_costs;
    }
    if (path == QOCX_PATH_LINDBLAD && ctx->lb.has_problem) {
        nc = ctx->lb.nc;
        Kr = ctx->lb.seed_channels();
        return &ctx->lb.control_costs;
    }
    return nullptr;
}

int qocx_set_control_costs(qocx_ctx* ctx, int32_t path, int32_t complex_controls, int32_t count,
                           const qocx_control_cost_desc* descs) {
    if (!ctx) return fail(QOCX_ERR_ARG, "ctx is NULL");
    if (path != QOCX_PATH_SCHROEDINGER && path != QOCX_PATH_LINDBLAD) return fail(QOCX_ERR_ARG, "unknown path");
    int nc = 0, Kr = 0;
    ControlCosts* ccp = control_costs_of(ctx, path, nc, Kr);
    if (!ccp) return fail(QOCX_ERR_STATE, "no problem set on this path");
    ControlCosts& cc = *ccp;
    cc.clear();
    if (count <= 0) return 0;
    if (!descs) return fail(QOCX_ERR_ARG, "descs is NULL");
    const int cplx = complex_controls ? 1 : 0;
    if (Kr < 1 || nc < 2) return fail(QOCX_ERR_ARG, "control costs need a problem with controls");
    if (Kr > 128) return fail(QOCX_ERR_ARG, "control costs take up to 128 control channels");
    if (cplx && Kr % 2) return fail(QOCX_ERR_ARG, "complex controls need an even number of channels");
    const int K = Kr >> cplx;
    HIP_TRY(hipSetDevice(ctx->device));
    std::vector<double> arrays;
    std::vector<int> ints;
    std::vector<qocx::CtrlCostDev> dev;
    std::vector<size_t> offsets;  // of max_norms | weights in `arrays`, per elementwise descriptor
    bool variation = false;
    for (int d = 0; d < count; ++d) {
        const qocx_control_cost_desc& c = descs[d];
        if (!std::isfinite(c.multiplier)) return fail(QOCX_ERR_ARG, "non-finite cost multiplier");
        for (int k = 0; k < K; ++k)
            if ((c.max_norms && !std::isfinite(c.max_norms[k])) || (c.weights && !std::isfinite(c.weights[k])))
                return fail(QOCX_ERR_ARG, "non-finite max_norms / weights");
        if (c.kind == QOCX_CONTROL_BANDWIDTH_MAX) {
            if (!c.bins || !c.bin_ptr || c.bin_ptr[0] != 0) return fail(QOCX_ERR_ARG, "bandwidth cost without bins");
            ControlCosts::Bandwidth bw;
            bw.multiplier = c.multiplier;
            bw.pmax = 0;
            for (int k = 0; k < K; ++k) {
                const int np = c.bin_ptr[k + 1] - c.bin_ptr[k];
                if (np < 1) return fail(QOCX_ERR_ARG, "a control without penalised DFT bins (empty P_k)");
                for (int i = c.bin_ptr[k]; i < c.bin_ptr[k + 1]; ++i)
                    if (c.bins[i] < 0 || c.bins[i] >= nc || (i > c.bin_ptr[k] && c.bins[i] <= c.bins[i - 1]))
                        return fail(QOCX_ERR_ARG, "DFT bins must be ascending and in 0..Nc-1");
                bw.pmax = std::max(bw.pmax, np);
            }
            bw.bins = ints.size();
            ints.insert(ints.end(), c.bins, c.bins + c.bin_ptr[K]);
            bw.bin_ptr = ints.size();
            ints.insert(ints.end(), c.bin_ptr, c.bin_ptr + K + 1);
            cc.bandwidth.push_back(bw);
            continue;
        }
        if (c.kind != QOCX_CONTROL_NORM && c.kind != QOCX_CONTROL_VARIATION && c.kind != QOCX_CONTROL_AREA) {
            cc.clear();
            return fail(QOCX_ERR_ARG, "unknown control cost kind");
        }
        if (c.kind == QOCX_CONTROL_VARIATION && (c.order < 1 || c.order >= nc)) {
            cc.clear();
            return fail(QOCX_ERR_ARG, "ControlVariation needs 1 <= order < control_eval_count");
        }
        if (c.kind == QOCX_CONTROL_AREA && !c.max_norms) {
            cc.clear();
            return fail(QOCX_ERR_ARG, "ControlArea needs max_norms");
        }
        variation = variation || c.kind == QOCX_CONTROL_VARIATION;
        qocx::CtrlCostDev e;
        e.kind = c.kind; e.order = c.order; e.multiplier = c.multiplier;
        e.max_norms = e.weights = nullptr;
        offsets.push_back(arrays.size());
        for (int k = 0; k < K; ++k) arrays.push_back(c.max_norms ? c.max_norms[k] : 1.0);
        for (int k = 0; k < K; ++k) arrays.push_back(c.weights ? c.weights[k] : 1.0);
        dev.push_back(e);
    }
    if (cc.arrays.upload(arrays, ctx->stream) || cc.ints.upload(ints, ctx->stream)) {
        cc.clear();
        return QOCX_ERR_HIP;
    }
    for (size_t d = 0; d < dev.size(); ++d) {
        dev[d].max_norms = cc.arrays.p + offsets[d];
        dev[d].weights = cc.arrays.p + offsets[d] + K;
    }
    if (!cc.bandwidth.empty()) {  // exp(-2 pi i m / Nc), m = 0 .. Nc-1, rounded from extended precision
        std::vector<double2> tw((size_t)nc);
        const long double two_pi = 6.283185307179586476925286766559005768L;
        for (int m = 0; m < nc; ++m) {
            const long double th = two_pi * (long double)m / (long double)nc;
            tw[m] = make_double2((double)cosl(th), (double)-sinl(th));
        }
        if (cc.twiddle.upload(tw, ctx->stream)) {
            cc.clear();
            return QOCX_ERR_HIP;
        }
    }
    if (cc.descs.upload(dev, ctx->stream)) {
        cc.clear();
        return QOCX_ERR_HIP;
    }
    cc.count = count;
    cc.cplx = cplx; cc.K = K; cc.Kr = Kr; cc.nc = nc;
    cc.elementwise = (int)dev.size();
    cc.variation = variation;
    return 0;
}

int qocx_eval_control_costs(qocx_ctx* ctx, int32_t path, int32_t batch, const double* controls,
                            double* cost_out, double* grad_out) {
    if (!ctx || !controls || !cost_out) return fail(QOCX_ERR_ARG, "NULL argument");
    if (batch < 1) return fail(QOCX_ERR_ARG, "batch must be >= 1");
    int nc = 0, Kr = 0;
    ControlCosts* cc = control_costs_of(ctx, path, nc, Kr);
    if (!cc || cc->count == 0) return fail(QOCX_ERR_STATE, "no control costs set on this path");
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t total = (size_t)batch * nc * Kr;
    if (cc->stage.ensure(total)) return QOCX_ERR_HIP;
    HIP_TRY(hipMemcpyAsync(cc->stage.p, controls, total * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    if (int rc = run_control_costs(ctx, *cc, batch, nc, Kr, cc->stage.p, grad_out != nullptr)) return rc;
    HIP_TRY(hipMemcpyAsync(cost_out, cc->cost.p, (size_t)batch * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (grad_out)
        HIP_TRY(hipMemcpyAsync(grad_out, cc->grad.p, total * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return 0;
}

int qocx_control_basis_apply(qocx_ctx* ctx, int32_t transpose, int32_t batch, int32_t nc, int32_t p,
                             int32_t channels, const double* matrix, const double* in, double* out) {
    if (!ctx || !matrix || !in || !out) return fail(QOCX_ERR_ARG, "NULL argument");
    if (batch < 1 || nc < 1 || p < 1 || channels < 1) return fail(QOCX_ERR_ARG, "batch, nc, p and channels must be >= 1");
    const size_t entries = (size_t)nc * p;
    const size_t wide = (size_t)batch * nc * channels, narrow = (size_t)batch * p * channels;
    if ((wide + 255) / 256 > 0x7fffffffu || (narrow + 255) / 256 > 0x7fffffffu)
        return fail(QOCX_ERR_ARG, "arrays too large for the basis kernels' grids");
    HIP_TRY(hipSetDevice(ctx->device));
    // (each kernel reads the matrix in the orientation in which its threads' index is contiguous)
    std::vector<double> mat(matrix, matrix + entries);
    if (!transpose)
        for (int j = 0; j < nc; ++j)
            for (int q = 0; q < p; ++q) mat[(size_t)q * nc + j] = matrix[(size_t)j * p + q];
    const size_t in_count = transpose ? wide : narrow, out_count = transpose ? narrow : wide;
    DevBuf<double> dmat, din, dout;
    if (dmat.upload(mat, ctx->stream) || din.ensure(in_count) || dout.ensure(out_count)) return QOCX_ERR_HIP;
    HIP_TRY(hipMemcpyAsync(din.p, in, in_count * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    if (transpose)
        qocx::launch_basis_project(dmat.p, din.p, dout.p, batch, nc, p, channels, ctx->stream);
    else
        qocx::launch_basis_expand(dmat.p, din.p, dout.p, batch, nc, p, channels, ctx->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, dout.p, out_count * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return 0;
}

int qocx_host_clip_controls(double* controls, int64_t batch, int64_t nc, int32_t k,
                            const double* max_norms) {
    if (!controls || !max_norms || batch < 0 || nc < 0 || k < 0) return fail(QOCX_ERR_ARG, "bad argument");
    host_parallel_rows(batch, [=](int64_t lo, int64_t hi) {
        for (int64_t b = lo; b < hi; ++b) {
            double* row = controls + (size_t)b * nc * k;
            for (int64_t j = 0; j < nc; ++j)
                for (int32_t c = 0; c < k; ++c) {
                    const double v = row[j * k + c], mod = fabs(v);
                    if (max_norms[c] < mod) row[j * k + c] = (v / mod) * max_norms[c];
                }
        }
    });
    return 0;
}

int qocx_host_optimizer_update(int32_t kind, double* params, const double* grads, double* moment,
                               double* square_moment, int64_t p, const int64_t* rows,
                               int64_t row_count, double learning_rate, double beta_1,
                               double beta_2, double epsilon, double corr_1, double corr_2,
                               int32_t apply_clip_grads, double clip_grads) {
    if (!params || !grads || !rows || p < 0 || row_count < 0) return fail(QOCX_ERR_ARG, "bad argument");
    if (kind != 0 && (!moment || !square_moment)) return fail(QOCX_ERR_ARG, "moments missing");
    const double one_m_b1 = 1 - beta_1, one_m_b2 = 1 - beta_2;
    host_parallel_rows(row_count, [=](int64_t lo, int64_t hi) {
// every product and sum is rounded on its own, as NumPy's array operations are
#pragma clang fp contract(off)
        for (int64_t r = lo; r < hi; ++r) {
            const size_t off = (size_t)rows[r] * (size_t)p;
            double* x = params + off;
            const double* g = grads + off;
            if (kind == 0) {
                for (int64_t i = 0; i < p; ++i) {
                    const double s = learning_rate * g[i];
                    x[i] = x[i] - s;
                }
                continue;
            }
            adam_row(x, g, moment + off, square_moment + off, p, learning_rate, beta_1, beta_2,
                     one_m_b1, one_m_b2, epsilon, corr_1, corr_2, apply_clip_grads, clip_grads);
        }
    });
    return 0;
}

}  // extern "C"
