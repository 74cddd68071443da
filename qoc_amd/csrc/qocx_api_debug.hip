// qocx_api_debug.hip - the debug and self-test entry points of the C ABI (include/qocx.h) and the
// counters the tests and tools read back.
#include "qocx_host.h"
#include "qocx_action_route.h"

namespace {

// column-major image -> row-major n x n complex; row_map (optional) gives the image row of each
// output row (the LU factors are stored in original row order: row_map = perm)
void from_image(const double2* img, int n, int np, const int* row_map, double* out) {
    for (int row = 0; row < n; ++row)
        for (int col = 0; col < n; ++col) {
            const int src = row_map ? row_map[row] : row;
            out[2 * ((size_t)row * n + col)] = img[(size_t)col * np + src].x;
            out[2 * ((size_t)row * n + col) + 1] = img[(size_t)col * np + src].y;
        }
}

}  // namespace

extern "C" {

// ---- debug -------------------------------------------------------------------------------

int qocx_debug_pade_factor(qocx_ctx* ctx, int32_t count, int32_t n, const double* a, double* q_out,
                           double* lu_out, int32_t* perm_out, double* dinv_out, int32_t* s_out) {
    if (!ctx || !a || count < 1) return fail(QOCX_ERR_ARG, "bad argument");
    if (n < 1 || n > 64) return fail(QOCX_ERR_ARG, "n must be in 1..64");
    HIP_TRY(hipSetDevice(ctx->device));
    const int nb = (n <= 16) ? 1 : (n <= 32 ? 2 : 4), np = 16 * nb, mat = np * np;
    DevBuf<double2> a_d, q_d, lu_d, dinv_d;
    DevBuf<int> perm_d, iperm_d, s_d;
    int rc = a_d.ensure((size_t)count * n * n) | q_d.ensure((size_t)count * mat) |
             lu_d.ensure((size_t)count * mat) | dinv_d.ensure((size_t)count * np) |
             perm_d.ensure((size_t)count * np) | iperm_d.ensure((size_t)count * np) |
             s_d.ensure(count);
    if (rc) return QOCX_ERR_HIP;
    HIP_TRY(hipMemcpy(a_d.p, a, (size_t)count * n * n * 16, hipMemcpyHostToDevice));
    HIP_TRY(hipMemsetAsync(ctx->status.p, 0, sizeof(int), ctx->stream));
    qocx::FactorArgs fa;
    memset(&fa, 0, sizeof(fa));
    fa.q_img = q_d.p; fa.lu_img = lu_d.p; fa.s_arr = s_d.p; fa.status = ctx->status.p;
    fa.nsteps = count; fa.step0 = 0; fa.seg_len = count; fa.n = n;
    fa.pade_policy = (int)ctx->knob("pade_order", 0);
    const bool inverse = nb <= 2 && ctx->knob("lu_inverse", 0) != 0;  // P^-1 instead of the factors
    const bool fused_lu = nb == 2 && !inverse && qocx::diag_getenv("QOCX_PQ1") == nullptr && ctx->knob("fuse_lu", 1) != 0;
    fa.fuse_lu = fused_lu ? 1 : 0;  // the same kernels the evaluation runs
    fa.lu_mfma = (int)ctx->knob("lu_mfma", 1);
    fa.lu_dpp = (int)ctx->knob("lu_dpp", 1);
    if (ctx->lu_fallbacks.ensure(1)) return QOCX_ERR_HIP;
    HIP_TRY(hipMemsetAsync(ctx->lu_fallbacks.p, 0, sizeof(int), ctx->stream));
    fa.lu_fallbacks = ctx->lu_fallbacks.p;
    fa.dinv = dinv_d.p; fa.perm = perm_d.p; fa.iperm = iperm_d.p;
    qocx::LuArgs la;
    la.lu_img = lu_d.p; la.dinv = dinv_d.p; la.perm = perm_d.p; la.iperm = iperm_d.p;
    la.status = ctx->status.p;
    la.nsteps = count; la.step0 = 0; la.seg_len = count; la.n = n;
    la.inverse = inverse ? 1 : 0;
    {   // the four-to-a-wave inverse of n <= 16 (qocx_lu5.h) where every matrix handed in qualifies
        double theta = 0.0;
        for (int c = 0; c < count; ++c) theta = std::max(theta, one_norm(a + (size_t)c * n * n * 2, n));
        la.all_dominant = (pade_eps_max(theta) <= 0.40 && ctx->knob("lu_dpp", 1) != 0) ? 1 : 0;
    }
    la.fallbacks = ctx->lu_fallbacks.p;
    DevBuf<int> redo_d;
    if (nb == 4 && ctx->knob("lu_mfma", 1) != 0) {
        if (redo_d.ensure((size_t)count)) return QOCX_ERR_HIP;
        la.redo = redo_d.p;
    }
    qocx::launch_pq_explicit(nb, a_d.p, n, fa, count, ctx->stream);
    if (!fused_lu) qocx::launch_lu(nb, la, (size_t)count, ctx->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    std::vector<double2> img((size_t)count * mat), dv((size_t)count * np);
    std::vector<int> pm((size_t)count * np), sv(count);
    HIP_TRY(hipMemcpy(pm.data(), perm_d.p, pm.size() * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(img.data(), q_d.p, img.size() * 16, hipMemcpyDeviceToHost));
    if (q_out)
        for (int m = 0; m < count; ++m)
            from_image(img.data() + (size_t)m * mat, n, np, nullptr, q_out + (size_t)m * n * n * 2);
    HIP_TRY(hipMemcpy(img.data(), lu_d.p, img.size() * 16, hipMemcpyDeviceToHost));
    if (lu_out && inverse) {  // the image is P^-1, column-major
        for (int m = 0; m < count; ++m)
            from_image(img.data() + (size_t)m * mat, n, np, nullptr, lu_out + (size_t)m * n * n * 2);
        if (s_out) {
            HIP_TRY(hipMemcpy(sv.data(), s_d.p, sv.size() * 4, hipMemcpyDeviceToHost));
            memcpy(s_out, sv.data(), count * sizeof(int));
        }
        int st_inv = 0;
        HIP_TRY(hipMemcpy(&st_inv, ctx->status.p, sizeof(int), hipMemcpyDeviceToHost));
        if (st_inv & 1) return fail(QOCX_ERR_SINGULAR, "Singular matrix");
        return 0;
    }
    if (lu_out)
        for (int m = 0; m < count; ++m) {
            std::vector<int> rows(pm.begin() + (size_t)m * np, pm.begin() + (size_t)(m + 1) * np);
            for (auto& r : rows) r = std::min(std::max(r, 0), np - 1);
            from_image(img.data() + (size_t)m * mat, n, np, rows.data(), lu_out + (size_t)m * n * n * 2);
        }
    HIP_TRY(hipMemcpy(dv.data(), dinv_d.p, dv.size() * 16, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(sv.data(), s_d.p, sv.size() * 4, hipMemcpyDeviceToHost));
    if (lu_out)  // the device stores U' = D^-1 U above the diagonal: undo the row scaling
        for (int m = 0; m < count; ++m)
            for (int r = 0; r < n; ++r) {
                const double2 d = dv[(size_t)m * np + r];
                const double den = d.x * d.x + d.y * d.y;
                const double ur = d.x / den, ui = -d.y / den;  // U_rr = 1 / dinv_r
                for (int c = r + 1; c < n; ++c) {
                    double* e = lu_out + 2 * (((size_t)m * n + r) * n + c);
                    const double xr = e[0], xi = e[1];
                    e[0] = xr * ur - xi * ui;
                    e[1] = xr * ui + xi * ur;
                }
            }
    for (int m = 0; m < count; ++m)
        for (int i = 0; i < n; ++i) {
            if (perm_out) perm_out[(size_t)m * n + i] = pm[(size_t)m * np + i];
            if (dinv_out) {
                dinv_out[2 * ((size_t)m * n + i)] = dv[(size_t)m * np + i].x;
                dinv_out[2 * ((size_t)m * n + i) + 1] = dv[(size_t)m * np + i].y;
            }
        }
    if (s_out) memcpy(s_out, sv.data(), count * sizeof(int));
    int status = 0;
    HIP_TRY(hipMemcpy(&status, ctx->status.p, sizeof(int), hipMemcpyDeviceToHost));
    if (status & 1) return fail(QOCX_ERR_SINGULAR, "Singular matrix");
    return 0;
}

int qocx_debug_mfma_peak(qocx_ctx* ctx, int32_t waves_per_simd, int32_t iters, double* tflops) {
    if (!ctx || !tflops || waves_per_simd < 1 || iters < 1) return fail(QOCX_ERR_ARG, "bad argument");
    HIP_TRY(hipSetDevice(ctx->device));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, ctx->device));
    const int blocks = prop.multiProcessorCount * 4 * waves_per_simd;
    DevBuf<double> out;
    if (out.ensure(8)) return QOCX_ERR_HIP;
    hipEvent_t e0, e1;
    HIP_TRY(hipEventCreate(&e0));
    HIP_TRY(hipEventCreate(&e1));
    const int peak_mode = (int)ctx->knob("peak_mode", 0);  // (diagnostic build: pipe_mix_kernel)
    (void)peak_mode;
#ifdef QOCX_DIAG
    if (peak_mode > 0) {
        qocx::launch_pipe_mix(out.p, blocks, 64, peak_mode, ctx->stream);
        HIP_TRY(hipEventRecord(e0, ctx->stream));
        qocx::launch_pipe_mix(out.p, blocks, iters, peak_mode, ctx->stream);
        HIP_TRY(hipEventRecord(e1, ctx->stream));
    } else
#endif
    {
    qocx::launch_mfma_peak(out.p, blocks, 64, ctx->stream);  // warm-up
    HIP_TRY(hipEventRecord(e0, ctx->stream));
    qocx::launch_mfma_peak(out.p, blocks, iters, ctx->stream);
    HIP_TRY(hipEventRecord(e1, ctx->stream));
    }
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    // one v_mfma_f64_16x16x4_f64 = 16*16*4 multiply-adds = 2048 flop per wave
    *tflops = (double)blocks * iters * 8.0 * 2048.0 / (ms * 1e-3) / 1e12;
    return 0;
}

int qocx_debug_selftest(qocx_ctx* ctx, int32_t* failures, char* report, int32_t report_len) {
    if (!ctx || !failures) return fail(QOCX_ERR_ARG, "bad argument");
    HIP_TRY(hipSetDevice(ctx->device));
    DevBuf<double> out;
    if (out.ensure(512)) return QOCX_ERR_HIP;
    qocx::launch_selftest(out.p, ctx->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    std::vector<double> h(512);
    HIP_TRY(hipMemcpy(h.data(), out.p, 512 * sizeof(double), hipMemcpyDeviceToHost));
    int bad = 0;
    std::string rep;
    double vmax = 0, vsum = 0;
    std::vector<double> v(64);
    for (int l = 0; l < 64; ++l) {
        v[l] = (double)((l * 37) % 64) + 0.25;
        vmax = std::max(vmax, v[l]);
        vsum += v[l];
    }
    for (int l = 0; l < 64; ++l) {
        if (h[l] != vmax) { ++bad; rep += "wave_max lane " + std::to_string(l) + "\n"; }
        if (fabs(h[64 + l] - vsum) > 1e-9) { ++bad; rep += "wave_sum lane " + std::to_string(l) + "\n"; }
        if (h[384 + l] != v[5]) { ++bad; rep += "readlane lane " + std::to_string(l) + "\n"; }
        const int mirror = (l & ~15) | (15 - (l & 15));
        if (h[448 + l] != v[mirror]) { ++bad; rep += "row_mirror lane " + std::to_string(l) + "\n"; }
        for (int r = 0; r < 4; ++r) {
            // C[row][col], row = (lane>>4) + 4 r, col = lane & 15 ; A[i][k] = i + 16k, B[k][j] = 100k + j
            const int row = (l >> 4) + 4 * r, col = l & 15;
            double ref = 0;
            for (int k = 0; k < 4; ++k) ref += (double)(row + 16 * k) * (double)(100 * k + col);
            if (h[128 + l * 4 + r] != ref) {
                ++bad;
                if (rep.size() < 2000)
                    rep += "mfma lane " + std::to_string(l) + " r " + std::to_string(r) + " got " +
                           std::to_string(h[128 + l * 4 + r]) + " want " + std::to_string(ref) + "\n";
            }
        }
    }
    *failures = bad;
    if (report && report_len > 0) {
        strncpy(report, rep.c_str(), report_len - 1);
        report[report_len - 1] = 0;
    }
    return 0;
}

int qocx_lu_fallbacks(qocx_ctx* ctx, int64_t* count) {
    if (!ctx || !count) return fail(QOCX_ERR_ARG, "NULL argument");
    *count = 0;
    if (ctx->lu_fallbacks.p == nullptr) return 0;
    HIP_TRY(hipSetDevice(ctx->device));
    int v = 0;
    HIP_TRY(hipMemcpy(&v, ctx->lu_fallbacks.p, sizeof(int), hipMemcpyDeviceToHost));
    *count = v;
    return 0;
}

int qocx_lindblad_last_subintervals(qocx_ctx* ctx, int64_t* total) {
    if (!ctx || !total) return fail(QOCX_ERR_ARG, "NULL argument");
    *total = ctx->lb.last_subintervals;
    return 0;
}

int qocx_pade_orders(qocx_ctx* ctx, int64_t* counts) {
    if (!ctx || !counts) return fail(QOCX_ERR_ARG, "NULL argument");
    if (!ctx->have_results) return fail(QOCX_ERR_STATE, "no evaluation results");
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t total = (size_t)ctx->last_chunk * ctx->nsteps;
    if (total == 0 || total > ctx->s_arr.count) return fail(QOCX_ERR_STATE, "no step table");
    std::vector<int> entries(total);
    HIP_TRY(hipMemcpy(entries.data(), ctx->s_arr.p, total * sizeof(int), hipMemcpyDeviceToHost));
    for (int i = 0; i < 5; ++i) counts[i] = 0;
    for (int e : entries) {
        const int o = (e >> 8) & 0xff;  // step_entry (qocx_wave.h): 0 means 13
        counts[o == 3 ? 0 : (o == 5 ? 1 : (o == 7 ? 2 : (o == 9 ? 3 : 4)))] += 1;
    }
    return 0;
}

int qocx_action_degrees(qocx_ctx* ctx, int64_t* counts) {
    if (!ctx || !counts) return fail(QOCX_ERR_ARG, "NULL argument");
    if (!ctx->have_results) return fail(QOCX_ERR_STATE, "no evaluation results");
    for (int i = 0; i < 19; ++i) counts[i] = 0;
    if (ctx->action_counts.p == nullptr) return 0;  // (no evaluation has reached the resident pipeline)
    HIP_TRY(hipSetDevice(ctx->device));
    int v[19];
    HIP_TRY(hipMemcpy(v, ctx->action_counts.p, sizeof(v), hipMemcpyDeviceToHost));
    for (int i = 0; i < 19; ++i) counts[i] = v[i];
    return 0;
}

int qocx_debug_spectral_bound(const double* m, int32_t n, double* bound) {
    if (!m || !bound) return fail(QOCX_ERR_ARG, "NULL argument");
    if (n < 1 || n > 64) return fail(QOCX_ERR_ARG, "n must be in 1..64");
    *bound = spectral_bound(m, n);
    return 0;
}

int qocx_debug_action_degree(double bound1, double bound2, int32_t rule, int32_t* degree) {
    if (!degree) return fail(QOCX_ERR_ARG, "NULL argument");
    if (rule != 0 && rule != 1) return fail(QOCX_ERR_ARG, "rule must be 0 or 1");
    *degree = qocx::action_degree_rule(bound1, bound2, rule);
    return 0;
}

int qocx_debug_action_route(const qocx_action_facts* facts, int32_t* kernel, int32_t* table, int32_t* m_max) {
    if (!facts || !kernel || !table || !m_max) return fail(QOCX_ERR_ARG, "NULL argument");
    const qocx::ActionPlan plan = qocx::action_plan(*facts);
    *kernel = plan.kernel; *table = plan.table; *m_max = plan.m_max;
    return 0;
}

int qocx_debug_lindblad_route(const qocx_lindblad_facts* facts, int32_t* kernels, int32_t* multi_wave,
                              int32_t* two_sided, int32_t* rate_sens, int32_t* form) {
    if (!facts || !kernels || !multi_wave || !two_sided || !rate_sens || !form)
        return fail(QOCX_ERR_ARG, "NULL argument");
    const qocx::LindbladFacts& f = *facts;
    const qocx::LindbladForm m = qocx::lindblad_form(
        f, [&](int mode, int nops) { return qocx::lindblad_lds_size(f.n, f.S, nops, mode, f.K); });
    const qocx::LindbladRoute r = qocx::lindblad_route(m, f);
    for (int ph = 0; ph < 3; ++ph) kernels[ph] = (int32_t)r.kernel[ph];
    *multi_wave = r.multi_wave; *two_sided = r.two_sided; *rate_sens = r.rate_sens;
    form[0] = m.scratch; form[1] = m.pad_op; form[2] = m.multi_wave; form[3] = m.cache_gen;
    return 0;
}

int qocx_debug_lindblad_pieces(int32_t want_grad, int32_t multi_wave, int64_t stage_budget,
                               int64_t stage_budget_seeds, int32_t min_piece, int32_t wave_mode, int32_t cu_count,
                               int32_t seeds, int64_t per_seed, int32_t capacity, int32_t* counts,
                               int32_t* keep_stages, int32_t* piece_multi_wave, int32_t* pieces, int64_t* sized_for) {
    if (!counts || !keep_stages || !piece_multi_wave || !pieces || !sized_for)
        return fail(QOCX_ERR_ARG, "NULL argument");
    if (stage_budget < 0 || stage_budget_seeds < 0 || min_piece < 1 || wave_mode < 0 || wave_mode > 2 ||
        cu_count < 1 || seeds < 1 || per_seed < 1 || capacity < 0)
        return fail(QOCX_ERR_ARG, "bad argument");
    const qocx::PieceRule rule{want_grad != 0, multi_wave != 0, (size_t)stage_budget, stage_budget_seeds, min_piece,
                               wave_mode, cu_count};
    std::vector<qocx::LindbladPiece> out;
    *sized_for = (int64_t)qocx::lindblad_group_pieces(rule, 1, 0, seeds, (size_t)per_seed, out);
    *pieces = (int32_t)out.size();
    for (size_t i = 0; i < out.size() && i < (size_t)capacity; ++i) {
        counts[i] = out[i].count; keep_stages[i] = out[i].keep_stages; piece_multi_wave[i] = out[i].multi_wave;
    }
    return 0;
}

int qocx_action_reruns(qocx_ctx* ctx, int64_t* count) {
    if (!ctx || !count) return fail(QOCX_ERR_ARG, "NULL argument");
    *count = ctx->action_reruns;
    return 0;
}

int qocx_debug_timeline(qocx_ctx* ctx, double* out, int64_t capacity, int64_t* count) {
    if (!ctx || !count) return fail(QOCX_ERR_ARG, "NULL argument");
    const int64_t n = (int64_t)(ctx->timeline.size() / 3);
    *count = n;
    if (out)
        for (int64_t i = 0; i < std::min(n, capacity) * 3; ++i) out[i] = ctx->timeline[(size_t)i];
    return 0;
}

int qocx_debug_read_stamps(qocx_ctx* ctx, uint64_t* out, int64_t count) {
    if (!ctx || !out) return fail(QOCX_ERR_ARG, "NULL argument");
    if ((size_t)count > ctx->stamps.count) return fail(QOCX_ERR_ARG, "more stamps than were collected");
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipMemcpy(out, ctx->stamps.p, (size_t)count * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return 0;
}

int qocx_debug_lindblad_knobs(qocx_ctx* ctx, int64_t stage_budget_seeds, int32_t min_piece,
                              int32_t wave_mode) {
    if (!ctx) return fail(QOCX_ERR_ARG, "ctx is NULL");
    if (stage_budget_seeds < 0 || min_piece < 1 || wave_mode < 0 || wave_mode > 2)
        return fail(QOCX_ERR_ARG, "bad knob value");
    ctx->lb.dbg_stage_seeds = stage_budget_seeds;
    ctx->lb.dbg_min_piece = min_piece;
    ctx->lb.dbg_wave_mode = wave_mode;
    return 0;
}

}  // extern "C"
