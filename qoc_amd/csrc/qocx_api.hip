// qocx_api.hip - host side of the C ABI declared in include/qocx.h: context, problem upload (what
// GrapeSchroedingerDiscreteState prepares for the evolve loop, qoc/models/programstate.py:33-61), the
// seed-level evaluation and downloads of the Schroedinger path, timing, knobs and the RCCL shim.
// qocx_host.h holds what the host files share; the evaluation of the uploaded items is
// qocx_host_resident.hip, the Lindblad path qocx_api_lindblad.hip, the multi-start driver
// qocx_api_multistart.hip, the debug entry points qocx_api_debug.hip.
#include <dlfcn.h>
#include <unistd.h>

#include <cfloat>

#include "qocx_host.h"
#include "qocx_action.h"

namespace {

thread_local std::string g_error;

}  // namespace

namespace qocx::host {

int fail(int code, const std::string& msg) {
    g_error = msg;
    return code;
}

const double THETA13 = 5.371920351148152;

int pade_scale_count(double norm1) {
    int s = 0;
    double th = THETA13;
    while (norm1 > th && s < 1000) {
        th *= 2.0;
        ++s;
    }
    return s;
}

int commit_step_bound(qocx_ctx* ctx, double bound, bool keep_larger, const char* needs, double bound2) {
    const int sb = pade_scale_count(bound);
    if (!keep_larger) ctx->sbound = sb, ctx->norm_bound = bound;  // (an upload: even where refused below)
    ctx->norm2_bound = keep_larger ? std::max(ctx->norm2_bound, bound2) : bound2;
    ctx->norm2_bound_mid = 1e300;
    if (sb > 10)
        return fail(QOCX_ERR_CAPACITY, std::string("||dt H||_1 ") + needs +
                                           " more than 2^10 squaring sub-steps per step; reduce dt");
    if (keep_larger) {  // qocx_opt_clip: the controls move on the device from here on
        ctx->sbound = std::max(ctx->sbound, sb);
        ctx->norm_bound = std::max(ctx->norm_bound, bound);
        ctx->norm_bound_mid = 1e300;
    }
    ctx->slot_cap = ((size_t)ctx->nsteps << ctx->sbound) + 1;
    return 0;
}

double one_norm(const double* m, int n) {  // complex row-major
    double best = 0;
    for (int c = 0; c < n; ++c) {
        double s = 0;
        for (int r = 0; r < n; ++r) s += hypot(m[2 * ((size_t)r * n + c)], m[2 * ((size_t)r * n + c) + 1]);
        best = std::max(best, s);
    }
    return best;
}

// An upper bound of the spectral radius of a Hermitian matrix (complex row-major, n <= 64), which is its
// 2-norm: rho(A) = rho(A^(2^k))^(1/2^k) <= ||A^(2^k)||_F^(1/2^k), and ||.||_F <= sqrt(n) rho for a normal
// matrix, so after k = 8 squarings the overshoot is at most n^(1/512) (0.82 % at n = 64). Every square is
// normalised by its Frobenius norm (no overflow or underflow whatever the scale of A) and the logarithms of
// the norms are carried: with B_0 = A / f_0, B_(j+1) = B_j^2 / f_(j+1), f_j = ||.||_F before the division,
//     ||A^(2^k)||_F^(1/2^k) = exp(sum_j log(f_j) / 2^j).
// The rounding of 8 products of n <= 64 terms moves the result by parts in 1e13; the final (1 + 1e-9) keeps
// it an upper bound. Zero matrix: 0. Not finite (or n out of range): NaN - the caller keeps the 1-norm.
double spectral_bound(const double* m, int n) {
    if (n < 1 || n > 64) return std::nan("");
    const size_t nn = (size_t)n * n;
    std::vector<double> a(m, m + 2 * nn), b(2 * nn);
    double log_sum = 0, weight = 1;
    for (int j = 0;; ++j) {
        double big = 0;
        for (size_t i = 0; i < 2 * nn; ++i)
            if (!(fabs(a[i]) <= big)) big = fabs(a[i]);  // (also catches NaN)
        if (big == 0 && j == 0) return 0;
        // (inf / NaN, or a square that vanished: A was nilpotent to rounding, which no Hermitian A is)
        if (!(big > 0 && big <= DBL_MAX)) return std::nan("");
        double f = 0;  // ||a||_F, scaled by its largest entry
        for (size_t i = 0; i < 2 * nn; ++i) f += (a[i] / big) * (a[i] / big);
        f = sqrt(f);
        log_sum += weight * (log(big) + log(f));
        for (size_t i = 0; i < 2 * nn; ++i) a[i] = a[i] / big / f;
        if (j == 8) break;
        weight *= 0.5;
        for (int r = 0; r < n; ++r)
            for (int c = 0; c < n; ++c) {
                double re = 0, im = 0;
                for (int q = 0; q < n; ++q) {
                    const double xr = a[2 * ((size_t)r * n + q)], xi = a[2 * ((size_t)r * n + q) + 1];
                    const double yr = a[2 * ((size_t)q * n + c)], yi = a[2 * ((size_t)q * n + c) + 1];
                    re += xr * yr - xi * yi;
                    im += xr * yi + xi * yr;
                }
                b[2 * ((size_t)r * n + c)] = re;
                b[2 * ((size_t)r * n + c) + 1] = im;
            }
        a.swap(b);
    }
    return exp(log_sum) * (1.0 + 1e-9);
}

}  // namespace qocx::host

struct ncclUniqueIdBytes {
    char internal[128];
};

namespace {

void c_image(const double* m, int n, int nb, double2* out) {
    for (int ti = 0; ti < nb; ++ti)
        for (int tj = 0; tj < nb; ++tj)
            for (int r = 0; r < 4; ++r)
                for (int lane = 0; lane < 64; ++lane) {
                    const int q = lane >> 4, c = lane & 15;
                    const int row = 16 * ti + 4 * r + q, col = 16 * tj + c;
                    double2 e = make_double2(0, 0);
                    if (row < n && col < n) {
                        e.x = m[2 * ((size_t)row * n + col)];
                        e.y = m[2 * ((size_t)row * n + col) + 1];
                    }
                    out[((ti * nb + tj) * 4 + r) * 64 + lane] = e;
                }
}

// Column-major NP x NP image of a row-major n x n matrix (or of its transpose), zero padded.
void r_image(const double* m, int n, int np, bool transpose, double2* out) {
    for (int col = 0; col < np; ++col)
        for (int row = 0; row < np; ++row) {
            int r = row, c = col;
            if (transpose) std::swap(r, c);
            double2 e = make_double2(0, 0);
            if (r < n && c < n) {
                e.x = m[2 * ((size_t)r * n + c)];
                e.y = m[2 * ((size_t)r * n + c) + 1];
            }
            out[(size_t)col * np + row] = e;
        }
}

// m equals its conjugate transpose bit for bit
bool hermitian_bitwise(const double* m, int n) {
    for (int r = 0; r < n; ++r)
        for (int c = r; c < n; ++c)
            if (m[2 * ((size_t)r * n + c)] != m[2 * ((size_t)c * n + r)] ||
                m[2 * ((size_t)r * n + c) + 1] != -m[2 * ((size_t)c * n + r) + 1])
                return false;
    return true;
}

// step j reads row j of a [nsteps][Ke] control array whole (EffectiveControls::interp_id)
std::vector<qocx::StepInterp> identity_interp(int nsteps) {
    std::vector<qocx::StepInterp> ident(nsteps);
    for (int j = 0; j < nsteps; ++j) ident[j] = qocx::StepInterp{j, j, 1.0, 0.0};
    return ident;
}

// timing events come from a grow-only pool: creating and destroying ~100 events per evaluation
// makes the runtime stall for tens of milliseconds every few evaluations
hipEvent_t pooled_event(qocx_ctx* ctx) {
    if (ctx->ev_used == ctx->ev_pool.size()) {
        hipEvent_t e = nullptr;
        (void)hipEventCreate(&e);
        ctx->ev_pool.push_back(e);
    }
    return ctx->ev_pool[ctx->ev_used++];
}

}  // namespace

namespace qocx::host {

int OperatorImages::build(const double* m, size_t count, int n, int nb, hipStream_t st, bool t_only) {
    const int np = 16 * nb;
    const size_t mat = (size_t)np * np, nn2 = (size_t)n * n * 2;
    std::vector<double2> img(count * mat);
    for (int pass = t_only ? 2 : 0; pass < 3; ++pass) {
        for (size_t i = 0; i < count; ++i) {
            if (pass == 0) c_image(m + i * nn2, n, nb, img.data() + i * mat);
            else r_image(m + i * nn2, n, np, pass == 2, img.data() + i * mat);
        }
        if (layout(pass).upload(img, st)) return QOCX_ERR_HIP;
    }
    return 0;
}

void time_begin(qocx_ctx* ctx, int which, hipStream_t st) {
    // timing 1: every launch; 2 + k: the launches of kernel k only (qocx_set_timing)
    ctx->time_active = ctx->timing == 1 || (ctx->timing >= 2 && which == ctx->timing - 2);
    if (!ctx->time_active) return;
    TimingRec r;
    r.which = which;
    r.a = pooled_event(ctx);
    r.b = pooled_event(ctx);
    (void)hipEventRecord(r.a, st);
    ctx->pending.push_back(r);
}

void time_end(qocx_ctx* ctx, hipStream_t st) {
    if (!ctx->time_active) return;
    (void)hipEventRecord(ctx->pending.back().b, st);
}

void time_collect(qocx_ctx* ctx) {
    ctx->timeline.clear();
    for (auto& r : ctx->pending) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, r.a, r.b) == hipSuccess) {
            ctx->t_ms[r.which] += ms;
            ctx->t_launch[r.which] += 1;
            float t0 = 0;
            if (hipEventElapsedTime(&t0, ctx->pending.front().a, r.a) == hipSuccess) {
                ctx->timeline.push_back((double)r.which);
                ctx->timeline.push_back((double)t0);
                ctx->timeline.push_back((double)t0 + ms);
            }
        }
    }
    ctx->pending.clear();
    ctx->ev_used = 0;
}

}  // namespace qocx::host

namespace {

int load_rccl(qocx_ctx* ctx) {
    if (ctx->rccl.lib) return 0;
    const char* names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
    void* lib = nullptr;
    for (const char* nm : names) {
        lib = dlopen(nm, RTLD_NOW | RTLD_GLOBAL);
        if (lib) break;
    }
    if (!lib) return fail(QOCX_ERR_RCCL, std::string("cannot load librccl: ") + dlerror());
    Rccl& r = ctx->rccl;
    r.lib = lib;
    *(void**)(&r.GetUniqueId) = dlsym(lib, "ncclGetUniqueId");
    *(void**)(&r.AllReduce) = dlsym(lib, "ncclAllReduce");
    *(void**)(&r.CommDestroy) = dlsym(lib, "ncclCommDestroy");
    *(void**)(&r.GetErrorString) = dlsym(lib, "ncclGetErrorString");
    if (!r.GetUniqueId || !dlsym(lib, "ncclCommInitRank") || !r.AllReduce || !r.CommDestroy)
        return fail(QOCX_ERR_RCCL, "librccl lacks the expected nccl* symbols");
    return 0;
}

// the cost table of a Schroedinger problem (DevCost, target vectors padded to np, forbid counts)
int upload_costs(qocx_ctx* ctx, const qocx_schroedinger_problem* p) {
    const int n = ctx->n, np = ctx->np, S = ctx->S;
    std::vector<qocx::DevCost> dcosts;
    std::vector<double2> pool;
    std::vector<int> counts;
    ctx->has_step_costs = 0;
    for (int ci = 0; ci < p->cost_count; ++ci) {
        const qocx_cost_desc& c = p->costs[ci];
        qocx::DevCost d;
        d.kind = c.kind;
        d.step_cost = c.step_cost ? 1 : 0;
        d.scale = c.scale;
        d.vec_offset = (int)(pool.size() / np);
        d.cnt_offset = (int)counts.size();
        if (!c.vectors) return fail(QOCX_ERR_ARG, "cost vectors missing");
        int nvec = S;
        if (c.kind == QOCX_COST_FORBID) {
            if (!c.counts) return fail(QOCX_ERR_ARG, "forbid counts missing");
            nvec = 0;
            for (int s = 0; s < S; ++s) {
                if (c.counts[s] < 1) return fail(QOCX_ERR_ARG, "forbid count < 1");
                counts.push_back(c.counts[s]);
                nvec += c.counts[s];
            }
        } else if (c.kind != QOCX_COST_TARGET_COHERENT && c.kind != QOCX_COST_TARGET_INCOHERENT) {
            return fail(QOCX_ERR_ARG, "unknown cost kind");
        }
        for (int v = 0; v < nvec; ++v)
            for (int i = 0; i < np; ++i) {
                double2 e = make_double2(0, 0);
                if (i < n) {
                    e.x = c.vectors[2 * ((size_t)v * n + i)];
                    e.y = c.vectors[2 * ((size_t)v * n + i) + 1];
                }
                pool.push_back(e);
            }
        if (d.step_cost) ctx->has_step_costs = 1;
        dcosts.push_back(d);
    }
    ctx->cost_count = (int)dcosts.size();
    // one final-state target cost whose cotangent is ONE scalar times the targets: coherent (any
    // number of states) or a single state
    ctx->unit_ok = dcosts.size() == 1 && !dcosts[0].step_cost &&
                   (dcosts[0].kind == QOCX_DEV_COST_COHERENT ||
                    (dcosts[0].kind == QOCX_DEV_COST_INCOHERENT && S == 1));
    if (ctx->costs.upload(dcosts, ctx->stream)) return QOCX_ERR_HIP;
    if (ctx->cost_vectors.upload(pool, ctx->stream)) return QOCX_ERR_HIP;
    if (ctx->cost_counts.upload(counts, ctx->stream)) return QOCX_ERR_HIP;
    return 0;
}

// ---- the stages of qocx_set_schroedinger_problem -------------------------------------------------

int check_problem(const qocx_schroedinger_problem* p) {
    if (p->struct_size != (int32_t)sizeof(qocx_schroedinger_problem))
        return fail(QOCX_ERR_ARG, "qocx_schroedinger_problem.struct_size does not match this "
                                  "library's header (stale binding?)");
    const int n = p->hilbert_size, S = p->state_count, K = p->control_count, N = p->system_eval_count;
    if (n < 1 || n > 1024)
        return fail(QOCX_ERR_ARG, "hilbert_size must be in 1..1024 (1..64: the wavefront kernels; 65..1024: the general "
                                  "path of qocx_general.hip)");
    // (a full propagator has n states: up to 256 of them on the general path)
    if (S < 1 || S > (n > 64 ? 1024 : 64)) return fail(QOCX_ERR_ARG, "state_count must be in 1..64 (1..1024 above hilbert_size 64)");
    if (K < 0 || K > 64) return fail(QOCX_ERR_ARG, "control_count must be in 0..64");
    if (N < 2) return fail(QOCX_ERR_ARG, "system_eval_count must be >= 2");
    if (K > 0 && p->control_eval_count < 2) return fail(QOCX_ERR_ARG, "control_eval_count must be >= 2");
    if (p->cost_eval_step < 1) return fail(QOCX_ERR_ARG, "cost_eval_step must be >= 1");
    if (p->magnus_policy != QOCX_MAGNUS_M2 && p->magnus_policy != QOCX_MAGNUS_M4 &&
        p->magnus_policy != QOCX_MAGNUS_M6)
        return fail(QOCX_ERR_ARG, "unknown magnus_policy");
    // quadrature nodes per step: magnus_policy / 2 = 1, 2, 3
    if (p->nt != 1 && p->nt != (N - 1) * (p->magnus_policy / 2))
        return fail(QOCX_ERR_ARG, "nt must be 1 or (N-1) * (quadrature nodes of the policy)");
    if (!p->h0 || !p->initial_states || (K > 0 && !p->g))
        return fail(QOCX_ERR_ARG, "h0 / g / initial_states missing");
    if (p->cost_count < 0 || (p->cost_count > 0 && !p->costs))
        return fail(QOCX_ERR_ARG, "costs missing");
    return 0;
}

// every h0[t], g[t][k] Hermitian bit for bit
void set_hermitian_flags(qocx_ctx* ctx, const qocx_schroedinger_problem* p) {
    const size_t nn2 = (size_t)ctx->n * ctx->n * 2;
    bool herm = true;
    for (int t = 0; t < ctx->nt && herm; ++t) {
        herm = hermitian_bitwise(p->h0 + (size_t)t * nn2, ctx->n);
        for (int k = 0; k < ctx->K && herm; ++k)
            herm = hermitian_bitwise(p->g + ((size_t)t * ctx->K + k) * nn2, ctx->n);
    }
    ctx->hermitian = herm ? 1 : 0;
    ctx->hermitian_linear = ctx->hermitian;
}

// Hamiltonian images + norms for the squaring bound
int upload_operators(qocx_ctx* ctx, const qocx_schroedinger_problem* p) {
    const int n = ctx->n, K = ctx->K, nt = ctx->nt;
    const size_t nn2 = (size_t)n * n * 2;
    ctx->h0_norm_max = 0;
    ctx->g_norm_max.assign(K, 0.0);
    for (int t = 0; t < nt; ++t) {
        ctx->h0_norm_max = std::max(ctx->h0_norm_max, one_norm(p->h0 + (size_t)t * nn2, n));
        for (int k = 0; k < K; ++k)
            ctx->g_norm_max[k] = std::max(ctx->g_norm_max[k], one_norm(p->g + ((size_t)t * K + k) * nn2, n));
    }
    // The spectral-norm bounds behind the Taylor degrees of the matrix-free route (qocx_action.h). They
    // sharpen the 1-norms only where that route can run - Hermitian operators, constant in time, n <= 64 -
    // and never exceed them (||A||_2 <= ||A||_1 for a Hermitian A; the bound may overshoot by 1 %).
    ctx->h0_norm2_max = ctx->h0_norm_max;
    ctx->g_norm2_max = ctx->g_norm_max;
    if (ctx->hermitian && nt == 1 && n <= 64) {
        auto sharpen = [&](const double* m, double norm1) {
            const double s = spectral_bound(m, n);
            return s <= norm1 ? s : norm1;  // (NaN: the 1-norm)
        };
        ctx->h0_norm2_max = sharpen(p->h0, ctx->h0_norm_max);
        for (int k = 0; k < K; ++k) ctx->g_norm2_max[k] = sharpen(p->g + (size_t)k * nn2, ctx->g_norm_max[k]);
    }
    // E_k = -i dt G_k for the gradient kernels of the matrix-free route at n <= 32 (qocx_action.hip, qocx_action16.hip):
    // (dt y, -dt x) of every element of the r image, the products the kernel formed per step before. Here,
    // because this is the one place that writes ctx->dt or the G_k images: the image cannot go stale.
    if (ctx->nb <= 2 && nt == 1 && K > 0) {
        const int np = ctx->np;
        const size_t mat = (size_t)np * np;
        std::vector<double2> img(K * mat);
        for (int k = 0; k < K; ++k) r_image(p->g + (size_t)k * nn2, n, np, false, img.data() + k * mat);
        for (double2& e : img) e = make_double2(ctx->dt * e.y, -ctx->dt * e.x);
        if (ctx->g_eimg.upload(img, ctx->stream)) return QOCX_ERR_HIP;
    } else {
        ctx->g_eimg.release();
    }
    return ctx->h0.build(p->h0, (size_t)nt, n, ctx->nb, ctx->stream) ||
                   ctx->g.build(p->g, (size_t)nt * K, n, ctx->nb, ctx->stream) ||
                   (K > 0 && (ctx->g_norm_dev.upload(ctx->g_norm_max, ctx->stream) ||  // step table
                              ctx->g_norm2_dev.upload(ctx->g_norm2_max, ctx->stream)))
               ? QOCX_ERR_HIP : 0;
}

// The tables of the matrix-free route on effective controls for the operators [first, first + count) of the
// augmented set (EffectiveControls::op_norm1, ::op_norm2, ::eimg); the caller has sized the host vectors and,
// where it is formed (n <= 32, nt == 1), the image for all Ke operators. The device copies of the norms are
// uploaded by the call that delivers the LAST operators.
int effective_operator_tables(qocx_ctx* ctx, const double* m, int first, int count) {
    EffectiveControls& eff = ctx->eff;
    const int n = ctx->n, np = ctx->np;
    const size_t nn2 = (size_t)n * n * 2, mat = (size_t)np * np;
    const bool sharpen = ctx->hermitian && ctx->nt == 1 && n <= 64;
    std::vector<double2> img(eff.eimg.p != nullptr ? count * mat : 0);
    for (int e = 0; e < count; ++e) {
        const double* op = m + (size_t)e * nn2;
        const double norm1 = one_norm(op, n);
        const double s = sharpen ? spectral_bound(op, n) : norm1;
        eff.op_norm1[first + e] = norm1;
        eff.op_norm2[first + e] = s <= norm1 ? s : norm1;  // (NaN: the 1-norm)
        if (!img.empty()) r_image(op, n, np, false, img.data() + e * mat);
    }
    if (!img.empty()) {
        for (double2& x : img) x = make_double2(ctx->dt * x.y, -ctx->dt * x.x);
        HIP_TRY(hipMemcpyAsync(eff.eimg.p + (size_t)first * mat, img.data(), img.size() * sizeof(double2),
                               hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));  // img is this scope's
    }
    if (first + count == (int)eff.op_norm1.size() &&
        (eff.op_norm1_dev.upload(eff.op_norm1, ctx->stream) || eff.op_norm2_dev.upload(eff.op_norm2, ctx->stream)))
        return QOCX_ERR_HIP;
    return 0;
}

// M4, time-independent H0 / G_k: the commutators leave the time loop (M4LinArgs). Constant
// matrices G_k, A_k = -i [G_k, H0], B_kl = -i [G_k, G_l] (k < l); Hermitian when H0 and the
// G_k are (made so bit for bit, the Hermitian kernel forms rely on it).
int upload_m4_commutators(qocx_ctx* ctx, const qocx_schroedinger_problem* p) {
    const int n = ctx->n, K = ctx->K, Ke = 2 * K + K * (K - 1) / 2;
    if (ctx->nodes != 2 || ctx->nt != 1 || K < 1 || K > QOCX_M4LIN_MAX_K) return 0;
    const size_t nn = (size_t)n * n;
    std::vector<double> ge((size_t)Ke * nn * 2);
    std::copy(p->g, p->g + (size_t)K * nn * 2, ge.begin());
    auto neg_i_commutator = [&](const double* x, const double* y, double* out) {
        for (int r = 0; r < n; ++r)
            for (int c = 0; c < n; ++c) {
                double re = 0, im = 0;  // (x y - y x)[r][c]
                for (int q = 0; q < n; ++q) {
                    const double* xa = x + 2 * ((size_t)r * n + q);
                    const double* yb = y + 2 * ((size_t)q * n + c);
                    const double* ya = y + 2 * ((size_t)r * n + q);
                    const double* xb = x + 2 * ((size_t)q * n + c);
                    re += xa[0] * yb[0] - xa[1] * yb[1] - (ya[0] * xb[0] - ya[1] * xb[1]);
                    im += xa[0] * yb[1] + xa[1] * yb[0] - (ya[0] * xb[1] + ya[1] * xb[0]);
                }
                out[2 * ((size_t)r * n + c)] = im;       // -i (re + i im) = im - i re
                out[2 * ((size_t)r * n + c) + 1] = -re;
            }
        if (ctx->hermitian)
            for (int r = 0; r < n; ++r)
                for (int c = r; c < n; ++c) {
                    double* a = out + 2 * ((size_t)r * n + c);
                    double* b = out + 2 * ((size_t)c * n + r);
                    const double re = 0.5 * (a[0] + b[0]), im = (r == c) ? 0.0 : 0.5 * (a[1] - b[1]);
                    a[0] = re; a[1] = im;
                    b[0] = re; b[1] = -im;
                }
    };
    for (int k = 0; k < K; ++k)
        neg_i_commutator(p->g + (size_t)k * nn * 2, p->h0, ge.data() + (size_t)(K + k) * nn * 2);
    int e = 2 * K;
    for (int k = 0; k < K; ++k)
        for (int l = k + 1; l < K; ++l, ++e)
            neg_i_commutator(p->g + (size_t)k * nn * 2, p->g + (size_t)l * nn * 2,
                             ge.data() + (size_t)e * nn * 2);
    if (ctx->eff.images.build(ge.data(), (size_t)Ke, n, ctx->nb, ctx->stream) ||
        ctx->eff.interp_id.upload(identity_interp(ctx->nsteps), ctx->stream))
        return QOCX_ERR_HIP;
    // norms and the E_e image of all Ke operators, for the matrix-free route (knob "action_eff")
    ctx->eff.op_norm1.assign(Ke, 0.0);
    ctx->eff.op_norm2.assign(Ke, 0.0);
    if (ctx->nb <= 2) {
        if (ctx->eff.eimg.ensure((size_t)Ke * ctx->np * ctx->np)) return QOCX_ERR_HIP;
    } else {
        ctx->eff.eimg.release();
    }
    if (int rc = effective_operator_tables(ctx, ge.data(), 0, Ke)) return rc;
    ctx->eff.kind = EffectiveControls::M4_LINEAR;
    ctx->eff.Ke = Ke;
    return 0;
}

// initial states, padded
int upload_initial_states(qocx_ctx* ctx, const qocx_schroedinger_problem* p) {
    const int n = ctx->n, np = ctx->np, S = ctx->S;
    std::vector<double2> psi((size_t)S * np, make_double2(0, 0));
    for (int s = 0; s < S; ++s)
        for (int i = 0; i < n; ++i)
            psi[(size_t)s * np + i] = make_double2(p->initial_states[2 * ((size_t)s * n + i)],
                                                   p->initial_states[2 * ((size_t)s * n + i) + 1]);
    return ctx->psi0.upload(psi, ctx->stream) ? QOCX_ERR_HIP : 0;
}

// interpolation table at the quadrature times t_j + c_q dt of the Magnus policy
// (mathmethods.py:54-65; nodes :72, :96-97, :125-127), and its transpose for scatter_kernel
int upload_interpolation(qocx_ctx* ctx, const qocx_schroedinger_problem* p) {
    const int K = ctx->K, nc = ctx->nc, nsteps = ctx->nsteps, nodes = ctx->nodes;
    static const double node_c[3][3] = {
        {0.5, 0, 0},
        {0.5 - std::sqrt(3.0) / 6, 0.5 + std::sqrt(3.0) / 6, 0},
        {0.5 - std::sqrt(15.0) / 10, 0.5, 0.5 + std::sqrt(15.0) / 10}};
    std::vector<qocx::StepInterp> interp((size_t)nsteps * nodes);
    std::vector<std::vector<std::pair<int, double>>> rows(K > 0 ? nc : 0);
    ctx->pwc = ctx->interp_policy == QOCX_INTERP_PIECEWISE_CONSTANT;
    if (K > 0 && ctx->pwc) {
        // piecewise constant: a node reads the slice it lies in, u = controls[min(floor(x nc / T), nc - 1)]
        // (right-continuous at the interior edges). i1 == i2, dx = 1, off = 0: control_at returns
        // y1 + ((y1 - y1) / 1) * 0 = y1 bit for bit, and the slice's row takes the node's cotangent whole.
        for (int j = 0; j < nsteps; ++j)
            for (int q = 0; q < nodes; ++q) {
                const double x = j * ctx->dt + ctx->dt * node_c[nodes - 1][q];
                const double f = std::floor(x * nc / p->evolution_time);
                const int slice = f >= nc - 1 ? nc - 1 : (f > 0 ? (int)f : 0);
                interp[(size_t)j * nodes + q] = qocx::StepInterp{slice, slice, 1.0, 0.0};
                rows[slice].push_back(std::make_pair(j * nodes + q, 1.0));
            }
    } else if (K > 0) {
        std::vector<double> xs(nc);
        const double stepx = p->evolution_time / (nc - 1);  // numpy.linspace
        for (int i = 0; i < nc; ++i) xs[i] = i * stepx;
        xs[nc - 1] = p->evolution_time;
        for (int j = 0; j < nsteps; ++j)
            for (int q = 0; q < nodes; ++q) {
                const double time = j * ctx->dt;
                const double x = time + ctx->dt * node_c[nodes - 1][q];
                int i1, i2;
                if (x <= xs[0]) {
                    i1 = 0; i2 = 1;
                } else if (x >= xs[nc - 1]) {
                    i1 = nc - 2; i2 = nc - 1;
                } else {
                    int idx = 0;
                    while (!(x <= xs[idx])) ++idx;
                    i1 = idx - 1; i2 = idx;
                }
                qocx::StepInterp& e = interp[(size_t)j * nodes + q];
                e.i1 = i1; e.i2 = i2;
                e.dx = xs[i2] - xs[i1];
                e.off = x - xs[i1];
                const double theta = e.off / e.dx;
                rows[i1].push_back(std::make_pair(j * nodes + q, 1.0 - theta));
                rows[i2].push_back(std::make_pair(j * nodes + q, theta));
            }
    } else {
        for (auto& e : interp) e = qocx::StepInterp{0, 0, 1.0, 0.0};
    }
    if (ctx->interp.upload(interp, ctx->stream)) return QOCX_ERR_HIP;
    std::vector<int> row_ptr(1, 0), col_step;
    std::vector<double> weight;
    for (auto& r : rows) {
        for (auto& e : r) {
            col_step.push_back(e.first);
            weight.push_back(e.second);
        }
        row_ptr.push_back((int)col_step.size());
    }
    if (ctx->row_ptr.upload(row_ptr, ctx->stream)) return QOCX_ERR_HIP;
    if (ctx->col_step.upload(col_step, ctx->stream)) return QOCX_ERR_HIP;
    if (ctx->weight.upload(weight, ctx->stream)) return QOCX_ERR_HIP;
    return 0;
}

}  // namespace

extern "C" {

const char* qocx_last_error(void) { return g_error.c_str(); }

int qocx_version(void) { return 100; }

int qocx_device_count(int* count) {
    if (!count) return fail(QOCX_ERR_ARG, "count is NULL");
    HIP_TRY(hipGetDeviceCount(count));
    return 0;
}

int qocx_create(int device, qocx_ctx** out) {
    if (!out) return fail(QOCX_ERR_ARG, "out is NULL");
    int count = 0;
    HIP_TRY(hipGetDeviceCount(&count));
    if (count <= 0) return fail(QOCX_ERR_HIP, "no HIP device visible");
    if (device < 0) {
        const char* lr = getenv("LOCAL_RANK");
        device = lr ? atoi(lr) : 0;
        device %= count;
    }
    if (device >= count) return fail(QOCX_ERR_ARG, "device index out of range");
    HIP_TRY(hipSetDevice(device));
    qocx_ctx* ctx = new qocx_ctx();
    ctx->device = device;
    {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess &&
            cus > 0)
            ctx->cu_count = cus;
    }
    hipError_t e = hipStreamCreate(&ctx->stream);
    if (e != hipSuccess) {
        delete ctx;
        return fail(QOCX_ERR_HIP, hipGetErrorString(e));
    }
    if (ctx->status.ensure(1)) {
        qocx_destroy(ctx);
        return QOCX_ERR_HIP;
    }
    // side streams of the latency-bound sweeps get the highest priority, so that their few
    // waves are placed as soon as a SIMD frees up under the compute stream's big grids
    int prio_least = 0, prio_greatest = 0;
    (void)hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest);
    if (hipStreamCreateWithFlags(&ctx->lu_stream, hipStreamNonBlocking) != hipSuccess) {
        ctx->lu_stream = nullptr;
        qocx_destroy(ctx);
        return fail(QOCX_ERR_HIP, "cannot create the pipeline streams");
    }
    for (int i = 0; i < 32; ++i) {
        hipEvent_t e0;
        if (hipEventCreateWithFlags(&e0, hipEventDisableTiming) != hipSuccess) {
            qocx_destroy(ctx);
            return fail(QOCX_ERR_HIP, "cannot create the pipeline streams");
        }
        ctx->ev_pq.push_back(e0);
    }
    for (int i = 0; i < 32; ++i) {
        hipStream_t st;
        hipEvent_t e1, e2, e3;
        if ((i < 2 &&
             hipStreamCreateWithPriority(&st, hipStreamNonBlocking, prio_greatest) != hipSuccess) ||
            hipEventCreateWithFlags(&e1, hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&e2, hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&e3, hipEventDisableTiming) != hipSuccess) {
            qocx_destroy(ctx);  // releases what has been created so far
            return fail(QOCX_ERR_HIP, "cannot create the pipeline streams");
        }
        if (i < 2) ctx->sweep_streams.push_back(st);  // forward | adjoint (two-sided pipeline)
        ctx->ev_factored.push_back(e1);
        ctx->ev_swept.push_back(e2);
        ctx->ev_fwd.push_back(e3);
    }
    // (diagnostic build only, qocx_diag.h: fuzz runs of the whole suite on another sweep)
    if (const char* env = qocx::diag_getenv("QOCX_SWEEP_IMPL")) ctx->knobs["sweep_impl"] = atoi(env);
    *out = ctx;
    return 0;
}

int qocx_destroy(qocx_ctx* ctx) {
    if (!ctx) return 0;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    time_collect(ctx);
    if (ctx->comm && ctx->rccl.CommDestroy) ctx->rccl.CommDestroy(ctx->comm);
    if (ctx->pin_controls) (void)hipHostFree(ctx->pin_controls);
    ctx->pin_controls = nullptr;
    for (auto e : ctx->ev_pool) (void)hipEventDestroy(e);
    for (auto st : ctx->sweep_streams) (void)hipStreamDestroy(st);
    if (ctx->lu_stream) (void)hipStreamDestroy(ctx->lu_stream);
    for (auto e : ctx->ev_pq) (void)hipEventDestroy(e);
    for (auto e : ctx->ev_factored) (void)hipEventDestroy(e);
    for (auto e : ctx->ev_swept) (void)hipEventDestroy(e);
    for (auto e : ctx->ev_fwd) (void)hipEventDestroy(e);
    (void)hipStreamDestroy(ctx->stream);
    delete ctx;
    return 0;
}

int qocx_synchronize(qocx_ctx* ctx) {
    if (!ctx) return fail(QOCX_ERR_ARG, "ctx is NULL");
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return 0;
}

int qocx_set_schroedinger_problem(qocx_ctx* ctx, const qocx_schroedinger_problem* p) {
    if (!ctx || !p) return fail(QOCX_ERR_ARG, "NULL argument");
    if (int rc = check_problem(p)) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    // matrices are padded to 16, 32 or 64: one, four or sixteen MFMA tiles (33 <= n <= 64 runs on
    // the four-wave K1a of qocx_pade4.hip and the NB = 4 forms of K1b / K2 / K3)
    // (n > 64: nb = ceil(n / 16) > 4 selects the general path; it reads the row-major padded matrices that
    // the t-images hold - the column-major images of the transposes)
    const int n = p->hilbert_size, N = p->system_eval_count;
    const int nb = (n <= 16) ? 1 : (n <= 32 ? 2 : (n <= 64 ? 4 : (n + 15) / 16));
    ctx->has_problem = false;
    ctx->control_costs.clear();
    ctx->n = n; ctx->nb = nb; ctx->np = 16 * nb; ctx->S = p->state_count; ctx->K = p->control_count;
    ctx->nc = p->control_eval_count; ctx->N = N; ctx->nsteps = N - 1; ctx->ces = p->cost_eval_step;
    ctx->nt = p->nt; ctx->nodes = p->magnus_policy / 2;
    ctx->T = p->evolution_time;
    ctx->dt = p->evolution_time / (N - 1);  // programstate.py:44
    ctx->eff.kind = EffectiveControls::NONE;  // a new problem clears the quadratic terms
    ctx->seeds.clear();                       // ... the ensemble or the sweep, with its duration search
    ctx->ens_qscales_set = false;

    set_hermitian_flags(ctx, p);
    if (int rc = upload_operators(ctx, p)) return rc;
    if (int rc = upload_m4_commutators(ctx, p)) return rc;
    if (int rc = upload_initial_states(ctx, p)) return rc;
    if (int rc = upload_interpolation(ctx, p)) return rc;
    if (int rc = upload_costs(ctx, p)) return rc;
    // More states than the wavefront sweep's LDS holds (33 <= n <= 64: more than 13 - a full propagator there
    // has n): the general path, whose sweep keeps its vectors in HBM, takes the problem where it can
    ctx->general_path = nb > 4 || qocx::sweep_lds_bytes(nb, ctx->S) > 160 * 1024;
    ctx->has_problem = true;
    ctx->have_results = false;
    ctx->B = 0;
    ctx->inj_count = 0;
    return 0;
}

int qocx_set_interpolation_policy(qocx_ctx* ctx, int32_t policy) {
    if (!ctx) return fail(QOCX_ERR_ARG, "ctx is NULL");
    if (policy != QOCX_INTERP_LINEAR && policy != QOCX_INTERP_PIECEWISE_CONSTANT)
        return fail(QOCX_ERR_ARG, "interpolation policy must be QOCX_INTERP_LINEAR or "
                                  "QOCX_INTERP_PIECEWISE_CONSTANT");
    ctx->interp_policy = policy;  // read by the next problem setter
    return 0;
}

int qocx_set_quadratic_terms(qocx_ctx* ctx, int32_t count, const int32_t* pairs, const double* matrices) {
    if (!ctx) return fail(QOCX_ERR_ARG, "ctx is NULL");
    if (!ctx->has_problem) return fail(QOCX_ERR_STATE, "no problem set (qocx_set_schroedinger_problem first)");
    if (count < 0) return fail(QOCX_ERR_ARG, "count must be >= 0");
    HIP_TRY(hipSetDevice(ctx->device));
    if (count == 0) {
        if (ctx->eff.kind == EffectiveControls::QUADRATIC) ctx->eff.kind = EffectiveControls::NONE;
        ctx->ens_qscales_set = false;
        ctx->hermitian = ctx->hermitian_linear;
        ctx->have_results = false;
        ctx->B = 0;  // the norm bound of the uploaded controls no longer applies
        return 0;
    }
    if (!pairs || !matrices) return fail(QOCX_ERR_ARG, "pairs / matrices missing");
    if (ctx->seeds.sweep())
        return fail(QOCX_ERR_STATE, "a sweep is set (qocx_set_sweep): it does not take quadratic terms");
    if (ctx->nodes != 1)
        return fail(QOCX_ERR_ARG, "quadratic terms need magnus_policy M2 (M4 / M6 take the callable's tangent)");
    if (ctx->explicit_mode) return fail(QOCX_ERR_ARG, "quadratic terms do not apply to explicit generators");
    const int n = ctx->n, K = ctx->K, nt = ctx->nt, np = ctx->np;
    if (K < 1) return fail(QOCX_ERR_ARG, "quadratic terms need control_count >= 1");
    // (with an ensemble K = K_r + J: the fixed channels count towards the limit, and the pairs index
    // the seeds' K_r channels - qocx_set_ensemble makes the same check when it comes second)
    if (K + count > 64) return fail(QOCX_ERR_ARG, "control_count + quadratic term count must be <= 64");
    for (int q = 0; q < count; ++q)
        if (pairs[2 * q] < 0 || pairs[2 * q] > pairs[2 * q + 1] || pairs[2 * q + 1] >= K)
            return fail(QOCX_ERR_ARG, "quadratic term pairs must satisfy 0 <= k <= l < control_count");
    if (ctx->seeds.M > 0)
        for (int q = 0; q < count; ++q)
            if (pairs[2 * q + 1] >= ctx->seeds.Kr)
                return fail(QOCX_ERR_ARG, "quadratic term pairs must index the ensemble's seed channels "
                                          "(l < control_count - fixed)");
    const size_t nn = (size_t)n * n, mat = (size_t)np * np;
    const int Ke = K + count;
    // With a time-dependent linear part the K1a / K3 tables are [nt][Ke]: every table entry carries
    // the Q_q again. Three images (one on the general path) of nt * Ke padded matrices: bounded here.
    const size_t images = ctx->general_path ? 1 : 3;
    if ((size_t)nt * Ke * mat * sizeof(double2) * images > ((size_t)4 << 30))
        return fail(QOCX_ERR_CAPACITY, "the augmented operator tables of the quadratic terms would exceed 4 GiB");
    std::vector<double> norms(count);
    bool herm = ctx->hermitian_linear != 0;
    for (int q = 0; q < count; ++q) {
        const double* m = matrices + (size_t)q * nn * 2;
        for (size_t e = 0; e < nn * 2; ++e)
            if (!std::isfinite(m[e])) return fail(QOCX_ERR_ARG, "non-finite quadratic term matrix");
        norms[q] = one_norm(m, n);
        herm = herm && hermitian_bitwise(m, n);
    }
    // augmented images [nt][G_0 .. G_K-1, Q_0 .. Q_count-1], built on the device from the G_k images
    OperatorImages q;
    if (q.build(matrices, (size_t)count, n, ctx->nb, ctx->stream, ctx->general_path)) return QOCX_ERR_HIP;
    const size_t gbytes = (size_t)K * mat * sizeof(double2), qbytes = (size_t)count * mat * sizeof(double2);
    for (int i = ctx->general_path ? 2 : 0; i < 3; ++i) {
        DevBuf<double2>& dst = ctx->eff.images.layout(i);
        if (dst.ensure((size_t)nt * Ke * mat)) return QOCX_ERR_HIP;
        HIP_TRY(hipMemcpy2DAsync(dst.p, gbytes + qbytes, ctx->g.layout(i).p, gbytes, gbytes, nt,
                                 hipMemcpyDeviceToDevice, ctx->stream));
        for (int t = 0; t < nt; ++t)
            HIP_TRY(hipMemcpyAsync(dst.p + ((size_t)t * Ke + K) * mat, q.layout(i).p, qbytes, hipMemcpyDeviceToDevice,
                                   ctx->stream));
    }
    std::vector<int> pr(pairs, pairs + 2 * (size_t)count);
    if (ctx->eff.interp_id.upload(identity_interp(ctx->nsteps), ctx->stream) ||
        ctx->eff.pairs_dev.upload(pr, ctx->stream))
        return QOCX_ERR_HIP;
    HIP_TRY(hipStreamSynchronize(ctx->stream));  // q is released at the end of this scope
    // The matrix-free route (knob "action_eff"; it takes the problem at nt == 1 only): the norms of the G_k as
    // upload_operators left them, those of the Q_q from spectral_bound where ALL operators are Hermitian, and
    // the E image of the G_k followed by that of the Q_q.
    ctx->hermitian = herm ? 1 : 0;  // (effective_operator_tables reads it)
    ctx->eff.op_norm1.assign(Ke, 0.0);
    ctx->eff.op_norm2.assign(Ke, 0.0);
    for (int k = 0; k < K; ++k) {
        ctx->eff.op_norm1[k] = ctx->g_norm_max[k];
        ctx->eff.op_norm2[k] = ctx->g_norm2_max[k];
    }
    if (ctx->nb <= 2 && nt == 1 && ctx->g_eimg.p != nullptr) {
        if (ctx->eff.eimg.ensure((size_t)Ke * mat)) return QOCX_ERR_HIP;
        HIP_TRY(hipMemcpyAsync(ctx->eff.eimg.p, ctx->g_eimg.p, gbytes, hipMemcpyDeviceToDevice, ctx->stream));
    } else {
        ctx->eff.eimg.release();
    }
    if (int rc = effective_operator_tables(ctx, matrices, K, count)) return rc;
    ctx->eff.pairs = pr;
    ctx->eff.norm = norms;
    ctx->eff.kind = EffectiveControls::QUADRATIC;
    ctx->eff.Ke = Ke;
    ctx->ens_qscales_set = false;  // (scales of the previous terms)
    ctx->hermitian = herm ? 1 : 0;
    ctx->have_results = false;
    ctx->B = 0;  // controls must be uploaded again: their norm bound now includes the Q_q
    return 0;
}

// What this path keeps beside seed tables just set: max_r |factor s_rk| and max_r |factor delta_rj| over
// their rows, for the bound qocx_opt_clip commits; and nothing of earlier uploads stands
static void seed_tables_were_set(qocx_ctx* ctx, const std::vector<double>& sc, const std::vector<double>& off,
                                 double factor) {
    const int rows = ctx->seeds.rows(), Kr = ctx->seeds.Kr, J = ctx->seeds.J;
    ctx->ens_scale_max.assign(Kr, 0.0);
    ctx->ens_offset_max.assign(J, 0.0);
    for (int r = 0; r < rows; ++r) {
        for (int k = 0; k < Kr; ++k)
            ctx->ens_scale_max[k] = std::max(ctx->ens_scale_max[k], fabs(factor * sc[(size_t)r * Kr + k]));
        for (int j = 0; j < J; ++j)
            ctx->ens_offset_max[j] = std::max(ctx->ens_offset_max[j], fabs(factor * off[(size_t)r * J + j]));
    }
    ctx->ens_B = 0;
    ctx->ens_stale = false;
    ctx->ens_qscales_set = false;  // (scales of the previous ensemble's members)
    ctx->have_results = false;
    ctx->B = 0;  // controls must be uploaded again (as seed controls: their staging takes the new tables)
    ctx->ms.batch = 0;
}

int qocx_set_ensemble(qocx_ctx* ctx, int32_t members, int32_t fixed, const double* scales,
                      const double* offsets, const double* weights) {
    if (!ctx) return fail(QOCX_ERR_ARG, "ctx is NULL");
    if (!ctx->has_problem) return fail(QOCX_ERR_STATE, "no problem set (qocx_set_schroedinger_problem first)");
    if (ctx->seeds.sweep())
        return fail(QOCX_ERR_STATE, "a sweep is set (qocx_set_sweep): a problem takes a sweep or an ensemble");
    // quadratic terms are products of the seeds' channels (qocx_set_quadratic_terms checks the same
    // when it comes second)
    for (int q = 0; q < ctx->eff.quad_count(); ++q)
        if (ctx->eff.pairs[2 * q + 1] >= ctx->K - fixed)
            return fail(QOCX_ERR_ARG, "quadratic term pairs must index the ensemble's seed channels "
                                      "(l < control_count - fixed)");
    HIP_TRY(hipSetDevice(ctx->device));
    if (int rc = set_seed_tables(ctx->seeds, false, ctx->K, members, fixed, scales, offsets, weights, ctx->stream))
        return rc;
    seed_tables_were_set(ctx, ctx->seeds.scales_h, ctx->seeds.offsets_h, 1.0);
    return 0;
}

int qocx_set_sweep(qocx_ctx* ctx, int32_t seeds, int32_t fixed, const double* scales, const double* offsets) {
    if (!ctx) return fail(QOCX_ERR_ARG, "ctx is NULL");
    if (!ctx->has_problem) return fail(QOCX_ERR_STATE, "no problem set (qocx_set_schroedinger_problem first)");
    if (ctx->seeds.M > 0 && !ctx->seeds.sweep())
        return fail(QOCX_ERR_STATE, "an ensemble is set (qocx_set_ensemble): a problem takes a sweep or an ensemble");
    if (ctx->eff.quad_count() > 0)
        return fail(QOCX_ERR_STATE, "quadratic terms are set (qocx_set_quadratic_terms): a sweep does not take them");
    HIP_TRY(hipSetDevice(ctx->device));
    if (int rc = set_seed_tables(ctx->seeds, true, ctx->K, seeds, fixed, scales, offsets, nullptr, ctx->stream))
        return rc;
    seed_tables_were_set(ctx, ctx->seeds.scales_h, ctx->seeds.offsets_h, 1.0);
    return 0;
}

int qocx_set_ensemble_quadratic_scales(qocx_ctx* ctx, int32_t members, int32_t count, const double* scales) {
    if (!ctx) return fail(QOCX_ERR_ARG, "ctx is NULL");
    if (!ctx->has_problem) return fail(QOCX_ERR_STATE, "no problem set (qocx_set_schroedinger_problem first)");
    if (ctx->seeds.M == 0 || ctx->seeds.swp_B > 0)
        return fail(QOCX_ERR_ARG, "quadratic term scales need an ensemble (qocx_set_ensemble)");
    if (ctx->eff.quad_count() == 0)
        return fail(QOCX_ERR_ARG, "quadratic term scales need quadratic terms (qocx_set_quadratic_terms)");
    if (members != ctx->seeds.M) return fail(QOCX_ERR_ARG, "members does not match the ensemble's");
    if (count != ctx->eff.quad_count()) return fail(QOCX_ERR_ARG, "count does not match the quadratic terms'");
    if (!scales) {
        ctx->ens_qscales_set = false;
    } else {
        std::vector<double> c(scales, scales + (size_t)members * count), cmax(count, 0.0);
        for (int m = 0; m < members; ++m)
            for (int q = 0; q < count; ++q) {
                const double v = c[(size_t)m * count + q];
                if (!std::isfinite(v)) return fail(QOCX_ERR_ARG, "non-finite quadratic term scale");
                cmax[q] = std::max(cmax[q], fabs(v));
            }
        HIP_TRY(hipSetDevice(ctx->device));
        if (ctx->ens_qscales.upload(c, ctx->stream)) return QOCX_ERR_HIP;
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        ctx->ens_qscale_max = cmax;
        ctx->ens_qscales_set = true;
    }
    ctx->have_results = false;
    ctx->B = 0;  // controls must be uploaded again: their norm bound includes the scales
    ctx->ms.batch = 0;
    return 0;
}

}  // extern "C"

namespace qocx::host {

// 1-norm bound of the step generator from the bound b >= ||dt a(t)|| of its node generators
// (mathmethods.py:96-164: m2 = b; m4 = dt/2 (a1 + a2) + sqrt(3)/12 dt^2 [a2, a1]; m6)
// max over the Pade orders of eps_m(theta) = sum_{j>=1} (b_j / b_0) theta^j (qocx_lu5.h)
double pade_eps_max(double theta) {
    const double b3[] = {120.0, 60.0, 12.0, 1.0};
    const double b5[] = {30240.0, 15120.0, 3360.0, 420.0, 30.0, 1.0};
    const double b7[] = {17297280.0, 8648640.0, 1995840.0, 277200.0, 25200.0, 1512.0, 56.0, 1.0};
    const double b9[] = {17643225600.0, 8821612800.0, 2075673600.0, 302702400.0, 30270240.0, 2162160.0,
                         110880.0, 3960.0, 90.0, 1.0};
    const double b13[] = {64764752532480000.0, 32382376266240000.0, 7771770303897600.0, 1187353796428800.0,
                          129060195264000.0, 10559470521600.0, 670442572800.0, 33522128640.0, 1323241920.0,
                          40840800.0, 960960.0, 16380.0, 182.0, 1.0};
    const double* tabs[] = {b3, b5, b7, b9, b13};
    const int orders[] = {3, 5, 7, 9, 13};
    if (!(theta >= 0.0) || !(theta < 1e300)) return 1e300;
    double worst = 0.0;
    for (int t = 0; t < 5; ++t) {
        double eps = 0.0, tp = 1.0;
        for (int j = 1; j <= orders[t]; ++j) {
            tp *= theta;
            eps += tabs[t][j] / tabs[t][0] * tp;
        }
        worst = std::max(worst, eps);
    }
    return worst;
}

double magnus_norm_bound(int nodes, double bound) {
    if (nodes == 2) return bound + (std::sqrt(3.0) / 12) * 2 * bound * bound;
    if (nodes == 3) {
        const double b1 = bound, b2 = (std::sqrt(15.0) / 3) * 2 * bound, b3 = (10.0 / 3) * 4 * bound;
        const double c12 = 2 * b1 * b2, x = 20 * b1 + b3 + c12, w = 2 * b3 + c12;
        const double y = b2 + (1.0 / 60) * 2 * b1 * w;
        return b1 + 0.5 * b3 + (1.0 / 240) * 2 * x * y;
    }
    return bound;
}

// sum_q ||Q_q||_1 umax[k_q] umax[l_q]: with umax[k] >= max_t |r_k(t)|, a bound of the quadratic
// terms' share of ||H(t)||_1 at every time, between knots included.
// With an ensemble umax are bounds of the SEEDS' channels and the bound is that of the expanded
// items: sum_q ||Q_q||_1 max_m |c_mq| (max_m |s_m,kq| umax[k_q]) (max_m |s_m,lq| umax[l_q]) - the
// product of the maxima over the members, not the (tighter) maximum over the members of the
// product: it needs no pass over the members per upload and can only cost a squaring, not digits.
double quad_bound(const qocx_ctx* ctx, const double* umax) {
    double b = 0.0;
    if (ctx->effctl_kind(false) != EffectiveControls::QUADRATIC) return b;
    const EffectiveControls& eff = ctx->eff;
    const bool ens = ctx->seeds.M > 0;
    for (int q = 0; q < eff.quad_count(); ++q) {
        const int k = eff.pairs[2 * q], l = eff.pairs[2 * q + 1];
        if (!ens) {
            b += eff.norm[q] * fabs(umax[k]) * fabs(umax[l]);
            continue;
        }
        const double c = ctx->ens_qscales_set ? ctx->ens_qscale_max[q] : 1.0;
        b += eff.norm[q] * c * (ctx->ens_scale_max[k] * fabs(umax[k])) * (ctx->ens_scale_max[l] * fabs(umax[l]));
    }
    return b;
}

// The seed-level view: with an ensemble the entry points of the host's optimizer loop (costs,
// gradients, qocx_opt_*) act on the seeds and their K_r channels, else on the items themselves.
int seed_count(const qocx_ctx* ctx) { return ctx->seeds.M > 0 ? ctx->ens_B : ctx->B; }
int seed_channels(const qocx_ctx* ctx) { return ctx->seeds.M > 0 ? ctx->seeds.Kr : ctx->K; }
double* seed_controls(qocx_ctx* ctx) { return ctx->seeds.M > 0 ? ctx->ens_controls.p : ctx->controls.p; }
double* seed_costs(qocx_ctx* ctx) { return ctx->seeds.M > 0 ? ctx->ens_cost.p : ctx->cost_out.p; }
double* seed_grads(qocx_ctx* ctx) { return ctx->seeds.M > 0 ? ctx->ens_grads.p : ctx->grads.p; }

}  // namespace qocx::host

namespace {

// max over `rows` rows of [rows][K] controls of |r_k|, per k (NaN propagates)
std::vector<double> quad_control_max(const double* rows_p, size_t rows, int K) {
    std::vector<double> m(K, 0.0);
    for (size_t row = 0; row < rows; ++row)
        for (int k = 0; k < K; ++k) {
            const double a = fabs(rows_p[row * K + k]);
            if (!(a <= m[k])) m[k] = a;
        }
    return m;
}

}  // namespace

// ---- Hamiltonian ensembles and sweeps: what both paths do with a SeedTables (qocx_host.h) -----------

namespace qocx::host {

int set_seed_tables(SeedTables& s, bool sweep, int K, int rows, int fixed, const double* scales,
                    const double* offsets, const double* weights, hipStream_t st) {
    const std::string kind = sweep ? "sweep" : "ensemble";
    if (sweep && rows < 1) return fail(QOCX_ERR_ARG, "sweep seeds must be >= 1");
    if (!sweep && (rows < 1 || rows > 1024)) return fail(QOCX_ERR_ARG, "ensemble members must be 1 .. 1024");
    if (fixed < 0) return fail(QOCX_ERR_ARG, "fixed channel count must be >= 0");
    if (fixed >= K)
        return fail(QOCX_ERR_ARG,
                    (sweep ? "a " : "an ") + kind + " needs fixed < control_count (at least one seed control)");
    if (fixed > 0 && !offsets) return fail(QOCX_ERR_ARG, "fixed channels need offsets");
    if (fixed == 0 && offsets) return fail(QOCX_ERR_ARG, "offsets need fixed >= 1 channels");
    if (!sweep && !weights) return fail(QOCX_ERR_ARG, "weights missing");
    const int J = fixed, Kr = K - fixed;
    std::vector<double> sc((size_t)rows * Kr, 1.0), off((size_t)rows * J), w;
    if (scales) sc.assign(scales, scales + sc.size());
    if (J > 0) off.assign(offsets, offsets + off.size());
    if (!sweep) w.assign(weights, weights + rows);
    for (double v : sc)
        if (!std::isfinite(v)) return fail(QOCX_ERR_ARG, "non-finite " + kind + " control scale");
    for (double v : off)
        if (!std::isfinite(v)) return fail(QOCX_ERR_ARG, "non-finite " + kind + " offset");
    for (double v : w)
        if (!std::isfinite(v) || !(v >= 0)) return fail(QOCX_ERR_ARG, "ensemble weights must be finite and >= 0");
    if (s.scales.upload(sc, st) || (!sweep && s.weights.upload(w, st)) || (J > 0 && s.offsets.upload(off, st)))
        return QOCX_ERR_HIP;
    HIP_TRY(hipStreamSynchronize(st));  // sc, off, w are local
    s.scales_h.swap(sc);
    s.offsets_h.swap(off);
    s.M = sweep ? 1 : rows;
    s.J = J;
    s.Kr = Kr;
    s.swp_B = sweep ? rows : 0;
    s.dur.clear();  // (a new sweep: no duration search)
    return 0;
}

int set_seed_durations(SeedTables& s, const double* tau, const double* base_scales, const double* base_offsets,
                       double tau_min, double tau_max, double time_weight, hipStream_t st, std::vector<double>& s0,
                       std::vector<double>& d0) {
    const int B = s.swp_B, Kr = s.Kr, J = s.J;
    if (J < 1 || !base_offsets)
        return fail(QOCX_ERR_ARG, "a duration search needs the drift as the first fixed channel (base_offsets [B][J], J >= 1)");
    if (!std::isfinite(tau_min) || !std::isfinite(tau_max) || !(tau_min > 0) || !(tau_min <= tau_max))
        return fail(QOCX_ERR_ARG, "the duration box needs finite 0 < tau_min <= tau_max");
    if (!std::isfinite(time_weight) || time_weight < 0)
        return fail(QOCX_ERR_ARG, "time_weight must be finite and >= 0");
    std::vector<double> t(tau, tau + B);
    s0.assign((size_t)B * Kr, 1.0);
    d0.assign(base_offsets, base_offsets + (size_t)B * J);
    if (base_scales) s0.assign(base_scales, base_scales + s0.size());
    for (double v : t)
        if (!std::isfinite(v)) return fail(QOCX_ERR_ARG, "non-finite duration");
    for (double v : s0)
        if (!std::isfinite(v)) return fail(QOCX_ERR_ARG, "non-finite base control scale");
    for (double v : d0)
        if (!std::isfinite(v)) return fail(QOCX_ERR_ARG, "non-finite base offset");
    if (s.dur.tau.upload(t, st) || s.dur.base_scales.upload(s0, st) || s.dur.base_offsets.upload(d0, st) ||
        s.scales.ensure(s0.size()) || s.offsets.ensure(d0.size()))
        return QOCX_ERR_HIP;
    s.dur.tau_min = tau_min; s.dur.tau_max = tau_max; s.dur.weight = time_weight;
    return 0;
}

int download_seed_durations(const SeedTables& s, hipStream_t st, bool gradient_stands, double* tau_out,
                            double* tau_grad_out) {
    if (tau_grad_out && !gradient_stands)
        return fail(QOCX_ERR_STATE, "duration gradients need an evaluation with gradients");
    const size_t bytes = (size_t)s.swp_B * sizeof(double);
    if (tau_out) HIP_TRY(hipMemcpyAsync(tau_out, s.dur.tau.p, bytes, hipMemcpyDeviceToHost, st));
    if (tau_grad_out) HIP_TRY(hipMemcpyAsync(tau_grad_out, s.dur.grad.p, bytes, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

qocx::EnsembleArgs ensemble_args(const SeedTables& s, int seeds, int nc, const SeedBuffers& b) {
    qocx::EnsembleArgs a;
    a.seed_controls = b.seed_controls; a.scales = s.scales.p;
    a.offsets = s.J > 0 ? s.offsets.p : nullptr; a.weights = s.weights.p;
    a.controls = b.items;
    a.member_cost = b.item_cost; a.member_grads = b.item_grads;
    a.cost = b.cost; a.grads = b.grads;
    a.B = seeds; a.M = s.M; a.nc = nc; a.K = s.Kr + s.J; a.Kr = s.Kr; a.J = s.J;
    return a;
}

qocx::SystemSweepArgs sweep_args(const SeedTables& s, int nc, const SeedBuffers& b) {
    qocx::SystemSweepArgs a;
    a.seed_controls = b.seed_controls; a.scales = s.scales.p;
    a.offsets = s.J > 0 ? s.offsets.p : nullptr;
    a.controls = b.items;
    a.item_cost = b.item_cost; a.item_grads = b.item_grads;
    a.cost = b.cost; a.grads = b.grads;
    a.scale_sens = s.scale_sens.p; a.offset_sens = s.offset_sens.p;
    a.B = s.swp_B; a.nc = nc; a.K = s.Kr + s.J; a.Kr = s.Kr; a.J = s.J;
    return a;
}

qocx::DurationArgs duration_args(const SeedTables& s, double* tau_grad, double* cost) {
    qocx::DurationArgs a;
    a.tau = s.dur.tau.p;
    a.base_scales = s.dur.base_scales.p; a.base_offsets = s.dur.base_offsets.p;  // (J >= 1)
    a.scales = s.scales.p; a.offsets = s.offsets.p;
    a.scale_sens = s.scale_sens.p; a.offset_sens = s.offset_sens.p;
    a.tau_grad = tau_grad;
    a.cost = cost;
    a.tau_min = s.dur.tau_min; a.tau_max = s.dur.tau_max; a.time_weight = s.dur.weight;
    a.B = s.swp_B; a.Kr = s.Kr; a.J = s.J;
    return a;
}

}  // namespace qocx::host

namespace {

SeedBuffers seed_buffers(qocx_ctx* ctx) {
    return {ctx->ens_controls.p, ctx->controls.p, ctx->cost_out.p, ctx->grads.p, ctx->ens_cost.p, ctx->ens_grads.p};
}
qocx::SystemSweepArgs sweep_args(qocx_ctx* ctx) {
    return qocx::host::sweep_args(ctx->seeds, ctx->nc, seed_buffers(ctx));
}

// The seeds' controls into the pinned staging buffer, and the bounds qocx_upload_controls takes from
// a control array: here those of the expanded [B][M][nc][K] array - the same per-row sum in the same
// order over the items' rows (s_rk u_bjk for k < K_r, delta_rj beyond; r = m of an ensemble, b of a
// sweep), so they equal bit for bit what an upload of the expanded array gives, and a sweep's item b
// takes the Pade orders, squarings and kernel variants of the plain problem.
void seeds_stage(const qocx_ctx* ctx, int batch, const double* controls, double* stage, double& smax, double& smid) {
    const SeedTables& t = ctx->seeds;
    const int M = t.M, Kr = t.Kr, J = t.J, nc = ctx->nc;
    const double* gn = ctx->g_norm_max.data();
    memcpy(stage, controls, (size_t)batch * nc * Kr * sizeof(double));
    double sprev = 0.0;
    for (int b = 0; b < batch; ++b)
        for (int m = 0; m < M; ++m) {
            const size_t r = t.sweep() ? b : m;
            const double* s = t.scales_h.data() + r * Kr;
            const double* d = t.offsets_h.data() + r * J;
            for (int j = 0; j < nc; ++j) {
                const double* u = controls + ((size_t)b * nc + j) * Kr;
                double srow = 0.0;
                for (int k = 0; k < Kr; ++k) srow += fabs(s[k] * u[k]) * gn[k];
                for (int k = 0; k < J; ++k) srow += fabs(d[k]) * gn[Kr + k];
                if (!(srow <= smax)) smax = srow;  // also catches NaN
                if (j != 0) {
                    const double mid = 0.5 * (sprev + srow);
                    if (!(mid <= smid)) smid = mid;
                }
                sprev = srow;
            }
        }
}

// expand the seeds' controls into the member items of ctx->controls (a sweep: into its B items)
int ensemble_expand(qocx_ctx* ctx, int seeds) {
    if (ctx->seeds.sweep()) qocx::launch_sweep_expand(sweep_args(ctx), ctx->stream);
    else qocx::launch_ensemble_expand(ensemble_args(ctx->seeds, seeds, ctx->nc, seed_buffers(ctx)), ctx->stream);
    HIP_TRY(hipGetLastError());
    ctx->ens_stale = false;
    return 0;
}

// the staged seed controls to the device, expanded there
int ensemble_upload(qocx_ctx* ctx, int batch, const double* stage) {
    const size_t seeds = (size_t)batch * ctx->nc * ctx->seeds.Kr;
    const size_t items = (size_t)batch * ctx->seeds.M * ctx->nc * ctx->K;
    if ((items + 255) / 256 > 0x7fffffffu) return fail(QOCX_ERR_ARG, "ensemble control arrays too large");
    if (ctx->ens_controls.ensure(seeds) || ctx->controls.ensure(items)) return QOCX_ERR_HIP;
    HIP_TRY(hipMemcpyAsync(ctx->ens_controls.p, stage, seeds * sizeof(double), hipMemcpyHostToDevice,
                           ctx->stream));
    return ensemble_expand(ctx, batch);
}

// A duration search's tables as the device holds them, into seeds.scales_h / seeds.offsets_h
int sweep_mirror_tables(qocx_ctx* ctx) {
    SeedTables& t = ctx->seeds;
    const size_t ns = (size_t)t.swp_B * t.Kr, no = (size_t)t.swp_B * t.J;
    t.scales_h.resize(ns);
    t.offsets_h.resize(no);
    HIP_TRY(hipMemcpyAsync(t.scales_h.data(), t.scales.p, ns * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (no > 0)
        HIP_TRY(hipMemcpyAsync(t.offsets_h.data(), t.offsets.p, no * sizeof(double), hipMemcpyDeviceToHost,
                               ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    t.dur.mirror_stale = false;
    return 0;
}

// The tail of an evaluation of a duration search: dE_b/dtau_b + time_weight from the sensitivities
// (with gradients), and time_weight tau_b onto the seed costs - after every other term of the cost
int duration_finish(qocx_ctx* ctx) {
    SeedTables& t = ctx->seeds;
    if (!t.dur.set) return 0;
    const size_t B = (size_t)t.swp_B;
    if (t.dur.grad.ensure(B) || t.scale_sens.ensure(B * t.Kr) || t.offset_sens.ensure(B * t.J)) return QOCX_ERR_HIP;
    if (ctx->have_grads) qocx::launch_sweep_sensitivity(sweep_args(ctx), ctx->stream);
    qocx::launch_duration_gradient(duration_args(t, ctx->have_grads ? t.dur.grad.p : nullptr, ctx->ens_cost.p),
                                   ctx->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    t.dur.have_grad = ctx->have_grads;
    return 0;
}

}  // namespace

extern "C" {

int qocx_upload_controls(qocx_ctx* ctx, int32_t batch, const double* controls) {
    if (!ctx) return fail(QOCX_ERR_ARG, "ctx is NULL");
    if (!ctx->has_problem) return fail(QOCX_ERR_STATE, "no problem set");
    if (batch < 1) return fail(QOCX_ERR_ARG, "batch must be >= 1");
    HIP_TRY(hipSetDevice(ctx->device));
    const bool ens = ctx->seeds.M > 0;
    if (ctx->seeds.swp_B > 0 && batch != ctx->seeds.swp_B)
        return fail(QOCX_ERR_ARG, "a sweep takes exactly its own seed count as the batch (qocx_set_sweep)");
    if (ens && (int64_t)batch * ctx->seeds.M > 0x7fffffff)
        return fail(QOCX_ERR_ARG, "seeds x ensemble members must fit in int32");
    // (with an ensemble the caller's array holds the seeds' K_r channels)
    const size_t per = (size_t)ctx->nc * (ens ? ctx->seeds.Kr : ctx->K);
    double bound = ctx->h0_norm_max;
    double bound2 = 1e300, bound2_mid = 1e300;  // of ||step generator||_2, where formed below
    if (ctx->K > 0) {
        if (!controls) return fail(QOCX_ERR_ARG, "controls is NULL");
        // One pass over the caller's array: the per-control maxima for the squaring bound, and a
        // copy into a pinned staging buffer the DMA engine reads without a driver-side bounce
        // (4 MB of pageable memory: 0.71 -> 0.27 ms per call at the headline size). The
        // copy is stream-ordered before the kernels of qocx_eval_resident; the staging buffer is
        // only rewritten by the next call, after that evaluation has been synchronised.
        const size_t total = (size_t)batch * per;
        if (ctx->pin_controls_cap < total) {
            if (ctx->pin_controls) (void)hipHostFree(ctx->pin_controls);
            ctx->pin_controls = nullptr;
            ctx->pin_controls_cap = 0;
            HIP_TRY(hipHostMalloc((void**)&ctx->pin_controls, total * sizeof(double), hipHostMallocDefault));
            ctx->pin_controls_cap = total;
        }
        HIP_TRY(hipStreamSynchronize(ctx->stream));  // nothing in flight still reads the staging buffer
        const int K = ctx->K;
        // sum_k |u_k(t)| ||G_k||_1 is largest at a control knot (u is linear between knots, the sum
        // convex): the largest knot sum bounds every step, every Magnus node, and the device's
        // per-step bound (launch_step_table) - tighter than sum_k max_t |u_k(t)| ||G_k||_1
        // (s2*: the same sums with the spectral-norm bounds, for the Taylor buffers of the matrix-free route;
        // an ensemble or sweep forms none and sizes them from the 1-norm)
        double smax = 0.0, smid = 0.0, sprev = 0.0;
        double s2max = 0.0, s2mid = 0.0, s2prev = 0.0;
        double* stage = ctx->pin_controls;
        if (ctx->seeds.dur.mirror_stale)  // (a duration search whose tables qocx_opt_clip has rewritten since)
            if (int rc = sweep_mirror_tables(ctx)) return rc;
        if (ens) seeds_stage(ctx, batch, controls, stage, smax, smid);
        for (size_t row = 0; !ens && row < (size_t)batch * ctx->nc; ++row) {
            const double* src = controls + row * K;
            double* dst = stage + row * K;
            double srow = 0.0, s2row = 0.0;
            for (int k = 0; k < K; ++k) {
                const double v = src[k];
                dst[k] = v;
                srow += fabs(v) * ctx->g_norm_max[k];
                s2row += fabs(v) * ctx->g_norm2_max[k];
            }
            if (!(srow <= smax)) smax = srow;  // also catches NaN
            if (!(s2row <= s2max)) s2max = s2row;
            // midpoint of two knots of the same seed: |u_mid| <= (|u_j| + |u_j+1|) / 2
            if (row % (size_t)ctx->nc != 0) {
                const double m = 0.5 * (sprev + srow), m2 = 0.5 * (s2prev + s2row);
                if (!(m <= smid)) smid = m;
                if (!(m2 <= s2mid)) s2mid = m2;
            }
            sprev = srow;
            s2prev = s2row;
        }
        // (piecewise constant: a step reads ONE slice, never the mean of two rows - the knot sums
        // above are then exact for every step and the midpoint bound does not apply)
        const bool mid_applies = ctx->nodes == 1 && ctx->nc == ctx->nsteps + 1 && ctx->eff.quad_count() == 0 && !ctx->pwc;
        if (mid_applies)
            ctx->norm_bound_mid = (bound + smid) * fabs(ctx->dt) * (1.0 + 1e-12);
        else
            ctx->norm_bound_mid = 1e300;
        // (the plain M2 problem alone: a problem on effective controls - knob "action_eff" - sizes its Taylor
        // buffers from the 1-norm bound, norm2_bound stays at 1e300)
        if (!ens && ctx->nodes == 1 && ctx->eff.quad_count() == 0) {
            bound2 = (ctx->h0_norm2_max + s2max) * fabs(ctx->dt);
            if (mid_applies) bound2_mid = (ctx->h0_norm2_max + s2mid) * fabs(ctx->dt) * (1.0 + 1e-12);
        }
        bound += smax;
        // Quadratic terms: r_k(t) r_l(t) is not convex between knots (r_k 0 -> a, r_l a -> 0 peaks at
        // a^2 / 4 mid-interval), so the knot sums above do not bound it. |r_k(t)| <= max over the knots of
        // |r_k| does hold everywhere (linear interpolation): ||Q_q||_1 max|r_k| max|r_l| bounds every step.
        // (with an ensemble the staging buffer holds the seeds' K_r channels, unscaled: quad_bound
        // applies the members' scales)
        if (ctx->eff.quad_count() > 0)
            bound += quad_bound(ctx, quad_control_max(stage, (size_t)batch * ctx->nc, ens ? ctx->seeds.Kr : K).data());
        if (ens) {
            if (int rc = ensemble_upload(ctx, batch, stage)) return rc;
        } else {
            if (ctx->controls.ensure(total)) return QOCX_ERR_HIP;
            HIP_TRY(hipMemcpyAsync(ctx->controls.p, stage, total * sizeof(double), hipMemcpyHostToDevice,
                                   ctx->stream));
        }
    }
    bound = magnus_norm_bound(ctx->nodes, bound * fabs(ctx->dt));
    if (!(bound < 1e300)) return fail(QOCX_ERR_ARG, "non-finite controls or Hamiltonian");
    if (!(bound2 < 1e300)) bound2 = bound2_mid = 1e300;
    if (int rc = commit_step_bound(ctx, bound, false, "bound needs", bound2)) return rc;
    ctx->norm2_bound_mid = bound2_mid;
    ctx->B = ens ? batch * ctx->seeds.M : batch;
    ctx->ens_B = ens ? batch : 0;
    ctx->have_results = false;
    ctx->explicit_mode = false;
    return 0;
}

int qocx_upload_generators(qocx_ctx* ctx, int32_t batch, const double* generators) {
    if (!ctx || !generators) return fail(QOCX_ERR_ARG, "NULL argument");
    if (!ctx->has_problem) return fail(QOCX_ERR_STATE, "no problem set");
    if (batch < 1) return fail(QOCX_ERR_ARG, "batch must be >= 1");
    if (ctx->K != 0 || ctx->nodes != 1)
        return fail(QOCX_ERR_STATE, "explicit generators need a problem with control_count = 0 and "
                                    "magnus_policy M2");
    HIP_TRY(hipSetDevice(ctx->device));
    const int n = ctx->n, np = ctx->np, nsteps = ctx->nsteps;
    const size_t count = (size_t)batch * nsteps, mat = (size_t)np * np;
    std::vector<double2> padded(count * mat, make_double2(0, 0));
    double worst = 0;
    bool skew = true;
    for (size_t m = 0; m < count; ++m) {
        const double* g = generators + m * (size_t)n * n * 2;
        double norm1 = 0;
        for (int c = 0; c < n; ++c) {
            double col = 0;
            for (int r = 0; r < n; ++r) {
                const double re = g[2 * ((size_t)r * n + c)], im = g[2 * ((size_t)r * n + c) + 1];
                col += std::hypot(re, im);
                padded[m * mat + (size_t)r * np + c] = make_double2(re, im);
                // skew-Hermitian bit for bit: a[r][c] == -conj(a[c][r])
                if (re != -g[2 * ((size_t)c * n + r)] || im != g[2 * ((size_t)c * n + r) + 1])
                    skew = false;
            }
            if (!(col <= norm1)) norm1 = col;
        }
        if (!(norm1 <= worst)) worst = norm1;
    }
    if (!(worst < 1e300)) return fail(QOCX_ERR_ARG, "non-finite generator");
    ctx->norm_bound_mid = 1e300;
    if (int rc = commit_step_bound(ctx, worst, false, "needs")) return rc;
    if (ctx->gen_rm.upload(padded, ctx->stream)) return QOCX_ERR_HIP;
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    ctx->B = batch;
    ctx->have_results = false;
    ctx->explicit_mode = true;
    ctx->explicit_hermitian = skew ? 1 : 0;
    return 0;
}

int qocx_download_generator_cotangents(qocx_ctx* ctx, double* out) {
    if (!ctx || !out) return fail(QOCX_ERR_ARG, "NULL argument");
    if (!ctx->have_results || !ctx->have_grads || !ctx->explicit_mode)
        return fail(QOCX_ERR_STATE, "no generator cotangents (qocx_upload_generators + "
                                    "qocx_eval_resident(want_grad = 1) first)");
    HIP_TRY(hipSetDevice(ctx->device));
    const int n = ctx->n, np = ctx->np;
    const size_t count = (size_t)ctx->B * ctx->nsteps, mat = (size_t)np * np;
    std::vector<double2> padded(count * mat);
    HIP_TRY(hipMemcpy(padded.data(), ctx->genbar_rm.p, padded.size() * sizeof(double2),
                      hipMemcpyDeviceToHost));
    for (size_t m = 0; m < count; ++m)
        for (int r = 0; r < n; ++r)
            for (int c = 0; c < n; ++c) {
                out[2 * ((m * n + r) * n + c)] = padded[m * mat + (size_t)r * np + c].x;
                out[2 * ((m * n + r) * n + c) + 1] = padded[m * mat + (size_t)r * np + c].y;
            }
    return 0;
}

int qocx_set_state_cotangents(qocx_ctx* ctx, int32_t batch, int32_t count, const int32_t* steps,
                              const double* bars) {
    if (!ctx) return fail(QOCX_ERR_ARG, "ctx is NULL");
    if (!ctx->has_problem) return fail(QOCX_ERR_STATE, "no problem set");
    if (count <= 0) {
        ctx->inj_count = 0;
        return 0;
    }
    if (batch < 1 || !steps || !bars) return fail(QOCX_ERR_ARG, "bad argument");
    HIP_TRY(hipSetDevice(ctx->device));
    const int n = ctx->n, np = ctx->np, S = ctx->S, nsteps = ctx->nsteps;
    std::vector<int> index(nsteps + 1, -1);
    for (int c = 0; c < count; ++c) {
        if (steps[c] < 1 || steps[c] > nsteps || index[steps[c]] >= 0)
            return fail(QOCX_ERR_ARG, "cotangent steps must be distinct and in 1..N-1");
        index[steps[c]] = c;
    }
    std::vector<double2> padded((size_t)batch * count * S * np, make_double2(0, 0));
    for (size_t v = 0; v < (size_t)batch * count * S; ++v)
        for (int i = 0; i < n; ++i)
            padded[v * np + i] = make_double2(bars[2 * (v * n + i)], bars[2 * (v * n + i) + 1]);
    if (ctx->inj_index.upload(index, ctx->stream) || ctx->inj_bars.upload(padded, ctx->stream))
        return QOCX_ERR_HIP;
    ctx->inj_count = count;
    ctx->inj_batch = batch;
    return 0;
}

int qocx_set_chunk(qocx_ctx* ctx, int32_t seeds_per_chunk) {
    if (!ctx) return fail(QOCX_ERR_ARG, "ctx is NULL");
    ctx->chunk_user = seeds_per_chunk < 0 ? 0 : seeds_per_chunk;
    return 0;
}

int qocx_set_pipeline(qocx_ctx* ctx, int32_t time_segments) {
    if (!ctx) return fail(QOCX_ERR_ARG, "ctx is NULL");
    ctx->pipe_user = time_segments < 0 ? 0 : time_segments;
    return 0;
}

int qocx_set_keep_step_states(qocx_ctx* ctx, int32_t keep) {
    if (!ctx) return fail(QOCX_ERR_ARG, "ctx is NULL");
    ctx->keep_step_states = keep ? 1 : 0;
    return 0;
}

// The evaluation of the seeds of the uploaded controls, without the costs of the controls alone
static int eval_seeds(qocx_ctx* ctx, int32_t want_grad) {
    if (ctx->seeds.M == 0) return eval_items(ctx, want_grad);
    // ensemble: the member items of the seeds' current controls, evaluated as any batch, then
    // reduced to seed costs and gradients
    if (!ctx->has_problem || ctx->B < 1) return fail(QOCX_ERR_STATE, "no problem / controls");
    HIP_TRY(hipSetDevice(ctx->device));
    const int seeds = ctx->ens_B;
    if (ctx->ens_stale)
        if (int rc = ensemble_expand(ctx, seeds)) return rc;
    if (int rc = eval_items(ctx, want_grad)) return rc;
    if (ctx->ens_cost.ensure((size_t)seeds) ||
        (ctx->have_grads && ctx->ens_grads.ensure((size_t)seeds * ctx->nc * ctx->seeds.Kr)))
        return QOCX_ERR_HIP;
    SeedBuffers buf = seed_buffers(ctx);
    if (!ctx->have_grads) buf.grads = nullptr;
    if (ctx->seeds.sweep()) qocx::launch_sweep_reduce(sweep_args(ctx->seeds, ctx->nc, buf), ctx->stream);
    else qocx::launch_ensemble_reduce(ensemble_args(ctx->seeds, seeds, ctx->nc, buf), ctx->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return 0;
}

int qocx_eval_resident(qocx_ctx* ctx, int32_t want_grad) {
    if (!ctx) return fail(QOCX_ERR_ARG, "ctx is NULL");
    if (int rc = eval_seeds(ctx, want_grad)) return rc;
    ControlCosts& cc = ctx->control_costs;
    if (cc.count == 0) return duration_finish(ctx);
    // the costs of the controls, once per seed on the controls that were evaluated (ensemble: the
    // seed's own, unscaled), added to the seed's cost and gradient
    const int seeds = seed_count(ctx);
    if (int rc = run_control_costs(ctx, cc, seeds, ctx->nc, seed_channels(ctx), seed_controls(ctx), ctx->have_grads))
        return rc;
    qocx::launch_add_control_costs(seed_costs(ctx), cc.cost.p, ctx->have_grads ? seed_grads(ctx) : nullptr,
                                   cc.grad.p, seeds, (size_t)ctx->nc * seed_channels(ctx), ctx->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return duration_finish(ctx);  // (the price of time comes after the costs of the controls)
}

int qocx_download_results(qocx_ctx* ctx, double* cost_out, double* grad_out, double* final_out) {
    if (!ctx) return fail(QOCX_ERR_ARG, "ctx is NULL");
    if (!ctx->have_results) return fail(QOCX_ERR_STATE, "no evaluation results");
    HIP_TRY(hipSetDevice(ctx->device));
    // (costs and gradients of the seeds, final states of every item: [B][M][S][n] with an ensemble)
    const int B = ctx->B, np = ctx->np, S = ctx->S, n = ctx->n, seeds = seed_count(ctx);
    if (cost_out)
        HIP_TRY(hipMemcpyAsync(cost_out, seed_costs(ctx), (size_t)seeds * sizeof(double),
                               hipMemcpyDeviceToHost, ctx->stream));
    if (grad_out) {
        if (!ctx->have_grads) return fail(QOCX_ERR_STATE, "gradients were not computed");
        HIP_TRY(hipMemcpyAsync(grad_out, seed_grads(ctx),
                               (size_t)seeds * ctx->nc * seed_channels(ctx) * sizeof(double),
                               hipMemcpyDeviceToHost, ctx->stream));
    }
    std::vector<double2> fin;
    if (final_out) {
        fin.resize((size_t)B * S * np);
        HIP_TRY(hipMemcpyAsync(fin.data(), ctx->final_out.p, fin.size() * sizeof(double2),
                               hipMemcpyDeviceToHost, ctx->stream));
    }
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (final_out)
        for (size_t v = 0; v < (size_t)B * S; ++v)
            for (int i = 0; i < n; ++i) {
                final_out[2 * (v * n + i)] = fin[v * np + i].x;
                final_out[2 * (v * n + i) + 1] = fin[v * np + i].y;
            }
    return 0;
}

int qocx_download_step_states(qocx_ctx* ctx, double* states_out) {
    if (!ctx || !states_out) return fail(QOCX_ERR_ARG, "NULL argument");
    if (!ctx->have_results || !ctx->have_step_states)
        return fail(QOCX_ERR_STATE, "step states were not kept (qocx_set_keep_step_states)");
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t nvec = (size_t)ctx->B * (ctx->nsteps + 1) * ctx->S;
    std::vector<double2> tmp(nvec * ctx->np);
    HIP_TRY(hipMemcpy(tmp.data(), ctx->step_states.p, tmp.size() * sizeof(double2),
                      hipMemcpyDeviceToHost));
    for (size_t v = 0; v < nvec; ++v)
        for (int i = 0; i < ctx->n; ++i) {
            states_out[2 * (v * ctx->n + i)] = tmp[v * ctx->np + i].x;
            states_out[2 * (v * ctx->n + i) + 1] = tmp[v * ctx->np + i].y;
        }
    return 0;
}

int qocx_eval_schroedinger(qocx_ctx* ctx, int32_t batch, const double* controls, int32_t want_grad,
                           double* cost_out, double* grad_out, double* final_out) {
    int rc = qocx_upload_controls(ctx, batch, controls);
    if (rc) return rc;
    rc = eval_seeds(ctx, want_grad);  // (host buffers in and out: without qocx_set_control_costs' terms)
    if (rc) return rc;
    if ((rc = duration_finish(ctx))) return rc;
    return qocx_download_results(ctx, cost_out, (want_grad && ctx->K > 0) ? grad_out : nullptr,
                                 final_out);
}

int qocx_set_timing(qocx_ctx* ctx, int32_t enable) {
    if (!ctx) return fail(QOCX_ERR_ARG, "ctx is NULL");
    if (enable < 0 || enable > 8) return fail(QOCX_ERR_ARG, "timing mode must be 0, 1 or 2 + kernel index");
    ctx->timing = enable;
    ctx->time_active = false;
    return 0;
}

int qocx_get_timing(qocx_ctx* ctx, int32_t which, int64_t* launches, double* total_ms) {
    if (!ctx || which < 0 || which > 6) return fail(QOCX_ERR_ARG, "bad argument");
    if (launches) *launches = ctx->t_launch[which];
    if (total_ms) *total_ms = ctx->t_ms[which];
    return 0;
}

int qocx_reset_timing(qocx_ctx* ctx) {
    if (!ctx) return fail(QOCX_ERR_ARG, "ctx is NULL");
    for (int i = 0; i < 7; ++i) {
        ctx->t_launch[i] = 0;
        ctx->t_ms[i] = 0;
    }
    return 0;
}

// Knobs: the variant switches every build accepts (each of them selects between paths that give
// the same numbers to rounding) and the diagnostic ones that exist in libqocx_diag.so only
// (qocx_diag.h): timing experiments that return garbage and the stamped kernel builds.
static const char* const kVariantKnobs[] = {
    "sweep_impl", "sweep_one", "sweep_dense", "sweep_inverse", "sweep_inverse_small", "sweep_umode", "bidir",
    "unit_adjoint", "latency", "fuse_lu", "lu_inverse", "lu_mfma", "lu_dpp", "pack8", "m4_linear", "magnus_4w",
    "pade_order", "k1a_three", "k1a_four", "k1a_share", "k1a_herm4", "general_split", "general_skew",
    "lindblad_two_sided", "lindblad_side_limit", "lindblad_q2", "lindblad_chain", "lindblad_real_ops", "lindblad_4t",
    "lindblad_hermitian", "lindblad_pad_operator", "lindblad_wide", "action", "action_states", "action_costs",
    "action_degree", "action_plan", "action_small", "action_eff", "action_eff_exact"};
static const char* const kDiagKnobs[] = {"dbg_skip", "sweep3_dbg", "sweep3_stamps", "lindblad_stamps",
                                         "k1a_stamps", "k1a_dbg", "peak_mode"};

int qocx_knob_kind(const char* name) {
    if (!name) return 0;
    for (const char* k : kVariantKnobs)
        if (strcmp(k, name) == 0) return 1;
    for (const char* k : kDiagKnobs)
        if (strcmp(k, name) == 0) return qocx::kDiagBuild ? 2 : -2;
    return 0;
}

int qocx_build_is_diag(void) { return qocx::kDiagBuild ? 1 : 0; }

int qocx_debug_set_knob(qocx_ctx* ctx, const char* name, int64_t value) {
    if (!ctx || !name) return fail(QOCX_ERR_ARG, "NULL argument");
    const int kind = qocx_knob_kind(name);
    if (kind > 0) {
        if (strcmp(name, "action_states") == 0 && value != 0 && (value < 2 || value > QOCX_ACTION_MAX_STATES))
            return fail(QOCX_ERR_ARG, "action_states must be 0 or 2 .. 4 (QOCX_ACTION_MAX_STATES)");
        for (const char* k : {"action_costs", "action_degree", "action_plan", "action_small", "action_eff", "action_eff_exact"})
            if (strcmp(name, k) == 0 && value != 0 && value != 1)
                return fail(QOCX_ERR_ARG, std::string(k) + " must be 0 or 1");
        ctx->knobs[name] = value;
        return 0;
    }
    if (kind == -2)
        return fail(QOCX_ERR_ARG, std::string("diagnostic knob '") + name +
                                      "' exists in libqocx_diag.so only (make diag, -DQOCX_DIAG)");
    return fail(QOCX_ERR_ARG, std::string("unknown knob: ") + name);
}

// ---- RCCL --------------------------------------------------------------------------------

int qocx_comm_unique_id(uint8_t* id128) {
    if (!id128) return fail(QOCX_ERR_ARG, "id128 is NULL");
    qocx_ctx tmp;
    int rc = load_rccl(&tmp);
    if (rc) return rc;
    int e = tmp.rccl.GetUniqueId((void*)id128);
    if (e != 0) return fail(QOCX_ERR_RCCL, "ncclGetUniqueId failed");
    return 0;
}

int qocx_comm_init(qocx_ctx* ctx, const uint8_t* id128, int32_t rank, int32_t world) {
    if (!ctx || !id128) return fail(QOCX_ERR_ARG, "NULL argument");
    HIP_TRY(hipSetDevice(ctx->device));
    int rc = load_rccl(ctx);
    if (rc) return rc;
    // ncclCommInitRank(ncclComm_t*, int nranks, ncclUniqueId id (by value), int rank)
    typedef int (*init_fn)(void**, int, ncclUniqueIdBytes, int);
    init_fn f = (init_fn)dlsym(ctx->rccl.lib, "ncclCommInitRank");
    ncclUniqueIdBytes uid;
    memcpy(uid.internal, id128, 128);
    if (world < 1 || rank < 0 || rank >= world) return fail(QOCX_ERR_ARG, "rank / world out of range");
    if (!f) return fail(QOCX_ERR_RCCL, "librccl has no ncclCommInitRank");
    if (getenv("QOCX_RCCL_DEBUG")) {  // (a log line only: what this rank hands to ncclCommInitRank)
        unsigned long long sum = 1469598103934665603ull;  // FNV-1a of the id: equal on every rank
        for (int i = 0; i < 128; ++i) sum = (sum ^ id128[i]) * 1099511628211ull;
        char bus[64] = "?";
        (void)hipDeviceGetPCIBusId(bus, sizeof(bus), ctx->device);
        int version = 0;
        typedef int (*ver_fn)(int*);
        if (ver_fn v = (ver_fn)dlsym(ctx->rccl.lib, "ncclGetVersion")) (void)v(&version);
        const char* ipc = getenv("HSA_ENABLE_IPC_MODE_LEGACY");
        fprintf(stderr, "[qocx rccl] ncclCommInitRank rank=%d world=%d hip_device=%d pci=%s id_fnv=%016llx "
                        "rccl_version=%d HSA_ENABLE_IPC_MODE_LEGACY=%s pid=%d\n",
                rank, world, ctx->device, bus, sum, version, ipc ? ipc : "(unset)", (int)getpid());
        fflush(stderr);
    }
    int e = f(&ctx->comm, world, uid, rank);
    if (e != 0)
        return fail(QOCX_ERR_RCCL, std::string("ncclCommInitRank: ") +
                                       (ctx->rccl.GetErrorString ? ctx->rccl.GetErrorString(e) : "?"));
    return 0;
}

static int comm_allreduce(qocx_ctx* ctx, double* buf, int64_t count, int op) {
    if (!ctx || !buf || count < 1) return fail(QOCX_ERR_ARG, "bad argument");
    if (!ctx->comm) return fail(QOCX_ERR_STATE, "communicator not initialised");
    HIP_TRY(hipSetDevice(ctx->device));
    if (ctx->comm_buf.ensure((size_t)count)) return QOCX_ERR_HIP;
    HIP_TRY(hipMemcpyAsync(ctx->comm_buf.p, buf, count * sizeof(double), hipMemcpyHostToDevice,
                           ctx->stream));
    // ncclFloat64 = 8 ; ncclSum = 0, ncclMax = 2
    int e = ctx->rccl.AllReduce(ctx->comm_buf.p, ctx->comm_buf.p, (size_t)count, 8, op, ctx->comm,
                                ctx->stream);
    if (e != 0)
        return fail(QOCX_ERR_RCCL, std::string("ncclAllReduce: ") +
                                       (ctx->rccl.GetErrorString ? ctx->rccl.GetErrorString(e) : "?"));
    HIP_TRY(hipMemcpyAsync(buf, ctx->comm_buf.p, count * sizeof(double), hipMemcpyDeviceToHost,
                           ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return 0;
}

int qocx_download_costs(qocx_ctx* ctx, double* cost_out) {
    if (!ctx || !cost_out) return fail(QOCX_ERR_ARG, "NULL argument");
    if (!ctx->have_results) return fail(QOCX_ERR_STATE, "no evaluation results");
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipMemcpyAsync(cost_out, seed_costs(ctx), (size_t)seed_count(ctx) * sizeof(double),
                           hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return 0;
}

int qocx_ensemble_download_members(qocx_ctx* ctx, double* cost_out) {
    if (!ctx || !cost_out) return fail(QOCX_ERR_ARG, "NULL argument");
    if (ctx->seeds.M == 0 || ctx->seeds.swp_B > 0) return fail(QOCX_ERR_STATE, "no ensemble set (qocx_set_ensemble)");
    if (!ctx->have_results) return fail(QOCX_ERR_STATE, "no evaluation results");
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipMemcpyAsync(cost_out, ctx->cost_out.p, (size_t)ctx->B * sizeof(double),
                           hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return 0;
}

int qocx_sweep_download_sensitivities(qocx_ctx* ctx, double* scales_out, double* offsets_out) {
    if (!ctx) return fail(QOCX_ERR_ARG, "ctx is NULL");
    if (ctx->seeds.swp_B == 0) return fail(QOCX_ERR_STATE, "no sweep set (qocx_set_sweep)");
    // (the seed controls on the device are those of the evaluation exactly while its results stand:
    // qocx_opt_clip / _step and an upload clear have_results)
    if (!ctx->have_results || !ctx->have_grads || ctx->ens_stale)
        return fail(QOCX_ERR_STATE, "sweep sensitivities need an evaluation with gradients");
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t ns = (size_t)ctx->seeds.swp_B * ctx->seeds.Kr, no = (size_t)ctx->seeds.swp_B * ctx->seeds.J;
    if (ctx->seeds.scale_sens.ensure(ns) || ctx->seeds.offset_sens.ensure(no)) return QOCX_ERR_HIP;
    qocx::launch_sweep_sensitivity(sweep_args(ctx), ctx->stream);
    HIP_TRY(hipGetLastError());
    if (scales_out)
        HIP_TRY(hipMemcpyAsync(scales_out, ctx->seeds.scale_sens.p, ns * sizeof(double), hipMemcpyDeviceToHost,
                               ctx->stream));
    if (offsets_out && no > 0)
        HIP_TRY(hipMemcpyAsync(offsets_out, ctx->seeds.offset_sens.p, no * sizeof(double), hipMemcpyDeviceToHost,
                               ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return 0;
}

int qocx_sweep_set_durations(qocx_ctx* ctx, const double* tau, const double* base_scales,
                             const double* base_offsets, double tau_min, double tau_max, double time_weight) {
    if (!ctx || !tau) return fail(QOCX_ERR_ARG, "NULL argument");
    if (!ctx->seeds.sweep()) return fail(QOCX_ERR_STATE, "no sweep set (qocx_set_sweep before qocx_sweep_set_durations)");
    HIP_TRY(hipSetDevice(ctx->device));
    std::vector<double> s0, d0;
    if (int rc = set_seed_durations(ctx->seeds, tau, base_scales, base_offsets, tau_min, tau_max, time_weight,
                                    ctx->stream, s0, d0))
        return rc;
    qocx::launch_duration_tables(duration_args(ctx->seeds, nullptr, nullptr), ctx->stream);
    HIP_TRY(hipGetLastError());
    if (int rc = sweep_mirror_tables(ctx)) return rc;
    // the bound qocx_opt_clip commits must hold for every tau the optimizer can reach: tau_max
    seed_tables_were_set(ctx, s0, d0, tau_max);
    ctx->seeds.dur.set = true;
    ctx->seeds.dur.have_grad = false;
    return 0;
}

int qocx_sweep_download_durations(qocx_ctx* ctx, double* tau_out, double* tau_grad_out) {
    if (!ctx) return fail(QOCX_ERR_ARG, "ctx is NULL");
    if (!ctx->seeds.dur.set) return fail(QOCX_ERR_STATE, "no durations set (qocx_sweep_set_durations)");
    HIP_TRY(hipSetDevice(ctx->device));
    const bool stands = ctx->have_results && ctx->have_grads && !ctx->ens_stale && ctx->seeds.dur.have_grad;
    return download_seed_durations(ctx->seeds, ctx->stream, stands, tau_out, tau_grad_out);
}

int qocx_reduce_results(qocx_ctx* ctx, int32_t allreduce, double* out, int64_t count) {
    if (!ctx || !out) return fail(QOCX_ERR_ARG, "NULL argument");
    if (!ctx->have_results) return fail(QOCX_ERR_STATE, "no evaluation results");
    if (allreduce && !ctx->comm) return fail(QOCX_ERR_STATE, "communicator not initialised");
    const int per_seed = count > 1 ? ctx->nc * seed_channels(ctx) : 0;  // count == 1: the cost only
    if (count != 1 + per_seed || (per_seed > 0 && !ctx->have_grads))
        return fail(QOCX_ERR_ARG, "count must be 1, or 1 + control_eval_count * control_count after "
                                  "an evaluation with gradients");
    HIP_TRY(hipSetDevice(ctx->device));
    if (ctx->comm_buf.ensure((size_t)count)) return QOCX_ERR_HIP;
    qocx::launch_reduce_results(seed_costs(ctx), seed_grads(ctx), seed_count(ctx), per_seed, ctx->comm_buf.p,
                                ctx->stream);
    if (allreduce) {  // ncclFloat64 = 8 ; ncclSum = 0
        int e = ctx->rccl.AllReduce(ctx->comm_buf.p, ctx->comm_buf.p, (size_t)count, 8, 0, ctx->comm,
                                    ctx->stream);
        if (e != 0)
            return fail(QOCX_ERR_RCCL, std::string("ncclAllReduce: ") +
                                           (ctx->rccl.GetErrorString ? ctx->rccl.GetErrorString(e) : "?"));
    }
    HIP_TRY(hipMemcpyAsync(out, ctx->comm_buf.p, count * sizeof(double), hipMemcpyDeviceToHost,
                           ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return 0;
}

int qocx_comm_allreduce_sum(qocx_ctx* ctx, double* buf_host, int64_t count) {
    return comm_allreduce(ctx, buf_host, count, 0);
}

int qocx_comm_allreduce_max(qocx_ctx* ctx, double* buf_host, int64_t count) {
    return comm_allreduce(ctx, buf_host, count, 2);
}

int qocx_comm_barrier(qocx_ctx* ctx) {
    double one = 1.0;
    return comm_allreduce(ctx, &one, 1, 0);
}

int qocx_comm_destroy(qocx_ctx* ctx) {
    if (!ctx) return 0;
    if (ctx->comm && ctx->rccl.CommDestroy) ctx->rccl.CommDestroy(ctx->comm);
    ctx->comm = nullptr;
    return 0;
}

}  // extern "C"
