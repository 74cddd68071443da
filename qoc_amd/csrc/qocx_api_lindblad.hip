// qocx_api_lindblad.hip - the Lindblad path of the C ABI (include/qocx.h): problem upload,
// sub-interval grids and sub-division planning, the evaluation from host buffers and the resident one
// of the multi-start driver, density cotangents and the downloads.
#include <time.h>

#include "dop853_tableau.h"
#include "qocx_host.h"

namespace {

// Largest singular value of a complex n x n matrix (row-major, interleaved), for the step-size
// rule of the Lindblad integrator: power iteration on A^H A from a fixed start vector, stopped at
// 1e-4 relative change; the estimate comes from below, so 2 % are added, and it never exceeds the
// rigorous bound sqrt(||A||_1 ||A||_inf). (The 1-norm used before over-estimates the 2-norm of a
// dense Hermitian matrix by 2-3x, i.e. made the integrator take 2-3x more sub-intervals than the
// same threshold on the operator norm asks for.)
double two_norm(const double* m, int n) {
    double n1 = one_norm(m, n), ninf = 0;
    for (int r = 0; r < n; ++r) {
        double sum = 0;
        for (int c = 0; c < n; ++c) sum += hypot(m[2 * ((size_t)r * n + c)], m[2 * ((size_t)r * n + c) + 1]);
        ninf = std::max(ninf, sum);
    }
    const double upper = std::sqrt(n1 * ninf);
    if (!(upper > 0) || !(upper < 1e300)) return upper;
    std::vector<double> v(2 * n), w(2 * n);
    double nv = 0;
    for (int i = 0; i < n; ++i) {
        v[2 * i] = 1.0 + 0.37 * i / n;
        v[2 * i + 1] = 0.11 * ((i * 7) % 5);
        nv += v[2 * i] * v[2 * i] + v[2 * i + 1] * v[2 * i + 1];
    }
    nv = std::sqrt(nv);
    for (auto& e : v) e /= nv;
    double sigma = 0, prev = -1;
    for (int it = 0; it < 200; ++it) {
        double nw = 0;
        for (int r = 0; r < n; ++r) {  // w = A v
            double re = 0, im = 0;
            for (int c = 0; c < n; ++c) {
                const double ar = m[2 * ((size_t)r * n + c)], ai = m[2 * ((size_t)r * n + c) + 1];
                re += ar * v[2 * c] - ai * v[2 * c + 1];
                im += ar * v[2 * c + 1] + ai * v[2 * c];
            }
            w[2 * r] = re; w[2 * r + 1] = im;
            nw += re * re + im * im;
        }
        sigma = std::sqrt(nw);  // ||A v||, ||v|| = 1
        if (!(sigma > 0)) break;
        if (it >= 6 && std::fabs(sigma - prev) <= 1e-4 * sigma) break;
        prev = sigma;
        double nn = 0;
        for (int c = 0; c < n; ++c) {  // v = A^H w, normalised
            double re = 0, im = 0;
            for (int r = 0; r < n; ++r) {
                const double ar = m[2 * ((size_t)r * n + c)], ai = m[2 * ((size_t)r * n + c) + 1];
                re += ar * w[2 * r] + ai * w[2 * r + 1];
                im += ar * w[2 * r + 1] - ai * w[2 * r];
            }
            v[2 * c] = re; v[2 * c + 1] = im;
            nn += re * re + im * im;
        }
        nn = std::sqrt(nn);
        if (!(nn > 0)) break;
        for (auto& e : v) e /= nn;
    }
    return std::min(1.02 * sigma, upper);
}

// C-layout dump of an n x n matrix padded to 16 nb: reg r of tile (ti, tj) of lane l <-> element
// (row 16 ti + 4 r + (l >> 4), col 16 tj + (l & 15)), index ((ti nb + tj) 4 + r) 64 + l
// (33 <= n <= 64: the 64 x 64 images of qocx_lindblad16t.hip)
int dump_tiles(int n) { return n <= 16 ? 1 : (n <= 32 ? 2 : 4); }

// f(dump index, row-major element index) for every element of the matrix; f(dump index, -1) for the padding
template <typename F>
void walk_c_dump(int n, F f) {
    const int nb = dump_tiles(n);
    for (int ti = 0; ti < nb; ++ti)
        for (int tj = 0; tj < nb; ++tj)
            for (int r = 0; r < 4; ++r)
                for (int lane = 0; lane < 64; ++lane) {
                    const int row = 16 * ti + 4 * r + (lane >> 4), col = 16 * tj + (lane & 15);
                    f(((ti * nb + tj) * 4 + r) * 64 + lane, (row < n && col < n) ? row * n + col : -1);
                }
}

}  // namespace

namespace qocx::host {

int dump_elems(int n) { return 256 * dump_tiles(n) * dump_tiles(n); }

void from_c_dump(const double2* d, int n, double* out) {
    walk_c_dump(n, [&](int at, int e) {
        if (e >= 0) { out[2 * e] = d[at].x; out[2 * e + 1] = d[at].y; }
    });
}

}  // namespace qocx::host

extern "C" {

// ---- Lindblad ----------------------------------------------------------------------------

extern "C++" {
namespace {

typedef std::vector<double> cmat;  // row-major n x n complex, interleaved

cmat cm_zero(int n) { return cmat((size_t)2 * n * n, 0.0); }

cmat cm_from(const double* p, int n) { return cmat(p, p + (size_t)2 * n * n); }

// M = M^H to rounding: max |M - M^H| <= 64 eps max |M|
bool cm_is_hermitian(const cmat& a, int n) {
    double big = 0, diff = 0;
    for (int r = 0; r < n; ++r)
        for (int c = 0; c <= r; ++c) {
            const double xr = a[2 * ((size_t)r * n + c)], xi = a[2 * ((size_t)r * n + c) + 1];
            const double yr = a[2 * ((size_t)c * n + r)], yi = a[2 * ((size_t)c * n + r) + 1];
            big = std::max(big, std::max(fabs(xr), fabs(xi)));
            diff = std::max(diff, std::max(fabs(xr - yr), fabs(xi + yi)));
        }
    return diff <= 1.5e-14 * big;
}

cmat cm_transpose(const cmat& a, int n, double imag_sign = 1.0) {
    cmat o = cm_zero(n);
    for (int r = 0; r < n; ++r)
        for (int c = 0; c < n; ++c) {
            o[2 * ((size_t)c * n + r)] = a[2 * ((size_t)r * n + c)];
            o[2 * ((size_t)c * n + r) + 1] = imag_sign * a[2 * ((size_t)r * n + c) + 1];
        }
    return o;
}

cmat cm_adjoint(const cmat& a, int n) { return cm_transpose(a, n, -1.0); }

cmat cm_mul(const cmat& a, const cmat& b, int n) {
    cmat o = cm_zero(n);
    for (int r = 0; r < n; ++r)
        for (int k = 0; k < n; ++k) {
            const double ar = a[2 * ((size_t)r * n + k)], ai = a[2 * ((size_t)r * n + k) + 1];
            for (int c = 0; c < n; ++c) {
                const double br = b[2 * ((size_t)k * n + c)], bi = b[2 * ((size_t)k * n + c) + 1];
                o[2 * ((size_t)r * n + c)] += ar * br - ai * bi;
                o[2 * ((size_t)r * n + c) + 1] += ar * bi + ai * br;
            }
        }
    return o;
}

// o = alpha * a (alpha complex)
cmat cm_scale(const cmat& a, double sr, double si) {
    cmat o(a.size());
    for (size_t e = 0; e < a.size(); e += 2) {
        o[e] = sr * a[e] - si * a[e + 1];
        o[e + 1] = sr * a[e + 1] + si * a[e];
    }
    return o;
}

void cm_axpy(cmat& y, double alpha, const cmat& x) {
    for (size_t e = 0; e < y.size(); ++e) y[e] += alpha * x[e];
}

void c_dump(const cmat& m, int n, double2* out) {
    walk_c_dump(n, [&](int at, int e) { out[at] = e >= 0 ? make_double2(m[2 * e], m[2 * e + 1]) : make_double2(0, 0); });
}

// Spectral norm of the control-free Liouvillian X -> A_L X + X A_R + sum_i gamma_i L_i X L_i^H as
// an operator on C^(n x n) (Frobenius inner product): matrix-free power iteration on its
// adjoint-times-itself, stopped at 1e-4 relative change, + 2 % (the estimate comes from below).
// The sum of the parts' bounds (2 ||H0||_2 + 2 sum gamma ||L||_2^2) over-estimates it 2-3x when
// the dissipators are stiff in a few levels only (a^H a of a 16-level oscillator), and the
// integrator's sub-division count is proportional to this number.
double liouvillian_norm(const cmat& al, const cmat& ar, const std::vector<cmat>& ops,
                        const std::vector<double>& gammas, int n) {
    const cmat alh = cm_adjoint(al, n), arh = cm_adjoint(ar, n);
    std::vector<cmat> opsh;
    for (const auto& o : ops) opsh.push_back(cm_adjoint(o, n));
    auto apply = [&](const cmat& x, bool adjoint) {
        cmat y = cm_mul(adjoint ? alh : al, x, n);
        cm_axpy(y, 1.0, cm_mul(x, adjoint ? arh : ar, n));
        for (size_t i = 0; i < ops.size(); ++i)
            cm_axpy(y, gammas[i], adjoint ? cm_mul(cm_mul(opsh[i], x, n), ops[i], n)
                                          : cm_mul(cm_mul(ops[i], x, n), opsh[i], n));
        return y;
    };
    auto fro = [](const cmat& x) {
        double s = 0;
        for (double e : x) s += e * e;
        return std::sqrt(s);
    };
    cmat x((size_t)2 * n * n);
    for (int r = 0; r < n; ++r)
        for (int c = 0; c < n; ++c) {
            x[2 * ((size_t)r * n + c)] = 1.0 / (1.0 + r + c) + (r == c ? 1.0 : 0.0);
            x[2 * ((size_t)r * n + c) + 1] = 0.3 * ((3 * r + c) % 4) - 0.4;
        }
    double nx = fro(x);
    for (auto& e : x) e /= nx;
    double sigma = 0, prev = -1;
    for (int it = 0; it < 400; ++it) {
        const cmat y = apply(x, false);
        sigma = fro(y);
        if (!(sigma > 0) || !(sigma < 1e300)) break;
        if (it >= 8 && std::fabs(sigma - prev) <= 1e-4 * sigma) break;
        prev = sigma;
        x = apply(y, true);
        nx = fro(x);
        if (!(nx > 0)) break;
        for (auto& e : x) e /= nx;
    }
    return 1.02 * sigma;
}

int upload_dumps(DevBuf<double2>& dst, const std::vector<cmat>& mats, int n, hipStream_t st) {
    const size_t md = dump_elems(n);
    std::vector<double2> img(mats.size() * md);
    for (size_t i = 0; i < mats.size(); ++i) c_dump(mats[i], n, img.data() + i * md);
    return dst.upload(img, st);
}

// The control-free part of a static problem as a function of (H0, L_i, gamma_i): A0L = -i H0 - decay / 2,
// A0R = +i H0 - decay / 2 with decay = sum_i gamma_i L_i^H L_i (mathmethods.py:188, :200-203), and the two
// bounds the sub-division rule reads. `ops` / `gammas` may end in the zero operator of pad_op; the first
// `L` are the problem's own. op_norms: ||L_i||_2 of those. The plain problem calls this once, per-member
// rates (qocx_lindblad_set_ensemble_rates) once per member: a member's generators and bounds are those of
// the plain problem with its rates, bit for bit.
struct ControlFree {
    cmat a0l, a0r, decay;
    double diss_norm = 0, l0_norm = 0;
};

ControlFree control_free_part(const cmat& h0, double h0_norm, const std::vector<cmat>& ops,
                              const std::vector<double>& gammas, const std::vector<double>& op_norms, int L,
                              int n) {
    ControlFree cf;
    cf.decay = cm_zero(n);
    for (int i = 0; i < L; ++i) {
        cm_axpy(cf.decay, gammas[i], cm_mul(cm_adjoint(ops[i], n), ops[i], n));
        // || rho -> gamma (L rho L^H - {L^H L, rho} / 2) || <= 2 gamma ||L||_2^2 (the factor 2 is
        // applied where the bound is formed)
        cf.diss_norm += fabs(gammas[i]) * op_norms[i] * op_norms[i];
    }
    cf.a0l = cm_scale(h0, 0.0, -1.0);
    cf.a0r = cm_scale(h0, 0.0, 1.0);
    cm_axpy(cf.a0l, -0.5, cf.decay);
    cm_axpy(cf.a0r, -0.5, cf.decay);
    // static problem: the control-free Liouvillian as a whole (never above the sum of the parts)
    cf.l0_norm = std::min(liouvillian_norm(cf.a0l, cf.a0r, ops, gammas, n), 2 * h0_norm + 2 * cf.diss_norm);
    if (!(cf.l0_norm < 1e300)) cf.l0_norm = 2 * h0_norm + 2 * cf.diss_norm;
    return cf;
}

// What the kernel of 33 <= n <= 64 does not serve, by name: every such feature has kernels of its own at n <= 32
std::string wide_only(const char* what) {
    return std::string(what) + " are not available at hilbert_size > 32: the kernel of 33 <= n <= 64 evaluates static "
           "problems in the classic launch only (knob lindblad_wide)";
}

// qocx_set_lindblad_problem by stage. First every refusal that reads the description alone: it runs before
// any state of the context is touched, so an argument fault leaves the previous problem in place
// (`wide`: the knob lindblad_wide - 33 <= n <= 64 on the kernel of qocx_lindblad16t.hip, static problems only)
int check_lindblad_problem(const qocx_lindblad_problem* p, bool wide) {
    const int n = p->hilbert_size, S = p->density_count, K = p->control_count;
    const int N = p->system_eval_count, nc = p->control_eval_count, L = p->operator_count;
    if (wide && n > 64)
        return fail(QOCX_ERR_ARG, "hilbert_size must be in 1..64 for the Lindblad engine (knob lindblad_wide = 1)");
    if (n < 1 || (n > 32 && !wide)) return fail(QOCX_ERR_ARG, "hilbert_size must be in 1..32 for the Lindblad engine");
    if (n > 32 && (p->fixed_subdivision > 0 || p->h0_stages != nullptr || p->op_stages != nullptr ||
                   p->g_stages != nullptr || p->diss_stages != nullptr))
        return fail(QOCX_ERR_ARG, wide_only("stage tables (fixed_subdivision > 0, h0_stages, g_stages, op_stages)"));
    if (S < 1 || S > 64) return fail(QOCX_ERR_ARG, "density_count must be in 1..64");
    if (K < 0 || K > QOCX_LINDBLAD_MAX_K) return fail(QOCX_ERR_ARG, "control_count must be in 0..8");
    // (1..4 operators: the several-wave / tile-per-wave stage loops; 5..8: the one-wave kernels, whose stage
    // loop walks any number of operators)
    if (L < 0 || L > 8) return fail(QOCX_ERR_ARG, "operator_count must be in 0..8");
    if (N < 2) return fail(QOCX_ERR_ARG, "system_eval_count must be >= 2");
    if (K > 0 && nc < 2) return fail(QOCX_ERR_ARG, "control_eval_count must be >= 2");
    if (p->cost_eval_step < 1) return fail(QOCX_ERR_ARG, "cost_eval_step must be >= 1");
    if (!p->initial_densities || (K > 0 && !p->g) || (L > 0 && (!p->operators || !p->dissipators)))
        return fail(QOCX_ERR_ARG, "missing problem arrays");
    const int scratch = (n > 16 || qocx::lindblad_lds_size(n, S, L, 0, K) > 160 * 1024) ? 1 : 0;  // (lindblad_form)
    if (qocx::lindblad_lds_size(n, S, L, scratch, K) > 160 * 1024)
        return fail(QOCX_ERR_ARG, "too many operators for the kernel's LDS");
    if ((p->op_stages != nullptr) != (p->diss_stages != nullptr))
        return fail(QOCX_ERR_ARG, "diss_stages and op_stages go together");
    if (p->op_stages != nullptr && L > 0 && p->fixed_subdivision <= 0)
        return fail(QOCX_ERR_ARG, "time-dependent lindblad_data needs fixed_subdivision > 0");
    if (p->fixed_subdivision > 0 && !p->h0_stages) return fail(QOCX_ERR_ARG, "h0_stages missing");
    for (int ci = 0; ci < p->cost_count; ++ci) {
        const qocx_cost_desc& c = p->costs[ci];
        if (!c.vectors) return fail(QOCX_ERR_ARG, "cost matrices missing");
        if (c.kind == QOCX_COST_FORBID_DENSITY) {
            if (!c.counts) return fail(QOCX_ERR_ARG, "forbid counts missing");
            for (int s = 0; s < S; ++s)
                if (c.counts[s] < 1) return fail(QOCX_ERR_ARG, "forbid count < 1");
        } else if (c.kind != QOCX_COST_TARGET_DENSITY) {
            return fail(QOCX_ERR_ARG, "cost kind not valid for the Lindblad path");
        }
    }
    return 0;
}

// What the route reads, from the context (the only place the Lindblad knobs are read): the problem as it is
// set, the evaluation, the knobs
// (a knob is an int64: saturated, no comparison of the decision changes)
qocx::LindbladFacts lindblad_facts(const qocx_ctx* ctx, int want_grad) {
    const auto& lb = ctx->lb;
    const auto knob = [ctx](const char* name, int64_t dflt) {
        return (int)std::min<int64_t>(std::max<int64_t>(ctx->knob(name, dflt), INT32_MIN), INT32_MAX);
    };
    qocx::LindbladFacts f{};
    f.n = lb.n; f.S = lb.S; f.K = lb.K; f.nops = lb.nops;
    f.stage_tables = lb.fixed_ksub > 0;
    f.g_tables = f.stage_tables && lb.gp_tab.p != nullptr; f.op_tables = f.stage_tables && lb.op_tab.p != nullptr;
    f.hermitian = lb.hermitian; f.ops_real = lb.ops_real; f.unit_ok = lb.unit_ok; f.inj_count = lb.inj_count;
    f.want_grad = want_grad != 0;
    f.rates = lb.ens_rates;
    // (a duration search asks for the rate sensitivities in every evaluation with gradients: dE/dtau needs its
    // rate part)
    f.sweep = lb.seeds.swp_B > 0; f.want_rate_sens = lb.swp_want_rates || lb.seeds.dur.set;
    f.side_streams = (int)ctx->sweep_streams.size(); f.cu_count = ctx->cu_count; f.dbg_wave_mode = lb.dbg_wave_mode;
    f.lindblad_4t = knob("lindblad_4t", 1); f.lindblad_two_sided = knob("lindblad_two_sided", 1);
    f.lindblad_hermitian = knob("lindblad_hermitian", 1); f.lindblad_q2 = knob("lindblad_q2", 1);
    f.lindblad_chain = knob("lindblad_chain", 1); f.lindblad_real_ops = knob("lindblad_real_ops", 1);
    f.lindblad_pad_operator = knob("lindblad_pad_operator", 1);
    f.lindblad_side_limit = knob("lindblad_side_limit", ctx->cu_count / 2);
    f.lindblad_stamps = knob("lindblad_stamps", 0);
    f.single_wave = qocx::diag_getenv("QOCX_LINDBLAD_SINGLE_WAVE") != nullptr;
    return f;
}

// The launch form of the problem: where its densities live, and how many waves work on a seed
// (lb holds the sizes of `p` already, its tables not yet: those facts come from the description)
void choose_launch_form(qocx_ctx* ctx, const qocx_lindblad_problem* p) {
    auto& lb = ctx->lb;
    qocx::LindbladFacts f = lindblad_facts(ctx, 0);
    f.stage_tables = p->fixed_subdivision > 0;
    f.g_tables = p->g_stages != nullptr; f.op_tables = p->op_stages != nullptr;
    lb.form = qocx::lindblad_form(
        f, [&](int mode, int nops) { return qocx::lindblad_lds_size(lb.n, lb.S, nops, mode, lb.K); });
}

// The control-free part (host copies, norm bounds) and the images of G_k; `decay`: sum gamma_i L_i^H L_i
int upload_static_part(qocx_ctx* ctx, const qocx_lindblad_problem* p, cmat& decay, bool& hermitian) {
    auto& lb = ctx->lb;
    const int n = lb.n, K = lb.K, L = lb.nops;
    const cmat h0 = p->h0 ? cm_from(p->h0, n) : cm_zero(n);
    std::vector<cmat> ops;
    std::vector<double> gammas(L), op_norms(L);
    for (int i = 0; i < L; ++i) {
        ops.push_back(cm_from(p->operators + (size_t)i * n * n * 2, n));
        gammas[i] = p->dissipators[i];
        op_norms[i] = two_norm(ops[i].data(), n);
    }
    if (lb.form.pad_op) {
        ops.push_back(cm_zero(n));
        gammas.push_back(0.0);
    }
    lb.ops_real = p->op_stages == nullptr;
    for (const cmat& op : ops)
        for (size_t e = 0; e < (size_t)n * n; ++e)
            if (op[2 * e + 1] != 0.0) lb.ops_real = false;
    lb.h0_norm = two_norm(h0.data(), n);
    const ControlFree cf = control_free_part(h0, lb.h0_norm, ops, gammas, op_norms, L, n);
    decay = cf.decay; lb.diss_norm = cf.diss_norm; lb.l0_norm = cf.l0_norm;
    hermitian = cm_is_hermitian(h0, n) && cm_is_hermitian(decay, n);
    // (kept for qocx_lindblad_set_ensemble_rates, which builds the members' control-free parts from them)
    lb.h0_h = h0; lb.ops_h = ops; lb.gammas_h = gammas; lb.op_norms_h = op_norms;
    std::vector<cmat> gp, gpd, gpt;
    lb.g_norm.assign(K, 0.0);
    for (int k = 0; k < K; ++k) {
        const cmat gk = cm_from(p->g + (size_t)k * n * n * 2, n);
        lb.g_norm[k] = two_norm(gk.data(), n);
        hermitian = hermitian && cm_is_hermitian(gk, n);
        gp.push_back(cm_scale(gk, 0.0, -1.0));  // Gp = -i G
        gpd.push_back(cm_adjoint(gp.back(), n));
        gpt.push_back(cm_transpose(gp.back(), n));
    }
    // (n > 32: the operators are left and right operands read from memory, so L_i^H is dumped behind them)
    std::vector<cmat> ops_both = ops;
    for (size_t i = 0; n > 32 && i < ops.size(); ++i) ops_both.push_back(cm_adjoint(ops[i], n));
    if (upload_dumps(lb.a0l, {cf.a0l}, n, ctx->stream) || upload_dumps(lb.a0r, {cf.a0r}, n, ctx->stream) ||
        upload_dumps(lb.a0ld, {cm_adjoint(cf.a0l, n)}, n, ctx->stream) ||
        upload_dumps(lb.a0rd, {cm_adjoint(cf.a0r, n)}, n, ctx->stream) ||
        upload_dumps(lb.gp, gp, n, ctx->stream) || upload_dumps(lb.gpd, gpd, n, ctx->stream) ||
        upload_dumps(lb.gpt, gpt, n, ctx->stream) || upload_dumps(lb.ops, n > 32 ? ops_both : ops, n, ctx->stream) ||
        lb.gammas.upload(gammas, ctx->stream))
        return QOCX_ERR_HIP;
    return 0;
}

// Time-dependent Hamiltonian: the samples at the stage times of the fixed sub-division
// (qocx_lindblad_stage_times) as per-stage dumps, and the norm bounds taken over the samples
int upload_stage_tables(qocx_ctx* ctx, const qocx_lindblad_problem* p, const cmat& decay) {
    auto& lb = ctx->lb;
    const int n = lb.n, K = lb.K, L = lb.nops;
    const bool td_ops = p->op_stages != nullptr && L > 0, td_g = p->g_stages != nullptr && K > 0;
    int64_t count = 0;
    // (piecewise constant: the slice edges are the cut points of nc + 1 linear knots)
    if (int rc = qocx_lindblad_stage_times(p->evolution_time, lb.N, lb.pwc ? lb.nc + 1 : lb.nc, K,
                                           p->fixed_subdivision, nullptr, 0, &count))
        return rc;
    const size_t md = dump_elems(n);
    std::vector<double2> tab((size_t)count * 4 * md), otab(td_ops ? (size_t)count * L * md : 0);
    std::vector<double2> gtab(td_g ? (size_t)count * K * 3 * md : 0);
    std::vector<double> gamtab(td_ops ? (size_t)count * L : 0);
    lb.h0_norm = 0;
    if (td_ops) lb.diss_norm = 0;
    if (td_g) lb.g_norm.assign(K, 0.0);
    for (int64_t st = 0; st < count; ++st) {
        // Norms on every fourth stage sample, and on the last: they vary smoothly in time, the host picked
        // the sub-division with a 25 % margin, and a power iteration per sample is what made this loop slow
        const bool norm_sample = (st % 4 == 0) || st == count - 1;
        const cmat h = cm_from(p->h0_stages + (size_t)st * n * n * 2, n);
        if (norm_sample) lb.h0_norm = std::max(lb.h0_norm, two_norm(h.data(), n));
        cmat l = cm_scale(h, 0.0, -1.0), r = cm_scale(h, 0.0, 1.0);
        cmat decay_st = decay;
        if (td_ops) {  // -1/2 sum_i gamma_i(t) L_i(t)^H L_i(t) of THIS stage time
            decay_st = cm_zero(n);
            double dn = 0;
            for (int i = 0; i < L; ++i) {
                const cmat li = cm_from(p->op_stages + ((size_t)st * L + i) * n * n * 2, n);
                const double gi = p->diss_stages[(size_t)st * L + i];
                cm_axpy(decay_st, gi, cm_mul(cm_adjoint(li, n), li, n));
                c_dump(li, n, otab.data() + ((size_t)st * L + i) * md);
                gamtab[(size_t)st * L + i] = gi;
                if (norm_sample) {
                    const double opn = two_norm(li.data(), n);
                    dn += fabs(gi) * opn * opn;
                }
            }
            lb.diss_norm = std::max(lb.diss_norm, dn);
        }
        cm_axpy(l, -0.5, decay_st);
        cm_axpy(r, -0.5, decay_st);
        double2* a0 = tab.data() + (size_t)st * 4 * md;
        c_dump(l, n, a0); c_dump(r, n, a0 + md);
        c_dump(cm_adjoint(l, n), n, a0 + 2 * md); c_dump(cm_adjoint(r, n), n, a0 + 3 * md);
        for (int k = 0; td_g && k < K; ++k) {
            const cmat gk = cm_from(p->g_stages + ((size_t)st * K + k) * n * n * 2, n);
            if (norm_sample) lb.g_norm[k] = std::max(lb.g_norm[k], two_norm(gk.data(), n));
            const cmat gpk = cm_scale(gk, 0.0, -1.0);
            double2* dst = gtab.data() + (((size_t)st * K + k) * 3) * md;
            c_dump(gpk, n, dst); c_dump(cm_adjoint(gpk, n), n, dst + md); c_dump(cm_transpose(gpk, n), n, dst + 2 * md);
        }
    }
    if (lb.a0_tab.upload(tab, ctx->stream)) return QOCX_ERR_HIP;
    if (td_ops && (lb.op_tab.upload(otab, ctx->stream) || lb.gamma_tab.upload(gamtab, ctx->stream)))
        return QOCX_ERR_HIP;
    if (td_g && lb.gp_tab.upload(gtab, ctx->stream)) return QOCX_ERR_HIP;
    lb.fixed_ksub = p->fixed_subdivision;
    return 0;
}

int upload_initial_densities(qocx_ctx* ctx, const qocx_lindblad_problem* p, bool& hermitian) {
    auto& lb = ctx->lb;
    std::vector<cmat> rho0;
    for (int s = 0; s < lb.S; ++s) rho0.push_back(cm_from(p->initial_densities + (size_t)s * lb.n * lb.n * 2, lb.n));
    if (upload_dumps(lb.rho0, rho0, lb.n, ctx->stream)) return QOCX_ERR_HIP;
    hermitian = true;
    for (const cmat& r : rho0) hermitian = hermitian && cm_is_hermitian(r, lb.n);
    return 0;
}

// The cost descriptors (checked by check_lindblad_problem) with their pooled matrices
int upload_lindblad_costs(qocx_ctx* ctx, const qocx_lindblad_problem* p, bool& hermitian) {
    auto& lb = ctx->lb;
    const int n = lb.n, S = lb.S;
    std::vector<qocx::DevCost> dcosts;
    std::vector<cmat> pool;
    std::vector<int> counts;
    lb.has_step_costs = 0;
    for (int ci = 0; ci < p->cost_count; ++ci) {
        const qocx_cost_desc& c = p->costs[ci];
        qocx::DevCost d;
        d.step_cost = c.step_cost ? 1 : 0; d.scale = c.scale;
        d.vec_offset = (int)pool.size(); d.cnt_offset = (int)counts.size();
        d.kind = c.kind == QOCX_COST_TARGET_DENSITY ? QOCX_DEV_COST_TARGET_DENSITY : QOCX_DEV_COST_FORBID_DENSITY;
        int nmat = S;
        if (c.kind == QOCX_COST_FORBID_DENSITY) {
            nmat = 0;
            for (int s = 0; s < S; ++s) {
                counts.push_back(c.counts[s]);
                nmat += c.counts[s];
            }
        }
        for (int m = 0; m < nmat; ++m) pool.push_back(cm_from(c.vectors + (size_t)m * n * n * 2, n));
        if (d.step_cost) lb.has_step_costs = 1;
        dcosts.push_back(d);
    }
    hermitian = true;
    for (const cmat& m : pool) hermitian = hermitian && cm_is_hermitian(m, n);
    lb.cost_count = (int)dcosts.size();
    lb.unit_ok = dcosts.size() == 1 && !dcosts[0].step_cost && dcosts[0].kind == QOCX_DEV_COST_TARGET_DENSITY;
    if (lb.costs.upload(dcosts, ctx->stream) || upload_dumps(lb.cost_matrices, pool, n, ctx->stream) ||
        lb.cost_counts.upload(counts, ctx->stream))
        return QOCX_ERR_HIP;
    return 0;
}

}  // namespace
}  // extern "C++"

int qocx_set_lindblad_problem(qocx_ctx* ctx, const qocx_lindblad_problem* p) {
    if (!ctx || !p) return fail(QOCX_ERR_ARG, "NULL argument");
    if (p->struct_size != (int32_t)sizeof(qocx_lindblad_problem))
        return fail(QOCX_ERR_ARG, "qocx_lindblad_problem.struct_size does not match this "
                                  "library's header (stale binding?)");
    HIP_TRY(hipSetDevice(ctx->device));
    if (int rc = check_lindblad_problem(p, ctx->knob("lindblad_wide", 0) != 0)) return rc;
    auto& lb = ctx->lb;
    lb.has_problem = false;
    lb.control_costs.clear();
    lb.n = p->hilbert_size; lb.S = p->density_count; lb.K = p->control_count; lb.nc = p->control_eval_count;
    lb.N = p->system_eval_count; lb.nsteps = lb.N - 1; lb.ces = p->cost_eval_step; lb.nops = p->operator_count;
    choose_launch_form(ctx, p);
    lb.T = p->evolution_time; lb.dt = p->evolution_time / lb.nsteps;
    lb.pwc = ctx->interp_policy == QOCX_INTERP_PIECEWISE_CONSTANT;
    lb.fixed_ksub = 0;
    lb.a0_tab.release(); lb.gp_tab.release(); lb.op_tab.release(); lb.gamma_tab.release();
    cmat decay;
    bool h_static = false, h_rho = false, h_costs = false;
    if (int rc = upload_static_part(ctx, p, decay, h_static)) return rc;
    if (p->fixed_subdivision > 0)
        if (int rc = upload_stage_tables(ctx, p, decay)) return rc;
    if (int rc = upload_initial_densities(ctx, p, h_rho)) return rc;
    if (int rc = upload_lindblad_costs(ctx, p, h_costs)) return rc;
    // (stage tables: the Hermitian shortcuts read constant generators)
    lb.hermitian = p->h0_stages == nullptr && p->g_stages == nullptr && p->op_stages == nullptr && h_static &&
                   h_rho && h_costs;
    lb.grids.clear();  // (frees the tables of the old problem's grids)
    lb.has_problem = true;
    lb.drop_resident();  // resident controls and optimizer states belong to the old problem
    lb.inj_count = 0;
    lb.seeds.clear();  // ... and so do the ensemble with its rates, or the sweep with its duration search
    lb.ens_rates = lb.swp_want_rates = false;
    return 0;
}

int qocx_lindblad_set_ensemble(qocx_ctx* ctx, int32_t members, int32_t fixed, const double* scales,
                               const double* offsets, const double* weights) {
    if (!ctx) return fail(QOCX_ERR_ARG, "ctx is NULL");
    auto& lb = ctx->lb;
    if (!lb.has_problem) return fail(QOCX_ERR_STATE, "no Lindblad problem set (qocx_set_lindblad_problem first)");
    if (lb.seeds.sweep())
        return fail(QOCX_ERR_STATE, "a sweep is set (qocx_lindblad_set_sweep): a problem takes a sweep or an ensemble");
    if (lb.inj_count > 0)
        return fail(QOCX_ERR_STATE, "density cotangents are set (qocx_set_density_cotangents): an ensemble "
                                    "takes none");
    HIP_TRY(hipSetDevice(ctx->device));
    // (control_count <= QOCX_LINDBLAD_MAX_K was checked by the problem setter: K_r + J <= 8)
    if (int rc = set_seed_tables(lb.seeds, false, lb.K, members, fixed, scales, offsets, weights, ctx->stream))
        return rc;
    lb.ens_rates = false;      // (qocx_lindblad_set_ensemble_rates comes after, as the quadratic scales do)
    lb.drop_resident();        // controls must be uploaded again (as seed controls)
    lb.control_costs.clear();  // (they were set for K channels: qocx_set_control_costs comes after)
    return 0;
}

extern "C++" {
namespace {

// The rates tables of `count` members (an ensemble's members, a sweep's seeds) from rate_scales [count][L]:
// member m is the control-free part of the plain problem with gamma_mi = c_mi * gamma_i (one product, one
// rounding); [count][4] dumps A0L, A0R, A0L^H, A0R^H and [count][L'] rates, L' with the zero operator of pad_op
// (the host part: the tables themselves, which a duration search keeps at tau = 1 as its base tables)
void rate_tables_host(const qocx_ctx::Lindblad& lb, int count, const double* rate_scales, std::vector<double2>& img,
                      std::vector<double>& gam, std::vector<double>& l0_norm) {
    const int M = count, L = lb.nops, n = lb.n;
    const size_t md = dump_elems(n), Lp = lb.gammas_h.size();
    img.assign((size_t)M * 4 * md, make_double2(0.0, 0.0));
    gam.assign((size_t)M * std::max<size_t>(Lp, 1), 0.0);
    l0_norm.assign(M, 0.0);
    for (int m = 0; m < M; ++m) {
        std::vector<double> gm(lb.gammas_h);
        for (int i = 0; i < L; ++i) gm[i] = rate_scales[(size_t)m * L + i] * lb.gammas_h[i];
        const ControlFree cf = control_free_part(lb.h0_h, lb.h0_norm, lb.ops_h, gm, lb.op_norms_h, L, n);
        c_dump(cf.a0l, n, img.data() + ((size_t)m * 4 + 0) * md);
        c_dump(cf.a0r, n, img.data() + ((size_t)m * 4 + 1) * md);
        c_dump(cm_adjoint(cf.a0l, n), n, img.data() + ((size_t)m * 4 + 2) * md);
        c_dump(cm_adjoint(cf.a0r, n), n, img.data() + ((size_t)m * 4 + 3) * md);
        for (size_t i = 0; i < Lp; ++i) gam[(size_t)m * Lp + i] = gm[i];
        l0_norm[m] = cf.l0_norm;
    }
}

int build_rate_tables(qocx_ctx* ctx, int count, const double* rate_scales) {
    auto& lb = ctx->lb;
    std::vector<double2> img;
    std::vector<double> gam;
    rate_tables_host(lb, count, rate_scales, img, gam, lb.rate_l0_norm);
    if (lb.rate_a0.upload(img, ctx->stream) || lb.rate_gammas.upload(gam, ctx->stream)) return QOCX_ERR_HIP;
    return 0;
}

}  // namespace
}  // extern "C++"

int qocx_lindblad_set_ensemble_rates(qocx_ctx* ctx, int32_t members, int32_t operators, const double* rate_scales) {
    if (!ctx) return fail(QOCX_ERR_ARG, "ctx is NULL");
    auto& lb = ctx->lb;
    if (!lb.has_problem || lb.seeds.M == 0 || lb.seeds.swp_B > 0)
        return fail(QOCX_ERR_STATE, "no Lindblad ensemble set (qocx_lindblad_set_ensemble first)");
    if (lb.n > 32 && rate_scales) return fail(QOCX_ERR_STATE, wide_only("per-member rates (rate_scales)"));
    if (lb.fixed_ksub > 0)
        return fail(QOCX_ERR_STATE, "per-member rates need a static problem: this one was set with stage tables "
                                    "(fixed_subdivision > 0), which hold one control-free generator per stage");
    if (!rate_scales) {
        lb.ens_rates = false;
        lb.drop_resident();
        return 0;
    }
    const int M = lb.seeds.M, L = lb.nops;
    if (members != M) return fail(QOCX_ERR_ARG, "rate_scales: members differs from the ensemble's");
    if (operators != L) return fail(QOCX_ERR_ARG, "rate_scales: operators differs from the problem's operator_count");
    for (size_t e = 0; e < (size_t)M * L; ++e)
        if (!std::isfinite(rate_scales[e]) || !(rate_scales[e] >= 0))
            return fail(QOCX_ERR_ARG, "rate_scales must be finite and >= 0");
    HIP_TRY(hipSetDevice(ctx->device));
    if (int rc = build_rate_tables(ctx, M, rate_scales)) return rc;
    lb.ens_rates = true;
    lb.drop_resident();
    return 0;
}

int qocx_lindblad_set_sweep(qocx_ctx* ctx, int32_t seeds, int32_t fixed, const double* scales, const double* offsets,
                            const double* rate_scales) {
    if (!ctx) return fail(QOCX_ERR_ARG, "ctx is NULL");
    auto& lb = ctx->lb;
    if (!lb.has_problem) return fail(QOCX_ERR_STATE, "no Lindblad problem set (qocx_set_lindblad_problem first)");
    if (lb.seeds.M > 0 && !lb.seeds.sweep())
        return fail(QOCX_ERR_STATE, "an ensemble is set (qocx_lindblad_set_ensemble): a problem takes a sweep or an "
                                    "ensemble");
    if (lb.inj_count > 0)
        return fail(QOCX_ERR_STATE, "density cotangents are set (qocx_set_density_cotangents): a sweep takes none");
    // (the rates tables hold at most this many members)
    if (seeds < 1 || seeds > 1024) return fail(QOCX_ERR_ARG, "sweep seeds must be 1 .. 1024");
    const int L = lb.nops, n = lb.n;
    const bool rates = rate_scales != nullptr && L > 0;
    if (rates && n > 32) return fail(QOCX_ERR_STATE, wide_only("per-seed rates (rate_scales)"));
    if (rates && lb.fixed_ksub > 0)
        return fail(QOCX_ERR_STATE, "per-seed rates need a static problem: this one was set with stage tables "
                                    "(fixed_subdivision > 0), which hold one control-free generator per stage");
    for (size_t e = 0; rates && e < (size_t)seeds * L; ++e)
        if (!std::isfinite(rate_scales[e]) || !(rate_scales[e] >= 0))
            return fail(QOCX_ERR_ARG, "rate_scales must be finite and >= 0");
    HIP_TRY(hipSetDevice(ctx->device));
    // (control_count <= QOCX_LINDBLAD_MAX_K was checked by the problem setter: K_r + J <= 8)
    if (int rc = set_seed_tables(lb.seeds, true, lb.K, seeds, fixed, scales, offsets, nullptr, ctx->stream)) return rc;
    lb.swp_want_rates = false;
    lb.ens_rates = false;      // (until the rates tables below stand)
    lb.drop_resident();        // controls must be uploaded again (as seed controls)
    lb.control_costs.clear();  // (they were set for K channels: qocx_set_control_costs comes after)
    // seed b: the control-free part of the plain problem with the rates c_b * gamma, built as the plain
    // setter builds its own (build_rate_tables)
    if (rates)
        if (int rc = build_rate_tables(ctx, seeds, rate_scales)) return rc;
    // M_l = L_l^H L_l of the problem's own operators, for the rate sensitivities
    if (L > 0) {
        std::vector<cmat> ldl;
        for (int i = 0; i < L; ++i) ldl.push_back(cm_mul(cm_adjoint(lb.ops_h[i], n), lb.ops_h[i], n));
        if (upload_dumps(lb.swp_ldl, ldl, n, ctx->stream)) return QOCX_ERR_HIP;
    }
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    lb.ens_rates = rates;
    return 0;
}

int qocx_lindblad_sweep_want_rate_sensitivities(qocx_ctx* ctx, int32_t on) {
    if (!ctx) return fail(QOCX_ERR_ARG, "ctx is NULL");
    if (ctx->lb.seeds.swp_B == 0) return fail(QOCX_ERR_STATE, "no sweep set (qocx_lindblad_set_sweep)");
    if (ctx->lb.n > 32 && on)
        return fail(QOCX_ERR_STATE, wide_only("rate sensitivities (they come out of the two-sided evaluation)"));
    ctx->lb.swp_want_rates = on != 0;
    return 0;
}

extern "C++" {
namespace {

// End points of the sub-intervals of system step `step`: `ksub` uniform pieces, cut at the
// control knots that fall inside the step.
std::vector<double> lindblad_points(double T, int nsteps, int nc, int K, int ksub, int step) {
    const double dt = T / nsteps;
    const double t0 = step * dt, t1 = (step + 1) * dt;
    std::vector<double> pts;
    for (int q = 0; q < ksub; ++q) pts.push_back(t0 + (t1 - t0) * q / ksub);
    pts.push_back(t1);
    if (K > 0)
        for (int i = 0; i < nc; ++i) {
            const double kn = (i == nc - 1) ? T : i * (T / (nc - 1));
            if (kn > t0 + 1e-12 * dt && kn < t1 - 1e-12 * dt) pts.push_back(kn);
        }
    std::sort(pts.begin(), pts.end());
    pts.erase(std::unique(pts.begin(), pts.end()), pts.end());
    return pts;
}
}  // extern "C++"

// Sub-interval table of one sub-division count: uniform pieces per system step, cut at control
// knots, with the interpolation weights of both ends and the CSR of their transpose.
int build_lindblad_grid(qocx_ctx* ctx, int ksub, qocx_ctx::Lindblad::Grid& gr) {
    auto& lb = ctx->lb;
    const int K = lb.K, nsteps = lb.nsteps;
    // Piecewise constant: the nc slices are the knot intervals of nc + 1 knots at j T / nc. A
    // sub-interval never straddles an edge, and both its ends take the value of the slice that
    // contains it: one index, weights (1, 0), so u_a = u_b = 1 * u + 0 * u bit for bit.
    const bool pwc = lb.pwc && K > 0;
    const int nc = pwc ? lb.nc + 1 : lb.nc;  // knots (rows of the control array: lb.nc)
    std::vector<double> knots(K > 0 ? nc : 0);
    for (int i = 0; i < (int)knots.size(); ++i) knots[i] = i * (lb.T / (nc - 1));
    if (!knots.empty()) knots.back() = lb.T;
    std::vector<qocx::SubStep> subs;
    for (int step = 0; step < nsteps; ++step) {
        const std::vector<double> pts = lindblad_points(lb.T, nsteps, nc, K, ksub, step);
        for (size_t i = 0; i + 1 < pts.size(); ++i) {
            qocx::SubStep ss;
            ss.h = pts[i + 1] - pts[i];
            // both ends interpolate on the knot interval that contains the sub-interval
            int m1 = 0, m2 = 0;
            if (!knots.empty()) {
                const double mid = 0.5 * (pts[i] + pts[i + 1]);
                if (mid <= knots[0]) { m1 = 0; m2 = 1; }
                else if (mid >= knots[nc - 1]) { m1 = nc - 2; m2 = nc - 1; }
                else {
                    int idx = 0;
                    while (!(mid <= knots[idx])) ++idx;
                    m1 = idx - 1; m2 = idx;
                }
            }
            auto end_weights = [&](double x, double& w1, double& w2) {
                if (knots.empty()) { w1 = 1; w2 = 0; return; }
                const double theta = (x - knots[m1]) / (knots[m2] - knots[m1]);
                w1 = 1.0 - theta; w2 = theta;
            };
            ss.ia1 = ss.ib1 = m1; ss.ia2 = ss.ib2 = m2;
            end_weights(pts[i], ss.wa1, ss.wa2);
            end_weights(pts[i + 1], ss.wb1, ss.wb2);
            if (pwc) {  // slice m1 (0 .. lb.nc - 1) at both ends
                ss.ia2 = ss.ib2 = m1;
                ss.wa1 = ss.wb1 = 1.0;
                ss.wa2 = ss.wb2 = 0.0;
            }
            ss.step = step;
            ss.first_of_step = (i == 0) ? 1 : 0;
            subs.push_back(ss);
        }
    }
    const int nsub = (int)subs.size();
    std::vector<std::vector<std::pair<int, double>>> rows(K > 0 ? lb.nc : 0);
    if (pwc)
        for (int q = 0; q < nsub; ++q) {
            rows[subs[q].ia1].push_back({2 * q, 1.0});
            rows[subs[q].ib1].push_back({2 * q + 1, 1.0});
        }
    else if (K > 0)
        for (int q = 0; q < nsub; ++q) {
            rows[subs[q].ia1].push_back({2 * q, subs[q].wa1});
            rows[subs[q].ia2].push_back({2 * q, subs[q].wa2});
            rows[subs[q].ib1].push_back({2 * q + 1, subs[q].wb1});
            rows[subs[q].ib2].push_back({2 * q + 1, subs[q].wb2});
        }
    std::vector<int> row_ptr(1, 0), col;
    std::vector<double> weight;
    for (auto& r : rows) {
        for (auto& e : r) { col.push_back(e.first); weight.push_back(e.second); }
        row_ptr.push_back((int)col.size());
    }
    if (gr.substeps.upload(subs, ctx->stream) || gr.row_ptr.upload(row_ptr, ctx->stream) ||
        gr.col.upload(col, ctx->stream) || gr.weight.upload(weight, ctx->stream))
        return QOCX_ERR_HIP;
    gr.nsub = nsub;
    return 0;
}

}  // namespace

int qocx_lindblad_stage_times(double evolution_time, int32_t system_eval_count,
                              int32_t control_eval_count, int32_t control_count,
                              int32_t subdivision, double* times_out, int64_t capacity,
                              int64_t* count_out) {
    if (system_eval_count < 2 || subdivision < 1 || !count_out ||
        (control_count > 0 && control_eval_count < 2))
        return fail(QOCX_ERR_ARG, "bad argument");
    const int nsteps = system_eval_count - 1;
    int64_t count = 0;
    for (int step = 0; step < nsteps; ++step) {
        const std::vector<double> pts = lindblad_points(evolution_time, nsteps, control_eval_count,
                                                        control_count, subdivision, step);
        for (size_t i = 0; i + 1 < pts.size(); ++i)
            for (int st = 0; st < QOCX_RK_STAGES; ++st) {
                if (times_out && count < capacity)
                    times_out[count] = pts[i] + QOCX_RK_C[st] * (pts[i + 1] - pts[i]);
                ++count;
            }
    }
    *count_out = count;
    return 0;
}

extern "C++" {
namespace {

// ---- qocx_eval_lindblad in three parts, shared with the resident driver (qocx_lindblad_*) ----------

// max_i |controls[b][i][k]| -> umax[b][k], in knot order (a NaN is carried as lindblad_subdivisions
// expects; control_maxima_kernel of qocx_optim.hip is the same scan on the device)
void lindblad_control_maxima(const double* controls, int B, int nc, int K, double* umax) {
    for (int b = 0; b < B; ++b)
        for (int k = 0; k < K; ++k) {
            double um = 0;
            for (int i = 0; i < nc; ++i) {
                const double a = fabs(controls[((size_t)b * nc + i) * K + k]);
                if (!(a <= um)) um = a;
            }
            umax[(size_t)b * K + k] = um;
        }
}

// The pinned staging buffer of the controls, at least `total` doubles, with nothing in flight that
// still reads it (a pageable source of 2 MB costs the copy 10-25 ms of page pinning per call at 256
// seeds; from pinned memory it is a DMA)
int pinned_controls(qocx_ctx* ctx, size_t total) {
    if (ctx->pin_controls_cap < total) {
        if (ctx->pin_controls) (void)hipHostFree(ctx->pin_controls);
        ctx->pin_controls = nullptr;
        ctx->pin_controls_cap = 0;
        HIP_TRY(hipHostMalloc((void**)&ctx->pin_controls, total * sizeof(double), hipHostMallocDefault));
        ctx->pin_controls_cap = total;
    }
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return 0;
}

// Each seed picks its own sub-division count from ITS controls (|| Liouvillian || * length <= 0.4
// per sub-interval), so a seed's result never depends on its batch neighbours. umax: [B][K] control
// maxima of the seeds; NULL with a fixed sub-division only (every seed then takes that one, unchecked).
int lindblad_subdivisions(qocx_ctx* ctx, int B, const double* umax, std::vector<int>& ksub_of) {
    auto& lb = ctx->lb;
    const int K = lb.K, nsteps = lb.nsteps;
    ksub_of.assign(B, lb.fixed_ksub);
    if (!umax) return lb.fixed_ksub > 0 ? 0 : fail(QOCX_ERR_STATE, "no control maxima");
    for (int b = 0; b < B; ++b) {
        // || Liouvillian ||_2 <= || control-free part ||_2 + sum_k |u_k| 2 ||G_k||_2; with a
        // time-dependent Hamiltonian / lindblad_data (tables) the control-free part is bounded by
        // the sum of its parts' bounds over the samples
        double ctl = 0;
        for (int k = 0; k < K; ++k) ctl += umax[(size_t)b * K + k] * lb.g_norm[k];
        // (per-member rates: B counts items b * M + m, and item (b, m) takes member m's bound - the
        // sub-division count the plain problem with that member's rates would pick; a sweep: item b is seed b)
        const double base = lb.fixed_ksub > 0 ? 2 * lb.h0_norm + 2 * lb.diss_norm
                            : lb.ens_rates    ? lb.rate_l0_norm[lb.seeds.swp_B > 0 ? b : b % lb.seeds.M]
                                              : lb.l0_norm;
        const double bound = base + 2 * ctl;
        if (!(bound < 1e300)) return fail(QOCX_ERR_ARG, "non-finite controls or operators");
        const double pieces = ceil(bound * fabs(lb.dt) / 0.4);
        if (pieces * nsteps > (double)(1 << 24))
            return fail(QOCX_ERR_CAPACITY, "too many sub-intervals");
        ksub_of[b] = std::max(1, (int)pieces);
        if (lb.fixed_ksub > 0) {
            // the time samples of the Hamiltonian exist for one grid only
            if (ksub_of[b] > lb.fixed_ksub)
                return fail(QOCX_ERR_CAPACITY,
                            "controls need a finer sub-division than the Hamiltonian was sampled for");
            ksub_of[b] = lb.fixed_ksub;
        }
    }
    return 0;
}

// What an evaluation of these sub-division counts launches: seeds with equal counts go together (`lb.order`
// lists the seeds group by group) in the pieces of the schedule above; the grid tables and buffers for them.
struct LindbladPlan {
    std::vector<qocx::LindbladPiece> pieces;  // launch order
    qocx::LindbladRoute route;                // the kernels of every launch, two-sided or not (qocx_lindblad_route.h)
    // a piece runs two-sided where the route does and the piece keeps its stage values
    bool two_sided(const qocx::LindbladPiece& pc) const { return route.two_sided && pc.keep_stages; }
    // rate sensitivities come out of the two-sided launches: one piece that recomputes its stages leaves the
    // evaluation without them
    bool rate_sens() const {
        return route.rate_sens &&
               std::all_of(pieces.begin(), pieces.end(), [](const qocx::LindbladPiece& pc) { return pc.keep_stages; });
    }
};

int lindblad_plan(qocx_ctx* ctx, int want_grad, const std::vector<int>& ksub_of, LindbladPlan& plan) {
    auto& lb = ctx->lb;
    const int n = lb.n, S = lb.S, K = lb.K, nc = lb.nc, nsteps = lb.nsteps, B = (int)ksub_of.size();
    const size_t md = dump_elems(n);
    std::map<int, std::vector<int>> groups;
    for (int b = 0; b < B; ++b) groups[ksub_of[b]].push_back(b);
    if (lb.grids.size() > 64) lb.grids.clear();  // bounded cache of sub-interval tables
    size_t ckpt_total = 0, gsub_total = 0;
    lb.order.clear();
    lb.last_subintervals = 0;
    for (auto& kv : groups) {
        if (lb.grids.find(kv.first) == lb.grids.end())
            if (int rc = build_lindblad_grid(ctx, kv.first, lb.grids[kv.first])) return rc;
        const size_t seed_subs = kv.second.size() * (size_t)lb.grids[kv.first].nsub;
        ckpt_total += seed_subs * S * md;
        gsub_total += seed_subs * 2 * std::max(K, 1);
        lb.last_subintervals += (int64_t)seed_subs;
        for (int b : kv.second) lb.order.push_back(b);
    }
    const qocx::LindbladRoute& route = plan.route = qocx::lindblad_route(lb.form, lindblad_facts(ctx, want_grad));
    // Two-sided evaluation (LindbladArgs::phase): the adjoint's stage cotangents need a buffer like the
    // forward's stage values, and gsub holds complex numbers
    if (route.two_sided && lb.lam_scale.ensure((size_t)B * S)) return QOCX_ERR_HIP;
    qocx::PieceRule rule{want_grad != 0, lb.form.multi_wave != 0, 0, lb.dbg_stage_seeds, lb.dbg_min_piece,
                         lb.dbg_wave_mode, ctx->cu_count};
    if (want_grad) {
        size_t free_b = 0, total_b = 0;
        HIP_TRY(hipMemGetInfo(&free_b, &total_b));
        rule.stage_budget =
            (size_t)(0.45 * (double)(free_b + (lb.ystages.count + lb.kbstages.count) * sizeof(double2))) / sizeof(double2);
        if (route.two_sided) rule.stage_budget /= 2;  // kbar_i beside Y_i
    }
    size_t stage_elems = 0;  // of the largest kept piece, before its round cap (lindblad_group_pieces)
    int first = 0;
    for (auto& kv : groups) {
        const int Bg = (int)kv.second.size();
        const size_t per_seed = (size_t)lb.grids[kv.first].nsub * S * md * 12;
        stage_elems = std::max(stage_elems, per_seed * qocx::lindblad_group_pieces(rule, kv.first, first, Bg, per_seed,
                                                                            plan.pieces));
        first += Bg;
    }
    if (stage_elems > 0 && (lb.ystages.ensure(stage_elems) || (route.two_sided && lb.kbstages.ensure(stage_elems))))
        return QOCX_ERR_HIP;
    if (lb.form.scratch && lb.scratch.ensure((size_t)B * qocx::lindblad_scratch_elems(n, S))) return QOCX_ERR_HIP;
    const size_t csz = (size_t)nc * K;
    if (lb.controls.ensure((size_t)B * std::max<size_t>(csz, 1)) || lb.cost_out.ensure(B) ||
        lb.grads.ensure((size_t)B * std::max<size_t>(csz, 1)) || lb.gsub.ensure(gsub_total) ||
        lb.checkpoints.ensure(ckpt_total) || lb.final_out.ensure((size_t)B * S * md))
        return QOCX_ERR_HIP;
    if (ctx->keep_step_states && lb.step_densities.ensure((size_t)B * (nsteps + 1) * S * md)) return QOCX_ERR_HIP;
    return 0;
}

// Host-supplied density cotangents (qocx_set_density_cotangents): dumps in launch order, the table step -> cotangent
int upload_density_cotangents(qocx_ctx* ctx) {
    auto& lb = ctx->lb;
    const int n = lb.n, B = (int)lb.order.size();
    const size_t md = dump_elems(n);
    if (lb.inj_batch != B) return fail(QOCX_ERR_STATE, "density cotangents were set for a different batch size");
    std::vector<int> index(lb.nsteps + 1, -1);
    for (int c = 0; c < lb.inj_count; ++c) index[lb.inj_steps[c]] = c;
    const size_t per_seed = (size_t)lb.inj_count * lb.S;
    std::vector<double2> dumps((size_t)B * per_seed * md);
    for (int pos = 0; pos < B; ++pos)
        for (size_t v = 0; v < per_seed; ++v) {
            cmat m(lb.inj_host.begin() + (((size_t)lb.order[pos] * per_seed + v) * n * n * 2),
                   lb.inj_host.begin() + (((size_t)lb.order[pos] * per_seed + v + 1) * n * n * 2));
            c_dump(m, n, dumps.data() + ((size_t)pos * per_seed + v) * md);
        }
    return (lb.inj_index.upload(index, ctx->stream) || lb.inj_bars.upload(dumps, ctx->stream)) ? QOCX_ERR_HIP : 0;
}

// The launches of one evaluation: the running offsets of the pieces into the evaluation's buffers
struct LindbladLaunch {
    qocx::LindbladMembers mem;  // per-member rates (lb.ens_rates): the strides; item_member is the piece's
    size_t ckpt_off = 0, gsub_off = 0, rate_off = 0;
};

// The arguments of the classic launch of piece `pc`; the two-sided launches add theirs (launch_two_sided)
qocx::LindbladArgs lindblad_piece_args(qocx_ctx* ctx, const qocx::LindbladRoute& route, int want_grad,
                                       const LindbladLaunch& ev, const qocx::LindbladPiece& pc) {
    auto& lb = ctx->lb;
    const int S = lb.S, nsteps = lb.nsteps;
    const size_t md = dump_elems(lb.n), csz = (size_t)lb.nc * lb.K, pos0 = pc.first;
    const auto& gr = lb.grids[pc.ksub];
    qocx::LindbladArgs la;
    la.controls = lb.controls.p + pos0 * csz; la.substeps = gr.substeps.p;
    la.a0l_cimg = lb.a0l.p; la.a0r_cimg = lb.a0r.p; la.a0ld_cimg = lb.a0ld.p; la.a0rd_cimg = lb.a0rd.p;
    la.gp_cimg = lb.gp.p; la.gpd_cimg = lb.gpd.p; la.gpt_cimg = lb.gpt.p; la.op_cimg = lb.ops.p;
    la.gammas = lb.gammas.p; la.rho0_cimg = lb.rho0.p;
    if (lb.ens_rates) {  // member 0's tables; a workgroup adds its member's stride (LindbladMembers)
        la.a0l_cimg = lb.rate_a0.p; la.a0r_cimg = lb.rate_a0.p + md;
        la.a0ld_cimg = lb.rate_a0.p + 2 * md; la.a0rd_cimg = lb.rate_a0.p + 3 * md;
        la.gammas = lb.rate_gammas.p;
    }
    la.a0_tab = lb.fixed_ksub > 0 ? lb.a0_tab.p : nullptr;
    la.gp_tab = (lb.fixed_ksub > 0 && lb.gp_tab.p) ? lb.gp_tab.p : nullptr;
    la.op_tab = (lb.fixed_ksub > 0 && lb.op_tab.p) ? lb.op_tab.p : nullptr;
    la.gamma_tab = la.op_tab ? lb.gamma_tab.p : nullptr;
    la.n = lb.n; la.S = S; la.K = lb.K; la.nc = lb.nc; la.nsub = gr.nsub; la.nsteps = nsteps;
    la.nops = (pc.multi_wave && lb.form.pad_op) ? 2 : lb.nops;
    la.cost_eval_step = lb.ces; la.want_grad = want_grad; la.has_step_costs = lb.has_step_costs; la.cost_count = lb.cost_count;
    la.costs = lb.costs.p; la.cost_matrices = lb.cost_matrices.p; la.cost_counts = lb.cost_counts.p;
    la.checkpoints = lb.checkpoints.p + ev.ckpt_off; la.gsub = lb.gsub.p + ev.gsub_off;
    la.ystages = pc.keep_stages ? lb.ystages.p : nullptr;     // reused piece after piece
    la.scratch = lb.form.scratch ? lb.scratch.p : nullptr;    // likewise
    // several waves per seed shorten a seed's serial chain by ~1.4x but hold one seed
    // per CU instead of two: worth it while the batch leaves CUs idle
    la.multi_wave = pc.multi_wave ? 1 : 0;
    la.cache_gen = (la.multi_wave && lb.form.cache_gen) ? 1 : 0;
    la.cost_out = lb.cost_out.p + pos0; la.final_out = lb.final_out.p + pos0 * S * md;
    la.step_densities = ctx->keep_step_states ? lb.step_densities.p + pos0 * (nsteps + 1) * S * md : nullptr;
    la.tile4 = route.tile4; la.hermitian = route.hermitian;
    // ([B] sets of the forward pass / classic launch, then [B] of the unit adjoint)
    la.stamps = route.stamps ? ctx->stamps.p + pos0 * 48 : nullptr;
    la.inj_count = lb.inj_count;
    la.inj_index = lb.inj_count > 0 ? lb.inj_index.p : nullptr;
    la.inj_bars = lb.inj_count > 0 ? lb.inj_bars.p + pos0 * lb.inj_count * S * md : nullptr;
    return la;
}

// One launch of piece `pc`, on the kernel the route names for the phase of `args`
// (per-member rates: kernels of their own, qocx_lindblad_rates.hip / qocx_lindblad4t_rates.hip, whose workgroup i
// reads the tables of member item_member[i]: behind the order, in launch order)
int launch_lindblad_piece(qocx_ctx* ctx, const qocx::LindbladRoute& route, const LindbladLaunch& ev,
                          const qocx::LindbladArgs& args, const qocx::LindbladPiece& pc, hipStream_t st) {
    auto& lb = ctx->lb;
    const qocx::LindbladKernel kernel = route.kernel[args.phase];
    int none = 0;
    time_begin(ctx, 5, st);
    if (lb.ens_rates) {
        qocx::LindbladMembers mem = ev.mem;
        mem.item_member = lb.order_dev.p + lb.order.size() + pc.first;
        none = qocx::launch_lindblad_rates(kernel, route.stamped, args, mem, pc.count, st);
    } else none = qocx::launch_lindblad(kernel, route.stamped, args, pc.count, st);
    time_end(ctx, st);
    // (every such problem was refused by name when it was set)
    return none ? fail(QOCX_ERR_STATE, "no Lindblad kernel for this problem at hilbert_size > 32") : 0;
}

// Two-sided: forward pass and unit adjoint as two launches, then the combine kernel on the whole chip.
// While both launches find CUs of their own they run on two streams (2 Bp CUs busy instead of Bp); a
// bigger piece runs them one after the other - the same three kernels, so a seed's result does not depend
// on the batch it is part of. Then, for a sweep that asked, the rate sensitivities of the piece.
int launch_two_sided(qocx_ctx* ctx, const LindbladPlan& plan, const LindbladLaunch& ev, qocx::LindbladArgs la,
                     const qocx::LindbladPiece& pc) {
    auto& lb = ctx->lb;
    const qocx::LindbladRoute& route = plan.route;
    hipStream_t side = pc.count <= route.side_limit ? ctx->sweep_streams[0] : ctx->stream;
    la.kbstages = lb.kbstages.p;
    la.lam_scale = lb.lam_scale.p + (size_t)pc.first * lb.S;
    // everything enqueued so far (uploads, earlier pieces that reuse the stage buffers)
    if (side != ctx->stream) {
        HIP_TRY(hipEventRecord(ctx->ev_factored[0], ctx->stream));
        HIP_TRY(hipStreamWaitEvent(side, ctx->ev_factored[0], 0));
    }
    qocx::LindbladArgs fwd = la, adj = la;
    fwd.phase = 1; adj.phase = 2;
    fwd.q2 = adj.q2 = route.q2; fwd.chain = adj.chain = route.chain; fwd.ops_real = adj.ops_real = route.ops_real;
    if (la.stamps != nullptr) adj.stamps = la.stamps + lb.order.size() * 48;
    if (int rc = launch_lindblad_piece(ctx, route, ev, fwd, pc, ctx->stream)) return rc;
    if (int rc = launch_lindblad_piece(ctx, route, ev, adj, pc, side)) return rc;
    if (side != ctx->stream) {
        HIP_TRY(hipEventRecord(ctx->ev_swept[0], side));
        HIP_TRY(hipStreamWaitEvent(ctx->stream, ctx->ev_swept[0], 0));
    }
    time_begin(ctx, 6, ctx->stream);
    qocx::launch_lindblad_combine(la, pc.count, ctx->stream);
    time_end(ctx, ctx->stream);
    if (lb.swp_rates_ok) {
        // on the stream of the forward launches, so before the next piece's (and, through
        // ev_factored, before its adjoint's on the side stream): they reuse the stage buffers
        qocx::RateSensArgs rs;
        rs.ldl_cimg = lb.swp_ldl.p; rs.gammas = lb.gammas.p; rs.nops = lb.nops;
        rs.partials = lb.swp_rate_partials.p + ev.rate_off;
        rs.out = lb.swp_rate_sens.p + (size_t)pc.first * lb.nops;
        qocx::launch_lindblad_ratesens(la, rs, pc.count, ctx->stream);
    }
    return 0;
}

// The launches piece by piece, as the plan lists them: results in lb.cost_out / grads / final_out in group
// order. The controls are in lb.controls, in group order, on ctx->stream before this.
int lindblad_launch_groups(qocx_ctx* ctx, int want_grad, const LindbladPlan& plan) {
    auto& lb = ctx->lb;
    const int n = lb.n, S = lb.S, K = lb.K, nc = lb.nc, B = (int)lb.order.size();
    const size_t md = dump_elems(n), csz = (size_t)nc * K;
    if (int rc = lb.inj_count > 0 ? upload_density_cotangents(ctx) : 0) return rc;
    // Rate sensitivities of a sweep (qocx_lindblad_sweep_want_rate_sensitivities): a launch of
    // qocx_lindblad_ratesens.hip behind every piece's combine launch
    lb.swp_rates_ok = plan.rate_sens();
    if (lb.swp_rates_ok && (lb.swp_rate_partials.ensure((size_t)lb.last_subintervals * lb.nops) ||
                            lb.swp_rate_sens.ensure((size_t)B * lb.nops)))
        return QOCX_ERR_HIP;
    LindbladLaunch ev;
    ev.mem.a0_stride = 4 * md; ev.mem.gamma_stride = lb.gammas_h.size();
    if (plan.route.stamps) {  // the whole buffer once: a piece's launches stamp only their own seeds' sets
        if (ctx->stamps.ensure((size_t)B * 96)) return QOCX_ERR_HIP;
        HIP_TRY(hipMemsetAsync(ctx->stamps.p, 0, (size_t)B * 96 * sizeof(unsigned long long), ctx->stream));
    }
    for (const qocx::LindbladPiece& pc : plan.pieces) {
        const auto& gr = lb.grids[pc.ksub];
        const qocx::LindbladArgs la = lindblad_piece_args(ctx, plan.route, want_grad, ev, pc);
        if (int rc = plan.two_sided(pc) ? launch_two_sided(ctx, plan, ev, la, pc)
                                        : launch_lindblad_piece(ctx, plan.route, ev, la, pc, ctx->stream))
            return rc;
        if (want_grad) {
            qocx::ScatterArgs sc;
            sc.gstep = la.gsub; sc.row_ptr = gr.row_ptr.p; sc.col_step = gr.col.p;
            sc.weight = gr.weight.p; sc.grads = lb.grads.p + (size_t)pc.first * csz;
            sc.B = pc.count; sc.nc = nc; sc.K = K; sc.nsteps = 2 * gr.nsub;
            time_begin(ctx, 3, ctx->stream);
            qocx::launch_scatter(sc, ctx->stream);
            time_end(ctx, ctx->stream);
        }
        ev.ckpt_off += (size_t)pc.count * gr.nsub * S * md;
        ev.gsub_off += (size_t)pc.count * gr.nsub * 2 * std::max(K, 1);
        ev.rate_off += (size_t)pc.count * gr.nsub * lb.nops;
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

// An evaluation of `items` control arrays [items][nc][K] on the device (umax as lindblad_subdivisions takes
// it): the plan, the order uploaded, the controls gathered into group order (the device-side form of
// qocx_eval_lindblad's staging copy), the launches. Results in lb.cost_out / grads / final_out in group order.
int lindblad_launch_items(qocx_ctx* ctx, int items, const double* controls, const double* umax, int want_grad) {
    auto& lb = ctx->lb;
    std::vector<int> ksub_of;
    LindbladPlan plan;
    if (int rc = lindblad_subdivisions(ctx, items, umax, ksub_of)) return rc;
    if (int rc = lindblad_plan(ctx, want_grad, ksub_of, plan)) return rc;
    std::vector<int> table(lb.order);
    // per-member rates, behind the order: every launched item's member (item_member; a sweep: the seed itself)
    for (int i = 0; lb.ens_rates && i < items; ++i)
        table.push_back(lb.seeds.swp_B > 0 ? lb.order[i] : lb.order[i] % lb.seeds.M);
    if (lb.order_dev.upload(table, ctx->stream)) return QOCX_ERR_HIP;
    qocx::launch_gather_seeds(controls, lb.controls.p, (size_t)lb.nc * lb.K, lb.order_dev.p, items, ctx->stream);
    return lindblad_launch_groups(ctx, want_grad, plan);
}

// Cost [B], gradients [B][csz], final dumps [B][dens] of B seeds into the caller's arrays (each optional), un-dumped
int download_seed_results(qocx_ctx* ctx, int B, size_t csz, size_t dens, const double* cost, const double* grads,
                          const double2* finals, double* cost_out, double* grad_out, double* final_out) {
    const size_t n = ctx->lb.n, md = dump_elems(ctx->lb.n);
    std::vector<double2> fin(final_out ? (size_t)B * dens * md : 0);
    if (cost_out)
        HIP_TRY(hipMemcpyAsync(cost_out, cost, (size_t)B * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (grad_out)
        HIP_TRY(hipMemcpyAsync(grad_out, grads, (size_t)B * csz * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (final_out)
        HIP_TRY(hipMemcpyAsync(fin.data(), finals, fin.size() * sizeof(double2), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    for (size_t v = 0; final_out && v < (size_t)B * dens; ++v)
        from_c_dump(fin.data() + v * md, n, final_out + v * n * n * 2);
    return 0;
}

// ---- Hamiltonian ensembles (qocx_lindblad_set_ensemble): the member items of `seeds` seeds ---------

// The maxima lindblad_subdivisions reads, per item: |s_mk| umax_bk on the seeds' channels, |delta_mj|
// beyond. |s u| = |s| |u| exactly and rounding is monotone, so these are the maxima of the expanded
// array, bit for bit (a NaN of umax is carried).
std::vector<double> lindblad_item_maxima(const qocx_ctx::Lindblad& lb, int seeds, const double* umax) {
    const int M = lb.seeds.M, Kr = lb.seeds.Kr, J = lb.seeds.J, K = lb.K;
    std::vector<double> out((size_t)seeds * M * K);
    const double* scales = lb.seeds.scales_h.data();
    const double* offsets = lb.seeds.offsets_h.data();
    for (int b = 0; b < seeds; ++b)
        for (int m = 0; m < M; ++m) {
            const size_t row = lb.seeds.sweep() ? b : m;  // (a sweep: M = 1 and the seed's own row)
            double* o = out.data() + ((size_t)b * M + m) * K;
            for (int k = 0; k < Kr; ++k) o[k] = fabs(scales[row * Kr + k]) * umax[(size_t)b * Kr + k];
            for (int j = 0; j < J; ++j) o[Kr + j] = fabs(offsets[row * J + j]);
        }
    return out;
}

// the Lindblad buffers the kernels of qocx_ensemble.hip / qocx_sweep.hip run on: seed controls -> items
// (expand), the items' results in item order -> the seeds' (reduce), and the channel sensitivities
SeedBuffers lindblad_buffers(qocx_ctx::Lindblad& lb, const double* seed_controls, double* cost, double* grads) {
    return {seed_controls, lb.ens_items.p, lb.ens_cost.p, lb.ens_grads.p, cost, grads};
}

// ---- duration search of a sweep (qocx_lindblad_sweep_set_durations, qocx_lindblad_duration.hip) -------

qocx::LindbladDurationArgs lindblad_generator_args(qocx_ctx* ctx) {
    auto& lb = ctx->lb;
    qocx::LindbladDurationArgs a;
    a.tau = lb.seeds.dur.tau.p;
    a.base_a0 = lb.dur_base_a0.p; a.a0 = lb.rate_a0.p;
    a.base_gammas = lb.dur_base_gammas.p; a.gammas = lb.rate_gammas.p;
    a.base_scales = lb.seeds.dur.base_scales.p; a.base_offsets = lb.seeds.dur.base_offsets.p;
    a.base_rates = lb.dur_base_rates.p;
    a.scale_sens = lb.seeds.scale_sens.p; a.offset_sens = lb.seeds.offset_sens.p;
    a.rate_sens = lb.swp_rate_sens.p;
    a.order = lb.order_dev.p;
    a.tau_grad = nullptr;
    a.cost = nullptr;
    a.time_weight = lb.seeds.dur.weight;
    a.a0_per_seed = 4 * (size_t)dump_elems(lb.n);
    a.B = lb.seeds.swp_B; a.Kr = lb.seeds.Kr; a.J = lb.seeds.J; a.L = lb.nops; a.Lp = (int)lb.gammas_h.size();
    return a;
}

// Before an evaluation of a duration search: if tau has moved on the device since the tables were
// written (a step without the clip behind it), they are rewritten and the host mirrors re-formed
int lindblad_duration_refresh(qocx_ctx* ctx) {
    auto& lb = ctx->lb;
    if (!lb.seeds.dur.set || !lb.seeds.dur.mirror_stale) return 0;
    lindblad_duration_tables(ctx);
    HIP_TRY(hipGetLastError());
    if (int rc = lindblad_duration_fetch(ctx)) return rc;
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    lindblad_duration_mirror(ctx);
    return 0;
}

// The tail of an evaluation of a duration search, on the seeds' costs `cost` [B] once every other term
// has joined them: dE_b/dtau_b + time_weight by the chain rule through the three tables (with
// gradients), and time_weight tau_b onto the costs. An evaluation with gradients whose rate
// sensitivities did not come about fails by name: it must not return a gradient without its rate part.
int lindblad_duration_finish(qocx_ctx* ctx, int want_grad, double* cost) {
    auto& lb = ctx->lb;
    if (!lb.seeds.dur.set) return 0;
    lb.seeds.dur.have_grad = false;
    if (want_grad && !lb.swp_rates_ok) {
        lb.drop_results();
        return fail(QOCX_ERR_STATE,
                    "a duration search (qocx_lindblad_sweep_set_durations) needs the rate sensitivities in every "
                    "evaluation with gradients, and a piece of this one did not run two-sided: that takes ONE "
                    "cost, a final target-density infidelity, 1 .. 4 operators, the two-sided kernels and stage "
                    "values that fit the device memory");
    }
    const size_t ns = (size_t)lb.seeds.swp_B * lb.seeds.Kr, no = (size_t)lb.seeds.swp_B * lb.seeds.J;
    if (lb.seeds.dur.grad.ensure((size_t)lb.seeds.swp_B) || lb.seeds.scale_sens.ensure(ns) ||
        lb.seeds.offset_sens.ensure(no))
        return QOCX_ERR_HIP;
    const SeedBuffers buf = lindblad_buffers(lb, lb.swp_seed_controls, nullptr, nullptr);
    if (want_grad) qocx::launch_sweep_sensitivity(sweep_args(lb.seeds, lb.nc, buf), ctx->stream);
    qocx::LindbladDurationArgs a = lindblad_generator_args(ctx);
    a.tau_grad = want_grad ? lb.seeds.dur.grad.p : nullptr;
    a.cost = cost;
    qocx::launch_lindblad_duration_gradient(a, ctx->stream);
    HIP_TRY(hipGetLastError());
    lb.seeds.dur.have_grad = want_grad != 0;
    return 0;
}

// The seeds' controls [seeds][nc][K_r] on the device expanded into their items, each item's own
// sub-division count, the plan, the items gathered into group order and the launches of any batch:
// results in lb.cost_out / grads / final_out in group order, lb.order / order_dev of the items.
// umax: [seeds][K_r] control maxima of the seeds; NULL on a fixed grid (as lindblad_subdivisions).
int lindblad_ensemble_launch(qocx_ctx* ctx, int seeds, const double* seed_controls, const double* umax,
                             int want_grad) {
    auto& lb = ctx->lb;
    if ((int64_t)seeds * lb.seeds.M > 0x7fffffff)
        return fail(QOCX_ERR_ARG, "seeds x ensemble members must fit in int32");
    const int items = seeds * lb.seeds.M;
    const size_t csz = (size_t)lb.nc * lb.K, total = (size_t)items * csz;
    if ((total + 255) / 256 > 0x7fffffffu) return fail(QOCX_ERR_ARG, "ensemble control arrays too large");
    if (csz > 65535u * 256u) return fail(QOCX_ERR_ARG, "control arrays too large for the driver kernels' grids");
    if (lb.ens_items.ensure(total)) return QOCX_ERR_HIP;
    const bool swp = lb.seeds.swp_B > 0;
    if (swp && seeds != lb.seeds.swp_B)
        return fail(QOCX_ERR_ARG, "a sweep takes exactly its own seed count as the batch (qocx_lindblad_set_sweep)");
    const SeedBuffers buf = lindblad_buffers(lb, seed_controls, nullptr, nullptr);
    if (swp) qocx::launch_sweep_expand(sweep_args(lb.seeds, lb.nc, buf), ctx->stream);
    else qocx::launch_ensemble_expand(ensemble_args(lb.seeds, seeds, lb.nc, buf), ctx->stream);
    HIP_TRY(hipGetLastError());
    lb.swp_seed_controls = swp ? seed_controls : nullptr;
    lb.swp_have_grads = false;
    std::vector<double> item_umax;
    if (umax) item_umax = lindblad_item_maxima(lb, seeds, umax);
    if (int rc = lindblad_launch_items(ctx, items, lb.ens_items.p, umax ? item_umax.data() : nullptr, want_grad))
        return rc;
    lb.swp_have_grads = swp && want_grad;
    return 0;
}

// The items' results back to item order (final densities into final_items [seeds][M][S] dumps) and
// folded in member order into the seeds' cost [seeds] and grads [seeds][nc][K_r].
int lindblad_ensemble_reduce(qocx_ctx* ctx, int seeds, int want_grad, double* cost, double* grads,
                             double2* final_items) {
    auto& lb = ctx->lb;
    const int items = seeds * lb.seeds.M;
    const size_t csz = (size_t)lb.nc * lb.K, md = dump_elems(lb.n);
    if (lb.ens_cost.ensure(items) || (want_grad && lb.ens_grads.ensure((size_t)items * csz))) return QOCX_ERR_HIP;
    qocx::launch_scatter_seeds(lb.cost_out.p, lb.ens_cost.p, want_grad ? lb.grads.p : nullptr, lb.ens_grads.p,
                               csz, lb.final_out.p, final_items, (size_t)lb.S * md, lb.order_dev.p, items,
                               ctx->stream);
    const SeedBuffers buf = lindblad_buffers(lb, nullptr, cost, want_grad ? grads : nullptr);
    if (lb.seeds.sweep()) qocx::launch_sweep_reduce(sweep_args(lb.seeds, lb.nc, buf), ctx->stream);
    else qocx::launch_ensemble_reduce(ensemble_args(lb.seeds, seeds, lb.nc, buf), ctx->stream);
    HIP_TRY(hipGetLastError());
    lb.ens_members_B = seeds;
    return 0;
}

// qocx_eval_lindblad with an ensemble set: controls, costs and gradients of the seeds, final densities
// of the items
int eval_lindblad_ensemble(qocx_ctx* ctx, int B, const double* controls, int want_grad, double* cost_out,
                           double* grad_out, double* final_out) {
    auto& lb = ctx->lb;
    const int S = lb.S, Kr = lb.seeds.Kr, nc = lb.nc, M = lb.seeds.M;
    const size_t csz = (size_t)nc * Kr, md = dump_elems(lb.n);
    if (!controls) return fail(QOCX_ERR_ARG, "controls is NULL");
    if ((int64_t)B * M > 0x7fffffff) return fail(QOCX_ERR_ARG, "seeds x ensemble members must fit in int32");
    const size_t items = (size_t)B * M;
    lb.have_results = false;
    if (int rc0 = lindblad_duration_refresh(ctx)) return rc0;
    std::vector<double> umax((size_t)B * Kr);
    lindblad_control_maxima(controls, B, nc, Kr, umax.data());
    if (lb.ens_seed_controls.ensure((size_t)B * csz) || lb.ens_seed_cost.ensure(B) ||
        (want_grad && lb.ens_seed_grads.ensure((size_t)B * csz)) || lb.ens_final.ensure(items * S * md))
        return QOCX_ERR_HIP;
    if (int rc2 = pinned_controls(ctx, (size_t)B * csz)) return rc2;
    memcpy(ctx->pin_controls, controls, (size_t)B * csz * sizeof(double));
    HIP_TRY(hipMemcpyAsync(lb.ens_seed_controls.p, ctx->pin_controls, (size_t)B * csz * sizeof(double),
                           hipMemcpyHostToDevice, ctx->stream));
    int rc = lindblad_ensemble_launch(ctx, B, lb.ens_seed_controls.p, umax.data(), want_grad);
    if (!rc) rc = lindblad_ensemble_reduce(ctx, B, want_grad, lb.ens_seed_cost.p, lb.ens_seed_grads.p, lb.ens_final.p);
    if (!rc) rc = lindblad_duration_finish(ctx, want_grad, lb.ens_seed_cost.p);
    if (rc) return rc;
    if (int rc3 = download_seed_results(ctx, B, csz, (size_t)M * S, lb.ens_seed_cost.p, lb.ens_seed_grads.p,
                                        lb.ens_final.p, cost_out, want_grad ? grad_out : nullptr, final_out))
        return rc3;
    time_collect(ctx);
    lb.results_stand((int)items, ctx->keep_step_states != 0);
    return 0;
}

}  // namespace

namespace qocx::host {

void lindblad_duration_tables(qocx_ctx* ctx) {
    qocx::launch_duration_tables(duration_args(ctx->lb.seeds, nullptr, nullptr), ctx->stream);
    qocx::launch_lindblad_duration_generators(lindblad_generator_args(ctx), ctx->stream);
}

int lindblad_duration_fetch(qocx_ctx* ctx) {
    auto& lb = ctx->lb;
    lb.dur_tau_h.resize((size_t)lb.seeds.swp_B);
    HIP_TRY(hipMemcpyAsync(lb.dur_tau_h.data(), lb.seeds.dur.tau.p, (size_t)lb.seeds.swp_B * sizeof(double),
                           hipMemcpyDeviceToHost, ctx->stream));
    return 0;
}

// seeds.scales_h, seeds.offsets_h and rate_l0_norm as the device holds the tables: the same single products
// of the clipped tau (a product alone is rounded once on either side)
void lindblad_duration_mirror(qocx_ctx* ctx) {
    auto& lb = ctx->lb;
    const int B = lb.seeds.swp_B, Kr = lb.seeds.Kr, J = lb.seeds.J;
    lb.seeds.scales_h.resize((size_t)B * Kr);
    lb.seeds.offsets_h.resize((size_t)B * J);
    lb.rate_l0_norm.resize((size_t)B);
    for (int b = 0; b < B; ++b) {
        const double tau = lb.dur_tau_h[b];
        for (int k = 0; k < Kr; ++k)
            lb.seeds.scales_h[(size_t)b * Kr + k] = tau * lb.dur_base_scales_h[(size_t)b * Kr + k];
        for (int j = 0; j < J; ++j)
            lb.seeds.offsets_h[(size_t)b * J + j] = tau * lb.dur_base_offsets_h[(size_t)b * J + j];
        lb.rate_l0_norm[b] = tau * lb.dur_l0_norm0[b];
    }
    lb.seeds.dur.mirror_stale = false;
}

}  // namespace qocx::host
}  // extern "C++"

int qocx_lindblad_sweep_set_durations(qocx_ctx* ctx, const double* tau, const double* base_scales,
                                      const double* base_offsets, const double* base_rate_scales, double tau_min,
                                      double tau_max, double time_weight) {
    if (!ctx || !tau) return fail(QOCX_ERR_ARG, "NULL argument");
    auto& lb = ctx->lb;
    if (!lb.has_problem || lb.seeds.swp_B == 0)
        return fail(QOCX_ERR_STATE, "no sweep set (qocx_lindblad_set_sweep before qocx_lindblad_sweep_set_durations)");
    if (lb.n > 32) return fail(QOCX_ERR_STATE, wide_only("per-seed durations (a duration sweep needs per-seed rates)"));
    if (lb.fixed_ksub > 0)
        return fail(QOCX_ERR_STATE, "a duration search needs a static problem: this one was set with stage tables "
                                    "(fixed_subdivision > 0), which hold one control-free generator per stage");
    if (!lb.ens_rates)
        return fail(QOCX_ERR_STATE, "a duration search needs per-seed rates (rate_scales of qocx_lindblad_set_sweep): "
                                    "tau_b scales the rates of seed b with its Hamiltonian");
    for (double v : lb.h0_h)
        if (v != 0.0)
            return fail(QOCX_ERR_STATE, "a duration search needs a problem whose own h0 is zero (the drift is the "
                                        "first fixed channel): the control-free part is then the dissipator alone "
                                        "and scales with tau as a whole");
    const int B = lb.seeds.swp_B, L = lb.nops;
    if (L < 1 || L > 4)
        return fail(QOCX_ERR_ARG, "a duration search takes 1 .. 4 Lindblad operators (the rate sensitivities exist for those)");
    std::vector<double> c0((size_t)B * L, 1.0);
    if (base_rate_scales) c0.assign(base_rate_scales, base_rate_scales + c0.size());
    for (double v : c0)
        if (!std::isfinite(v) || !(v >= 0)) return fail(QOCX_ERR_ARG, "base_rate_scales must be finite and >= 0");
    HIP_TRY(hipSetDevice(ctx->device));
    std::vector<double> s0, d0;
    if (int rc = set_seed_durations(lb.seeds, tau, base_scales, base_offsets, tau_min, tau_max, time_weight, ctx->stream,
                                    s0, d0))
        return rc;
    lb.dur_base_scales_h.swap(s0);
    lb.dur_base_offsets_h.swap(d0);
    // the base tables, once: every seed's control-free generators, rates and norm bound at tau = 1, built
    // as the plain setter builds its own (a later call of the same search with the same c0 - the host loop
    // sets tau every iteration - keeps them)
    if (!lb.seeds.dur.set || lb.dur_base_rates_h != c0) {
        std::vector<double2> img;
        std::vector<double> gam;
        lb.seeds.dur.set = false;
        rate_tables_host(lb, B, c0.data(), img, gam, lb.dur_l0_norm0);
        if (lb.dur_base_a0.upload(img, ctx->stream) || lb.dur_base_gammas.upload(gam, ctx->stream) ||
            lb.rate_a0.ensure(img.size()) || lb.rate_gammas.ensure(gam.size()) ||
            lb.dur_base_rates.upload(c0, ctx->stream))
            return QOCX_ERR_HIP;
        lb.dur_base_rates_h = c0;
    }
    lindblad_duration_tables(ctx);
    HIP_TRY(hipGetLastError());
    if (int rc = lindblad_duration_fetch(ctx)) return rc;
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    lindblad_duration_mirror(ctx);
    lb.seeds.dur.set = true;
    lb.seeds.dur.have_grad = false;
    lb.drop_resident();  // controls must be uploaded again, and the driver begun again
    return 0;
}

int qocx_lindblad_sweep_download_durations(qocx_ctx* ctx, double* tau_out, double* tau_grad_out) {
    if (!ctx) return fail(QOCX_ERR_ARG, "ctx is NULL");
    auto& lb = ctx->lb;
    if (!lb.seeds.dur.set) return fail(QOCX_ERR_STATE, "no durations set (qocx_lindblad_sweep_set_durations)");
    HIP_TRY(hipSetDevice(ctx->device));
    return download_seed_durations(lb.seeds, ctx->stream, lb.have_results && lb.swp_have_grads && lb.seeds.dur.have_grad,
                                   tau_out, tau_grad_out);
}

int qocx_eval_lindblad(qocx_ctx* ctx, int32_t batch, const double* controls, int32_t want_grad,
                       double* cost_out, double* grad_out, double* final_out) {
    if (!ctx) return fail(QOCX_ERR_ARG, "ctx is NULL");
    auto& lb = ctx->lb;
    if (!lb.has_problem) return fail(QOCX_ERR_STATE, "no Lindblad problem set");
    if (batch < 1) return fail(QOCX_ERR_ARG, "batch must be >= 1");
    HIP_TRY(hipSetDevice(ctx->device));
    const int n = lb.n, S = lb.S, K = lb.K, nc = lb.nc, B = batch;
    const size_t md = dump_elems(n);
    want_grad = (want_grad && K > 0) ? 1 : 0;
    if (lb.seeds.M > 0) return eval_lindblad_ensemble(ctx, B, controls, want_grad, cost_out, grad_out, final_out);
    if (K > 0 && !controls) return fail(QOCX_ERR_ARG, "controls is NULL");
    const bool trace_host = qocx::diag_getenv("QOCX_TRACE_HOST") != nullptr;
    auto now_ms = [] {
        timespec ts;
        clock_gettime(CLOCK_MONOTONIC, &ts);
        return ts.tv_sec * 1e3 + ts.tv_nsec * 1e-6;
    };
    const double t_enter = now_ms();
    double t_alloc = 0, t_enq = 0, t_sync = 0;

    std::vector<double> umax(std::max<size_t>(1, (size_t)B * K));
    lindblad_control_maxima(controls, B, nc, K, umax.data());
    std::vector<int> ksub_of;
    LindbladPlan plan;
    int rc = lindblad_subdivisions(ctx, B, umax.data(), ksub_of);
    if (!rc) rc = lindblad_plan(ctx, want_grad, ksub_of, plan);
    if (rc) return rc;
    const size_t csz = (size_t)nc * K;
    if (K > 0) {
        // gathered group by group into the pinned staging buffer
        const size_t total = (size_t)B * csz;
        if (int rc2 = pinned_controls(ctx, total)) return rc2;
        for (int pos = 0; pos < B; ++pos)
            memcpy(ctx->pin_controls + (size_t)pos * csz, controls + (size_t)lb.order[pos] * csz,
                   csz * sizeof(double));
        HIP_TRY(hipMemcpyAsync(lb.controls.p, ctx->pin_controls, total * sizeof(double),
                               hipMemcpyHostToDevice, ctx->stream));
    }
    t_alloc = now_ms();
    rc = lindblad_launch_groups(ctx, want_grad, plan);
    if (rc) return rc;
    t_enq = now_ms();
    std::vector<double2> fin(final_out ? (size_t)B * S * md : 0);
    std::vector<double> cst(B), grd(want_grad && grad_out ? (size_t)B * csz : 0);
    HIP_TRY(hipMemcpyAsync(cst.data(), lb.cost_out.p, (size_t)B * sizeof(double),
                           hipMemcpyDeviceToHost, ctx->stream));
    if (!grd.empty())
        HIP_TRY(hipMemcpyAsync(grd.data(), lb.grads.p, grd.size() * sizeof(double),
                               hipMemcpyDeviceToHost, ctx->stream));
    if (final_out)
        HIP_TRY(hipMemcpyAsync(fin.data(), lb.final_out.p, fin.size() * sizeof(double2),
                               hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    t_sync = now_ms();
    time_collect(ctx);
    if (trace_host)
        fprintf(stderr, "qocx_eval_lindblad B=%d: set-up %.2f ms, enqueue %.2f ms, wait %.2f ms\n", B,
                t_alloc - t_enter, t_enq - t_alloc, t_sync - t_enq);
    for (int pos = 0; pos < B; ++pos) {
        const int b = lb.order[pos];
        if (cost_out) cost_out[b] = cst[pos];
        if (!grd.empty())
            memcpy(grad_out + (size_t)b * csz, grd.data() + (size_t)pos * csz, csz * sizeof(double));
        if (final_out)
            for (int s = 0; s < S; ++s)
                from_c_dump(fin.data() + ((size_t)pos * S + s) * md, n,
                            final_out + ((size_t)b * S + s) * n * n * 2);
    }
    lb.results_stand(B, ctx->keep_step_states != 0);
    return 0;
}

int qocx_set_density_cotangents(qocx_ctx* ctx, int32_t batch, int32_t count, const int32_t* steps,
                                const double* bars) {
    if (!ctx) return fail(QOCX_ERR_ARG, "ctx is NULL");
    auto& lb = ctx->lb;
    if (!lb.has_problem) return fail(QOCX_ERR_STATE, "no Lindblad problem set");
    if (count <= 0) {
        lb.inj_count = 0;
        return 0;
    }
    if (batch < 1 || !steps || !bars) return fail(QOCX_ERR_ARG, "bad argument");
    if (lb.seeds.M > 0)
        return fail(QOCX_ERR_STATE, lb.seeds.swp_B > 0
                                        ? "density cotangents are not taken with a sweep (qocx_lindblad_set_sweep)"
                                        : "density cotangents are not taken with an ensemble (qocx_lindblad_set_ensemble)");
    std::vector<bool> seen(lb.nsteps + 1, false);
    for (int c = 0; c < count; ++c) {
        if (steps[c] < 1 || steps[c] > lb.nsteps || seen[steps[c]])
            return fail(QOCX_ERR_ARG, "cotangent steps must be distinct and in 1..N-1");
        seen[steps[c]] = true;
    }
    lb.inj_steps.assign(steps, steps + count);
    lb.inj_host.assign(bars, bars + (size_t)batch * count * lb.S * lb.n * lb.n * 2);
    lb.inj_count = count;
    lb.inj_batch = batch;
    return 0;
}

int qocx_download_step_densities(qocx_ctx* ctx, double* densities_out) {
    if (!ctx || !densities_out) return fail(QOCX_ERR_ARG, "NULL argument");
    auto& lb = ctx->lb;
    if (!lb.have_results || !lb.have_steps)
        return fail(QOCX_ERR_STATE, "step densities were not kept (qocx_set_keep_step_states)");
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t per_seed = (size_t)(lb.nsteps + 1) * lb.S;
    const size_t md = dump_elems(lb.n);
    std::vector<double2> tmp((size_t)lb.B * per_seed * md);
    HIP_TRY(hipMemcpy(tmp.data(), lb.step_densities.p, tmp.size() * sizeof(double2),
                      hipMemcpyDeviceToHost));
    for (int pos = 0; pos < lb.B; ++pos)
        for (size_t v = 0; v < per_seed; ++v)
            from_c_dump(tmp.data() + ((size_t)pos * per_seed + v) * md, lb.n,
                        densities_out + ((size_t)lb.order[pos] * per_seed + v) * lb.n * lb.n * 2);
    return 0;
}

// ---- the Lindblad multi-start driver: resident controls, results and optimizer states ------------

int qocx_lindblad_upload_controls(qocx_ctx* ctx, int32_t batch, const double* controls) {
    if (!ctx || !controls) return fail(QOCX_ERR_ARG, "NULL argument");
    auto& lb = ctx->lb;
    if (!lb.has_problem || lb.K < 1)
        return fail(QOCX_ERR_STATE, "qocx_lindblad_upload_controls needs a Lindblad problem with controls");
    if (batch < 1) return fail(QOCX_ERR_ARG, "batch must be >= 1");
    if (lb.seeds.swp_B > 0 && batch != lb.seeds.swp_B)
        return fail(QOCX_ERR_ARG, "a sweep takes exactly its own seed count as the batch (qocx_lindblad_set_sweep)");
    // (with an ensemble the caller's array holds the seeds' K_r channels)
    const int Ks = lb.seed_channels();
    const size_t csz = (size_t)lb.nc * Ks;
    if (csz > 65535u * 256u) return fail(QOCX_ERR_ARG, "control arrays too large for the driver kernels' grids");
    if ((int64_t)batch * (int64_t)lb.seed_items() > 0x7fffffff)
        return fail(QOCX_ERR_ARG, "seeds x ensemble members must fit in int32");
    HIP_TRY(hipSetDevice(ctx->device));
    if (lb.res_controls.ensure((size_t)batch * csz)) return QOCX_ERR_HIP;
    HIP_TRY(hipMemcpyAsync(lb.res_controls.p, controls, (size_t)batch * csz * sizeof(double),
                           hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));  // controls is the caller's memory
    // the host has these controls: their maxima cost nothing here and spare eval_resident a round trip
    lb.umax_host.assign((size_t)batch * Ks, 0.0);
    lindblad_control_maxima(controls, batch, lb.nc, Ks, lb.umax_host.data());
    lb.res_B = batch;
    lb.resident_controls_moved(true);
    lb.swp_have_grads = false;  // (the seed controls of the last evaluation may just have been overwritten)
    return 0;
}

int qocx_eval_lindblad_resident(qocx_ctx* ctx, int32_t want_grad) {
    if (!ctx) return fail(QOCX_ERR_ARG, "ctx is NULL");
    auto& lb = ctx->lb;
    if (!lb.has_problem || lb.res_B < 1)
        return fail(QOCX_ERR_STATE, "no resident Lindblad controls (qocx_lindblad_upload_controls)");
    HIP_TRY(hipSetDevice(ctx->device));
    // (K: the seeds' channels - with an ensemble K_r, and `items` evaluated items per seed)
    const int B = lb.res_B, K = lb.seed_channels(), S = lb.S;
    const size_t csz = (size_t)lb.nc * K, md = dump_elems(lb.n), items = lb.seed_items();
    const bool ens = lb.seeds.M > 0;
    want_grad = want_grad ? 1 : 0;
    lb.res_have_results = false;
    // (a duration search whose tau has moved since the clip: tau comes back with the maxima below)
    const bool refresh = lb.seeds.dur.set && lb.seeds.dur.mirror_stale;
    if (refresh) {
        lindblad_duration_tables(ctx);
        HIP_TRY(hipGetLastError());
        if (int rc0 = lindblad_duration_fetch(ctx)) return rc0;
    }
    // the sub-division decision needs the control maxima on the host, except on a fixed grid
    if (lb.fixed_ksub == 0 && !lb.umax_valid) {
        if (lb.umax.ensure((size_t)B * K)) return QOCX_ERR_HIP;
        lb.umax_host.resize((size_t)B * K);
        qocx::launch_control_maxima(lb.res_controls.p, B, lb.nc, K, lb.umax.p, ctx->stream);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(lb.umax_host.data(), lb.umax.p, (size_t)B * K * sizeof(double),
                               hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        lb.umax_valid = true;
    } else if (refresh) {
        HIP_TRY(hipStreamSynchronize(ctx->stream));
    }
    if (refresh) lindblad_duration_mirror(ctx);
    const double* umax = lb.fixed_ksub == 0 ? lb.umax_host.data() : nullptr;
    if (lb.res_cost.ensure(B) || lb.res_grads.ensure((size_t)B * csz) ||
        lb.res_final.ensure((size_t)B * items * S * md))
        return QOCX_ERR_HIP;
    if (ens) {
        // the member items of the seeds' current controls (expanded anew: the driver may have moved
        // them), evaluated as any batch, then reduced in member order into the seeds' results
        int rc = lindblad_ensemble_launch(ctx, B, lb.res_controls.p, umax, want_grad);
        if (!rc) rc = lindblad_ensemble_reduce(ctx, B, want_grad, lb.res_cost.p, lb.res_grads.p, lb.res_final.p);
        if (rc) return rc;
    } else {
        if (int rc = lindblad_launch_items(ctx, B, lb.res_controls.p, umax, want_grad)) return rc;
        qocx::launch_scatter_seeds(lb.cost_out.p, lb.res_cost.p, want_grad ? lb.grads.p : nullptr,
                                   lb.res_grads.p, csz, lb.final_out.p, lb.res_final.p, (size_t)S * md,
                                   lb.order_dev.p, B, ctx->stream);
        HIP_TRY(hipGetLastError());
    }
    if (lb.control_costs.count > 0) {  // the costs of the controls, once per seed on its resident controls
        ControlCosts& cc = lb.control_costs;
        if (int rc2 = run_control_costs(ctx, cc, B, lb.nc, K, lb.res_controls.p, want_grad != 0)) return rc2;
        qocx::launch_add_control_costs(lb.res_cost.p, cc.cost.p, want_grad ? lb.res_grads.p : nullptr, cc.grad.p,
                                       B, csz, ctx->stream);
        HIP_TRY(hipGetLastError());
    }
    // (a duration search: the price of time comes after the costs of the controls)
    if (int rc3 = lindblad_duration_finish(ctx, want_grad, lb.res_cost.p)) return rc3;
    if (ctx->timing) {  // (the events of the launches are read once they have run)
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        time_collect(ctx);
    }
    lb.results_stand(B * (int)items, ctx->keep_step_states != 0);
    lb.res_have_results = true;
    lb.res_have_grads = want_grad != 0;
    return 0;
}

int qocx_lindblad_download_results(qocx_ctx* ctx, double* cost_out, double* grad_out, double* final_out) {
    if (!ctx) return fail(QOCX_ERR_ARG, "ctx is NULL");
    auto& lb = ctx->lb;
    if (!lb.res_have_results) return fail(QOCX_ERR_STATE, "no resident Lindblad evaluation results");
    if (grad_out && !lb.res_have_grads) return fail(QOCX_ERR_STATE, "the last evaluation had no gradients");
    HIP_TRY(hipSetDevice(ctx->device));
    // (with an ensemble: the seeds' K_r channels, the final densities of every item)
    return download_seed_results(ctx, lb.res_B, (size_t)lb.nc * lb.seed_channels(), lb.S * lb.seed_items(),
                                 lb.res_cost.p, lb.res_grads.p, lb.res_final.p, cost_out, grad_out, final_out);
}

int qocx_lindblad_download_costs(qocx_ctx* ctx, double* cost_out) {
    if (!ctx || !cost_out) return fail(QOCX_ERR_ARG, "NULL argument");
    return qocx_lindblad_download_results(ctx, cost_out, nullptr, nullptr);
}

int qocx_lindblad_ensemble_download_members(qocx_ctx* ctx, double* cost_out) {
    if (!ctx || !cost_out) return fail(QOCX_ERR_ARG, "NULL argument");
    auto& lb = ctx->lb;
    if (lb.seeds.M == 0 || lb.seeds.swp_B > 0) return fail(QOCX_ERR_STATE, "no ensemble set (qocx_lindblad_set_ensemble)");
    if (lb.ens_members_B < 1 || !lb.have_results) return fail(QOCX_ERR_STATE, "no evaluation results");
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipMemcpyAsync(cost_out, lb.ens_cost.p, (size_t)lb.ens_members_B * lb.seeds.M * sizeof(double),
                           hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return 0;
}

int qocx_lindblad_sweep_download_sensitivities(qocx_ctx* ctx, double* scales_out, double* offsets_out,
                                               double* rates_out) {
    if (!ctx) return fail(QOCX_ERR_ARG, "ctx is NULL");
    auto& lb = ctx->lb;
    if (lb.seeds.swp_B == 0) return fail(QOCX_ERR_STATE, "no sweep set (qocx_lindblad_set_sweep)");
    // (the seed controls on the device are those of the evaluation exactly while its results stand: the
    // resident ones move with qocx_lindblad_opt_clip / _step, which clear res_have_results)
    const bool resident = lb.swp_seed_controls != nullptr && lb.swp_seed_controls == lb.res_controls.p;
    if (!lb.have_results || !lb.swp_have_grads || lb.swp_seed_controls == nullptr ||
        (resident && !(lb.res_have_results && lb.res_have_grads)))
        return fail(QOCX_ERR_STATE, "sweep sensitivities need an evaluation with gradients");
    if (rates_out && !lb.swp_rates_ok)
        return fail(QOCX_ERR_STATE, "no rate sensitivities: the last evaluation was not asked for them "
                                    "(qocx_lindblad_sweep_want_rate_sensitivities), or a piece of it did not run "
                                    "two-sided with 1 .. 4 operators");
    HIP_TRY(hipSetDevice(ctx->device));
    const int B = lb.seeds.swp_B, L = lb.nops;
    const size_t ns = (size_t)B * lb.seeds.Kr, no = (size_t)B * lb.seeds.J;
    if (lb.seeds.scale_sens.ensure(ns) || lb.seeds.offset_sens.ensure(no)) return QOCX_ERR_HIP;
    // (the items' gradients in item order are the reduce launch's input, ens_grads)
    const SeedBuffers buf = lindblad_buffers(lb, lb.swp_seed_controls, nullptr, nullptr);
    qocx::launch_sweep_sensitivity(sweep_args(lb.seeds, lb.nc, buf), ctx->stream);
    HIP_TRY(hipGetLastError());
    if (scales_out)
        HIP_TRY(hipMemcpyAsync(scales_out, lb.seeds.scale_sens.p, ns * sizeof(double), hipMemcpyDeviceToHost,
                               ctx->stream));
    if (offsets_out && no > 0)
        HIP_TRY(hipMemcpyAsync(offsets_out, lb.seeds.offset_sens.p, no * sizeof(double), hipMemcpyDeviceToHost,
                               ctx->stream));
    std::vector<double> launched(rates_out ? (size_t)B * L : 0);
    if (rates_out)
        HIP_TRY(hipMemcpyAsync(launched.data(), lb.swp_rate_sens.p, launched.size() * sizeof(double),
                               hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (rates_out)  // launch order -> seed order
        for (int pos = 0; pos < B; ++pos)
            memcpy(rates_out + (size_t)lb.order[pos] * L, launched.data() + (size_t)pos * L, L * sizeof(double));
    return 0;
}

}  // extern "C"
