// qocx_action.hip - the matrix-free route of ONE state per seed, Hermitian H, 17 <= n <= 32: the sweeps
// apply exp(a_j), a_j = -i dt H(u_mid), to their vector by the truncated Taylor series (Al-Mohy &
// Higham 2011, qocx_action.h) instead of solving with the factors of a Pade denominator. Nothing is
// factored and no matrix is stored: n^2 work per Taylor term, m terms per step, against the n^3 of a
// Pade step that only ever served one vector.
//
//   forward   v_0 = psi,     v_p = a v_(p-1) / p,   psi'   = sum_{p=0..m} v_p      (keeps v_0 .. v_(m-1))
//   adjoint   w_0 = lambda', w_p = -a w_(p-1) / p,  lambda = sum_{p=0..m} w_p      (a^H = -a; keeps w_0 .. w_(m-1))
//   generator cotangent   abar = sum_{i<m} w_i rho_i^H,  rho_i = sum_{l<m-i} c_il v_l,  c_il = i! l! / (i + l + 1)!
//   - the exact reverse rule of psi' = T_m(a) psi: d(a^p)/p! in direction E is sum_{i+l=p-1} a^i E a^l / p!,
//   and a^i / i!, a^l / l! applied to lambda', psi are w_i (up to (-1)^i (-1)^i = 1 through a^H = -a), v_l.
//   step gradient   gamma_k = sum conj(abar) (.) (-i dt G_k), a complex pair per (step, k) as K3 leaves
//   it under the unit adjoint (KrylovArgs::gstep): the adjoint runs on the target and the scatter
//   kernel applies the cost's scalar.
//
// The degree m of a step comes from the step table (bits 24..29 of its entry), decided from the same
// bound as the Pade order. A step's arithmetic depends on nothing but its inputs, so results are bit
// identical however the steps are cut into launches.
#include "qocx_sweep_common.h"
#include "qocx_action.h"

namespace qocx {

namespace action {

constexpr int MMAX = QOCX_ACTION_MAX_DEGREE;

struct InvTable {  // 1 / p
    double v[MMAX + 2];
    constexpr InvTable() : v{} {
        for (int p = 1; p < MMAX + 2; ++p) v[p] = 1.0 / (double)p;
    }
};
struct CoefTable {  // c_il = i! l! / (i + l + 1)! = c_(i,l-1) l / (i + l + 1), c_i0 = 1 / (i + 1)
    double c[MMAX * MMAX];
    constexpr CoefTable() : c{} {
        for (int i = 0; i < MMAX; ++i) {
            double v = 1.0 / (double)(i + 1);
            c[i * MMAX] = v;
            for (int l = 1; l < MMAX; ++l) {
                v = v * (double)l / (double)(i + l + 1);
                c[i * MMAX + l] = v;
            }
        }
    }
};
__device__ __constant__ const InvTable INV_P = InvTable();
__device__ __constant__ const CoefTable COEF = CoefTable();

// Four columns K0 .. K0 + 3 of y += a x with the broadcast of x INSIDE the multiply-add (v_fmac_f64_dpp
// row_newbcast, as the triangular solves of qocx_sweep_core.h): lane k of every row of 16 lanes holds
// x[column k of the lane's block], so a column costs four instructions and no trip through LDS. Two
// accumulator pairs in turn. (s_nop: a DPP operand may not be read in the two cycles after the VALU
// instruction that wrote it, and the compiler does not look into the block.)
template <int K0>
__device__ __forceinline__ void dpp_cmac4(double& r0, double& i0, double& r1, double& i1, double xr, double xi,
                                          double a0r, double a0i, double a1r, double a1i, double a2r,
                                          double a2i, double a3r, double a3i) {
#define QOCX_ACTION_CMAC(R, I, AR, AI, BC)                                                        \
    "v_fmac_f64_dpp %[" R "], %[xr], %[" AR "] row_newbcast:%[" BC "] row_mask:0xf bank_mask:0xf\n\t"  \
    "v_fmac_f64_dpp %[" I "], %[xi], %[" AR "] row_newbcast:%[" BC "] row_mask:0xf bank_mask:0xf\n\t"  \
    "v_fmac_f64_dpp %[" R "], -%[xi], %[" AI "] row_newbcast:%[" BC "] row_mask:0xf bank_mask:0xf\n\t" \
    "v_fmac_f64_dpp %[" I "], %[xr], %[" AI "] row_newbcast:%[" BC "] row_mask:0xf bank_mask:0xf\n\t"
    asm("s_nop 1\n\t" QOCX_ACTION_CMAC("r0", "i0", "a0r", "a0i", "k0") QOCX_ACTION_CMAC("r1", "i1", "a1r", "a1i", "k1")
            QOCX_ACTION_CMAC("r0", "i0", "a2r", "a2i", "k2") QOCX_ACTION_CMAC("r1", "i1", "a3r", "a3i", "k3")
        : [r0] "+v"(r0), [i0] "+v"(i0), [r1] "+v"(r1), [i1] "+v"(i1)
        : [xr] "v"(xr), [xi] "v"(xi), [a0r] "v"(a0r), [a0i] "v"(a0i), [a1r] "v"(a1r), [a1i] "v"(a1i),
          [a2r] "v"(a2r), [a2i] "v"(a2i), [a3r] "v"(a3r), [a3i] "v"(a3i), [k0] "i"(K0), [k1] "i"(K0 + 1),
          [k2] "i"(K0 + 2), [k3] "i"(K0 + 3));
#undef QOCX_ACTION_CMAC
}

// x on the rows of 16 lanes a lane group multiplies with: lane group 0 (lanes 0 .. 31) the entries
// 0 .. 15 in both of its rows, lane group 1 the entries 16 .. 31. In: lane (h, i) holds x[i].
__device__ __forceinline__ double spread_halves(double v, int h) {
    const unsigned lo = (unsigned)__double2loint(v), hi = (unsigned)__double2hiint(v);
    // (swap of a register with itself: [0] the even rows in every row pair, [1] the odd rows)
    auto a = __builtin_amdgcn_permlane16_swap(lo, lo, false, false);
    auto b = __builtin_amdgcn_permlane16_swap(hi, hi, false, false);
    return h == 0 ? make_f64((int)a[0], (int)b[0]) : make_f64((int)a[1], (int)b[1]);
}

// KR: the G_k images held in registers beside H0 (those of further controls are read per step)
template <int NB, int KR>
__global__ __launch_bounds__(64) void action_sweep_kernel(ActionArgs args) {
    typedef Geo<NB> G;
    constexpr int NP = G::NP, CPL = G::CPL, H = G::H;
    __shared__ __attribute__((aligned(16))) double2 turn[NP];  // the vector where the cost code reads / writes it
    const SweepArgs& sw = args.sw;
    const int b = blockIdx.x;
    const int lane = lane_id(), i = lane % NP, h = lane / NP;
    const bool g0 = (h == 0);
    const int nsteps = sw.nsteps, K = args.K, m_max = args.m_max;
    const int jb = sw.j_begin, je = sw.j_end;
    const double dt = args.dt;
    __builtin_amdgcn_s_setprio(3);  // the serial chain of the evaluation goes first on its SIMD

    // -i dt H0 and -i dt G_k, lane (h, i): row i, columns 16 h + cc - the block its lane group multiplies
    // (re, im of -i dt (x + i y) = dt y, -dt x). Element (i, c) of a column-major image sits at
    // (c / H) 64 + (c % H) NP + i.
    static_assert(NB == 2 && CPL == 16, "one block of 16 columns per lane group");
    auto image_at = [&](int cc) { return ((16 * h + cc) / H) * 64 + ((16 * h + cc) % H) * NP + i; };
    double h0r[CPL], h0i[CPL], gr[KR][CPL], gi[KR][CPL];
#pragma unroll
    for (int cc = 0; cc < CPL; ++cc) {
        const double2 e = args.h0_rimg[image_at(cc)];
        h0r[cc] = dt * e.y;
        h0i[cc] = -dt * e.x;
    }
#pragma unroll
    for (int k = 0; k < KR; ++k)
#pragma unroll
        for (int cc = 0; cc < CPL; ++cc) {
            const double2 e = k < K ? args.g_rimg[(size_t)k * G::MAT + image_at(cc)] : make_double2(0, 0);
            gr[k][cc] = dt * e.y;
            gi[k][cc] = -dt * e.x;
        }

    const int* words = sw.s_arr + (size_t)b * nsteps;
    const double* u_b = args.ustep + (size_t)b * nsteps * K;
    double are[CPL], aim[CPL];
    auto build = [&](int step) __attribute__((always_inline)) {
        const double* u = u_b + (size_t)step * K;
#pragma unroll
        for (int cc = 0; cc < CPL; ++cc) {
            are[cc] = h0r[cc];
            aim[cc] = h0i[cc];
        }
#pragma unroll
        for (int k = 0; k < KR; ++k)
            if (k < K) {
                const double uk = u[k];
#pragma unroll
                for (int cc = 0; cc < CPL; ++cc) {
                    are[cc] = fma(uk, gr[k][cc], are[cc]);
                    aim[cc] = fma(uk, gi[k][cc], aim[cc]);
                }
            }
        for (int k = KR; k < K; ++k) {
            const double uk = u[k] * dt;
#pragma unroll
            for (int cc = 0; cc < CPL; ++cc) {
                const double2 e = args.g_rimg[(size_t)k * G::MAT + image_at(cc)];
                are[cc] = fma(uk, e.y, are[cc]);
                aim[cc] = fma(-uk, e.x, aim[cc]);
            }
        }
    };
    // y = a x, x in registers (every lane group holds x[i]): the lane group's 16 columns, then the sum
    // of the two lane groups of the row
    auto matvec = [&](double xr, double xi, double& yr, double& yi) __attribute__((always_inline)) {
        const double sxr = spread_halves(xr, h), sxi = spread_halves(xi, h);
        double s0r = 0, s0i = 0, s1r = 0, s1i = 0;
        for_each_const(
            [&](auto Q) __attribute__((always_inline)) {
                constexpr int k = 4 * decltype(Q)::value;
                dpp_cmac4<k>(s0r, s0i, s1r, s1i, sxr, sxi, are[k], aim[k], are[k + 1], aim[k + 1],
                             are[k + 2], aim[k + 2], are[k + 3], aim[k + 3]);
            },
            std::make_integer_sequence<int, 4>{});
        yr = sum_groups<NB>(s0r + s1r);
        yi = sum_groups<NB>(s0i + s1i);
    };
    // One step: the vector (vr, vi) - every lane group holds it - becomes sum_p (sign a)^p / p! v; the
    // terms 0 .. m - 1 go to `keep`. False: the degree is outside the buffers.
    double vr = 0, vi = 0;
    int count = 0;  // lane l: steps at degree l
    auto step_apply = [&](int step, double sign, double2* keep_base) __attribute__((always_inline)) {
        const int m = step_degree(words[step]);
        if (m < 1 || m > m_max) return false;
        build(step);
        double2* keep = keep_base ? keep_base + ((size_t)b * nsteps + step) * m_max * NP : nullptr;
        count += (lane == m) ? 1 : 0;
        double sr = vr, si = vi;
        for (int p = 1; p <= m; ++p) {
            if (keep != nullptr && g0) keep[(size_t)(p - 1) * NP + i] = make_double2(vr, vi);
            double yr, yi;
            matvec(vr, vi, yr, yi);
            const double f = sign * INV_P.v[p];
            vr = f * yr;
            vi = f * yi;
            sr += vr;
            si += vi;
        }
        vr = sr;
        vi = si;
        return true;
    };
    auto refuse = [&]() {  // never clamped: the host runs the evaluation again on the Pade route
        if (lane == 0) atomicOr(sw.status, 8);
    };

    // ---- forward sweep ----------------------------------------------------------------------
    if (sw.phase & 1) {
        const double2 p0 = jb == 0 ? sw.psi0[i] : args.carry_f[(size_t)b * NP + i];
        vr = p0.x;
        vi = p0.y;
        for (int step = jb; step < je; ++step)
            if (!step_apply(step, 1.0, args.kv_f)) {
                refuse();
                return;
            }
        if (count > 0 && lane <= MMAX) atomicAdd(args.degree_counts + lane, count);
        if (je == nsteps) {
            turn[i] = make_double2(vr, vi);  // (every lane group holds the same value: all store)
            wave_sync();
            const double cost = eval_costs<NB>(sw, false, true, turn, nullptr, h, i);
            if (sw.unit_adjoint && sw.want_grad) unit_adjoint_scales<NB>(sw, turn, b, h, i);
            if (g0) sw.final_out[(size_t)b * NP + i] = make_double2(vr, vi);
            if (lane == 0) sw.cost_out[b] = cost;
        } else if (g0) {
            args.carry_f[(size_t)b * NP + i] = make_double2(vr, vi);
        }
    }
    if (!(sw.phase & 2)) return;

    // ---- adjoint sweep: the back-propagated target (unit adjoint) ------------------------------
    wave_sync();
    if (je == nsteps) {
        unit_adjoint_seed<NB>(sw, turn, 0, 1, h, i);
        wave_sync();
        const double2 t = turn[i];
        vr = t.x;
        vi = t.y;
    } else {
        const double2 t = sw.lam_buf[(size_t)b * NP + i];
        vr = t.x;
        vi = t.y;
    }
    for (int step = je - 1; step >= jb; --step)
        if (!step_apply(step, -1.0, args.kv_b)) {
            refuse();
            return;
        }
    if (jb > 0 && g0) sw.lam_buf[(size_t)b * NP + i] = make_double2(vr, vi);
}

// One wave per (step, seed). LDS: v_0 .. v_(m-1) [m_max][NP], then two slots for the current rho.
template <int NB>
__global__ __launch_bounds__(64, 3) void action_grad_kernel(ActionGradArgs args) {
    typedef Geo<NB> G;
    constexpr int NP = G::NP, CPL = G::CPL, H = G::H;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double2* vl = reinterpret_cast<double2*>(smem);
    double2* rho = vl + (size_t)args.m_max * NP;
    const int step = args.step0 + blockIdx.x, b = blockIdx.y;
    const int lane = lane_id(), i = lane % NP, h = lane / NP;
    const int K = args.K;
    const size_t idx = (size_t)b * args.nsteps + step;
    const int m = step_degree(args.s_arr[idx]);
    if (m < 1 || m > args.m_max) return;  // (the sweeps have raised the status bit)
    const double2* vf = args.kv_f + idx * args.m_max * NP;
    const double2* wb = args.kv_b + idx * args.m_max * NP;
    for (int l = h; l < m; l += H) vl[l * NP + i] = vf[(size_t)l * NP + i];
    double abr[CPL], abi[CPL];
#pragma unroll
    for (int cc = 0; cc < CPL; ++cc) {
        abr[cc] = 0;
        abi[cc] = 0;
    }
    wave_sync();
    double2 tv = wb[i];
    for (int ii = 0; ii < m; ++ii) {
        // rho_ii: the lane groups share the terms, l = h, h + H, ...
        double rr = 0, ri = 0;
        for (int l = h; l < m - ii; l += H) {
            const double c = COEF.c[ii * MMAX + l];
            const double2 v = vl[l * NP + i];
            rr = fma(c, v.x, rr);
            ri = fma(c, v.y, ri);
        }
        rr = sum_groups<NB>(rr);
        ri = sum_groups<NB>(ri);
        double2* slot = rho + (ii & 1) * NP;  // two slots in turn: one sync per term
        slot[i] = make_double2(rr, ri);
        wave_sync();
        const double2 w = tv;
        if (ii + 1 < m) tv = wb[(size_t)(ii + 1) * NP + i];
#pragma unroll
        for (int cc = 0; cc < CPL; ++cc) {
            const double2 r = slot[cc * H + h];
            // w * conj(rho)
            abr[cc] = fma(w.y, r.y, fma(w.x, r.x, abr[cc]));
            abi[cc] = fma(-w.x, r.y, fma(w.y, r.x, abi[cc]));
        }
    }
    // gamma_k = sum conj(abar) E_k, E_k = -i dt G_k (krylov_grad_body, unit adjoint)
    const double dts = args.dt;
    for (int k = 0; k < K; ++k) {
        double acc = 0, acc_im = 0;
#pragma unroll
        for (int cc = 0; cc < CPL; ++cc) {
            const double2 e = args.g_rimg[(size_t)k * G::MAT + cc * 64 + lane];
            acc = fma(abi[cc], -dts * e.x, fma(abr[cc], dts * e.y, acc));
            acc_im = fma(abi[cc], -dts * e.y, fma(abr[cc], -dts * e.x, acc_im));
        }
        acc = wave_sum(acc);
        acc_im = wave_sum(acc_im);
        if (lane == 0) {
            args.gstep[(idx * K + k) * 2] = acc;
            args.gstep[(idx * K + k) * 2 + 1] = acc_im;
        }
    }
}

}  // namespace action

int action_grad_lds_bytes(int m_max) { return (m_max + 2) * Geo<2>::NP * (int)sizeof(double2); }

void launch_action_sweep(const ActionArgs& a, int batch, hipStream_t st) {
    if (batch <= 0 || a.sw.j_end <= a.sw.j_begin) return;
    hipLaunchKernelGGL((action::action_sweep_kernel<2, 2>), dim3(batch), dim3(64), 0, st, a);
}

void launch_action_grad(const ActionGradArgs& a, int nsteps, int batch, hipStream_t st) {
    if (batch <= 0 || nsteps <= 0) return;
    hipLaunchKernelGGL((action::action_grad_kernel<2>), dim3(nsteps, batch), dim3(64),
                       action_grad_lds_bytes(a.m_max), st, a);
}

}  // namespace qocx
