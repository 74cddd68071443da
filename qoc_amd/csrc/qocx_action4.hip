// qocx_action4.hip - the matrix-free route of qocx_action.hip at 33 <= n <= 64 (knob "action" = 2): the
// same truncated Taylor series, step degrees, buffers and reverse rule, for matrices that no longer fit
// the registers of one wave. Every image and vector of these sizes is padded to NP = 64 (qocx_api.hip).
// A workgroup of NW waves (NW = 3: n <= 48, NW = 4: n <= 64) serves one (seed, direction): wave w holds
// the columns 16 w .. 16 w + 15 of -i dt H0, of -i dt G_k (k < KR) and of the built a_j, lane i their
// row i. (n <= 48: the columns 48 .. 63 are zero and no wave is spent on them.)
//
//   per Taylor term   wave w: y_w = a[:, 16 w .. 16 w + 15] x[16 w .. 16 w + 15]  (v_fmac_f64_dpp row_newbcast,
//                     as qocx_action.hip) -> LDS slot [w][64]; ONE workgroup barrier; every wave then adds
//                     the NW partial vectors in the order w = 0 .. NW - 1, once at lane = row (the term, the
//                     running sum) and once at the indices of its own column block (the next operand).
//
// Every wave holds bit-identical sums, nothing is added atomically, and a step's arithmetic depends on
// nothing but its inputs: results are bit identical however the steps are cut into launches. Two sets
// of partial slots in turn (the parity runs on across the steps), so one barrier per term suffices.
// Rows n .. 63 of the images are zero, so the padding entries of every vector stay exact zeros.
#include "qocx_sweep_common.h"
#include "qocx_action.h"

namespace qocx {

namespace action4 {

constexpr int MMAX = QOCX_ACTION_MAX_DEGREE;

struct InvTable {  // 1 / p
    double v[MMAX + 2];
    constexpr InvTable() : v{} {
        for (int p = 1; p < MMAX + 2; ++p) v[p] = 1.0 / (double)p;
    }
};
struct CoefTable {  // c_il = i! l! / (i + l + 1)! (qocx_action.hip)
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

// Four columns K0 .. K0 + 3 of y += a x, the broadcast of x inside the multiply-add (qocx_action.hip:
// lane k of every row of 16 lanes holds x[column k of the wave's block])
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

// KR: the G_k images held in registers beside H0 (those of further controls are read per step). ONE: with
// H0, one G_k and the built generator a wave stays within 256 registers, so the workgroups of a seed's
// two directions share a CU and each SIMD has a second wave to issue while one waits at the barrier.
template <int NW, int KR>
__global__ __launch_bounds__(64 * NW, 2) void action4_sweep_kernel(ActionArgs args) {
    typedef Geo<4> G;
    constexpr int NP = G::NP, CW = 16;
    static_assert(NP == 64 && NW * CW <= NP, "lane = row; a wave per block of 16 columns");
    __shared__ __attribute__((aligned(16))) double2 turn[NP];          // the vector where the cost code reads / writes it
    __shared__ __attribute__((aligned(16))) double2 part[2][NW][NP];   // the waves' partial products, two sets in turn
    const SweepArgs& sw = args.sw;
    const int b = blockIdx.x;
    const int lane = lane_id(), w = threadIdx.x >> 6;
    const int xcol = CW * w + (lane & 15);   // the entry of the operand this lane holds for the broadcast
    const bool w0 = (w == 0);
    const int nsteps = sw.nsteps, K = args.K, m_max = args.m_max;
    const int jb = sw.j_begin, je = sw.j_end;
    const double dt = args.dt;
    __builtin_amdgcn_s_setprio(3);  // the serial chain of the evaluation goes first on its SIMD

    // -i dt H0 and -i dt G_k, wave w, lane i: row i, columns 16 w + cc (re, im of -i dt (x + i y) = dt y,
    // -dt x). The images are plain column-major NP x NP: element (i, c) at c NP + i.
    auto image_at = [&](int cc) { return (CW * w + cc) * NP + lane; };
    double h0r[CW], h0i[CW], gr[KR][CW], gi[KR][CW];
#pragma unroll
    for (int cc = 0; cc < CW; ++cc) {
        const double2 e = args.h0_rimg[image_at(cc)];
        h0r[cc] = dt * e.y;
        h0i[cc] = -dt * e.x;
    }
#pragma unroll
    for (int k = 0; k < KR; ++k)
#pragma unroll
        for (int cc = 0; cc < CW; ++cc) {
            const double2 e = k < K ? args.g_rimg[(size_t)k * G::MAT + image_at(cc)] : make_double2(0, 0);
            gr[k][cc] = dt * e.y;
            gi[k][cc] = -dt * e.x;
        }

    const int* words = sw.s_arr + (size_t)b * nsteps;
    const double* u_b = args.ustep + (size_t)b * nsteps * K;
    double are[CW], aim[CW];
    auto build = [&](int step) __attribute__((always_inline)) {
        const double* u = u_b + (size_t)step * K;
#pragma unroll
        for (int cc = 0; cc < CW; ++cc) {
            are[cc] = h0r[cc];
            aim[cc] = h0i[cc];
        }
#pragma unroll
        for (int k = 0; k < KR; ++k)
            if (k < K) {
                const double uk = u[k];
#pragma unroll
                for (int cc = 0; cc < CW; ++cc) {
                    are[cc] = fma(uk, gr[k][cc], are[cc]);
                    aim[cc] = fma(uk, gi[k][cc], aim[cc]);
                }
            }
        for (int k = KR; k < K; ++k) {
            const double uk = u[k] * dt;
#pragma unroll
            for (int cc = 0; cc < CW; ++cc) {
                const double2 e = args.g_rimg[(size_t)k * G::MAT + image_at(cc)];
                are[cc] = fma(uk, e.y, are[cc]);
                aim[cc] = fma(-uk, e.x, aim[cc]);
            }
        }
    };
    // The vector twice: (vr, vi) at lane = row, (xr, xi) at the lane's entry of the wave's column block.
    double vr = 0, vi = 0, xr = 0, xi = 0;
    int par = 0;    // the set of partial slots the next term writes
    int count = 0;  // wave 0, lane l: steps at degree l
    auto load_vector = [&](const double2* src) __attribute__((always_inline)) {
        const double2 a = src[lane], c = src[xcol];
        vr = a.x; vi = a.y; xr = c.x; xi = c.y;
    };
    // One step: the vector becomes sum_p (sign a)^p / p! v; the terms 0 .. m - 1 go to `keep`. False
    // (for every wave of the workgroup alike): the degree is outside the buffers.
    auto step_apply = [&](int step, double sign, double2* keep_base) __attribute__((always_inline)) {
        const int m = step_degree(words[step]);
        if (m < 1 || m > m_max) return false;
        build(step);
        double2* keep = keep_base ? keep_base + ((size_t)b * nsteps + step) * m_max * NP : nullptr;
        count += (lane == m) ? 1 : 0;
        double sr = vr, si = vi, sxr = xr, sxi = xi;
        double f = sign * INV_P.v[1];
        for (int p = 1; p <= m; ++p) {
            if (keep != nullptr && w0) keep[(size_t)(p - 1) * NP + lane] = make_double2(vr, vi);
            const double f_next = sign * INV_P.v[p + 1];  // (asked for a term early: a trip to the constant cache)
            double s0r = 0, s0i = 0, s1r = 0, s1i = 0;
            for_each_const(
                [&](auto Q) __attribute__((always_inline)) {
                    constexpr int k = 4 * decltype(Q)::value;
                    dpp_cmac4<k>(s0r, s0i, s1r, s1i, xr, xi, are[k], aim[k], are[k + 1], aim[k + 1],
                                 are[k + 2], aim[k + 2], are[k + 3], aim[k + 3]);
                },
                std::make_integer_sequence<int, 4>{});
            double2(*slot)[NP] = part[par];
            par ^= 1;
            slot[w][lane] = make_double2(s0r + s1r, s0i + s1i);
            __syncthreads();
            double2 pa[NW], pc[NW];
#pragma unroll
            for (int q = 0; q < NW; ++q) {
                pa[q] = slot[q][lane];
                pc[q] = slot[q][xcol];
            }
            double yr = pa[0].x, yi = pa[0].y, zr = pc[0].x, zi = pc[0].y;
#pragma unroll
            for (int q = 1; q < NW; ++q) {  // the fixed order of the sum
                yr += pa[q].x; yi += pa[q].y;
                zr += pc[q].x; zi += pc[q].y;
            }
            vr = f * yr; vi = f * yi;
            xr = f * zr; xi = f * zi;
            sr += vr; si += vi;
            sxr += xr; sxi += xi;
            f = f_next;
        }
        vr = sr; vi = si;
        xr = sxr; xi = sxi;
        return true;
    };
    auto refuse = [&]() {  // never clamped: the host runs the evaluation again on the Pade route
        if (threadIdx.x == 0) atomicOr(sw.status, 8);
    };

    // ---- forward sweep ----------------------------------------------------------------------
    if (sw.phase & 1) {
        load_vector(jb == 0 ? sw.psi0 : args.carry_f + (size_t)b * NP);
        for (int step = jb; step < je; ++step)
            if (!step_apply(step, 1.0, args.kv_f)) {
                refuse();
                return;
            }
        if (w0 && count > 0 && lane <= MMAX) atomicAdd(args.degree_counts + lane, count);
        if (je == nsteps) {
            if (w0) {  // (lane = row i of the one lane group of NP = 64)
                turn[lane] = make_double2(vr, vi);
                wave_sync();
                const double cost = eval_costs<4>(sw, false, true, turn, nullptr, 0, lane);
                if (sw.unit_adjoint && sw.want_grad) unit_adjoint_scales<4>(sw, turn, b, 0, lane);
                sw.final_out[(size_t)b * NP + lane] = make_double2(vr, vi);
                if (lane == 0) sw.cost_out[b] = cost;
            }
        } else if (w0) {
            args.carry_f[(size_t)b * NP + lane] = make_double2(vr, vi);
        }
    }
    if (!(sw.phase & 2)) return;

    // ---- adjoint sweep: the back-propagated target (unit adjoint) ------------------------------
    if (je == nsteps) {
        if (w0) {
            wave_sync();
            unit_adjoint_seed<4>(sw, turn, 0, 1, 0, lane);
        }
        __syncthreads();
        load_vector(turn);
    } else {
        load_vector(sw.lam_buf + (size_t)b * NP);
    }
    for (int step = je - 1; step >= jb; --step)
        if (!step_apply(step, -1.0, args.kv_b)) {
            refuse();
            return;
        }
    if (jb > 0 && w0) sw.lam_buf[(size_t)b * NP + lane] = make_double2(vr, vi);
}

// LDS of the gradient kernel, per wave: v_0 .. v_(m-1) at the 16 indices of the wave's column block
// [m_max][16], two slots [16] for the current rho; then the waves' shares of gamma [NW][K].
__host__ __device__ inline int grad_lds_bytes(int nw, int m_max, int K) {
    return (nw * (m_max + 2) * 16 + nw * K) * (int)sizeof(double2);
}

// One workgroup of NW waves per (step, seed): wave w forms the columns 16 w .. 16 w + 15 of abar (lane i:
// row i) - rho_i only at its own 16 indices, so the loop over the terms needs no workgroup barrier -
// and its share of gamma_k; thread k adds the shares in the order w = 0 .. NW - 1.
template <int NW>
__global__ __launch_bounds__(64 * NW) void action4_grad_kernel(ActionGradArgs args) {
    typedef Geo<4> G;
    constexpr int NP = G::NP, CW = 16;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = lane_id(), w = threadIdx.x >> 6;
    const int K = args.K;
    double2* vl = reinterpret_cast<double2*>(smem) + (size_t)w * (args.m_max + 2) * CW;
    double2* rho = vl + (size_t)args.m_max * CW;
    double2* share = reinterpret_cast<double2*>(smem) + (size_t)NW * (args.m_max + 2) * CW;  // [NW][K]
    const int step = args.step0 + blockIdx.x, b = blockIdx.y;
    const int c16 = lane & 15, q4 = lane >> 4;
    const size_t idx = (size_t)b * args.nsteps + step;
    const int m = step_degree(args.s_arr[idx]);
    if (m < 1 || m > args.m_max) return;  // (the sweeps have raised the status bit; the same for every wave)
    const double2* vf = args.kv_f + idx * args.m_max * NP;
    const double2* wb = args.kv_b + idx * args.m_max * NP;
    for (int l = q4; l < m; l += 4) vl[l * CW + c16] = vf[(size_t)l * NP + CW * w + c16];
    double abr[CW], abi[CW];
#pragma unroll
    for (int cc = 0; cc < CW; ++cc) {
        abr[cc] = 0;
        abi[cc] = 0;
    }
    wave_sync();
    double2 tv = wb[lane];
    for (int ii = 0; ii < m; ++ii) {
        // rho_ii at index 16 w + c16 (every row of 16 lanes forms the same sum)
        double rr = 0, ri = 0;
        for (int l = 0; l < m - ii; ++l) {
            const double c = COEF.c[ii * MMAX + l];
            const double2 v = vl[l * CW + c16];
            rr = fma(c, v.x, rr);
            ri = fma(c, v.y, ri);
        }
        double2* slot = rho + (ii & 1) * CW;  // two slots in turn: one sync per term
        if (q4 == 0) slot[c16] = make_double2(rr, ri);
        wave_sync();
        const double2 wv = tv;
        if (ii + 1 < m) tv = wb[(size_t)(ii + 1) * NP + lane];
#pragma unroll
        for (int cc = 0; cc < CW; ++cc) {
            const double2 r = slot[cc];
            // w * conj(rho)
            abr[cc] = fma(wv.y, r.y, fma(wv.x, r.x, abr[cc]));
            abi[cc] = fma(-wv.x, r.y, fma(wv.y, r.x, abi[cc]));
        }
    }
    // gamma_k = sum conj(abar) E_k, E_k = -i dt G_k (qocx_action.hip)
    const double dts = args.dt;
    for (int k = 0; k < K; ++k) {
        double acc = 0, acc_im = 0;
#pragma unroll
        for (int cc = 0; cc < CW; ++cc) {
            const double2 e = args.g_rimg[(size_t)k * G::MAT + (size_t)(CW * w + cc) * NP + lane];
            acc = fma(abi[cc], -dts * e.x, fma(abr[cc], dts * e.y, acc));
            acc_im = fma(abi[cc], -dts * e.y, fma(abr[cc], -dts * e.x, acc_im));
        }
        acc = wave_sum(acc);
        acc_im = wave_sum(acc_im);
        if (lane == 0) share[w * K + k] = make_double2(acc, acc_im);
    }
    __syncthreads();
    for (int k = threadIdx.x; k < K; k += 64 * NW) {
        double acc = 0, acc_im = 0;
#pragma unroll
        for (int q = 0; q < NW; ++q) {
            acc += share[q * K + k].x;
            acc_im += share[q * K + k].y;
        }
        args.gstep[(idx * K + k) * 2] = acc;
        args.gstep[(idx * K + k) * 2 + 1] = acc_im;
    }
}

}  // namespace action4

// waves of a workgroup: a block of 16 columns each, and none for zero columns
static int action4_waves(int n) { return n <= 48 ? 3 : 4; }

int action4_grad_lds_bytes(int n, int m_max, int K) { return action4::grad_lds_bytes(action4_waves(n), m_max, K); }

void launch_action4_sweep(int n, const ActionArgs& a, int batch, hipStream_t st) {
    if (batch <= 0 || a.sw.j_end <= a.sw.j_begin) return;
    if (action4_waves(n) == 3) hipLaunchKernelGGL((action4::action4_sweep_kernel<3, 1>), dim3(batch), dim3(192), 0, st, a);
    else hipLaunchKernelGGL((action4::action4_sweep_kernel<4, 1>), dim3(batch), dim3(256), 0, st, a);
}

void launch_action4_grad(int n, const ActionGradArgs& a, int nsteps, int batch, hipStream_t st) {
    if (batch <= 0 || nsteps <= 0) return;
    const int lds = action4_grad_lds_bytes(n, a.m_max, a.K);
    if (action4_waves(n) == 3) hipLaunchKernelGGL((action4::action4_grad_kernel<3>), dim3(nsteps, batch), dim3(192), lds, st, a);
    else hipLaunchKernelGGL((action4::action4_grad_kernel<4>), dim3(nsteps, batch), dim3(256), lds, st, a);
}

}  // namespace qocx
