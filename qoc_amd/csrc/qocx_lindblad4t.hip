// qocx_lindblad4t.hip - the Lindblad engine at 17 <= n <= 32 with the density tile-wise on four waves.
//
// Replaces (reference): _evaluate_lindblad_discrete (qoc/core/lindbladdiscrete.py:357-441) with its
// right-hand side _get_rhs_lindbladian (:444-495) / get_lindbladian (qoc/core/mathmethods.py:169-206) and
// integrate_rkdp5 (mathmethods.py:352-480 - here the fixed-step DOP853 of qocx_lindblad.hip on
// sub-intervals the host sizes); the gradient autograd takes through them is the discrete adjoint of the
// scheme. Density costs: targetdensityinfidelity.py:41-69, forbiddensities.py:53-85.
//
// One workgroup = one seed = four waves; wave w owns tile (w & 1, w >> 1) of every 32 x 32 matrix - of
// the density, of the stage value, of every stage derivative k_j, of the cotangents. A stage
//     k = A_L(c) Y + Y A_R(c) + sum_i gamma_i L_i Y L_i^H        (adjoint: A^H, L_i^H . L_i)
// is three rounds of LDS-operand products with one workgroup barrier before each: the generator
// products, t_i = gamma_i L_i Y (stored over the generators), t_i L_i^H (the operators two at a time: the
// last two rounds again for a third and fourth). No partial sums are exchanged -
// every wave computes ITS tile of every product - and the Runge-Kutta combinations are tile
// arithmetic: a wave writes its tile of k_j to the seed's HBM scratch and reads only that tile back (L2
// hits, no synchronisation; twelve 16 KB matrices fit neither LDS next to the operands nor - as the
// compiler allocates them - the accumulation registers). The stage loops stay ROLLED: unrolled, the
// kernel is 258 KB of straight-line code against 64 KB of instruction cache and runs at the pace of
// the instruction fetch (11 us per stage). The one-wave form of qocx_lindblad.hip (LB<2, true, false>)
// carries four tiles per matrix in one wave; it stays behind the knob lindblad_4t = 0 as the form the
// tests hold this one against.
#include "qocx_lindblad4t_core.h"

namespace qocx {

namespace lindblad4t {

template <bool HERM>
__global__ __launch_bounds__(256) void lindblad4t_kernel(LindbladArgs a) {
#include "qocx_lindblad4t_body.inc"
}

// Two-sided evaluation, third kernel: the control cotangents of sub-interval q of seed b from the stage
// values Y_i (phase 1) and the stage cotangents kbar_i of the unit adjoint (phase 2),
//     g_k += Re( conj(c_s) tr(Z_i Gp_k) ),  Z_i = Y_i kbar_i^H - kbar_i^H Y_i,  c_s = lam_scale[b][s],
// with the weights (1 - c_i, c_i) of the sub-interval's end points: gsub[B][nsub][2][K] as the classic
// launch writes it. HERM: Z = W - W^H, W = Y kbar, and tr(Z Gp_k) = 2 Re tr(W Gp_k). Throughput work on
// the whole chip: nsub x B workgroups of four waves, two LDS matrices each.
template <bool HERM>
__global__ __launch_bounds__(256) void lindblad4t_combine_kernel(LindbladArgs a) {
    __shared__ __attribute__((aligned(16))) char smem[2 * D::MBYTES + 2 * 4 * 16];
    Ctx cx{a, make_wave<G>(smem, false), reinterpret_cast<double2*>(smem + 2 * D::MBYTES), 0};
    const W& wv = cx.wv;
    const int q = blockIdx.x, b = blockIdx.y, S = a.S, K = a.K, nsub = a.nsub;
    double ga[QOCX_LINDBLAD_MAX_K], gb[QOCX_LINDBLAD_MAX_K];
#pragma unroll
    for (int k = 0; k < QOCX_LINDBLAD_MAX_K; ++k) {
        ga[k] = 0;
        gb[k] = 0;
    }
    for (int s = 0; s < S; ++s) {
        const double2 cs = a.lam_scale[(size_t)b * S + s];
        const size_t base = ((((size_t)b * nsub + q) * S + s) * STAGES) * MAT;
#pragma unroll 1
        for (int i = 0; i < STAGES; ++i) {
            wv.store(cx.load_dump(a.ystages + base + (size_t)i * MAT), 0);
            wv.store(cx.load_dump(a.kbstages + base + (size_t)i * MAT), 1);
            __syncthreads();
            T z = tile_zero<G>();
            if (HERM) {
                wv.template mm<false, false>(z, 0, 1, 2.0);
            } else {
                wv.template mm<false, true>(z, 0, 1, 1.0);
                wv.template mm<true, false>(z, 1, 0, -1.0);
            }
            const double ci = RK.c[i];
#pragma unroll
            for (int k = 0; k < QOCX_LINDBLAD_MAX_K; ++k)
                if (k < K) {
                    const T gt = cx.load_dump(a.gpt_cimg + (size_t)k * MAT);
                    double pr = 0, pi = 0;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        pr += z.re[0][r] * gt.re[0][r] - z.im[0][r] * gt.im[0][r];
                        pi += z.re[0][r] * gt.im[0][r] + z.im[0][r] * gt.re[0][r];
                    }
                    // Re(conj(c) gamma); HERM: gamma = 2 Re tr(W Gp_k) is real
                    const double gk = HERM ? cs.x * pr : fma(cs.y, pi, cs.x * pr);
                    ga[k] += (1.0 - ci) * gk;
                    gb[k] += ci * gk;
                }
            __syncthreads();  // the two matrices are free again
        }
    }
#pragma unroll
    for (int k = 0; k < QOCX_LINDBLAD_MAX_K; ++k)
        if (k < K) {
            double x = ga[k], y = gb[k];
            cx.block_sum(x, y);
            if (wv.tid == 0) {
                a.gsub[(((size_t)b * nsub + q) * 2 + 0) * K + k] = x;
                a.gsub[(((size_t)b * nsub + q) * 2 + 1) * K + k] = y;
            }
        }
}

}  // namespace lindblad4t

void launch_lindblad4t_combine(const LindbladArgs& a, int batch, hipStream_t st) {
    if (a.hermitian)
        hipLaunchKernelGGL(lindblad4t::lindblad4t_combine_kernel<true>, dim3(a.nsub, batch), dim3(256), 0, st, a);
    else
        hipLaunchKernelGGL(lindblad4t::lindblad4t_combine_kernel<false>, dim3(a.nsub, batch), dim3(256), 0, st, a);
}

void launch_lindblad4t(bool hermitian, const LindbladArgs& a, int batch, hipStream_t st) {
    static bool attr_set = false;
    if (!attr_set) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(lindblad4t::lindblad4t_kernel<false>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, lindblad4t::LDS_BYTES);
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(lindblad4t::lindblad4t_kernel<true>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, lindblad4t::LDS_BYTES);
        attr_set = true;
    }
    if (hermitian)
        hipLaunchKernelGGL(lindblad4t::lindblad4t_kernel<true>, dim3(batch), dim3(256), lindblad4t::LDS_BYTES, st, a);
    else
        hipLaunchKernelGGL(lindblad4t::lindblad4t_kernel<false>, dim3(batch), dim3(256), lindblad4t::LDS_BYTES, st, a);
}

}  // namespace qocx
