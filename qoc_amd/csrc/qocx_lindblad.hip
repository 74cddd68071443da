// qocx_lindblad.hip - the kernels and launchers of the Lindblad GRAPE path at n <= 32: the engine of
// qocx_lindblad_core.h as the kernels every run without per-member rates launches (an ensemble with
// rates: qocx_lindblad_rates.hip), the combine kernel of the two-sided evaluation, the sizes the host asks
// for. 17 <= n <= 32 goes to the tile-per-wave kernels of qocx_lindblad4t.hip where they apply.
#include "qocx_lindblad_core.h"

namespace qocx {

namespace {

template <int LNB, bool GS, bool MW, bool MW4, bool STAMP = false, bool Q2 = false, bool CH = false>
__global__ __launch_bounds__(MW ? (MW4 ? 256 : 384) : 64) void lindblad_kernel(LindbladArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    LB<LNB, GS, MW, (LNB == 1 && !GS && !MW), STAMP, MW4, Q2, CH>::run(a, smem);
}

struct Launch {  // (lindblad_dispatch)
    const LindbladArgs& a;
    int batch;
    hipStream_t st;
    template <int LNB, bool GS, bool MW, bool MW4, bool STAMP, bool Q2, bool CH>
    void operator()(int bytes, int threads) const {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(lindblad_kernel<LNB, GS, MW, MW4, STAMP, Q2, CH>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
        hipLaunchKernelGGL((lindblad_kernel<LNB, GS, MW, MW4, STAMP, Q2, CH>), dim3(batch), dim3(threads), bytes, st, a);
    }
};

// Two-sided evaluation, third kernel: one wave per (sub-interval, seed) contracts the forward
// stage values Y_i with the stage cotangents kbar_i of the unit adjoint into
//   gamma_k = tr(Z_i Gp_k),  Z_i = Y_i kbar_i^H - kbar_i^H Y_i   (complex: kbar_i belongs to the
// back-propagated TARGET; the true stage cotangent is c_s kbar_i with the scalar c_s phase 1 left
// in lam_scale), adds Re(conj(c_s) gamma_k) over stages and densities and splits it between the
// sub-interval's end points with weights (1 - c_i, c_i): gsub[B][nsub][2][K], as the classic
// launch writes it. Throughput work on the whole chip (nsub x B waves).
__global__ __launch_bounds__(64) void lindblad_combine_kernel(LindbladArgs a) {
    typedef LB<1, false, false> I;
    typedef I::Mat Mat;
    __shared__ __attribute__((aligned(16))) char smem[2 * I::SLOT_BYTES];
    const Slot slot_zk = I::slot_at(smem), slot_zy = I::slot_at(smem + I::SLOT_BYTES);
    const int q = blockIdx.x, b = blockIdx.y, S = a.S, K = a.K, nsub = a.nsub;
    double ga[QOCX_LINDBLAD_MAX_K], gb[QOCX_LINDBLAD_MAX_K];
#pragma unroll
    for (int k = 0; k < QOCX_LINDBLAD_MAX_K; ++k) ga[k] = gb[k] = 0;
    for (int s = 0; s < S; ++s) {
        const double2 cs = a.lam_scale[(size_t)b * S + s];
        const size_t base = ((((size_t)b * nsub + q) * S + s) * STAGES) * I::MAT;
        for (int i = 0; i < STAGES; ++i) {
            Mat y, kb, kbd, z, z2;
            I::dump_load(y, a.ystages + base + (size_t)i * I::MAT);
            I::dump_load(kb, a.kbstages + base + (size_t)i * I::MAT);
            if (a.hermitian) {
                // Hermitian Y_i, kbar_i, anti-Hermitian Gp_k (host-checked): Z = P - P^H with P = Y kbar, and
                // tr(Z Gp_k) = 2 Re tr(P Gp_k) - ONE product, its left operand the conjugate of Y's own
                // registers (the C layout of Y^T), nothing through LDS
                double yr[4], yi[4];
#pragma unroll
                for (int kk = 0; kk < 4; ++kk) {
                    yr[kk] = y.re[0][0][kk];
                    yi[kk] = -y.im[0][0][kk];
                }
                I::mat_zero(z);
                I::Wave::gemm_r(z, yr, yi, kb);
                const double ci = RK_C_DEV[i];
                for (int k = 0; k < K; ++k) {
                    Mat gt;
                    I::dump_load(gt, a.gpt_cimg + (size_t)k * I::MAT);
                    double pr = 0;
#pragma unroll
                    for (int r = 0; r < 4; ++r) pr += z.re[0][0][r] * gt.re[0][0][r] - z.im[0][0][r] * gt.im[0][0][r];
                    const double g = cs.x * (2.0 * wave_sum(pr));
#pragma unroll
                    for (int kk = 0; kk < QOCX_LINDBLAD_MAX_K; ++kk)
                        if (kk == k) {
                            ga[kk] += (1.0 - ci) * g;
                            gb[kk] += ci * g;
                        }
                }
                continue;
            }
            wave_sync();
            cmat_to_lds<1>(kb, slot_zk.re, slot_zk.im);
            wave_sync();
            I::load_adjoint(kbd, slot_zk);
            I::mat_zero(z2);
            I::template gemm<true>(z2, slot_zk, y);  // kbar^H Y
            wave_sync();
            cmat_to_lds<1>(y, slot_zy.re, slot_zy.im);
            wave_sync();
            I::mat_zero(z);
            I::template gemm<false>(z, slot_zy, kbd);  // Y kbar^H
            I::mat_axpy(z, -1.0, z2);
            const double ci = RK_C_DEV[i];
            for (int k = 0; k < K; ++k) {
                Mat gt;
                I::dump_load(gt, a.gpt_cimg + (size_t)k * I::MAT);
                double pr = 0, pi = 0;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    pr += z.re[0][0][r] * gt.re[0][0][r] - z.im[0][0][r] * gt.im[0][0][r];
                    pi += z.re[0][0][r] * gt.im[0][0][r] + z.im[0][0][r] * gt.re[0][0][r];
                }
                const double g = fma(cs.y, wave_sum(pi), cs.x * wave_sum(pr));  // Re(conj(c) gamma)
#pragma unroll
                for (int kk = 0; kk < QOCX_LINDBLAD_MAX_K; ++kk)
                    if (kk == k) {
                        ga[kk] += (1.0 - ci) * g;
                        gb[kk] += ci * g;
                    }
            }
        }
    }
    if (lane_id() == 0)
#pragma unroll
        for (int kk = 0; kk < QOCX_LINDBLAD_MAX_K; ++kk)
            if (kk < K) {
                a.gsub[(((size_t)b * nsub + q) * 2 + 0) * K + kk] = ga[kk];
                a.gsub[(((size_t)b * nsub + q) * 2 + 1) * K + kk] = gb[kk];
            }
}

}  // namespace

void launch_lindblad_combine(const LindbladArgs& a, int batch, hipStream_t st) {
    if (batch <= 0 || a.nsub <= 0) return;
    if (a.n > 16) {
        launch_lindblad4t_combine(a, batch, st);
        return;
    }
    hipLaunchKernelGGL(lindblad_combine_kernel, dim3(a.nsub, batch), dim3(64), 0, st, a);
}

int launch_lindblad(LindbladKernel kernel, bool stamped, const LindbladArgs& a, int batch, hipStream_t st) {
    switch (kernel) {
    case LindbladKernel::NONE: return 1;
    case LindbladKernel::TILE16: launch_lindblad16t(a, batch, st); return 0;
    case LindbladKernel::TILE4:
    case LindbladKernel::TILE4_HERM: launch_lindblad4t(kernel == LindbladKernel::TILE4_HERM, a, batch, st); return 0;
    default: return lindblad_dispatch(kernel, stamped, a, Launch{a, batch, st}) ? 0 : 1;
    }
}

// LDS bytes of one seed. mode 0: one wave, everything in LDS; 1: one wave, stage derivatives /
// densities / cotangents in HBM scratch (always for n > 16); 2: nops + 2 waves per seed; 3: as 2
// with the constant generator dumps of K controls cached in LDS
int lindblad_lds_size(int n, int S, int nops, int mode, int K) {
    if (n > 32) return lindblad16t_lds_bytes();  // two matrices, whatever the problem
    if (n > 16) return LB<2, true, false>::lds_bytes(S, nops);
    if (mode == 1) return LB<1, true, false>::lds_bytes(S, nops);
    if (mode == 2) return LB<1, false, true>::lds_bytes(S, nops);
    if (mode == 3) return LB<1, false, true>::lds_bytes(S, nops, K);
    return LB<1, false, false>::lds_bytes(S, nops);
}

// complex elements of per-seed HBM scratch when it is used
// (n > 16: a second set of stage dumps - the two passes of the two-sided evaluation run side by side -
// and a third for stage values recomputed from a checkpoint)
size_t lindblad_scratch_elems(int n, int S) {
    if (n > 32) return lindblad16t_scratch_elems(S);
    return n > 16 ? (size_t)(2 * S + 3 * STAGES) * 1024 : (size_t)(2 * S + STAGES) * 256;
}

}  // namespace qocx
