// Hamiltonians quadratic in the real controls (qocx_set_quadratic_terms, QuadArgs):
//
//   H(r, t) = H0(t) + sum_k r_k G_k(t) + sum_q r_kq r_lq Q_q
//
// is linear in the Ke = K + count effective controls w = (r_k, r_kq r_lq) over the augmented
// operator set {G_k} u {Q_q}. The controls kernel writes w at every step midpoint; K1a reads it
// through the identity interpolation (one row per step), the sweeps and K3 run unchanged on Ke
// controls, and the chain kernel folds the Ke per-step cotangents back into the K real controls
// before the usual scatter_kernel carries them to the knots.
//
// With an ensemble whose members scale the terms (QuadArgs::term_scales) item i carries
// c_(i % M, q) r_kq r_lq in effective control K + q, and its cotangent takes the same factor on the
// way back. SCALED is a template parameter: without scales the kernels are the ones they were.
#include "qocx_device.h"
#include "qocx_wave.h"

namespace qocx {

// One thread per (seed, step): w = [r_k(t_mid), r_kq(t_mid) r_lq(t_mid)].
template <bool SCALED>
__global__ __launch_bounds__(256) void quad_controls_kernel(QuadArgs args) {
    const size_t w = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= args.total) return;
    const int step = (int)(w % args.nsteps), K = args.K;
    const size_t b = w / args.nsteps;
    const double* ctl_b = args.controls + b * args.nc * K;
    const StepInterp si = args.interp[step];
    double* v = args.veff + w * args.Ke;
    for (int k = 0; k < K; ++k) v[k] = control_at(ctl_b, si, K, k);
    // (control_at again rather than a local array indexed by the pair: no scratch, same bits)
    const double* cm = nullptr;  // the item's member's term scales
    (void)cm;
    if constexpr (SCALED) cm = args.term_scales + ((args.item0 + b) % (size_t)args.M) * (size_t)args.count;
    for (int q = 0; q < args.count; ++q) {
        const double rr = control_at(ctl_b, si, K, args.pairs[2 * q]) * control_at(ctl_b, si, K, args.pairs[2 * q + 1]);
        if constexpr (SCALED) v[K + q] = cm[q] * rr;
        else v[K + q] = rr;
    }
}

// One thread per (seed, step): dC/dr_k = gbar_k + sum_q c_q r_other gbar_(K+q), c_q = 2 for a
// square, 1 for a cross pair. Writes greal [B][nsteps][K] (real), which scatter_kernel reads.
// SCALED: gbar_(K+q) is first multiplied by the item's c_(m,q).
template <bool SCALED>
__global__ __launch_bounds__(256) void quad_chain_kernel(QuadArgs args) {
    const size_t w = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= args.total) return;
    const int step = (int)(w % args.nsteps), K = args.K, Ke = args.Ke;
    const size_t b = w / args.nsteps;
    const double* ctl_b = args.controls + b * args.nc * K;
    const StepInterp si = args.interp[step];
    // cotangent of effective control e
    auto ge_plain = [&](int e) -> double {
        if (args.lam_scale != nullptr) {  // unit adjoint: Re(conj(c) gamma), as scatter_kernel
            const double2 c = args.lam_scale[b * args.S];
            const double* g = args.gstep + (w * Ke + e) * 2;
            return fma(c.y, g[1], c.x * g[0]);
        }
        return args.gstep[w * Ke + e];
    };
    const double* cm = nullptr;
    (void)cm;
    if constexpr (SCALED) cm = args.term_scales + ((args.item0 + b) % (size_t)args.M) * (size_t)args.count;
    auto ge = [&](int e) -> double {
        if constexpr (SCALED)
            if (e >= K) return cm[e - K] * ge_plain(e);
        return ge_plain(e);
    };
    double* out = args.greal + w * K;
    for (int k = 0; k < K; ++k) {
        double acc = ge(k);
        for (int q = 0; q < args.count; ++q) {
            const int kq = args.pairs[2 * q], lq = args.pairs[2 * q + 1];
            if (kq == k && lq == k) acc += 2.0 * control_at(ctl_b, si, K, k) * ge(K + q);
            else if (kq == k) acc += control_at(ctl_b, si, K, lq) * ge(K + q);
            else if (lq == k) acc += control_at(ctl_b, si, K, kq) * ge(K + q);
        }
        out[k] = acc;
    }
}

void launch_quad_controls(const QuadArgs& a, hipStream_t st) {
    if (a.term_scales != nullptr) {
        hipLaunchKernelGGL(quad_controls_kernel<true>, dim3((unsigned)((a.total + 255) / 256)), dim3(256), 0, st, a);
        return;
    }
    hipLaunchKernelGGL(quad_controls_kernel<false>, dim3((unsigned)((a.total + 255) / 256)), dim3(256), 0, st, a);
}
void launch_quad_chain(const QuadArgs& a, hipStream_t st) {
    if (a.term_scales != nullptr) {
        hipLaunchKernelGGL(quad_chain_kernel<true>, dim3((unsigned)((a.total + 255) / 256)), dim3(256), 0, st, a);
        return;
    }
    hipLaunchKernelGGL(quad_chain_kernel<false>, dim3((unsigned)((a.total + 255) / 256)), dim3(256), 0, st, a);
}

}  // namespace qocx
