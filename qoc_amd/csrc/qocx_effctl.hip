// Effective controls (EffCtlArgs): two problems that are not M2 run the M2 kernels unchanged, their
// step generator being LINEAR in Ke effective controls over an augmented operator set. The controls
// kernel writes the Ke values of every step; K1a reads them through the identity interpolation (one
// row per step), the sweeps and K3 run on Ke controls, and the chain kernel folds the Ke per-step
// cotangents back before the usual scatter_kernel carries them to the knots.
//   M4-linear (M4LinArgs): M4 on time-independent H0 / G_k - qocx_device.h has v, w, z.
//   Quadratic (QuadArgs): H(r, t) = H0(t) + sum_k r_k G_k(t) + sum_q r_kq r_lq Q_q, w = (r_k, r_kq r_lq)
//     over {G_k} u {Q_q}. With an ensemble whose members scale the terms (QuadArgs::term_scales) item i
//     carries c_(i % M, q) r_kq r_lq in effective control K + q, and its cotangent takes the same factor
//     on the way back. SCALED is a template parameter: without scales the kernels are what they were.
#include "qocx_effctl.h"

namespace qocx {

// cotangent of effective control e of work item w = (seed b, step)
__device__ inline double effctl_cotangent(const EffCtlArgs& args, size_t w, size_t b, int e) {
    if (args.lam_scale != nullptr) {  // unit adjoint: Re(conj(c) gamma), as scatter_kernel
        const double2 c = args.lam_scale[b * args.S];
        const double* g = args.gstep + (w * args.Ke + e) * 2;
        return fma(c.y, g[1], c.x * g[0]);
    }
    return args.gstep[w * args.Ke + e];
}

// M4-linear. One thread per (seed, step). mathmethods.py:96-122 with a(t) = -i (H0 + sum u_k(t) G_k).
__global__ __launch_bounds__(256) void m4lin_controls_kernel(M4LinArgs args) {
    const size_t w = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= args.total) return;
    QOCX_M4LIN_EFFECTIVE(args, w)
}

// Writes gchain [B][nsteps * 2][K]: the cotangents of the controls at the two nodes of every step.
__global__ __launch_bounds__(256) void m4lin_chain_kernel(M4LinArgs args) {
    const size_t w = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= args.total) return;
    const int step = (int)(w % args.nsteps), K = args.K;
    const size_t b = w / args.nsteps;
    const double* ctl_b = args.controls + b * args.nc * K;
    const StepInterp s1 = args.interp[(size_t)step * 2], s2 = args.interp[(size_t)step * 2 + 1];
    double u1[QOCX_M4LIN_MAX_K], u2[QOCX_M4LIN_MAX_K], g1[QOCX_M4LIN_MAX_K], g2[QOCX_M4LIN_MAX_K];
    for (int k = 0; k < K; ++k) {
        u1[k] = control_at(ctl_b, s1, K, k);
        u2[k] = control_at(ctl_b, s2, K, k);
        const double gv = effctl_cotangent(args, w, b, k), gw = effctl_cotangent(args, w, b, K + k);
        g1[k] = 0.5 * gv - args.f0dt * gw;
        g2[k] = 0.5 * gv + args.f0dt * gw;
    }
    int e = 2 * K;
    for (int k = 0; k < K; ++k)
        for (int l = k + 1; l < K; ++l) {
            const double gz = args.f0dt * effctl_cotangent(args, w, b, e++);  // z = F0 dt (u2_k u1_l - u2_l u1_k)
            g1[l] += gz * u2[k];
            g1[k] -= gz * u2[l];
            g2[k] += gz * u1[l];
            g2[l] -= gz * u1[k];
        }
    double* out = args.gchain + (b * (size_t)args.nsteps * 2 + (size_t)step * 2) * K;
    for (int k = 0; k < K; ++k) {
        out[k] = g1[k];
        out[K + k] = g2[k];
    }
}

// Quadratic. One thread per (seed, step): w = [r_k(t_mid), r_kq(t_mid) r_lq(t_mid)].
template <bool SCALED>
__global__ __launch_bounds__(256) void quad_controls_kernel(QuadArgs args) {
    const size_t w = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= args.total) return;
    QOCX_QUAD_EFFECTIVE(args, w, SCALED)
}

// One thread per (seed, step): dC/dr_k = gbar_k + sum_q c_q r_other gbar_(K+q), c_q = 2 for a
// square, 1 for a cross pair. Writes gchain [B][nsteps][K].
// SCALED: gbar_(K+q) is first multiplied by the item's c_(m,q).
template <bool SCALED>
__global__ __launch_bounds__(256) void quad_chain_kernel(QuadArgs args) {
    const size_t w = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= args.total) return;
    const int step = (int)(w % args.nsteps), K = args.K;
    const size_t b = w / args.nsteps;
    const double* ctl_b = args.controls + b * args.nc * K;
    const StepInterp si = args.interp[step];
    const double* cm = nullptr;
    (void)cm;
    if constexpr (SCALED) cm = args.term_scales + ((args.item0 + b) % (size_t)args.M) * (size_t)args.count;
    auto ge = [&](int e) -> double {
        if constexpr (SCALED)
            if (e >= K) return cm[e - K] * effctl_cotangent(args, w, b, e);
        return effctl_cotangent(args, w, b, e);
    };
    double* out = args.gchain + w * K;
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

template <class Kernel, class Args>
static void launch_per_step(Kernel kernel, const Args& a, hipStream_t st) {
    hipLaunchKernelGGL(kernel, dim3((unsigned)((a.total + 255) / 256)), dim3(256), 0, st, a);
}
void launch_m4lin_controls(const M4LinArgs& a, hipStream_t st) { launch_per_step(m4lin_controls_kernel, a, st); }
void launch_m4lin_chain(const M4LinArgs& a, hipStream_t st) { launch_per_step(m4lin_chain_kernel, a, st); }
void launch_quad_controls(const QuadArgs& a, hipStream_t st) {
    if (a.term_scales != nullptr) launch_per_step(quad_controls_kernel<true>, a, st);
    else launch_per_step(quad_controls_kernel<false>, a, st);
}
void launch_quad_chain(const QuadArgs& a, hipStream_t st) {
    if (a.term_scales != nullptr) launch_per_step(quad_chain_kernel<true>, a, st);
    else launch_per_step(quad_chain_kernel<false>, a, st);
}

}  // namespace qocx
