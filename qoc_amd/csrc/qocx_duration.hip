// qocx_duration.hip - duration search of a Hamiltonian sweep (qocx_sweep_set_durations,
// DurationArgs): tau_b = T_b / T, the duration of seed b in units of the problem's evolution time, is
// one more optimised parameter of the seed. The sweep's tables are derived from it on the device,
//
//   s_bk = tau_b s0_bk        delta_bj = tau_b delta0_bj      (one product, one rounding each;
//                                                              delta0_b0 = 1: the drift)
//
// with tau_b clipped to [tau_min, tau_max] first (duration_tables_kernel; the clipped value is
// written back, as the clip of real controls acts in place on the optimizer's parameters).
//
// The gradient with respect to tau_b is the chain rule through the tables, from the sensitivities
// dE_b/ds_bk and dE_b/ddelta_bj that sweep_sensitivity_kernel (qocx_sweep.hip, launched as it is) has
// left behind. Summation order of duration_gradient_kernel, one thread per seed:
//
//   g = +0.0
//   g = g + s0_bk     * dE_b/ds_bk        k = 0 .. K_r - 1 ascending
//   g = g + delta0_bj * dE_b/ddelta_bj    j = 0 .. J - 1 ascending
//   g = g + time_weight
//
// Every product and every sum is rounded on its own (no contraction into fused multiply-adds), so
// NumPy restates it as  g = 0.0; for k: g = g + s0[b, k] * ss[b, k]; for j: g = g + d0[b, j] * os[b, j];
// g = g + lam.  The same kernel adds the price of time to the seed's cost, last of all terms:
//
//   cost_b = cost_b + time_weight * tau_b     (one product, one sum)
//
// duration_step_kernel keeps tau_b of the improved seeds as their best and steps tau_b of the
// flagged seeds by the rule of the controls: optimizer_update_element (qocx_device.h), the one
// definition optimizer_update_kernel executes, gradient clipping included.
//
// Access: the tables kernel is one FP64 entry per thread in memory order, scales then offsets
// (coalesced); the per-seed kernels are one thread per seed over [B] arrays, K_r + J strided reads
// each of rows a few doubles long. All three are launch-bound (microseconds at B = 256).
#include "qocx_device.h"

namespace qocx {

#pragma clang fp contract(off)

__device__ __forceinline__ double duration_clip(double tau, double lo, double hi) {
    return tau < lo ? lo : (tau > hi ? hi : tau);
}

// One thread per table entry: e < B K_r a scale, then B J offsets. The thread of a seed's first
// entry (k = 0 of the scales; K_r >= 1 always) writes the clipped tau_b back - every thread of the
// seed reads tau_b before or after that store and clips it to the same value (the clip is idempotent).
__global__ __launch_bounds__(256) void duration_tables_kernel(DurationArgs a) {
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t ns = (size_t)a.B * a.Kr, no = (size_t)a.B * a.J;
    if (e >= ns + no) return;
    if (e < ns) {
        const size_t b = e / a.Kr;
        const double tau = duration_clip(a.tau[b], a.tau_min, a.tau_max);
        a.scales[e] = tau * a.base_scales[e];
        if (e % a.Kr == 0) a.tau[b] = tau;
        return;
    }
    const size_t o = e - ns, b = o / a.J;
    const double tau = duration_clip(a.tau[b], a.tau_min, a.tau_max);
    a.offsets[o] = tau * a.base_offsets[o];
}

// One thread per seed: the order of the header. tau_grad == nullptr: the cost term alone.
__global__ __launch_bounds__(256) void duration_gradient_kernel(DurationArgs a) {
    const size_t b = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= (size_t)a.B) return;
    if (a.tau_grad != nullptr) {
        double g = 0.0;
        for (int k = 0; k < a.Kr; ++k) {
            const double t = a.base_scales[b * a.Kr + k] * a.scale_sens[b * a.Kr + k];
            g = g + t;
        }
        for (int j = 0; j < a.J; ++j) {
            const double t = a.base_offsets[b * a.J + j] * a.offset_sens[b * a.J + j];
            g = g + t;
        }
        g = g + a.time_weight;
        a.tau_grad[b] = g;
    }
    const double price = a.time_weight * a.tau[b];
    a.cost[b] = a.cost[b] + price;
}

// One thread per seed: best_tau[b] = tau[b] where improved, then the optimizer's step where flagged
__global__ __launch_bounds__(256) void duration_step_kernel(DurationStepArgs a) {
    const size_t b = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= (size_t)a.B) return;
    if (a.improved[b]) a.best_tau[b] = a.rule.params[b];
    if (!a.rule.update[b]) return;
    optimizer_update_element(a.rule, b);
}

void launch_duration_tables(const DurationArgs& a, hipStream_t st) {
    const size_t total = (size_t)a.B * ((size_t)a.Kr + a.J);
    if (total == 0) return;
    hipLaunchKernelGGL(duration_tables_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, a);
}
void launch_duration_gradient(const DurationArgs& a, hipStream_t st) {
    if (a.B <= 0) return;
    hipLaunchKernelGGL(duration_gradient_kernel, dim3((unsigned)((a.B + 255) / 256)), dim3(256), 0, st, a);
}
void launch_duration_step(const DurationStepArgs& a, hipStream_t st) {
    if (a.B <= 0) return;
    hipLaunchKernelGGL(duration_step_kernel, dim3((unsigned)((a.B + 255) / 256)), dim3(256), 0, st, a);
}

}  // namespace qocx
