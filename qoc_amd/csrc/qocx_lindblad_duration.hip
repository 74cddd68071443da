// qocx_lindblad_duration.hip - duration search of a Lindblad sweep (qocx_lindblad_sweep_set_durations,
// LindbladDurationArgs): tau_b = T_b / T is one more optimised parameter of seed b of a duration sweep
// of open systems. Seed b is tau_b times the whole Lindbladian; in a duration sweep the drift is the
// fixed channel D_0 and the problem's own H0 is zero, so the control-free generators are the dissipator
// alone and scale with tau_b as a whole. duration_tables_kernel (qocx_duration.hip, launched as it is)
// has clipped tau_b in place and written tau_b s0_bk and tau_b delta0_bj before either kernel here runs.
//
// lindblad_duration_generators_kernel derives the per-seed tables behind the member table from the
// base tables the setter built on the host at tau = 1 (rates c0_bl gamma_l):
//
//   rate_a0[b][i][e]  = tau_b * base_a0[b][i][e]     i = A0L, A0R, A0L^H, A0R^H; two products per double2
//   rate_gammas[b][l] = tau_b * base_gammas[b][l]    l < L' (with the zero operator of a padded problem)
//
// one thread per double2 of [B][4][md], then one per rate of [B][L'], loads and stores in memory order.
//
// lindblad_duration_gradient_kernel is the chain rule through all three tables, one thread per seed,
// from the channel sensitivities of sweep_sensitivity_kernel and the rate sensitivities of
// qocx_lindblad_ratesens.hip (both launched as they are). Summation order:
//
//   g = +0.0
//   g = g + s0_bk     * dE_b/ds_bk        k = 0 .. K_r - 1 ascending
//   g = g + delta0_bj * dE_b/ddelta_bj    j = 0 .. J - 1 ascending
//   g = g + c0_bl     * dE_b/dc_bl        l = 0 .. L - 1 ascending
//   g = g + time_weight
//
// Every product and every sum is rounded on its own (no contraction into fused multiply-adds), so NumPy
// restates it term by term. The same kernel adds the price of time to the seed's cost, last of all terms:
//
//   cost_b = cost_b + time_weight * tau_b     (one product, one sum)
//
// The rate sensitivities lie in launch order (seeds grouped by sub-division count): thread p takes the
// seed order[p] of the evaluation's order table and row p of the rate sensitivities, so every seed is
// still one thread. duration_step_kernel (qocx_duration.hip) steps tau_b and keeps the best.
//
// Access: the generators kernel streams [B][4][md] double2 once each way, coalesced; the gradient kernel
// reads K_r + J + L short strided rows per seed. Both are launch-bound at the sizes of a sweep
// (B <= 1024, md <= 1024).
#include "qocx_device.h"

namespace qocx {

#pragma clang fp contract(off)

__global__ __launch_bounds__(256) void lindblad_duration_generators_kernel(LindbladDurationArgs a) {
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t na = (size_t)a.B * a.a0_per_seed, ng = (size_t)a.B * a.Lp;
    if (e >= na + ng) return;
    if (e < na) {
        const double tau = a.tau[e / a.a0_per_seed];
        const double2 v = a.base_a0[e];
        a.a0[e] = make_double2(tau * v.x, tau * v.y);
        return;
    }
    const size_t r = e - na;
    a.gammas[r] = a.tau[r / a.Lp] * a.base_gammas[r];
}

// One thread per seed, in launch order: the order of the header. tau_grad == nullptr: the cost term alone.
__global__ __launch_bounds__(256) void lindblad_duration_gradient_kernel(LindbladDurationArgs a) {
    const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= (size_t)a.B) return;
    const size_t b = (size_t)a.order[p];
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
        for (int l = 0; l < a.L; ++l) {
            const double t = a.base_rates[b * a.L + l] * a.rate_sens[p * a.L + l];
            g = g + t;
        }
        g = g + a.time_weight;
        a.tau_grad[b] = g;
    }
    const double price = a.time_weight * a.tau[b];
    a.cost[b] = a.cost[b] + price;
}

void launch_lindblad_duration_generators(const LindbladDurationArgs& a, hipStream_t st) {
    const size_t total = (size_t)a.B * (a.a0_per_seed + (size_t)a.Lp);
    if (total == 0) return;
    hipLaunchKernelGGL(lindblad_duration_generators_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0,
                       st, a);
}
void launch_lindblad_duration_gradient(const LindbladDurationArgs& a, hipStream_t st) {
    if (a.B <= 0) return;
    hipLaunchKernelGGL(lindblad_duration_gradient_kernel, dim3((unsigned)((a.B + 255) / 256)), dim3(256), 0, st,
                       a);
}

}  // namespace qocx
