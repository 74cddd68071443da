// qocx_sweep.hip - Hamiltonian sweeps (qocx_set_sweep, SystemSweepArgs): B seeds, each a system of its
// own on the problem's K = K_r + J channels. Item b IS seed b:
//
//   r_b[j][k] = s_bk u_b[j][k]      (k < K_r: the seed's own controls, scaled per seed)
//   r_b[j][k] = delta_b(k - K_r)    (k >= K_r: the fixed channels, constant in time)
//
// The expand kernel writes the B items, the evaluation runs on them as on any batch, and the
// reduce kernel takes the items' results back to the seeds:
//
//   cost_b = c_b      grad_b[j][k] = s_bk dc_b/dr[j][k]   (k < K_r; one product, one rounding)
//
// The sensitivity kernel gives the derivatives of a seed's cost with respect to its own table
// entries (qocx_sweep_download_sensitivities):
//
//   dE_b/ds_bk     = sum over j of u_b[j][k] g_b[j][k]          (k < K_r)
//   dE_b/ddelta_bi = sum over j of g_b[j][K_r + i]              (i < J)
//
// with g_b = dc_b/dr the item's gradient. Summation order of one such sum over the Nc knots,
// QOCX_SWEEP_LANES = 64 partial sums first, then a fixed tree:
//
//   p[l] = ((t[l] + t[l + 64]) + t[l + 128]) + ...   knots l, l + 64, ... ascending, from +0.0
//                                                     (t[j] the rounded product, or g itself)
//   for h = 32, 16, 8, 4, 2, 1:   p[l] = p[l] + p[l + h]   for l < h
//   result = p[0]
//
// Product and sum are each rounded on their own (no contraction into fused multiply-adds), a lane
// without knots contributes +0.0, and IEEE addition commutes, so the butterfly below leaves in
// every lane the bits of that tree: the result depends on Nc alone, never on the launch. NumPy
// restates it as  p = [sum_in_order(t[l::64]) for l in range(64)]; h = 32 ...: p = p[:h] + p[h:2h].
//
// Access: expand and reduce are one FP64 element per thread in memory order (coalesced). The
// sensitivity kernel runs one workgroup of four waves per seed; a wave takes one channel at a
// time and lays its 64 lanes over 64 consecutive knots of that channel, so the four waves of the
// workgroup read the same K-wide rows of the seed together and every fetched line is used whole
// by the workgroup. It runs once per download, not per iteration.
#include "qocx_device.h"

namespace qocx {

#pragma clang fp contract(off)

// One thread per element of the expanded [B][nc][K] controls.
__global__ __launch_bounds__(256) void sweep_expand_kernel(SystemSweepArgs a) {
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t total = (size_t)a.B * a.nc * a.K;
    if (e >= total) return;
    const int k = (int)(e % a.K);
    const size_t row = e / a.K;  // b * nc + j
    const size_t b = row / a.nc;
    a.controls[e] = k < a.Kr ? a.scales[b * a.Kr + k] * a.seed_controls[row * a.Kr + k]
                             : a.offsets[b * a.J + (k - a.Kr)];
}

// One thread per seed cost (e < B), then one per seed gradient element (e - B < B nc K_r).
__global__ __launch_bounds__(256) void sweep_reduce_kernel(SystemSweepArgs a) {
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < (size_t)a.B) {
        a.cost[e] = a.item_cost[e];
        return;
    }
    if (a.grads == nullptr) return;
    const size_t g = e - a.B;
    if (g >= (size_t)a.B * a.nc * a.Kr) return;
    const int k = (int)(g % a.Kr);
    const size_t row = g / a.Kr;  // b * nc + j
    const size_t b = row / a.nc;
    a.grads[g] = a.scales[b * a.Kr + k] * a.item_grads[row * a.K + k];
}

// the tree of the header over the 64 partial sums of a wave: every lane ends with p[0]'s bits
__device__ __forceinline__ double sweep_lane_tree(double p) {
#pragma unroll
    for (int h = QOCX_SWEEP_LANES / 2; h >= 1; h >>= 1) {
        const double other = __shfl_xor(p, h, QOCX_SWEEP_LANES);
        p = p + other;
    }
    return p;
}

// Workgroup b: seed b; wave w takes the channels w, w + 4, ... of the K; lane l the knots l, l + 64, ...
__global__ __launch_bounds__(256) void sweep_sensitivity_kernel(SystemSweepArgs a) {
    const size_t b = blockIdx.x;
    const int lane = threadIdx.x % QOCX_SWEEP_LANES, wave = threadIdx.x / QOCX_SWEEP_LANES;
    const int waves = blockDim.x / QOCX_SWEEP_LANES;
    const double* g = a.item_grads + b * (size_t)a.nc * a.K;
    const double* u = a.seed_controls + b * (size_t)a.nc * a.Kr;
    for (int k = wave; k < a.K; k += waves) {
        double p = 0.0;
        if (k < a.Kr) {
            for (int j = lane; j < a.nc; j += QOCX_SWEEP_LANES) {
                const double t = u[(size_t)j * a.Kr + k] * g[(size_t)j * a.K + k];
                p = p + t;
            }
        } else {
            for (int j = lane; j < a.nc; j += QOCX_SWEEP_LANES) p = p + g[(size_t)j * a.K + k];
        }
        p = sweep_lane_tree(p);
        if (lane == 0) {
            if (k < a.Kr) a.scale_sens[b * a.Kr + k] = p;
            else a.offset_sens[b * a.J + (k - a.Kr)] = p;
        }
    }
}

void launch_sweep_expand(const SystemSweepArgs& a, hipStream_t st) {
    const size_t total = (size_t)a.B * a.nc * a.K;
    if (total == 0) return;
    hipLaunchKernelGGL(sweep_expand_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, a);
}
void launch_sweep_reduce(const SystemSweepArgs& a, hipStream_t st) {
    const size_t total = (size_t)a.B + (a.grads ? (size_t)a.B * a.nc * a.Kr : 0);
    if (total == 0) return;
    hipLaunchKernelGGL(sweep_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, a);
}
void launch_sweep_sensitivity(const SystemSweepArgs& a, hipStream_t st) {
    if (a.B == 0 || a.K == 0) return;
    hipLaunchKernelGGL(sweep_sensitivity_kernel, dim3((unsigned)a.B), dim3(256), 0, st, a);
}

}  // namespace qocx
