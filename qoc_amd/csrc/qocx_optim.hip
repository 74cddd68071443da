// qocx_optim.hip - the multi-start GRAPE driver's per-iteration arithmetic on the device: control
// clipping (qoc/core/common.py:8-30), best-so-far bookkeeping and the Adam / SGD update
// (qoc/standard/optimizers/adam.py:110-165, sgd.py) for B control sets resident in HBM. Plain
// elementwise kernels, HBM bound (seven 4 MB arrays per update at the headline size: ~10 us).
//
// Every product and sum is rounded on its own (no contraction into fused multiply-adds) and
// division / square root are the IEEE ones, so a seed walks the trajectory of the reference's
// NumPy arithmetic bit for bit (tests/test_gpu_api.py: B = 8 equals eight single-seed runs).
#include "qocx_device.h"

namespace qocx {

#pragma clang fp contract(off)

__global__ void clip_controls_kernel(double* controls, size_t total, int k, const double* max_norms) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const double v = controls[idx], mod = fabs(v), mx = max_norms[idx % k];
    if (mx < mod) controls[idx] = (v / mod) * mx;
}

// complex controls (channels 2k, 2k+1 of a knot): the parameters clipped by modulus into the buffer
// that is evaluated, as clip_control_norms acts on the complex array slap_controls builds - NumPy
// divides the complex entry by its real modulus through the reciprocal
__global__ void clip_complex_kernel(const double* params, double* controls, size_t pairs, int k,
                                    const double* max_norms) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= pairs) return;
    double re = params[2 * idx], im = params[2 * idx + 1];
    const double mod = hypot(re, im), mx = max_norms[idx % k];
    if (mx < mod) {
        const double inv = 1.0 / mod;
        re = (re * inv) * mx;
        im = (im * inv) * mx;
    }
    controls[2 * idx] = re;
    controls[2 * idx + 1] = im;
}

// best_controls[b] = controls[b], best_final[b] = final[b] for the seeds flagged in `improved`
__global__ void keep_best_kernel(const double* controls, double* best_controls, size_t per_seed,
                                 const double2* final_states, double2* best_final, size_t final_per_seed,
                                 const unsigned char* improved) {
    const size_t b = blockIdx.x;  // (the seed index on grid.x: no 65535 limit on the batch)
    if (!improved[b]) return;
    const size_t idx = (size_t)blockIdx.y * blockDim.x + threadIdx.x;
    if (idx < per_seed) best_controls[b * per_seed + idx] = controls[b * per_seed + idx];
    if (idx < final_per_seed) best_final[b * final_per_seed + idx] = final_states[b * final_per_seed + idx];
}

__global__ void optimizer_update_kernel(OptimArgs a) {
    const size_t b = blockIdx.x;
    if (!a.update[b]) return;
    const size_t idx = (size_t)blockIdx.y * blockDim.x + threadIdx.x;
    if (idx >= a.per_seed) return;
    optimizer_update_element(a, b * a.per_seed + idx);  // (qocx_device.h: shared with qocx_duration.hip)
}

// ---- the Lindblad multi-start driver (qocx_lindblad_*): resident controls and results in seed
// order, the evaluation's buffers in sub-division group order (device position -> seed: order[]).

// umax[b][k] = max_i |controls[b][i][k]|, scanned in knot order with the host's update rule of
// qocx_eval_lindblad (`if (!(a <= um)) um = a;`), so a NaN is carried exactly as the host carries it
__global__ void control_maxima_kernel(const double* controls, int batch, int nc, int k, double* umax) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= batch * k) return;
    const int b = idx / k, kk = idx % k;
    const double* u = controls + (size_t)b * nc * k + kk;
    double um = 0;
    for (int i = 0; i < nc; ++i) {
        const double a = fabs(u[(size_t)i * k]);
        if (!(a <= um)) um = a;
    }
    umax[idx] = um;
}

// dst[pos] = src[order[pos]], per_seed doubles per seed
__global__ void gather_seeds_kernel(const double* src, double* dst, size_t per_seed, const int* order) {
    const size_t pos = blockIdx.x;
    const size_t idx = (size_t)blockIdx.y * blockDim.x + threadIdx.x;
    if (idx < per_seed) dst[pos * per_seed + idx] = src[(size_t)order[pos] * per_seed + idx];
}

// the results of position pos go to seed order[pos]: cost, gradients, final-density dumps
__global__ void scatter_seeds_kernel(const double* cost, double* cost_out, const double* grads,
                                     double* grads_out, size_t grad_per_seed, const double2* final_states,
                                     double2* final_out, size_t final_per_seed, const int* order) {
    const size_t pos = blockIdx.x, b = (size_t)order[pos];
    const size_t idx = (size_t)blockIdx.y * blockDim.x + threadIdx.x;
    if (idx == 0) cost_out[b] = cost[pos];
    if (grads && idx < grad_per_seed) grads_out[b * grad_per_seed + idx] = grads[pos * grad_per_seed + idx];
    if (idx < final_per_seed) final_out[b * final_per_seed + idx] = final_states[pos * final_per_seed + idx];
}

void launch_control_maxima(const double* controls, int batch, int nc, int k, double* umax, hipStream_t st) {
    if (batch <= 0 || k <= 0) return;
    hipLaunchKernelGGL(control_maxima_kernel, dim3((unsigned)((batch * k + 63) / 64)), dim3(64), 0, st,
                       controls, batch, nc, k, umax);
}
void launch_gather_seeds(const double* src, double* dst, size_t per_seed, const int* order, int batch,
                         hipStream_t st) {
    if (batch <= 0 || per_seed == 0) return;
    hipLaunchKernelGGL(gather_seeds_kernel, dim3(batch, (unsigned)((per_seed + 255) / 256)), dim3(256), 0,
                       st, src, dst, per_seed, order);
}
void launch_scatter_seeds(const double* cost, double* cost_out, const double* grads, double* grads_out,
                          size_t grad_per_seed, const double2* final_states, double2* final_out,
                          size_t final_per_seed, const int* order, int batch, hipStream_t st) {
    size_t widest = final_per_seed > 1 ? final_per_seed : 1;
    if (grads && grad_per_seed > widest) widest = grad_per_seed;
    if (batch <= 0) return;
    hipLaunchKernelGGL(scatter_seeds_kernel, dim3(batch, (unsigned)((widest + 255) / 256)), dim3(256), 0,
                       st, cost, cost_out, grads, grads_out, grad_per_seed, final_states, final_out,
                       final_per_seed, order);
}

void launch_clip_controls(double* controls, size_t total, int k, const double* max_norms, hipStream_t st) {
    if (total == 0 || k <= 0) return;
    hipLaunchKernelGGL(clip_controls_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st,
                       controls, total, k, max_norms);
}
void launch_clip_complex(const double* params, double* controls, size_t pairs, int k,
                         const double* max_norms, hipStream_t st) {
    if (pairs == 0 || k <= 0) return;
    hipLaunchKernelGGL(clip_complex_kernel, dim3((unsigned)((pairs + 255) / 256)), dim3(256), 0, st,
                       params, controls, pairs, k, max_norms);
}
void launch_keep_best(const double* controls, double* best_controls, size_t per_seed,
                      const double2* final_states, double2* best_final, size_t final_per_seed,
                      const unsigned char* improved, int batch, hipStream_t st) {
    const size_t widest = per_seed > final_per_seed ? per_seed : final_per_seed;
    if (batch <= 0 || widest == 0) return;
    hipLaunchKernelGGL(keep_best_kernel, dim3(batch, (unsigned)((widest + 255) / 256)), dim3(256), 0, st,
                       controls, best_controls, per_seed, final_states, best_final, final_per_seed,
                       improved);
}
void launch_optimizer_update(const OptimArgs& a, int batch, hipStream_t st) {
    if (batch <= 0 || a.per_seed == 0) return;
    hipLaunchKernelGGL(optimizer_update_kernel, dim3(batch, (unsigned)((a.per_seed + 255) / 256)),
                       dim3(256), 0, st, a);
}

}  // namespace qocx
