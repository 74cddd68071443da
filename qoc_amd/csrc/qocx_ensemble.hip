// Hamiltonian ensembles (qocx_set_ensemble, EnsembleArgs): member m of seed b is the problem's
// structured Hamiltonian on the K = K_r + J channel controls
//
//   r_(b,m)[j][k] = s_mk u_b[j][k]     (k < K_r: the seed's controls, scaled per member)
//   r_(b,m)[j][k] = delta_m(k - K_r)   (k >= K_r: the fixed perturbation channels, constant in time)
//
// The expand kernel writes these B x M items in the order b * M + m; the evaluation runs on them
// unchanged, and the reduce kernel folds the member results back into seed results:
//
//   cost_b = sum_m w_m c_(b,m)      grad_b[j][k] = sum_m (w_m s_mk) dc_(b,m)/dr[j][k]   (k < K_r)
//
// Both kernels are FP64 loads and stores with one output element per thread; the sums run over
// the members in index order with explicit fma, so their results do not depend on the launch.
#include "qocx_device.h"

namespace qocx {

// One thread per element of the expanded [B][M][nc][K] controls.
__global__ __launch_bounds__(256) void ensemble_expand_kernel(EnsembleArgs a) {
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t total = (size_t)a.B * a.M * a.nc * a.K;
    if (e >= total) return;
    const int k = (int)(e % a.K);
    const size_t row = e / a.K;  // item * nc + j
    const int j = (int)(row % a.nc);
    const size_t item = row / a.nc;
    const int m = (int)(item % a.M);
    const size_t b = item / a.M;
    a.controls[e] = k < a.Kr ? a.scales[(size_t)m * a.Kr + k] * a.seed_controls[(b * a.nc + j) * a.Kr + k]
                             : a.offsets[(size_t)m * a.J + (k - a.Kr)];
}

// One thread per seed cost (e < B), then one per seed gradient element (e - B < B nc K_r).
__global__ __launch_bounds__(256) void ensemble_reduce_kernel(EnsembleArgs a) {
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < (size_t)a.B) {
        double acc = 0.0;
        for (int m = 0; m < a.M; ++m) acc = fma(a.weights[m], a.member_cost[e * a.M + m], acc);
        a.cost[e] = acc;
        return;
    }
    if (a.grads == nullptr) return;
    const size_t g = e - a.B;
    if (g >= (size_t)a.B * a.nc * a.Kr) return;
    const int k = (int)(g % a.Kr);
    const size_t row = g / a.Kr;  // b * nc + j
    const int j = (int)(row % a.nc);
    const size_t b = row / a.nc;
    double acc = 0.0;
    for (int m = 0; m < a.M; ++m) {
        const double ws = a.weights[m] * a.scales[(size_t)m * a.Kr + k];
        acc = fma(ws, a.member_grads[((b * a.M + m) * a.nc + j) * a.K + k], acc);
    }
    a.grads[g] = acc;
}

void launch_ensemble_expand(const EnsembleArgs& a, hipStream_t st) {
    const size_t total = (size_t)a.B * a.M * a.nc * a.K;
    if (total == 0) return;
    hipLaunchKernelGGL(ensemble_expand_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, a);
}
void launch_ensemble_reduce(const EnsembleArgs& a, hipStream_t st) {
    const size_t total = (size_t)a.B + (a.grads ? (size_t)a.B * a.nc * a.Kr : 0);
    if (total == 0) return;
    hipLaunchKernelGGL(ensemble_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, a);
}

}  // namespace qocx
