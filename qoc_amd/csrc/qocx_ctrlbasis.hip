// qocx_ctrlbasis.hip - the linear map of a control basis on the device (qocx_opt_begin_basis,
// qocx_control_basis_apply): the optimizer's coefficients coef [B][P][C] to the evaluated pulse
// u [B][Nc][C] through a real matrix M [Nc][P], and the pulse's gradient back to the coefficients.
// qoc_amd/standard/controlbasis.py states the arithmetic; these kernels are that file's two loops:
//   expand   u[b][j][c] = sum over p = 0 .. P-1  of M[j][p] * coef[b][p][c]
//   project  h[b][p][c] = sum over j = 0 .. Nc-1 of M[j][p] * g[b][j][c]
// each as acc = acc + M * x in increasing index from +0.0, one thread per output, sequential in the
// summed index. The discipline of qocx_optim.hip holds: the product and the sum are each rounded on
// their own (no contraction into fused multiply-adds), so an output has the bits of
// ControlBasis.expand / project whatever the batch and whatever the launch geometry.
//
// Access: the outputs of a seed are contiguous and the threads are laid over them in memory order, so
// stores are coalesced. Neighbouring threads differ in the channel first and then in the knot j
// (expand) or the coefficient p (project); with the matrix read in the orientation in which that index
// is contiguous - the transpose Mt [P][Nc] for expand, M [Nc][P] for project - a wave reads 64 / C
// neighbouring doubles of one matrix line per term, and the C input values of the term, which every
// thread of the seed shares, come from the cache. The driver keeps both orientations on the device.
// No LDS stage: a line of the matrix is used once per wave and term. Each thread issues the loads of
// eight terms together, so that the memory latency is paid once per eight terms, not once per term.
//
// Work at the headline shape (B = 256, Nc = 1001, C = 4): sine(1001, 16) is 16 M multiply-adds each
// way; a square filter (P = Nc) is 1 G each way, the one case in which these kernels are not small
// beside the clip and the optimizer update.
//
// Resources (hipcc -O3, gfx950, -Rpass-analysis=kernel-resource-usage): both kernels 44 VGPRs, 8 waves
// per SIMD, no LDS, scratch 0; the sums compile to v_mul_f64 / v_add_f64 pairs, no v_fma_f64.
#include "qocx_device.h"

namespace qocx {

#pragma clang fp contract(off)

// sum_i m[i * m_stride] * x[i * x_stride], i = 0 .. count-1 in increasing order from +0.0. The loads of
// eight terms are issued together (they do not depend on the sum), the sum itself stays one chain.
__device__ __forceinline__ double sum_in_order(const double* __restrict__ m, size_t m_stride,
                                               const double* __restrict__ x, size_t x_stride, int count) {
    double acc = 0.0;
    int i = 0;
    for (; i + 8 <= count; i += 8) {
        double mm[8], xx[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            mm[u] = m[(size_t)(i + u) * m_stride];
            xx[u] = x[(size_t)(i + u) * x_stride];
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const double prod = mm[u] * xx[u];
            acc = acc + prod;
        }
    }
    for (; i < count; ++i) {
        const double prod = m[(size_t)i * m_stride] * x[(size_t)i * x_stride];
        acc = acc + prod;
    }
    return acc;
}

// out[b][j][c], one per thread; idx runs over [B][Nc][C] in memory order
__global__ void __launch_bounds__(256)
basis_expand_kernel(const double* __restrict__ matrix_t, const double* __restrict__ coef,
                    double* __restrict__ out, size_t total, int nc, int p_count, int channels) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const size_t per_out = (size_t)nc * channels;
    const size_t b = idx / per_out, r = idx - b * per_out;
    const size_t j = r / channels, c = r - j * channels;
    out[idx] = sum_in_order(matrix_t + j, (size_t)nc, coef + b * (size_t)p_count * channels + c,
                            (size_t)channels, p_count);
}

// out[b][p][c], one per thread; idx runs over [B][P][C] in memory order
__global__ void __launch_bounds__(256)
basis_project_kernel(const double* __restrict__ matrix, const double* __restrict__ grads,
                     double* __restrict__ out, size_t total, int nc, int p_count, int channels) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const size_t per_out = (size_t)p_count * channels;
    const size_t b = idx / per_out, r = idx - b * per_out;
    const size_t p = r / channels, c = r - p * channels;
    out[idx] = sum_in_order(matrix + p, (size_t)p_count, grads + b * (size_t)nc * channels + c,
                            (size_t)channels, nc);
}

// matrix_t [P][Nc], coef [B][P][C] -> out [B][Nc][C]
void launch_basis_expand(const double* matrix_t, const double* coef, double* out, int batch, int nc,
                         int p_count, int channels, hipStream_t st) {
    const size_t total = (size_t)batch * nc * channels;
    if (total == 0 || p_count <= 0) return;
    hipLaunchKernelGGL(basis_expand_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st,
                       matrix_t, coef, out, total, nc, p_count, channels);
}

// matrix [Nc][P], grads [B][Nc][C] -> out [B][P][C]
void launch_basis_project(const double* matrix, const double* grads, double* out, int batch, int nc,
                          int p_count, int channels, hipStream_t st) {
    const size_t total = (size_t)batch * p_count * channels;
    if (total == 0 || nc <= 0) return;
    hipLaunchKernelGGL(basis_project_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st,
                       matrix, grads, out, total, nc, p_count, channels);
}

}  // namespace qocx
