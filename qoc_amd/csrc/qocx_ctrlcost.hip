// qocx_ctrlcost.hip - the four built-in costs of the controls alone and their gradients for B
// control sets resident in HBM (qoc/standard/costs/controlnorm.py:48-73, controlvariation.py:47-75,
// controlarea.py:43-67, controlbandwidthmax.py:52-77), so that a multi-start GRAPE run with
// pulse-shaping penalties keeps its controls and gradients on the device.
//
// ControlNorm, ControlVariation and ControlArea run in one workgroup per seed
// (control_costs_kernel): elementwise arithmetic in the order of the NumPy expressions, every
// product and sum rounded on its own, sums in a fixed order - a seed's numbers do not depend on
// the batch it is part of.
//
// ControlBandwidthMax needs the DFT of every control at the bins P_k above its bandwidth only, and
// the inverse DFT of cotangents that live on those bins only: two products with the |P_k| x nc
// matrix of twiddles exp(-2 pi i j f / nc) over the B columns of control k. The twiddles are read
// from ONE table of nc entries at the exactly reduced phase (j f) mod nc, which the loops carry
// along by additions; a thread owns one bin (forwards) or one knot (backwards) of eight columns
// and sums in index order with explicit fma.
#include "../../include/qocx.h"
#include "qocx_device.h"

namespace qocx {

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;
constexpr int kColumns = 8;    // columns of a control per workgroup of the DFT kernels
constexpr int kKnotTile = 128; // knots of the columns staged in LDS at a time (forwards)
constexpr int kBinTile = 64;   // bins of the columns staged in LDS at a time (backwards)
constexpr int kTwiddleLds = 3072;  // tables up to this many entries (48 KB) are copied to LDS

// sum over the workgroup in a fixed tree; every thread returns the total
__device__ double block_sum(double v, double* lds) {
    const int t = threadIdx.x;
    __syncthreads();
    lds[t] = v;
    __syncthreads();
    for (int s = kThreads / 2; s > 0; s >>= 1) {
        if (t < s) lds[t] = lds[t] + lds[t + s];
        __syncthreads();
    }
    return lds[0];
}

// u / max as NumPy forms it: a real quotient, but a complex array divided by a real one goes
// through the complex quotient, which multiplies by the reciprocal of the divisor
__device__ __forceinline__ double quotient(double u, double mx, int cplx) {
    return cplx ? u * (1.0 / mx) : u / mx;
}

// NumPy's pairwise summation of a contiguous complex array (the add reduction of
// numpy/core/src/umath/loops_utils.h), for one part (Re or Im) of ONE complex control: up to 64
// entries in four strided partial sums combined as (r0 + r1) + (r2 + r3) plus a tail, longer ranges
// split at (len - len % 8) / 2 and their halves added. x[2 j] / mx is entry j. The recursion runs
// on an explicit stack of frames (a range halves at every level: 40 levels never fill).
constexpr int kPairwiseDepth = 40;
struct PairwiseFrame {
    int start, len, state;
    double left;
};

__device__ double pairwise_leaf(const double* x, int len, double inv) {
    if (len < 4) {
        double r = 0.0;
        for (int i = 0; i < len; ++i) r = r + x[2 * i] * inv;
        return r;
    }
    double r0 = x[0] * inv, r1 = x[2] * inv, r2 = x[4] * inv, r3 = x[6] * inv;
    int i = 4;
    for (; i < len - len % 4; i += 4) {
        r0 = r0 + x[2 * i] * inv;
        r1 = r1 + x[2 * i + 2] * inv;
        r2 = r2 + x[2 * i + 4] * inv;
        r3 = r3 + x[2 * i + 6] * inv;
    }
    double r = (r0 + r1) + (r2 + r3);
    for (; i < len; ++i) r = r + x[2 * i] * inv;
    return r;
}

__device__ double pairwise_knot_sum(const double* x, int nc, double mx, PairwiseFrame* f) {
    const double inv = 1.0 / mx;  // (the complex quotient by a real number: see quotient())
    int d = 0;
    double ret = 0.0;
    f[0].start = 0; f[0].len = nc; f[0].state = 0;
    while (d >= 0) {
        const int start = f[d].start, len = f[d].len, half = (len - len % 8) / 2;
        if (f[d].state == 0) {
            if (len <= 64 || d + 1 >= kPairwiseDepth) {
                ret = pairwise_leaf(x + 2 * (size_t)start, len, inv);
                --d;
                continue;
            }
            f[d].state = 1;
            f[d + 1].start = start; f[d + 1].len = half; f[d + 1].state = 0;
            ++d;
        } else if (f[d].state == 1) {
            f[d].left = ret;
            f[d].state = 2;
            f[d + 1].start = start + half; f[d + 1].len = len - half; f[d + 1].state = 0;
            ++d;
        } else {
            ret = f[d].left + ret;
            --d;
        }
    }
    return ret;
}

}  // namespace

// One workgroup per seed. Element e = j * Kr + ch of a seed is always handled by thread e % 256.
__global__ __launch_bounds__(kThreads) void control_costs_kernel(CtrlCostArgs a) {
    __shared__ double red[kThreads];
    __shared__ double sums[128];  // ControlArea: the sum of every channel (Kr <= 128)
    __shared__ PairwiseFrame frames[2][kPairwiseDepth];  // ... of the two channels of a single complex control
    const int t = threadIdx.x, nc = a.nc, Kr = a.Kr, cplx = a.cplx;
    const int per = nc * Kr;
    const size_t base = (size_t)blockIdx.x * per;
    const double* u = a.controls + base;
    double* g = a.grad ? a.grad + base : nullptr;
    double* w0 = a.work0 + base;
    double* w1 = a.work1 + base;
    if (g)
        for (int e = t; e < per; e += kThreads) g[e] = 0.0;
    double total = 0.0;
    for (int d = 0; d < a.count; ++d) {
        const CtrlCostDev c = a.descs[d];
        if (c.kind == QOCX_CONTROL_NORM) {
            double part = 0.0;
            for (int e = t; e < per; e += kThreads) {
                const int k = (e % Kr) >> cplx;
                const double x = quotient(u[e], c.max_norms[k], cplx) * c.weights[k];
                part = part + x * x;
                if (g) {
                    const double f = (1.0 / c.max_norms[k]) * c.weights[k];
                    g[e] = g[e] + ((2.0 * c.multiplier) * u[e]) * (f * f);
                }
            }
            total = total + block_sum(part, red) * c.multiplier;
        } else if (c.kind == QOCX_CONTROL_VARIATION) {
            for (int e = t; e < per; e += kThreads) w0[e] = quotient(u[e], c.max_norms[(e % Kr) >> cplx], cplx);
            __syncthreads();
            double* src = w0;
            double* dst = w1;
            for (int p = 1; p <= c.order; ++p) {  // forward differences along the knots
                const int len = (nc - p) * Kr;
                for (int e = t; e < len; e += kThreads) dst[e] = src[e + Kr] - src[e];
                __syncthreads();
                double* tmp = src; src = dst; dst = tmp;
            }
            const int len = (nc - c.order) * Kr;
            double part = 0.0;
            for (int e = t; e < len; e += kThreads) part = part + src[e] * src[e];
            total = total + block_sum(part, red) * c.multiplier;
            if (g) {
                for (int e = t; e < len; e += kThreads) src[e] = (2.0 * c.multiplier) * src[e];
                __syncthreads();
                for (int p = c.order; p >= 1; --p) {  // the transposed differences, one per pass
                    const int rows = nc - p;          // src has `rows` knots, dst rows + 1
                    for (int e = t; e < (rows + 1) * Kr; e += kThreads) {
                        const int j = e / Kr;
                        const double up = j >= 1 ? src[e - Kr] : 0.0;
                        dst[e] = j < rows ? up - src[e] : up;
                    }
                    __syncthreads();
                    double* tmp = src; src = dst; dst = tmp;
                }
                for (int e = t; e < per; e += kThreads)
                    g[e] = g[e] + quotient(src[e], c.max_norms[(e % Kr) >> cplx], cplx);
            }
            __syncthreads();
        } else if (c.kind == QOCX_CONTROL_AREA) {
            // The direction sum / |sum| of a complex control is only as good as the sum, and a sum
            // that cancels loses digits to its order. So the knots are added in the order of
            // numpy.sum(controls / max, axis=0): knot by knot for several controls, and for a single
            // complex control - one contiguous column - NumPy's pairwise scheme (pairwise_knot_sum).
            for (int ch = t; ch < Kr; ch += kThreads) {
                const double mx = c.max_norms[ch >> cplx];
                if (cplx && Kr == 2) {
                    sums[ch] = pairwise_knot_sum(u + ch, nc, mx, frames[ch]);
                    continue;
                }
                double s = 0.0;
                for (int j = 0; j < nc; ++j) s = s + quotient(u[j * Kr + ch], mx, cplx);
                sums[ch] = s;
            }
            __syncthreads();
            double area = 0.0;
            for (int k = 0; k < (Kr >> cplx); ++k)
                area = area + (cplx ? hypot(sums[2 * k], sums[2 * k + 1]) : fabs(sums[k]));
            total = total + area * c.multiplier;
            if (g)
                for (int e = t; e < per; e += kThreads) {
                    const int ch = e % Kr, k = ch >> cplx;
                    const double mod = cplx ? hypot(sums[2 * k], sums[2 * k + 1]) : fabs(sums[k]);
                    const double dir = mod > 0.0 ? quotient(sums[ch], mod, cplx) : 0.0;
                    g[e] = g[e] + quotient(c.multiplier * dir, c.max_norms[k], cplx);
                }
            __syncthreads();
        }
    }
    if (t == 0) a.cost[blockIdx.x] = total;
}

// ---- ControlBandwidthMax ----------------------------------------------------------------------

// spectrum[b][ch][i] = sum_j u_b[j][ch] exp(-2 pi i j f_i / nc) for the bins f_i of the control of
// channel ch. Grid: (bin tiles, groups of eight columns of the control, controls).
template <bool kLds>
__global__ __launch_bounds__(kThreads) void bandwidth_forward_kernel(BandwidthArgs a) {
    __shared__ double tile[kKnotTile][kColumns];
    __shared__ double2 table[kLds ? kTwiddleLds : 1];
    const int t = threadIdx.x, nc = a.nc, k = blockIdx.z, nch = 1 + a.cplx;
    const int first = a.bin_ptr[k], np = a.bin_ptr[k + 1] - first;
    const int i = blockIdx.x * kThreads + t;
    if ((int)(blockIdx.x * kThreads) >= np) return;  // (the whole workgroup: no bins of this control here)
    const int ncols = a.B * nch, col0 = blockIdx.y * kColumns;
    if (kLds) {
        for (int m = t; m < nc; m += kThreads) table[m] = a.twiddle[m];
    }
    const double2* tw = kLds ? table : a.twiddle;
    const bool valid = i < np;
    const int f = valid ? a.bins[first + i] : 0;
    double re[kColumns], im[kColumns];
#pragma unroll
    for (int c = 0; c < kColumns; ++c) re[c] = im[c] = 0.0;
    int idx = 0;  // (j f) mod nc
    for (int j0 = 0; j0 < nc; j0 += kKnotTile) {
        __syncthreads();
        for (int e = t; e < kKnotTile * kColumns; e += kThreads) {
            const int jj = e / kColumns, c = e % kColumns, j = j0 + jj, col = col0 + c;
            double v = 0.0;
            if (j < nc && col < ncols)
                v = a.controls[((size_t)(col / nch) * nc + j) * a.Kr + k * nch + col % nch];
            tile[jj][c] = v;
        }
        __syncthreads();
        const int jn = min(kKnotTile, nc - j0);
        if (valid)
            for (int jj = 0; jj < jn; ++jj) {
                const double2 w = tw[idx];
#pragma unroll
                for (int c = 0; c < kColumns; ++c) {
                    re[c] = fma(tile[jj][c], w.x, re[c]);
                    im[c] = fma(tile[jj][c], w.y, im[c]);
                }
                idx += f;
                if (idx >= nc) idx -= nc;
            }
    }
    if (!valid) return;
#pragma unroll
    for (int c = 0; c < kColumns; ++c) {
        const int col = col0 + c;
        if (col < ncols)
            a.spectrum[((size_t)(col / nch) * a.Kr + k * nch + col % nch) * a.pmax + i] = make_double2(re[c], im[c]);
    }
}

// One workgroup per seed, control after control: the moduli of the bins, their sum and first
// maximum, the cost term sum / (|P| top) and the cotangents ybar of the bins.
__global__ __launch_bounds__(kThreads) void bandwidth_weights_kernel(BandwidthArgs a) {
    __shared__ double red[kThreads];
    __shared__ double top_v[kThreads];
    __shared__ int top_i[kThreads];
    const int t = threadIdx.x, b = blockIdx.x, nch = 1 + a.cplx;
    double total = 0.0;
    for (int k = 0; k < a.K; ++k) {
        const int np = a.bin_ptr[k + 1] - a.bin_ptr[k];
        const double2* xa = a.spectrum + ((size_t)b * a.Kr + k * nch) * a.pmax;
        const double2* xb = xa + a.pmax;  // the imaginary channel of a complex control
        double part = 0.0, best = -1.0;
        int where = 0x7fffffff;
        for (int i = t; i < np; i += kThreads) {
            const double xr = a.cplx ? xa[i].x - xb[i].y : xa[i].x;
            const double xi = a.cplx ? xa[i].y + xb[i].x : xa[i].y;
            const double mag = hypot(xr, xi);
            part = part + mag;
            if (mag > best) { best = mag; where = i; }
        }
        const double sum = block_sum(part, red);
        top_v[t] = best;
        top_i[t] = where;
        __syncthreads();
        for (int s = kThreads / 2; s > 0; s >>= 1) {  // the first of the largest, as numpy.argmax
            if (t < s && (top_v[t + s] > top_v[t] || (top_v[t + s] == top_v[t] && top_i[t + s] < top_i[t]))) {
                top_v[t] = top_v[t + s];
                top_i[t] = top_i[t + s];
            }
            __syncthreads();
        }
        const double top = top_v[0];
        const int arg = top_i[0];
        const double scale = (double)np * top;
        total = total + sum / scale;
        if (a.grad) {
            const double weight = 1.0 / scale, at_top = weight - sum / (scale * top);
            double2* y = a.ybar + ((size_t)b * a.K + k) * a.pmax;
            for (int i = t; i < np; i += kThreads) {
                const double xr = a.cplx ? xa[i].x - xb[i].y : xa[i].x;
                const double xi = a.cplx ? xa[i].y + xb[i].x : xa[i].y;
                const double mag = hypot(xr, xi), w = i == arg ? at_top : weight;
                const double inv = 1.0 / (mag > 0.0 ? mag : 1.0);
                y[i] = make_double2((w * xr) * inv, (w * xi) * inv);
            }
        }
        __syncthreads();
    }
    if (t == 0) a.cost[b] = a.cost[b] + total * a.multiplier;
}

// grad[b][j][channels of k] += multiplier * sum_i ybar[b][k][i] exp(+2 pi i j f_i / nc) (its real
// part for a real control). Grid: (knot tiles, groups of eight seeds, controls).
template <bool kLds, bool kCplx>
__global__ __launch_bounds__(kThreads) void bandwidth_backward_kernel(BandwidthArgs a) {
    __shared__ double2 tile[kBinTile][kColumns];
    __shared__ double2 table[kLds ? kTwiddleLds : 1];
    const int t = threadIdx.x, nc = a.nc, k = blockIdx.z, nch = kCplx ? 2 : 1;
    const int first = a.bin_ptr[k], np = a.bin_ptr[k + 1] - first;
    const int j = blockIdx.x * kThreads + t, b0 = blockIdx.y * kColumns;
    if (kLds) {
        for (int m = t; m < nc; m += kThreads) table[m] = a.twiddle[m];
    }
    const double2* tw = kLds ? table : a.twiddle;
    double gr[kColumns], gi[kColumns];
#pragma unroll
    for (int c = 0; c < kColumns; ++c) gr[c] = gi[c] = 0.0;
    int idx = 0, prev = 0, delta = -nc - 1, step = 0;  // idx = (j f) mod nc, carried from bin to bin
    for (int i0 = 0; i0 < np; i0 += kBinTile) {
        __syncthreads();
        for (int e = t; e < kBinTile * kColumns; e += kThreads) {
            const int ii = e / kColumns, c = e % kColumns, i = i0 + ii, b = b0 + c;
            tile[ii][c] = (i < np && b < a.B) ? a.ybar[((size_t)b * a.K + k) * a.pmax + i] : make_double2(0.0, 0.0);
        }
        __syncthreads();
        const int in = min(kBinTile, np - i0);
        for (int ii = 0; ii < in; ++ii) {
            const int f = a.bins[first + i0 + ii];
            if (f - prev != delta) {  // (the same for every thread; bins above a bandwidth are consecutive)
                delta = f - prev;
                step = (int)(((long long)j % nc * (((long long)delta % nc + nc) % nc)) % nc);
            }
            prev = f;
            idx += step;
            if (idx >= nc) idx -= nc;
            const double2 w = tw[idx];  // exp(-i theta); the sum needs its conjugate
#pragma unroll
            for (int c = 0; c < kColumns; ++c) {
                const double2 y = tile[ii][c];
                gr[c] = fma(y.x, w.x, gr[c]);
                gr[c] = fma(y.y, w.y, gr[c]);
                if (kCplx) {
                    gi[c] = fma(y.y, w.x, gi[c]);
                    gi[c] = fma(-y.x, w.y, gi[c]);
                }
            }
        }
    }
    if (j >= nc) return;
#pragma unroll
    for (int c = 0; c < kColumns; ++c) {
        const int b = b0 + c;
        if (b >= a.B) continue;
        double* g = a.grad + ((size_t)b * nc + j) * a.Kr + k * nch;
        g[0] = g[0] + gr[c] * a.multiplier;
        if (kCplx) g[1] = g[1] + gi[c] * a.multiplier;
    }
}

__global__ void add_control_costs_kernel(double* cost, const double* add_cost, double* grads,
                                         const double* add_grad, size_t per_seed) {
    const size_t b = blockIdx.x;
    const size_t idx = (size_t)blockIdx.y * blockDim.x + threadIdx.x;
    if (idx == 0) cost[b] = cost[b] + add_cost[b];
    if (grads && idx < per_seed) grads[b * per_seed + idx] = grads[b * per_seed + idx] + add_grad[b * per_seed + idx];
}

void launch_control_costs(const CtrlCostArgs& a, hipStream_t st) {
    if (a.B <= 0) return;
    hipLaunchKernelGGL(control_costs_kernel, dim3(a.B), dim3(kThreads), 0, st, a);
}

void launch_bandwidth_cost(const BandwidthArgs& a, hipStream_t st) {
    if (a.B <= 0 || a.K <= 0 || a.pmax <= 0) return;
    const bool lds = a.nc <= kTwiddleLds;
    const int nch = 1 + a.cplx;
    const dim3 fwd((a.pmax + kThreads - 1) / kThreads, (a.B * nch + kColumns - 1) / kColumns, a.K);
    if (lds)
        hipLaunchKernelGGL(bandwidth_forward_kernel<true>, fwd, dim3(kThreads), 0, st, a);
    else
        hipLaunchKernelGGL(bandwidth_forward_kernel<false>, fwd, dim3(kThreads), 0, st, a);
    hipLaunchKernelGGL(bandwidth_weights_kernel, dim3(a.B), dim3(kThreads), 0, st, a);
    if (!a.grad) return;
    const dim3 bwd((a.nc + kThreads - 1) / kThreads, (a.B + kColumns - 1) / kColumns, a.K);
    if (lds && a.cplx)
        hipLaunchKernelGGL((bandwidth_backward_kernel<true, true>), bwd, dim3(kThreads), 0, st, a);
    else if (lds)
        hipLaunchKernelGGL((bandwidth_backward_kernel<true, false>), bwd, dim3(kThreads), 0, st, a);
    else if (a.cplx)
        hipLaunchKernelGGL((bandwidth_backward_kernel<false, true>), bwd, dim3(kThreads), 0, st, a);
    else
        hipLaunchKernelGGL((bandwidth_backward_kernel<false, false>), bwd, dim3(kThreads), 0, st, a);
}

void launch_add_control_costs(double* cost, const double* add_cost, double* grads, const double* add_grad,
                              int batch, size_t per_seed, hipStream_t st) {
    if (batch <= 0) return;
    const size_t widest = grads && per_seed > 1 ? per_seed : 1;
    hipLaunchKernelGGL(add_control_costs_kernel, dim3(batch, (unsigned)((widest + kThreads - 1) / kThreads)),
                       dim3(kThreads), 0, st, cost, add_cost, grads, add_grad, per_seed);
}

}  // namespace qocx
