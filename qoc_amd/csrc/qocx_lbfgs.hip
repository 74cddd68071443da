// qocx_lbfgs.hip - L-BFGS with an Armijo backtracking line search for the seeds of the multi-start
// GRAPE driver, its state resident in HBM. qoc_amd/standard/optimizers/lbfgs.py states the algorithm
// (a per-seed state machine: one evaluation in, the next trial point out); this kernel is that file's
// arithmetic for B seeds, one workgroup of 256 threads per seed.
//
// The discipline of qocx_optim.hip holds: every product and sum is rounded on its own (no contraction
// into fused multiply-adds), division and square root are the IEEE ones. Every inner product runs in
// the one order lbfgs.py's dot() defines - thread l accumulates the elements l, l + 256, l + 512, ...
// in increasing index as acc = acc + a[i] * b[i], then the 256 partial sums are folded by the tree
// partial[l] += partial[l + stride], stride = 128 .. 1 - so a seed walks the host loop's trajectory
// bit for bit, whatever the batch it is part of.
//
// Thread l owns the elements l, l + 256, ... (in the host's element order) of every vector of its seed:
// it alone reads and writes them, in the elementwise passes and in the products of a reduction alike,
// so the vectors need no synchronisation in HBM; the threads meet only in the LDS tree. The pairs
// (s, y) are a ring in HBM walked by age, the two-loop recursion's coefficients live in LDS. Every
// branch below is taken on a reduced value or a scalar of the seed, hence by all threads of the
// workgroup together.
//
// Cost: a step with m pairs stored is up to 2 m + 6 reductions over P elements and reads about
// 4 m + 8 vectors of P doubles - a few hundred KB per seed at the headline size (P = 4000, m = 10),
// beside an evaluation of milliseconds. It is written to be deterministic and independent of B, not to
// be fast.
#include "qocx_device.h"

namespace qocx {

#pragma clang fp contract(off)

namespace {

constexpr int LANES = 256;

// where element i of the host's parameter vector lives in the seed's device arrays
struct Layout {
    size_t per_seed, half;
    int interleaved;
    __device__ size_t at(size_t i) const {
        if (!interleaved) return i;
        return i < half ? 2 * i : 2 * (i - half) + 1;
    }
};

// f(e) for every element this thread owns; e is where the element lives
template <class F>
__device__ void each_own(const Layout& lay, F f) {
    for (size_t i = threadIdx.x; i < lay.per_seed; i += LANES) f(lay.at(i));
}

// sum_i term(e_i) in the defined order, the same value in every thread; e_i is where element i lives.
// partial: LANES doubles of LDS
template <class Term>
__device__ double block_sum(const Layout& lay, double* partial, Term term) {
    const int l = threadIdx.x;
    double acc = 0.0;
    for (size_t i = l; i < lay.per_seed; i += LANES) {
        const double prod = term(lay.at(i));
        acc = acc + prod;
    }
    partial[l] = acc;
    __syncthreads();
    for (int stride = LANES / 2; stride > 0; stride >>= 1) {
        if (l < stride) partial[l] = partial[l] + partial[l + stride];
        __syncthreads();
    }
    const double total = partial[0];
    __syncthreads();  // (partial is free for the next reduction)
    return total;
}

__device__ double block_dot(const double* a, const double* b, const Layout& lay, double* partial) {
    return block_sum(lay, partial, [=](size_t e) { return a[e] * b[e]; });
}

// (a - c) . (b - e): the products of the differences, each difference rounded first
__device__ double block_dot_diffs(const double* a, const double* c, const double* b, const double* e,
                                  const Layout& lay, double* partial) {
    return block_sum(lay, partial, [=](size_t i) {
        const double u = a[i] - c[i];
        const double v = b[i] - e[i];
        return u * v;
    });
}

}  // namespace

__global__ __launch_bounds__(256) void lbfgs_step_kernel(LbfgsArgs a) {
    __shared__ double partial[LANES];
    __shared__ double alpha[LBFGS_MAX_HISTORY];
    const size_t b = blockIdx.x;
    const int l = threadIdx.x;
    LbfgsSeed sd = a.seed[b];
    __syncthreads();  // (thread 0 stores the scalars back at the end: every thread has read them)
    if (!a.update[b]) {
        if (l == 0) a.finished[b] = (unsigned char)sd.finished;
        return;
    }
    const Layout lay{a.per_seed, a.per_seed / 2, a.interleaved};
    const size_t P = a.per_seed, H = (size_t)a.history;
    double* p = a.params + b * P;
    const double* gp = a.grads + b * P;
    double* x = a.x + b * P;
    double* g = a.g + b * P;
    double* d = a.d + b * P;
    double* ring_s = a.s + b * H * P;
    double* ring_y = a.y + b * H * P;
    double* rho = a.rho + b * H;
    const double fp = a.cost[b];

    bool restart = false;
    if (sd.finished) {  // frozen at its last accepted point
        each_own(lay, [=](size_t e) { p[e] = x[e]; });
        if (l == 0) a.finished[b] = 1;
        return;
    }
    if (!sd.started) {  // the first evaluation of a seed is accepted unconditionally
        each_own(lay, [=](size_t e) {
            x[e] = p[e];
            g[e] = gp[e];
        });
        sd.f = fp;
        sd.started = 1;
        restart = true;
    } else {
        // Armijo on the step p - x (for real controls p is the clipped trial point)
        const double gs = block_sum(lay, partial, [=](size_t e) {
            const double step = p[e] - x[e];
            return g[e] * step;
        });
        const double slope = a.armijo * gs;
        const double bound = sd.f + slope;
        if (!(fp <= bound)) {  // rejected (a NaN error rejects): backtrack
            sd.bt += 1;
            sd.t = sd.t * a.shrink;
            if (sd.bt > a.max_backtracks) {
                if (sd.steepest) {  // steepest descent out of backtracks: the seed is finished
                    sd.finished = 1;
                    each_own(lay, [=](size_t e) { p[e] = x[e]; });
                    if (l == 0) {
                        a.seed[b] = sd;
                        a.finished[b] = 1;
                    }
                    return;
                }
                restart = true;
            }
        } else {
            // accepted: the pair (s, y) = (p - x, grads - g)
            const double sy = block_dot_diffs(p, x, gp, g, lay, partial);
            const double ss = block_dot_diffs(p, x, p, x, lay, partial);
            const double yy = block_dot_diffs(gp, g, gp, g, lay, partial);
            const double floor_ss = 1e-20 * ss;
            if (sy > 0 && sy * sy > floor_ss * yy) {  // curvature safely positive: the pair is kept,
                // in the slot after the newest - that of the oldest pair once the ring is full
                const int slot = sd.count < a.history ? (sd.head + sd.count) % a.history : sd.head;
                double* sn = ring_s + (size_t)slot * P;
                double* yn = ring_y + (size_t)slot * P;
                each_own(lay, [=](size_t e) {
                    sn[e] = p[e] - x[e];
                    yn[e] = gp[e] - g[e];
                });
                if (sd.count < a.history) {
                    sd.count += 1;
                } else {
                    sd.head = (sd.head + 1) % a.history;  // (it took the oldest pair's slot)
                }
                if (l == 0) rho[slot] = 1.0 / sy;
                sd.gamma = sy / yy;
            }
            each_own(lay, [=](size_t e) {
                x[e] = p[e];
                g[e] = gp[e];
            });
            sd.f = fp;
            if (sd.count == 0) {
                restart = true;
            } else {
                // d = -H g by the two-loop recursion; q lives in d
                each_own(lay, [=](size_t e) { d[e] = g[e]; });
                for (int age = 0; age < sd.count; ++age) {  // newest to oldest
                    const int k = (sd.head + sd.count - 1 - age) % a.history;
                    const double sq = block_dot(ring_s + (size_t)k * P, d, lay, partial);
                    // (rho[slot] was written by thread 0 before the barriers of the reductions above)
                    const double al = rho[k] * sq;
                    if (l == 0) alpha[k] = al;
                    const double* yk = ring_y + (size_t)k * P;
                    each_own(lay, [=](size_t e) {
                        const double t = al * yk[e];
                        d[e] = d[e] - t;
                    });
                }
                const double gamma = sd.gamma;
                each_own(lay, [=](size_t e) { d[e] = d[e] * gamma; });
                __syncthreads();  // alpha[] of thread 0 is visible
                for (int age = sd.count - 1; age >= 0; --age) {  // oldest to newest
                    const int k = (sd.head + sd.count - 1 - age) % a.history;
                    const double yq = block_dot(ring_y + (size_t)k * P, d, lay, partial);
                    const double beta = rho[k] * yq;
                    const double c = alpha[k] - beta;
                    const double* sk = ring_s + (size_t)k * P;
                    each_own(lay, [=](size_t e) {
                        const double t = c * sk[e];
                        d[e] = d[e] + t;
                    });
                }
                each_own(lay, [=](size_t e) { d[e] = -d[e]; });
                sd.t = 1.0;
                sd.bt = 0;
                sd.steepest = 0;
                const double gd = block_dot(g, d, lay, partial);
                if (!(gd < 0)) restart = true;  // not a descent direction
            }
        }
    }
    if (restart) {  // drop the pairs, steepest descent with the step first_step / |g|
        sd.head = 0;
        sd.count = 0;
        sd.steepest = 1;
        sd.bt = 0;
        each_own(lay, [=](size_t e) { d[e] = -g[e]; });
        const double gg = block_dot(g, g, lay, partial);
        sd.t = gg != 0 ? a.first_step / sqrt(gg) : 0.0;
    }
    // the next trial point
    const double step = sd.t;
    each_own(lay, [=](size_t e) {
        const double t = step * d[e];
        p[e] = x[e] + t;
    });
    if (l == 0) {
        a.seed[b] = sd;
        a.finished[b] = 0;
    }
}

void launch_lbfgs_step(const LbfgsArgs& a, int batch, hipStream_t st) {
    if (batch <= 0) return;
    hipLaunchKernelGGL(lbfgs_step_kernel, dim3((unsigned)batch), dim3(LANES), 0, st, a);
}

}  // namespace qocx
