// qocx_lindblad16t.hip - the Lindblad engine at 33 <= n <= 64 (knob lindblad_wide): the density tile-wise on
// sixteen waves.
//
// Replaces (reference): _evaluate_lindblad_discrete (qoc/core/lindbladdiscrete.py:357-441) with its
// right-hand side _get_rhs_lindbladian (:444-495) / get_lindbladian (qoc/core/mathmethods.py:169-206) and
// integrate_rkdp5 (mathmethods.py:352-480 - here the fixed-step DOP853 on sub-intervals the host sizes);
// the gradient autograd takes through them is the discrete adjoint of the scheme.
// Density costs: targetdensityinfidelity.py:41-69, forbiddensities.py:53-85.
//
// Geometry: one workgroup = one seed = sixteen waves (1024 threads, four waves per SIMD, 128 registers
// each); wave w owns tile (w & 3, w >> 2) of every 64 x 64 matrix - of the density, of the stage value,
// of every stage derivative k_j, of the cotangents - exactly as the four waves of qocx_lindblad4t.hip own
// the tiles of a 32 x 32 one. What differs is where the operands of a product live. A 64 x 64 complex
// matrix at pitch 65 is 66 560 B: TWO fit the LDS, the stage argument Y and one temporary
// t_i = gamma_i L_i Y. The generators and the operators are read from memory as MFMA fragments
// (qocx_lindblad16t_core.h: a fragment is one coalesced KiB of a C-dump): the operators from the problem's
// dumps - all seeds share them, they stay in L2, and since nothing of them is held in LDS the engine's
// eight are taken -, the generators at the stage's time as LA + c LD from six images the workgroup forms
// once per sub-interval in the seed's scratch. A stage
//     k = A_L(c) Y + Y A_R(c) + sum_i gamma_i L_i Y L_i^H        (adjoint: A^H, L_i^H . L_i)
// is the general one for Hermitian and non-Hermitian H0 alike. No partial sums are exchanged - every
// wave computes ITS tile of every product - and the Runge-Kutta combinations are tile arithmetic on dumps
// in the seed's scratch of which a wave reads back only the tile it wrote. Nothing but the tile at hand
// is carried in registers across a product: no scratch memory, no spilled vector registers (127 of 128);
// the stage loops stay rolled (see qocx_lindblad4t.hip for what unrolling them costs).
// Waves whose tile is padding only (n <= 48: seven of sixteen) skip their products; the k-loops stop at
// ceil(n / 16) tiles of four k-steps. The pad rows and columns of every image are zero and stay zero
// through every product.
// Measured (profiles/lindblad_wide.jsonl; 64 seeds x 200 steps, L = 2, K = 2, forward + gradient): n = 40
// 495 ms, n = 48 661 ms, n = 64 1.55 s - 0.83 / 0.83 / 1.29 ms per sub-interval of a seed.
// The classic launch only (LindbladArgs::phase == 0), constant tables only: the host decides neither
// two-sided evaluation nor stage tables above n = 32.
#include "qocx_lindblad16t_core.h"

namespace qocx {

namespace lindblad16t {

__global__ __launch_bounds__(1024) void lindblad16t_kernel(LindbladArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    Ctx cx{a, make_wave<G>(smem, false), reinterpret_cast<double2*>(smem + RED_OFF),
           reinterpret_cast<double*>(smem + GRED_OFF), 0, 0, 0, 0, 0, false};
    const W& wv = cx.wv;
    cx.kt = (a.n + 15) >> 4;
    cx.dump_off = (unsigned)wv.cimg(0, 0) * 16;
    cx.fa_off = (unsigned)(wv.ti(0) * 256 + wv.lane) * 16;
    cx.fb_off = (unsigned)(wv.tj() * 256 + wv.lane) * 16;
    cx.live = 16 * wv.ti(0) < a.n && 16 * wv.tj() < a.n;
    const int S = a.S, K = a.K, nsub = a.nsub;
    const int b = blockIdx.x;
    double2* dens = a.scratch + (size_t)b * (2 * S + SCRATCH_EXTRA) * MAT;
    double2* lam = dens + (size_t)S * MAT;
    double2* kdump = lam + (size_t)S * MAT;          // k_j / Ybar_j
    double2* ysdump = kdump + (size_t)STAGES * MAT;  // stage values recomputed from a checkpoint
    double2* gen = ysdump + (size_t)STAGES * MAT;    // the generator images of the sub-interval at hand
    double2* lamnew = gen + (size_t)GEN_COUNT * MAT;
    double2* ckpt_b = a.checkpoints + (size_t)b * nsub * S * MAT;
    const double* ctl = a.controls + (size_t)b * a.nc * K;

    for (int s = 0; s < S; ++s) cx.store_dump(cx.load_dump(a.rho0_cimg + (size_t)s * MAT), dens + (size_t)s * MAT);

    // ---- forward ----------------------------------------------------------------------------------
    // (a wave reads back from `dens`, `lam`, `kdump`, `ckpt` only the tile it wrote itself: no fences needed)
    // the twelve stages of a sub-interval of step h on the density dump `src`; the density at its end goes
    // to `dst` and the stage values to `ys`, each if not null
    auto forward_stages = [&](double h, const double2* src, double2* dst, double2* ys) {
#pragma unroll 1
        for (int i = 0; i < STAGES; ++i) {
            T y = cx.load_dump(src);
#pragma unroll 1
            for (int j = 0; j < i; ++j) {
                const double aij = RK.a[i * STAGES + j];
                if (aij != 0.0) tile_axpy<G>(y, h * aij, cx.load_dump(kdump + (size_t)j * MAT));
            }
            if (ys != nullptr) cx.store_dump(y, ys + (size_t)i * MAT);
            const T k = cx.template rhs<false>(y, gen, RK.c[i]);
            cx.store_dump(k, kdump + (size_t)i * MAT);
        }
        if (dst == nullptr) return;
        T y = cx.load_dump(src);
#pragma unroll 1
        for (int i = 0; i < STAGES; ++i) {
            const double bi = RK.b[i];
            if (bi != 0.0) tile_axpy<G>(y, h * bi, cx.load_dump(kdump + (size_t)i * MAT));
        }
        cx.store_dump(y, dst);
    };
    // lambda += host-supplied cotangent of the densities at system step `step`, if there is one
    auto inject = [&](int step) {
        if (a.inj_index == nullptr) return;
        const int row = a.inj_index[step];
        if (row < 0) return;
        for (int s = 0; s < S; ++s) {
            T l = cx.load_dump(lam + (size_t)s * MAT);
            tile_axpy<G>(l, 1.0, cx.load_dump(a.inj_bars + (((size_t)b * a.inj_count + row) * S + s) * MAT));
            cx.store_dump(l, lam + (size_t)s * MAT);
        }
    };
    double cost = 0;
    for (int q = 0; q < nsub; ++q) {
        const SubStep ss = a.substeps[q];
        if (ss.first_of_step) {
            if (a.has_step_costs && ss.step != 0 && (ss.step % a.cost_eval_step) == 0)
                cost += cx.costs(true, false, dens, nullptr);
            if (a.step_densities != nullptr)
                for (int s = 0; s < S; ++s)
                    cx.store_dump(cx.load_dump(dens + (size_t)s * MAT),
                                  a.step_densities + (((size_t)b * (a.nsteps + 1) + ss.step) * S + s) * MAT);
        }
        cx.form_generators(ss, ctl, gen);
        for (int s = 0; s < S; ++s) {
            double2* rho = dens + (size_t)s * MAT;
            cx.store_dump(cx.load_dump(rho), ckpt_b + ((size_t)q * S + s) * MAT);
            double2* ys = a.ystages != nullptr ? a.ystages + ((((size_t)b * nsub + q) * S + s) * STAGES) * MAT : nullptr;
            forward_stages(ss.h, rho, rho, ys);
        }
    }
    if (a.has_step_costs && (a.nsteps % a.cost_eval_step) == 0) cost += cx.costs(true, false, dens, nullptr);
    cost += cx.costs(false, true, dens, nullptr);
    if (wv.tid == 0) a.cost_out[b] = cost;
    for (int s = 0; s < S; ++s) {
        const T rho = cx.load_dump(dens + (size_t)s * MAT);
        cx.store_dump(rho, a.final_out + ((size_t)b * S + s) * MAT);
        if (a.step_densities != nullptr)
            cx.store_dump(rho, a.step_densities + (((size_t)b * (a.nsteps + 1) + a.nsteps) * S + s) * MAT);
    }
    if (!a.want_grad) return;

    // ---- discrete adjoint -------------------------------------------------------------------------
    for (int s = 0; s < S; ++s) cx.store_dump(tile_zero<G>(), lam + (size_t)s * MAT);
    (void)cx.costs((a.nsteps % a.cost_eval_step) == 0, true, dens, lam);
    inject(a.nsteps);
    for (int q = nsub - 1; q >= 0; --q) {
        const SubStep ss = a.substeps[q];
        const double h = ss.h;
        cx.form_generators(ss, ctl, gen);
        // control cotangents at the two ends of the sub-interval: lane k of every wave carries the wave's
        // partial sums of control k
        double ga = 0, gb = 0;
        for (int s = 0; s < S; ++s) {
            const double2* ys = a.ystages + ((((size_t)b * nsub + q) * S + s) * STAGES) * MAT;
            if (a.ystages == nullptr) {  // the stage values again, from the checkpoint
                forward_stages(h, ckpt_b + ((size_t)q * S + s) * MAT, nullptr, ysdump);
                ys = ysdump;
            }
            double2* lambda = lam + (size_t)s * MAT;
#pragma unroll 1
            for (int i = STAGES - 1; i >= 0; --i) {
                // kbar_i = h (b_i lambda + sum_{j > i} a_ji Ybar_j)
                const double ci = RK.c[i];
                T kb = cx.load_dump(lambda);
                tile_scale<G>(kb, h * RK.b[i]);
#pragma unroll 1
                for (int j = i + 1; j < STAGES; ++j) {
                    const double aji = RK.a[j * STAGES + i];
                    if (aji != 0.0) tile_axpy<G>(kb, h * aji, cx.load_dump(kdump + (size_t)j * MAT));
                }
                {
                    const T yb = cx.template rhs<true>(kb, gen, ci);
                    cx.store_dump(yb, kdump + (size_t)i * MAT);
                    T ln = cx.load_dump(i == STAGES - 1 ? lambda : lamnew);
                    tile_axpy<G>(ln, 1.0, yb);
                    cx.store_dump(ln, lamnew);
                }
                if (K == 0) continue;
                // control cotangent of this stage: Re <kbar, Gp_k Y - Y Gp_k> = Re tr(Z Gp_k),
                // Z = Y kbar^H - kbar^H Y (kbar is still in M_ARG; Y_i takes the place of the last t_i)
                __syncthreads();  // t_i has been read
                wv.store(cx.load_dump(ys + (size_t)i * MAT), M_T);
                __syncthreads();
                if (!cx.live) continue;  // Z's tile is zero
                T z = tile_zero<G>();
                const double2* ym = wv.mat(M_T);
                const double2* km = wv.mat(M_ARG);
                cx.mm(z, 1.0, [&](int k4, int u) { return cx.lds_a(ym, k4, u); },
                      [&](int k4, int u) { return cx.lds_bh(km, k4, u); });
                cx.mm(z, -1.0, [&](int k4, int u) { return cx.lds_ah(km, k4, u); },
                      [&](int k4, int u) { return cx.lds_b(ym, k4, u); });
#pragma unroll 1
                for (int k = 0; k < K; ++k) {
                    const T gt = cx.load_dump(a.gpt_cimg + (size_t)k * MAT);
                    double pr = 0;
#pragma unroll
                    for (int r = 0; r < 4; ++r) pr += z.re[0][r] * gt.re[0][r] - z.im[0][r] * gt.im[0][r];
                    pr = wave_sum(pr);
                    if (wv.lane == k) {
                        ga += (1.0 - ci) * pr;
                        gb += ci * pr;
                    }
                }
            }
            cx.store_dump(cx.load_dump(lamnew), lambda);
        }
        if (K > 0) {
            // the sixteen waves' partial sums in one fixed order
            if (wv.lane < QOCX_LINDBLAD_MAX_K) {
                cx.gred[(wv.w * 2 + 0) * QOCX_LINDBLAD_MAX_K + wv.lane] = ga;
                cx.gred[(wv.w * 2 + 1) * QOCX_LINDBLAD_MAX_K + wv.lane] = gb;
            }
            __syncthreads();
            if (wv.tid < 2 * QOCX_LINDBLAD_MAX_K && (wv.tid & (QOCX_LINDBLAD_MAX_K - 1)) < K) {
                double sum = 0;
#pragma unroll
                for (int w = 0; w < G::WAVES; ++w) sum += cx.gred[w * 2 * QOCX_LINDBLAD_MAX_K + wv.tid];
                a.gsub[(((size_t)b * nsub + q) * 2 + (wv.tid >> 3)) * K + (wv.tid & (QOCX_LINDBLAD_MAX_K - 1))] = sum;
            }
            // (the next sub-interval's form_generators has the barrier that frees the partial sums)
        }
        // step costs are evaluated on the densities at the START of their system step
        if (ss.first_of_step && ss.step != 0) {
            if ((ss.step % a.cost_eval_step) == 0 && a.has_step_costs) {
                for (int s = 0; s < S; ++s)
                    cx.store_dump(cx.load_dump(ckpt_b + ((size_t)q * S + s) * MAT), dens + (size_t)s * MAT);
                (void)cx.costs(true, false, dens, lam);
            }
            inject(ss.step);
        }
    }
}

}  // namespace lindblad16t

int lindblad16t_lds_bytes() { return lindblad16t::LDS_BYTES; }

size_t lindblad16t_scratch_elems(int S) { return (size_t)(2 * S + lindblad16t::SCRATCH_EXTRA) * lindblad16t::MAT; }

void launch_lindblad16t(const LindbladArgs& a, int batch, hipStream_t st) {
    static bool attr_set = false;
    if (!attr_set) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(lindblad16t::lindblad16t_kernel),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, lindblad16t::LDS_BYTES);
        attr_set = true;
    }
    hipLaunchKernelGGL(lindblad16t::lindblad16t_kernel, dim3(batch), dim3(1024), lindblad16t::LDS_BYTES, st, a);
}

}  // namespace qocx
