// qocx_lindblad4t_body.inc - the body of lindblad4t_kernel<HERM> (qocx_lindblad4t.hip) and of
// lindblad4t_rates_kernel<HERM> (qocx_lindblad4t_rates.hip), included inside both; `a` is the kernel's
// LindbladArgs, the names are those of qocx_lindblad4t_core.h. Text, not a function: with the body in an
// inlined __device__ function the compiler loads the argument block's fields up front instead of where
// they are used and allocates registers differently (117 -> 149 spilled scalar registers, non-Hermitian
// build), and runs without per-member rates must execute what they executed before.
    extern __shared__ __attribute__((aligned(16))) char smem[];
    Ctx cx{a, make_wave<G>(smem, false), reinterpret_cast<double2*>(smem + RED_OFF), 0};
    const W& wv = cx.wv;
    const int S = a.S, K = a.K, nsub = a.nsub, nops = a.nops;
    const int b = blockIdx.x;
    // Two-sided evaluation (LindbladArgs::phase; one final TargetDensityInfidelity): phase 1 is the
    // forward pass alone and leaves the scalars of the final cotangents, phase 2 the adjoint of the
    // TARGETS - beside it, on other CUs - which stores its stage cotangents kbar_i instead of
    // contracting them; lindblad4t_combine_kernel does that afterwards over the whole chip.
    const int phase = a.phase;
    double2* dens = a.scratch + (size_t)b * (2 * S + 3 * STAGES) * MAT;
    double2* lam = dens + (size_t)S * MAT;
    // k_j / Ybar_j: [STAGES] dumps, a set of its own for the pass that runs beside the forward
    double2* kdump = lam + (size_t)S * MAT + (phase == 2 ? (size_t)STAGES * MAT : 0);
    // stage values recomputed from a checkpoint when the batch's did not fit into HBM (ystages == nullptr)
    double2* ysdump = lam + (size_t)S * MAT + 2 * (size_t)STAGES * MAT;
    double2* ckpt_b = a.checkpoints + (size_t)b * nsub * S * MAT;
    const double* ctl = a.controls + (size_t)b * a.nc * K;

    for (int i = 0; i < nops; ++i) wv.store(cx.load_dump(a.op_cimg + (size_t)i * MAT), M_OP0 + i);
    if (phase != 2)
        for (int s = 0; s < S; ++s) cx.store_dump(cx.load_dump(a.rho0_cimg + (size_t)s * MAT), dens + (size_t)s * MAT);
    __syncthreads();

    // ---- forward ----------------------------------------------------------------------------------
    // (a wave reads back from `dens`, `lam`, `ckpt` only the tile it wrote itself: no fences needed)
    // the twelve stages of sub-interval q on y0 (in: the density at its start, out: at its end); the
    // stage values go to `ys` if that is not null
    auto forward_stages = [&](const SubStep& ss, const Ctx::Gen& g, int q, T& y0, double2* ys) {
        const double h = ss.h;
        T klast = tile_zero<G>();
#pragma unroll 1
        for (int i = 0; i < STAGES; ++i) {
            T y = y0;
#pragma unroll 1
            for (int j = 0; j + 1 < i; ++j) {
                const double aij = RK.a[i * STAGES + j];
                if (aij != 0.0) tile_axpy<G>(y, h * aij, cx.load_dump(kdump + (size_t)j * MAT));
            }
            if (i > 0) tile_axpy<G>(y, h * RK.a[i * STAGES + i - 1], klast);
            if (ys != nullptr) cx.store_dump(y, ys + (size_t)i * MAT);
            klast = cx.template rhs<false, HERM>(y, g, RK.c[i], ss, ctl, (size_t)q * STAGES + i);
            cx.store_dump(klast, kdump + (size_t)i * MAT);
        }
#pragma unroll 1
        for (int i = 0; i < STAGES; ++i) {
            const double bi = RK.b[i];
            if (bi != 0.0) tile_axpy<G>(y0, h * bi, cx.load_dump(kdump + (size_t)i * MAT));
        }
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
    for (int q = 0; q < (phase == 2 ? 0 : nsub); ++q) {
        const SubStep ss = a.substeps[q];
        if (ss.first_of_step) {
            if (a.has_step_costs && ss.step != 0 && (ss.step % a.cost_eval_step) == 0)
                cost += cx.costs(true, false, dens, nullptr);
            if (a.step_densities != nullptr)
                for (int s = 0; s < S; ++s)
                    cx.store_dump(cx.load_dump(dens + (size_t)s * MAT),
                                  a.step_densities + (((size_t)b * (a.nsteps + 1) + ss.step) * S + s) * MAT);
        }
        const Ctx::Gen g = cx.generators(ss, ctl, false);
        for (int s = 0; s < S; ++s) {
            T y0 = cx.load_dump(dens + (size_t)s * MAT);
            cx.store_dump(y0, ckpt_b + ((size_t)q * S + s) * MAT);
            double2* ys = a.ystages != nullptr ? a.ystages + ((((size_t)b * nsub + q) * S + s) * STAGES) * MAT : nullptr;
            forward_stages(ss, g, q, y0, ys);
            cx.store_dump(y0, dens + (size_t)s * MAT);
        }
    }
    if (phase != 2) {
        if (a.has_step_costs && (a.nsteps % a.cost_eval_step) == 0) cost += cx.costs(true, false, dens, nullptr);
        cost += cx.costs(false, true, dens, nullptr);
        if (wv.tid == 0) a.cost_out[b] = cost;
        for (int s = 0; s < S; ++s) {
            const T rho = cx.load_dump(dens + (size_t)s * MAT);
            cx.store_dump(rho, a.final_out + ((size_t)b * S + s) * MAT);
            if (a.step_densities != nullptr)
                cx.store_dump(rho, a.step_densities + (((size_t)b * (a.nsteps + 1) + a.nsteps) * S + s) * MAT);
            if (phase == 1) {
                // cotangent of final density s = (f zr + i f zi) T_s, f = -scale / (S n |z|), z = tr(T_s^H rho_s)
                // (costs()): the scalars the combine kernel applies
                const DevCost c = a.costs[0];
                double zr, zi;
                Ctx::frob_part(cx.load_dump(a.cost_matrices + ((size_t)c.vec_offset + s) * MAT), rho, zr, zi);
                cx.block_sum(zr, zi);
                const double mag = sqrt(zr * zr + zi * zi);
                const double f = mag > 0 ? -c.scale / ((double)S * a.n * mag) : 0.0;
                if (wv.tid == 0) a.lam_scale[(size_t)b * S + s] = make_double2(f * zr, f * zi);
            }
        }
    }
    if (!a.want_grad || phase == 1) return;

    // ---- discrete adjoint -------------------------------------------------------------------------
    __syncthreads();  // (the forward's last products are done with the slots)
    if (phase == 2) {  // lambda_s = the target of density s
        for (int s = 0; s < S; ++s)
            cx.store_dump(cx.load_dump(a.cost_matrices + ((size_t)a.costs[0].vec_offset + s) * MAT), lam + (size_t)s * MAT);
    } else {
        for (int s = 0; s < S; ++s) cx.store_dump(tile_zero<G>(), lam + (size_t)s * MAT);
        (void)cx.costs((a.nsteps % a.cost_eval_step) == 0, true, dens, lam);
        inject(a.nsteps);
    }
    for (int q = nsub - 1; q >= 0; --q) {
        const SubStep ss = a.substeps[q];
        const Ctx::Gen g = cx.generators(ss, ctl, true);
        // control cotangents at the two ends of the sub-interval: per-lane partial sums
        double ga[QOCX_LINDBLAD_MAX_K], gb[QOCX_LINDBLAD_MAX_K];
#pragma unroll
        for (int k = 0; k < QOCX_LINDBLAD_MAX_K; ++k) {
            ga[k] = 0;
            gb[k] = 0;
        }
        for (int s = 0; s < S; ++s) {
            const size_t stage0 = ((((size_t)b * nsub + q) * S + s) * STAGES) * MAT;
            const double2* ys = a.ystages + stage0;
            if (a.ystages == nullptr) {  // the stage values again, from the checkpoint
                const Ctx::Gen gf = cx.generators(ss, ctl, false);
                T y0 = cx.load_dump(ckpt_b + ((size_t)q * S + s) * MAT);
                forward_stages(ss, gf, q, y0, ysdump);
                ys = ysdump;
                __syncthreads();  // (the forward's last products are done with the slots)
            }
            const T lambda = cx.load_dump(lam + (size_t)s * MAT);
            T lambda_new = lambda;
            const double h = ss.h;
            T yblast = tile_zero<G>();
#pragma unroll 1
            for (int i = STAGES - 1; i >= 0; --i) {
                // kbar_i = h (b_i lambda + sum_{j > i} a_ji Ybar_j)
                const double ci = RK.c[i];
                T kb = lambda;
                tile_scale<G>(kb, h * RK.b[i]);
#pragma unroll 1
                for (int j = i + 2; j < STAGES; ++j) {
                    const double aji = RK.a[j * STAGES + i];
                    if (aji != 0.0) tile_axpy<G>(kb, h * aji, cx.load_dump(kdump + (size_t)j * MAT));
                }
                if (i + 1 < STAGES) tile_axpy<G>(kb, h * RK.a[(i + 1) * STAGES + i], yblast);
                if (phase == 2) cx.store_dump(kb, a.kbstages + stage0 + (size_t)i * MAT);
                else wv.store(cx.load_dump(ys + (size_t)i * MAT), M_YS);
                yblast = cx.template rhs<true, HERM>(kb, g, ci, ss, ctl, (size_t)q * STAGES + i);
                cx.store_dump(yblast, kdump + (size_t)i * MAT);
                tile_axpy<G>(lambda_new, 1.0, yblast);
                if (phase == 2) {
                    __syncthreads();  // M_ARG free for the next stage
                    continue;
                }
                // control cotangent of this stage: Re <kbar, Gp_k Y - Y Gp_k> = Re tr(Z Gp_k),
                // Z = Y kbar^H - kbar^H Y (kbar is still in M_ARG, Y_i in M_YS since before rhs's barriers).
                // HERM: Z = W - W^H with W = Y kbar, and Re tr(W^H Gp_k) = -Re tr(W Gp_k) as Gp_k^H = -Gp_k
                T z = tile_zero<G>();
                if (HERM) {
                    wv.template mm<false, false>(z, M_YS, M_ARG, 2.0);
                } else {
                    wv.template mm<false, true>(z, M_YS, M_ARG, 1.0);
                    wv.template mm<true, false>(z, M_ARG, M_YS, -1.0);
                }
#pragma unroll
                for (int k = 0; k < QOCX_LINDBLAD_MAX_K; ++k)
                    if (k < K) {
                        const T gt = (!HERM && a.gp_tab != nullptr)
                                         ? cx.load_dump(a.gp_tab + ((((size_t)q * STAGES + i) * K + k) * 3 + 2) * MAT)
                                         : cx.load_dump(a.gpt_cimg + (size_t)k * MAT);
                        double pr = 0;
#pragma unroll
                        for (int r = 0; r < 4; ++r) pr += z.re[0][r] * gt.re[0][r] - z.im[0][r] * gt.im[0][r];
                        ga[k] += (1.0 - ci) * pr;
                        gb[k] += ci * pr;
                    }
                __syncthreads();  // M_ARG, M_YS free for the next stage
            }
            cx.store_dump(lambda_new, lam + (size_t)s * MAT);
        }
        if (phase == 2) continue;
#pragma unroll
        for (int k = 0; k < QOCX_LINDBLAD_MAX_K; ++k)
            if (k < K) {
                double x = ga[k], y = gb[k];
                cx.block_sum(x, y);
                if (wv.tid == 0) {
                    a.gsub[(((size_t)b * nsub + q) * 2 + 0) * K + k] = x;
                    a.gsub[(((size_t)b * nsub + q) * 2 + 1) * K + k] = y;
                }
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
