// qocx_action_costs.hip - the matrix-free route of qocx_action.hip under ANY set of device state-cost
// descriptors (knob "action_costs"): one state per seed, Hermitian H, 17 <= n <= 32, costs of the kinds
// COHERENT, INCOHERENT and FORBID, final or step, one or several. The step is that of
// action_sweep_kernel - the generator built in registers, the DPP matrix-vector product, the Taylor
// terms kept for the gradient kernel - but the adjoint sweep carries the TRUE cotangent instead of the
// back-propagated target (the "general adjoint" of the Pade sweeps):
//
//   forward   at every system step j != 0 with j % cost_eval_step == 0 the step costs are evaluated on
//             psi_j before the step leaves it, at the end first the step costs (if the final step is a
//             cost step), then the final costs - the order of sweep1_kernel and of the reference
//   adjoint   lambda_N = the cotangent of the costs evaluated on the final state; per step
//             lambda <- T_m(a)^H lambda (w_0 .. w_(m-1) kept), then, if the step is a cost step, the
//             cotangent of its step costs at psi_j = v_0 of step j (read back from the forward terms)
//   gradient  abar = sum_i w_i rho_i^H as action_grad_kernel forms it; lambda is the true cotangent, so
//             the step gradient is the real number Re sum conj(abar) (.) (-i dt G_k): one double per
//             (step, k), the layout K3 leaves without the unit adjoint, and the scatter kernel applies
//             no scalar
//
// The forward sweep runs first and the adjoint sweep behind it (the one-sided schedule): the cotangent
// needs the forward states. A step's arithmetic depends on nothing but its inputs and every sum has a
// fixed order, so results are bit identical however the steps are cut into launches, and a forward-only
// evaluation returns the costs of the evaluation with gradient.
//
// (The step body is restated here rather than shared with action_sweep_kernel: that kernel's code
// object stays what it was.)
#include "qocx_action_core.h"

namespace qocx {

namespace action {

template <int NB, int KR>
__global__ __launch_bounds__(64) void action_costs_sweep_kernel(ActionArgs args) {
    typedef Geo<NB> G;
    constexpr int NP = G::NP, CPL = G::CPL, H = G::H;
    // the state the cost code reads, and the cotangent it adds to
    __shared__ __attribute__((aligned(16))) double2 turn[NP];
    __shared__ __attribute__((aligned(16))) double2 lam[NP];
    const SweepArgs& sw = args.sw;
    const int b = blockIdx.x;
    const int lane = lane_id(), i = lane % NP, h = lane / NP;
    const bool g0 = (h == 0);
    const int nsteps = sw.nsteps, K = args.K, m_max = args.m_max;
    const int jb = sw.j_begin, je = sw.j_end;
    const int ces = sw.cost_eval_step;
    const bool step_costs = sw.has_step_costs != 0;
    const double dt = args.dt;
    __builtin_amdgcn_s_setprio(3);  // the serial chain of the evaluation goes first on its SIMD

    // -i dt H0 and -i dt G_k in registers, as action_sweep_kernel holds them
    static_assert(NB == 2 && CPL == 16, "one block of 16 columns per lane group");
    auto image_at = [&](int cc) { return ((16 * h + cc) / H) * 64 + ((16 * h + cc) % H) * NP + i; };
    double h0r[CPL], h0i[CPL], gr[KR][CPL], gi[KR][CPL];
#pragma unroll
    for (int cc = 0; cc < CPL; ++cc) {
        const double2 e = args.h0_rimg[image_at(cc)];
        h0r[cc] = dt * e.y;
        h0i[cc] = -dt * e.x;
    }
#pragma unroll
    for (int k = 0; k < KR; ++k)
#pragma unroll
        for (int cc = 0; cc < CPL; ++cc) {
            const double2 e = k < K ? args.g_rimg[(size_t)k * G::MAT + image_at(cc)] : make_double2(0, 0);
            gr[k][cc] = dt * e.y;
            gi[k][cc] = -dt * e.x;
        }

    const int* words = sw.s_arr + (size_t)b * nsteps;
    const double* u_b = args.ustep + (size_t)b * nsteps * K;
    double are[CPL], aim[CPL];
    auto build = [&](int step) __attribute__((always_inline)) {
        const double* u = u_b + (size_t)step * K;
#pragma unroll
        for (int cc = 0; cc < CPL; ++cc) {
            are[cc] = h0r[cc];
            aim[cc] = h0i[cc];
        }
#pragma unroll
        for (int k = 0; k < KR; ++k)
            if (k < K) {
                const double uk = u[k];
#pragma unroll
                for (int cc = 0; cc < CPL; ++cc) {
                    are[cc] = fma(uk, gr[k][cc], are[cc]);
                    aim[cc] = fma(uk, gi[k][cc], aim[cc]);
                }
            }
        for (int k = KR; k < K; ++k) {
            const double uk = u[k] * dt;
#pragma unroll
            for (int cc = 0; cc < CPL; ++cc) {
                const double2 e = args.g_rimg[(size_t)k * G::MAT + image_at(cc)];
                are[cc] = fma(uk, e.y, are[cc]);
                aim[cc] = fma(-uk, e.x, aim[cc]);
            }
        }
    };
    auto matvec = [&](double xr, double xi, double& yr, double& yi) __attribute__((always_inline)) {
        const double sxr = spread_halves(xr, h), sxi = spread_halves(xi, h);
        double s0r = 0, s0i = 0, s1r = 0, s1i = 0;
        for_each_const(
            [&](auto Q) __attribute__((always_inline)) {
                constexpr int k = 4 * decltype(Q)::value;
                dpp_cmac4<k>(s0r, s0i, s1r, s1i, sxr, sxi, are[k], aim[k], are[k + 1], aim[k + 1],
                             are[k + 2], aim[k + 2], are[k + 3], aim[k + 3]);
            },
            std::make_integer_sequence<int, 4>{});
        yr = sum_groups<NB>(s0r + s1r);
        yi = sum_groups<NB>(s0i + s1i);
    };
    // One step: (vr, vi) becomes sum_p (sign a)^p / p! v, the terms 0 .. m - 1 go to `keep`. False: the
    // degree is outside the buffers.
    double vr = 0, vi = 0;
    int count = 0;  // lane l: steps of the forward sweep at degree l
    auto step_apply = [&](int step, double sign, double2* keep_base, bool counted) __attribute__((always_inline)) {
        const int m = step_degree(words[step]);
        if (m < 1 || m > m_max) return false;
        build(step);
        double2* keep = keep_base ? keep_base + ((size_t)b * nsteps + step) * m_max * NP : nullptr;
        if (counted) count += (lane == m) ? 1 : 0;
        double sr = vr, si = vi;
        for (int p = 1; p <= m; ++p) {
            if (keep != nullptr && g0) keep[(size_t)(p - 1) * NP + i] = make_double2(vr, vi);
            double yr, yi;
            matvec(vr, vi, yr, yi);
            const double f = sign * INV_P.v[p];
            vr = f * yr;
            vi = f * yi;
            sr += vr;
            si += vi;
        }
        vr = sr;
        vi = si;
        return true;
    };
    auto refuse = [&]() {  // never clamped: the host runs the evaluation again on the Pade route
        if (lane == 0) atomicOr(sw.status, 8);
    };
    auto cost_step = [&](int step) { return step != 0 && step_costs && (step % ces) == 0; };
    // the vector in registers (every lane group holds the same value: all store) to where the cost code reads it
    auto to_turn = [&]() {
        wave_sync();
        turn[i] = make_double2(vr, vi);
        wave_sync();
    };

    // ---- forward sweep ----------------------------------------------------------------------
    if (sw.phase & 1) {
        const double2 p0 = jb == 0 ? sw.psi0[i] : args.carry_f[(size_t)b * NP + i];
        vr = p0.x;
        vi = p0.y;
        double cost = jb == 0 ? 0.0 : sw.cost_out[b];  // the partial cost of the segments before
        for (int step = jb; step < je; ++step) {
            if (cost_step(step)) {  // psi_step, before the step leaves it
                to_turn();
                cost += eval_costs<NB>(sw, true, false, turn, nullptr, h, i);
            }
            if (!step_apply(step, 1.0, args.kv_f, true)) {
                refuse();
                return;
            }
        }
        if (count > 0 && lane <= MMAX) atomicAdd(args.degree_counts + lane, count);
        if (je == nsteps) {
            to_turn();
            if (cost_step(nsteps)) cost += eval_costs<NB>(sw, true, false, turn, nullptr, h, i);
            cost += eval_costs<NB>(sw, false, true, turn, nullptr, h, i);
            if (g0) sw.final_out[(size_t)b * NP + i] = make_double2(vr, vi);
        } else if (g0) {
            args.carry_f[(size_t)b * NP + i] = make_double2(vr, vi);
        }
        if (lane == 0) sw.cost_out[b] = cost;
    }
    if (!(sw.phase & 2)) return;

    // ---- adjoint sweep: the true cotangent ------------------------------------------------------
    wave_sync();
    if (je == nsteps) {
        if (!(sw.phase & 1) && g0) turn[i] = sw.final_out[(size_t)b * NP + i];  // where the forward segments left it
        if (g0) lam[i] = make_double2(0, 0);
        wave_sync();
        // the costs of the final state: the final ones, and the step costs if the final step is a cost step
        (void)eval_costs<NB>(sw, cost_step(nsteps), true, turn, lam, h, i);
        wave_sync();
        const double2 t = lam[i];
        vr = t.x;
        vi = t.y;
    } else {
        const double2 t = sw.lam_buf[(size_t)b * NP + i];
        vr = t.x;
        vi = t.y;
    }
    for (int step = je - 1; step >= jb; --step) {
        if (!step_apply(step, -1.0, args.kv_b, false)) {
            refuse();
            return;
        }
        if (cost_step(step)) {
            // step costs were evaluated on the state before the step: term v_0 of its forward series
            wave_sync();
            if (g0) {  // (lane group 0 wrote the terms and is the one the cost code reads with)
                turn[i] = args.kv_f[((size_t)b * nsteps + step) * m_max * NP + i];
                lam[i] = make_double2(vr, vi);
            }
            wave_sync();
            (void)eval_costs<NB>(sw, true, false, turn, lam, h, i);
            wave_sync();
            const double2 t = lam[i];
            vr = t.x;
            vi = t.y;
        }
    }
    if (jb > 0 && g0) sw.lam_buf[(size_t)b * NP + i] = make_double2(vr, vi);
}

// One wave per (step, seed): action_grad_kernel's rho / rank-1 loop, and ONE real per (step, k) at the end.
// LDS: v_0 .. v_(m-1) [m_max][NP], then two slots for the current rho.
template <int NB>
__global__ __launch_bounds__(64, 3) void action_costs_grad_kernel(ActionGradArgs args) {
    typedef Geo<NB> G;
    constexpr int NP = G::NP, CPL = G::CPL, H = G::H;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double2* vl = reinterpret_cast<double2*>(smem);
    double2* rho = vl + (size_t)args.m_max * NP;
    const int step = args.step0 + blockIdx.x, b = blockIdx.y;
    const int lane = lane_id(), i = lane % NP, h = lane / NP;
    const int K = args.K;
    const size_t idx = (size_t)b * args.nsteps + step;
    const int m = step_degree(args.s_arr[idx]);
    if (m < 1 || m > args.m_max) return;  // (the sweeps have raised the status bit)
    const double2* vf = args.kv_f + idx * args.m_max * NP;
    const double2* wb = args.kv_b + idx * args.m_max * NP;
    for (int l = h; l < m; l += H) vl[l * NP + i] = vf[(size_t)l * NP + i];
    double abr[CPL], abi[CPL];
#pragma unroll
    for (int cc = 0; cc < CPL; ++cc) {
        abr[cc] = 0;
        abi[cc] = 0;
    }
    wave_sync();
    double2 tv = wb[i];
    for (int ii = 0; ii < m; ++ii) {
        // rho_ii: the lane groups share the terms, l = h, h + H, ...
        double rr = 0, ri = 0;
        for (int l = h; l < m - ii; l += H) {
            const double c = COEF.c[ii * MMAX + l];
            const double2 v = vl[l * NP + i];
            rr = fma(c, v.x, rr);
            ri = fma(c, v.y, ri);
        }
        rr = sum_groups<NB>(rr);
        ri = sum_groups<NB>(ri);
        double2* slot = rho + (ii & 1) * NP;  // two slots in turn: one sync per term
        slot[i] = make_double2(rr, ri);
        wave_sync();
        const double2 w = tv;
        if (ii + 1 < m) tv = wb[(size_t)(ii + 1) * NP + i];
#pragma unroll
        for (int cc = 0; cc < CPL; ++cc) {
            const double2 r = slot[cc * H + h];
            // w * conj(rho)
            abr[cc] = fma(w.y, r.y, fma(w.x, r.x, abr[cc]));
            abi[cc] = fma(-w.x, r.y, fma(w.y, r.x, abi[cc]));
        }
    }
    // Re sum conj(abar) E_k, E_k = -i dt G_k (krylov_grad_body without the unit adjoint)
    const double dts = args.dt;
    for (int k = 0; k < K; ++k) {
        double acc = 0;
#pragma unroll
        for (int cc = 0; cc < CPL; ++cc) {
            const double2 e = args.g_rimg[(size_t)k * G::MAT + cc * 64 + lane];
            acc = fma(abi[cc], -dts * e.x, fma(abr[cc], dts * e.y, acc));
        }
        acc = wave_sum(acc);
        if (lane == 0) args.gstep[idx * K + k] = acc;
    }
}

}  // namespace action

void launch_action_costs_sweep(const ActionArgs& a, int batch, hipStream_t st) {
    if (batch <= 0 || a.sw.j_end <= a.sw.j_begin) return;
    hipLaunchKernelGGL((action::action_costs_sweep_kernel<2, 2>), dim3(batch), dim3(64), 0, st, a);
}

void launch_action_costs_grad(const ActionGradArgs& a, int nsteps, int batch, hipStream_t st) {
    if (batch <= 0 || nsteps <= 0) return;
    hipLaunchKernelGGL((action::action_costs_grad_kernel<2>), dim3(nsteps, batch), dim3(64),
                       action_grad_lds_bytes(a.m_max), st, a);
}

}  // namespace qocx
