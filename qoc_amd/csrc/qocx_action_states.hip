// qocx_action_states.hip - the matrix-free route of qocx_action.hip for TWO TO FOUR states per seed
// (knob "action_states"), Hermitian H, 17 <= n <= 32, one coherent final TargetStateInfidelity.
//
// Under the unit adjoint the cotangent of final state s is c t_s with ONE scalar c for every state
// (qocx_sweep_common.h), and the chains of the states are independent of each other: a workgroup of S
// waves serves one (seed, direction), wave s the state s, each wave with the arithmetic of the one-state
// kernel - its own copy of -i dt H0 and of two -i dt G_k in registers, its own built a_j (sharing it
// would cost a workgroup barrier per step for K 32 multiply-adds). S <= 4 waves land one per SIMD of a
// CU, so each keeps the whole register file. The waves meet once, at the end of the forward sweep,
// where wave 0 evaluates the cost on all final states.
//
//   terms        kv_f / kv_b  [B][nsteps][S][m_max][NP]
//   gradient     abar = sum_s sum_{i<m} w_(s,i) rho_(s,i)^H in one set of registers, the states in the
//                order s = 0 .. S - 1; ONE contraction with the G_k per step; gamma_k as the one-state
//                kernel leaves it, and the scatter kernel applies c.
//
// Every wave reads the same step words, so a refusal (degree beyond the buffers) is uniform across the
// workgroup and happens before its barrier. No sum is formed atomically and the order of every sum is
// fixed: results are bit identical however the steps are cut into launches.
#include "qocx_action_core.h"

namespace qocx {

namespace action {

// KR: the G_k images held in registers beside H0 (those of further controls are read per step)
template <int NB, int KR>
__global__ __launch_bounds__(64 * QOCX_ACTION_MAX_STATES) void action_states_sweep_kernel(ActionArgs args) {
    typedef Geo<NB> G;
    constexpr int NP = G::NP, CPL = G::CPL, H = G::H;
    __shared__ __attribute__((aligned(16))) double2 turn[QOCX_ACTION_MAX_STATES * NP];  // the final states, [S][NP], for the cost code
    const SweepArgs& sw = args.sw;
    const int b = blockIdx.x;
    const int s = threadIdx.x >> 6, S = sw.S;  // (blockDim.x = 64 S)
    const int lane = lane_id(), i = lane % NP, h = lane / NP;
    const bool g0 = (h == 0), w0 = (s == 0);
    const int nsteps = sw.nsteps, K = args.K, m_max = args.m_max;
    const int jb = sw.j_begin, je = sw.j_end;
    const double dt = args.dt;
    __builtin_amdgcn_s_setprio(3);  // the serial chain of the evaluation goes first on its SIMD

    // -i dt H0 and -i dt G_k, lane (h, i): row i, columns 16 h + cc - the block its lane group multiplies
    // (qocx_action.hip)
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
    // y = a x, x in registers (every lane group holds x[i]): the lane group's 16 columns, then the sum
    // of the two lane groups of the row
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
    // One step of this wave's state: the vector (vr, vi) becomes sum_p (sign a)^p / p! v; the terms
    // 0 .. m - 1 go to `keep`. False (for every wave of the workgroup alike): the degree is outside the
    // buffers.
    double vr = 0, vi = 0;
    int count = 0;  // lane l: steps at degree l
    auto step_apply = [&](int step, double sign, double2* keep_base) __attribute__((always_inline)) {
        const int m = step_degree(words[step]);
        if (m < 1 || m > m_max) return false;
        build(step);
        double2* keep = keep_base ? keep_base + (((size_t)b * nsteps + step) * S + s) * m_max * NP : nullptr;
        count += (lane == m) ? 1 : 0;
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
        if (threadIdx.x == 0) atomicOr(sw.status, 8);
    };
    const size_t vec = ((size_t)b * S + s) * NP + i;  // this wave's entry of an [B][S][NP] buffer

    // ---- forward sweep ----------------------------------------------------------------------
    if (sw.phase & 1) {
        const double2 p0 = jb == 0 ? sw.psi0[s * NP + i] : args.carry_f[vec];
        vr = p0.x;
        vi = p0.y;
        for (int step = jb; step < je; ++step)
            if (!step_apply(step, 1.0, args.kv_f)) {
                refuse();
                return;
            }
        // (wave 0 alone: the counts stay those of (seed, step) pairs)
        if (w0 && count > 0 && lane <= MMAX) atomicAdd(args.degree_counts + lane, count);
        if (je == nsteps) {
            turn[s * NP + i] = make_double2(vr, vi);  // (every lane group holds the same value: all store)
            __syncthreads();
            if (w0) {
                const double cost = eval_costs<NB>(sw, false, true, turn, nullptr, h, i);
                if (sw.unit_adjoint && sw.want_grad) unit_adjoint_scales<NB>(sw, turn, b, h, i);
                if (lane == 0) sw.cost_out[b] = cost;
            }
            if (g0) sw.final_out[vec] = make_double2(vr, vi);
        } else if (g0) {
            args.carry_f[vec] = make_double2(vr, vi);
        }
    }
    if (!(sw.phase & 2)) return;

    // ---- adjoint sweep: the back-propagated target of this wave's state (unit adjoint) -------------
    // (lam_s = t_s as unit_adjoint_seed leaves it, read where it lies: `turn` may still be read by wave 0)
    {
        const double2* pool = sw.cost_vectors + (size_t)sw.costs[0].vec_offset * NP;
        const double2 t = je == nsteps ? pool[s * NP + i] : sw.lam_buf[vec];
        vr = t.x;
        vi = t.y;
    }
    for (int step = je - 1; step >= jb; --step)
        if (!step_apply(step, -1.0, args.kv_b)) {
            refuse();
            return;
        }
    if (jb > 0 && g0) sw.lam_buf[vec] = make_double2(vr, vi);
}

// One wave per (step, seed), the states one after the other through the same LDS: v_(s,0) .. v_(s,m-1)
// [m_max][NP], then two slots for the current rho.
template <int NB>
__global__ __launch_bounds__(64, 3) void action_states_grad_kernel(ActionStatesGradArgs sargs) {
    typedef Geo<NB> G;
    constexpr int NP = G::NP, CPL = G::CPL, H = G::H;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const ActionGradArgs& args = sargs.g;
    double2* vl = reinterpret_cast<double2*>(smem);
    double2* rho = vl + (size_t)args.m_max * NP;
    const int step = args.step0 + blockIdx.x, b = blockIdx.y;
    const int lane = lane_id(), i = lane % NP, h = lane / NP;
    const int K = args.K, S = sargs.S;
    const size_t idx = (size_t)b * args.nsteps + step;
    const int m = step_degree(args.s_arr[idx]);
    if (m < 1 || m > args.m_max) return;  // (the sweeps have raised the status bit)
    double abr[CPL], abi[CPL];
#pragma unroll
    for (int cc = 0; cc < CPL; ++cc) {
        abr[cc] = 0;
        abi[cc] = 0;
    }
    for (int s = 0; s < S; ++s) {
        const double2* vf = args.kv_f + (idx * S + s) * args.m_max * NP;
        const double2* wb = args.kv_b + (idx * S + s) * args.m_max * NP;
        if (s > 0) wave_sync();  // (the terms and rho slots of the state before have been read)
        for (int l = h; l < m; l += H) vl[l * NP + i] = vf[(size_t)l * NP + i];
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
    }
    // gamma_k = sum conj(abar) E_k, E_k = -i dt G_k, once for the sum over the states
    const double dts = args.dt;
    for (int k = 0; k < K; ++k) {
        double acc = 0, acc_im = 0;
#pragma unroll
        for (int cc = 0; cc < CPL; ++cc) {
            const double2 e = args.g_rimg[(size_t)k * G::MAT + cc * 64 + lane];
            acc = fma(abi[cc], -dts * e.x, fma(abr[cc], dts * e.y, acc));
            acc_im = fma(abi[cc], -dts * e.y, fma(abr[cc], -dts * e.x, acc_im));
        }
        acc = wave_sum(acc);
        acc_im = wave_sum(acc_im);
        if (lane == 0) {
            args.gstep[(idx * K + k) * 2] = acc;
            args.gstep[(idx * K + k) * 2 + 1] = acc_im;
        }
    }
}

}  // namespace action

void launch_action_states_sweep(const ActionArgs& a, int batch, hipStream_t st) {
    if (batch <= 0 || a.sw.j_end <= a.sw.j_begin) return;
    if (a.sw.S < 2 || a.sw.S > QOCX_ACTION_MAX_STATES) return;  // (the host's route admits 2 .. 4 only)
    hipLaunchKernelGGL((action::action_states_sweep_kernel<2, 2>), dim3(batch), dim3(64 * a.sw.S), 0, st, a);
}

void launch_action_states_grad(const ActionStatesGradArgs& a, int nsteps, int batch, hipStream_t st) {
    if (batch <= 0 || nsteps <= 0) return;
    hipLaunchKernelGGL((action::action_states_grad_kernel<2>), dim3(nsteps, batch), dim3(64),
                       action_grad_lds_bytes(a.g.m_max), st, a);
}

}  // namespace qocx
