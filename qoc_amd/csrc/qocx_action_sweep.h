// qocx_action_sweep.h - the sweeps of the matrix-free route of one state per seed at 17 <= n <= 32
// (qocx_action.hip has the scheme): the body of one seed's sweeps on one wave, shared by the kernels of
// qocx_action.hip and the builds of qocx_action_eff.hip that hold more operator images in registers.
#ifndef QOCX_ACTION_SWEEP_H
#define QOCX_ACTION_SWEEP_H

#include "qocx_action_core.h"

namespace qocx {

namespace action {

// What an EARLIER launch wrote and every lane reads at one address - the step words, the step controls -
// goes through the scalar unit: such a load is counted by lgkmcnt and does not wait, as a vector load's
// vmcnt does, for the stores of the step before it.
#define QOCX_SCALAR_MEM __attribute__((address_space(4)))
typedef const QOCX_SCALAR_MEM int* ScalarInts;
typedef const QOCX_SCALAR_MEM double* ScalarDoubles;

// 1 / p from a table the code addresses relative to its own position (INV_P, which the host can see, is
// reached through a pointer that a sweep fetched anew in every step)
static __device__ __forceinline__ double inv_p(int p) {
    constexpr InvTable table;
    return table.v[p];
}

// The 16 columns of a lane group's block in ONE block of 64 multiply-adds: dpp_cmac4<0>, <4>, <8>, <12> of
// qocx_action_core.h one after the other - the same instructions on the same accumulator pairs in the same
// order - behind a single s_nop, since x is written once before the first of them.
__device__ __forceinline__ void dpp_cmac16(double& r0, double& i0, double& r1, double& i1, double xr, double xi,
                                           const double (&ar)[16], const double (&ai)[16]) {
#define QOCX_ACTION_CMAC(R, I, C)                                                                          \
    "v_fmac_f64_dpp %[" R "], %[xr], %[ar" #C "] row_newbcast:" #C " row_mask:0xf bank_mask:0xf\n\t"         \
    "v_fmac_f64_dpp %[" I "], %[xi], %[ar" #C "] row_newbcast:" #C " row_mask:0xf bank_mask:0xf\n\t"         \
    "v_fmac_f64_dpp %[" R "], -%[xi], %[ai" #C "] row_newbcast:" #C " row_mask:0xf bank_mask:0xf\n\t"        \
    "v_fmac_f64_dpp %[" I "], %[xr], %[ai" #C "] row_newbcast:" #C " row_mask:0xf bank_mask:0xf\n\t"
#define QOCX_ACTION_CMAC2(C, D) QOCX_ACTION_CMAC("r0", "i0", C) QOCX_ACTION_CMAC("r1", "i1", D)
#define QOCX_ACTION_COL(C) [ar##C] "v"(ar[C]), [ai##C] "v"(ai[C])
    asm("s_nop 1\n\t" QOCX_ACTION_CMAC2(0, 1) QOCX_ACTION_CMAC2(2, 3) QOCX_ACTION_CMAC2(4, 5) QOCX_ACTION_CMAC2(6, 7)
            QOCX_ACTION_CMAC2(8, 9) QOCX_ACTION_CMAC2(10, 11) QOCX_ACTION_CMAC2(12, 13) QOCX_ACTION_CMAC2(14, 15)
        : [r0] "+v"(r0), [i0] "+v"(i0), [r1] "+v"(r1), [i1] "+v"(i1)
        : [xr] "v"(xr), [xi] "v"(xi), QOCX_ACTION_COL(0), QOCX_ACTION_COL(1), QOCX_ACTION_COL(2), QOCX_ACTION_COL(3),
          QOCX_ACTION_COL(4), QOCX_ACTION_COL(5), QOCX_ACTION_COL(6), QOCX_ACTION_COL(7), QOCX_ACTION_COL(8),
          QOCX_ACTION_COL(9), QOCX_ACTION_COL(10), QOCX_ACTION_COL(11), QOCX_ACTION_COL(12), QOCX_ACTION_COL(13),
          QOCX_ACTION_COL(14), QOCX_ACTION_COL(15));
#undef QOCX_ACTION_COL
#undef QOCX_ACTION_CMAC2
#undef QOCX_ACTION_CMAC
}

// The sweeps of one seed on one wave. KR: the G_k images held in registers beside H0 (those of further
// controls are read per step). EXACT: K == KR, known to the compiler - a = fma(u1, g1, fma(u0, g0, h0))
// with no copy of h0 and no branch.
// The vector lives in SPREAD FORM (qocx_action_core.h) from the launch's first load to its last store: lane
// L holds the entry idx = 16 (L >> 5) + (L & 15), which is what the multiply-adds broadcast from, and the
// exchange that sums the lane groups' partial products leaves its result in that form again. Only the
// loads and stores of the vector know about it (the lanes with (L & 16) == 0 store, one per entry); the
// generator's images stay where they were, lane (h, i): row i, columns 16 h ..
template <int NB, int KR, bool EXACT>
static __device__ __forceinline__ void action_sweep_body(const ActionArgs& args, double2* turn) {
    typedef Geo<NB> G;
    constexpr int NP = G::NP, CPL = G::CPL, H = G::H;
    const SweepArgs& sw = args.sw;
    const int b = blockIdx.x;
    const int lane = lane_id(), i = lane % NP, h = lane / NP;
    const int idx = spread_index(lane);       // the entry of the vector this lane holds
    const bool holder = spread_holder(lane);  // ... and stores
    const int nsteps = sw.nsteps, K = EXACT ? KR : args.K, m_max = args.m_max;
    const int jb = sw.j_begin, je = sw.j_end;
    const double dt = args.dt;
    __builtin_amdgcn_s_setprio(3);  // the serial chain of the evaluation goes first on its SIMD

    // -i dt H0 and -i dt G_k, lane (h, i): row i, columns 16 h + cc - the block its lane group multiplies
    // (re, im of -i dt (x + i y) = dt y, -dt x). Element (i, c) of a column-major image sits at
    // (c / H) 64 + (c % H) NP + i.
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

    const ScalarInts words = (ScalarInts)(sw.s_arr + (size_t)b * nsteps);
    const ScalarDoubles u_b = (ScalarDoubles)(args.ustep + (size_t)b * nsteps * K);
    // What a step reads first: its word and its controls in registers. The sweep asks for those of the
    // step after the one it is about to run, so that no step begins by waiting on memory.
    struct StepHead {
        int word;
        double u[KR];
    };
    auto fetch = [&](int step) __attribute__((always_inline)) {
        StepHead s;
        s.word = words[step];
#pragma unroll
        for (int k = 0; k < KR; ++k) s.u[k] = k < K ? u_b[(size_t)step * K + k] : 0.0;
        return s;
    };
    double are[CPL], aim[CPL];
    auto build = [&](int step, const StepHead& s) __attribute__((always_inline)) {
        if constexpr (EXACT) {
#pragma unroll
            for (int cc = 0; cc < CPL; ++cc) {
                double r = h0r[cc], im = h0i[cc];
#pragma unroll
                for (int k = 0; k < KR; ++k) {
                    r = fma(s.u[k], gr[k][cc], r);
                    im = fma(s.u[k], gi[k][cc], im);
                }
                are[cc] = r;
                aim[cc] = im;
            }
        } else {
#pragma unroll
            for (int cc = 0; cc < CPL; ++cc) {
                are[cc] = h0r[cc];
                aim[cc] = h0i[cc];
            }
#pragma unroll
            for (int k = 0; k < KR; ++k)
                if (k < K) {
                    const double uk = s.u[k];
#pragma unroll
                    for (int cc = 0; cc < CPL; ++cc) {
                        are[cc] = fma(uk, gr[k][cc], are[cc]);
                        aim[cc] = fma(uk, gi[k][cc], aim[cc]);
                    }
                }
            for (int k = KR; k < K; ++k) {
                const double uk = u_b[(size_t)step * K + k] * dt;
#pragma unroll
                for (int cc = 0; cc < CPL; ++cc) {
                    const double2 e = args.g_rimg[(size_t)k * G::MAT + image_at(cc)];
                    are[cc] = fma(uk, e.y, are[cc]);
                    aim[cc] = fma(-uk, e.x, aim[cc]);
                }
            }
        }
    };
    // y = a x, x and y in spread form: the lane group's 16 columns, then the sum of the two lane groups'
    // partial products of a row, delivered to the lanes that hold that row's entry
    auto matvec = [&](double xr, double xi, double& yr, double& yi) __attribute__((always_inline)) {
        double s0r = 0, s0i = 0, s1r = 0, s1i = 0;
        dpp_cmac16(s0r, s0i, s1r, s1i, xr, xi, are, aim);
        sum_spread2(s0r + s1r, s0i + s1i, yr, yi);
    };
    // One step: the vector (vr, vi), in spread form, becomes sum_p (sign a)^p / p! v; the terms
    // 0 .. m - 1 go to `keep`. False: the degree is outside the buffers.
    double vr = 0, vi = 0;
    int count = 0;  // lane l: steps at degree l
    auto step_apply = [&](int step, const StepHead& s, double sign, double2* keep_base)
                          __attribute__((always_inline)) {
        // (one value for the wave, and said so: the branch below is the scalar unit's)
        const int m = step_degree(__builtin_amdgcn_readfirstlane(s.word));
        if (m < 1 || m > m_max) return false;
        build(step, s);
        double2* keep = keep_base ? keep_base + ((size_t)b * nsteps + step) * m_max * NP : nullptr;
        count += (lane == m) ? 1 : 0;
        double sr = vr, si = vi;
        for (int p = 1; p <= m; ++p) {
            const double f = sign * inv_p(p);  // (asked for before the products, used after them)
            if (keep != nullptr && holder) keep[(size_t)(p - 1) * NP + idx] = make_double2(vr, vi);
            double yr, yi;
            matvec(vr, vi, yr, yi);
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

    // ---- forward sweep ----------------------------------------------------------------------
    if (sw.phase & 1) {
        const double2 p0 = jb == 0 ? sw.psi0[idx] : args.carry_f[(size_t)b * NP + idx];
        vr = p0.x;
        vi = p0.y;
        StepHead head = fetch(jb);
        for (int step = jb; step < je; ++step) {
            // (the look-ahead of the launch's last step stays inside [jb, je): it reads that step again)
            const StepHead next = fetch(step + 1 < je ? step + 1 : step);
            if (!step_apply(step, head, 1.0, args.kv_f)) {
                refuse();
                return;
            }
            head = next;
        }
        if (count > 0 && lane <= MMAX) atomicAdd(args.degree_counts + lane, count);
        if (je == nsteps) {
            turn[idx] = make_double2(vr, vi);  // (both holders of an entry hold the same value: all store)
            wave_sync();
            const double cost = eval_costs<NB>(sw, false, true, turn, nullptr, h, i);
            if (sw.unit_adjoint && sw.want_grad) unit_adjoint_scales<NB>(sw, turn, b, h, i);
            if (holder) sw.final_out[(size_t)b * NP + idx] = make_double2(vr, vi);
            if (lane == 0) sw.cost_out[b] = cost;
        } else if (holder) {
            args.carry_f[(size_t)b * NP + idx] = make_double2(vr, vi);
        }
    }
    if (!(sw.phase & 2)) return;

    // ---- adjoint sweep: the back-propagated target (unit adjoint) ------------------------------
    wave_sync();
    if (je == nsteps) {
        unit_adjoint_seed<NB>(sw, turn, 0, 1, h, i);
        wave_sync();
        const double2 t = turn[idx];
        vr = t.x;
        vi = t.y;
    } else {
        const double2 t = sw.lam_buf[(size_t)b * NP + idx];
        vr = t.x;
        vi = t.y;
    }
    StepHead head = fetch(je - 1);
    for (int step = je - 1; step >= jb; --step) {
        const StepHead next = fetch(step - 1 >= jb ? step - 1 : step);
        if (!step_apply(step, head, -1.0, args.kv_b)) {
            refuse();
            return;
        }
        head = next;
    }
    if (jb > 0 && holder) sw.lam_buf[(size_t)b * NP + idx] = make_double2(vr, vi);
}

}  // namespace action

}  // namespace qocx

#endif
