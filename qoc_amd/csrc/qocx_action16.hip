// qocx_action16.hip - the matrix-free route of qocx_action.hip at n <= 16 (knob "action_small" = 1): ONE
// state per seed, Hermitian H, the sweeps apply exp(a_j), a_j = -i dt H(u_mid), by the truncated Taylor
// series and leave its terms to the gradient kernel. The recursions, the reverse rule, the degrees from the
// step table and the buffers are those of qocx_action.hip with NP = 16: terms [B][nsteps][m_max][16].
//
// The mapping of the sweep. A complex product y = a x of 16 x 16 is four REAL ones,
//     yr = ar xr + (-ai) xi,   yi = ai xr + ar xi,
// and a wave has four rows of 16 lanes: row q of 16 lanes does one of them, lane (q, l) holding row l of
//     q = 0: ar    q = 1: ai    q = 2: -ai    q = 3: ar       (16 doubles)
// The vector lives in SPLIT FORM: lane (q, l) holds Re x[l] in the rows 0 and 1, Im x[l] in the rows 2 and 3 -
// so lane c of EVERY row holds entry c of the operand that row multiplies with, which is what an immediate
// row_newbcast:c needs, and a term is 16 multiply-adds a lane with the broadcast inside. The four partial
// products p0 .. p3 meet by the exchange of sum_spread2 (qocx_action_core.h) on one double,
//     permlane16_swap of p with itself   X = [p0, p0, p2, p2], Y = [p1, p1, p3, p3]
//     permlane32_swap of X and Y         X = [p0, p0, p1, p1], Y = [p2, p2, p3, p3]
// and X + Y is [yr, yr, yi, yi]: split form again, both holders of a number adding the same two addends.
// Nothing is rotated. (The split into column quarters - lane (q, l): row l, columns 4q .. 4q + 3, half the
// registers per image - leaves every row with p[l] at lane l where row q must broadcast x[4q ..]: a rotation
// of row q by 4q, twelve masked DPP moves a term on top of two exchange stages of a complex number.)
// Order of the sums, whatever n is: a row's product is ((c0 + c4 + c8 + c12) + (c1 + ..)) + ((c2 + ..) +
// (c3 + ..)), each bracket in increasing column, then p0 + p2 resp. p1 + p3. Rows and columns of a beyond n
// are zero, so the pad entries of every term stay exactly zero.
#include "qocx_action_core.h"

namespace qocx {

namespace action16 {

using action::CoefTable;
using action::InvTable;
using action::MMAX;

constexpr int NP = 16, MAT = NP * NP;
// The images of a lane, 16 doubles each: the step generator `a` and KR controls in registers; H0 and the next
// KL controls as the lane's own doubles in LDS (8 KB each: a lane reads back what it wrote), the eight reads
// of an image in flight together - with H0 in registers too, 96 of the 128 would be images and every read of
// a step would wait for the one before it -; any further control from its image in every step. One
// arithmetic for all three: a = h0, then a += u_k g_k on the same numbers in the order of k.
constexpr int KR = 1, KL = 3;

#define QOCX_SCALAR_MEM __attribute__((address_space(4)))
typedef const QOCX_SCALAR_MEM int* ScalarInts;
typedef const QOCX_SCALAR_MEM double* ScalarDoubles;

static __device__ __forceinline__ double inv_p(int p) {
    constexpr InvTable table;
    return table.v[p];
}

// The lane's row of 16 numbers times the operand of its row of 16 lanes: lane c of the row holds x[c], the
// broadcast sits inside the multiply-adds (v_fmac_f64_dpp row_newbcast). Four chains, column c on chain c % 4.
// (s_nop: a DPP operand may not be read in the two cycles after the VALU instruction that wrote it.)
__device__ __forceinline__ double dpp_rowdot16(double x, const double (&a)[16]) {
    double s0 = 0, s1 = 0, s2 = 0, s3 = 0;  // (gfx950 has no DPP form of v_mul_f64: every column is a multiply-add)
#define QOCX_ACTION16_MAC(S, C) \
    "v_fmac_f64_dpp %[" S "], %[x], %[a" #C "] row_newbcast:" #C " row_mask:0xf bank_mask:0xf\n\t"
#define QOCX_ACTION16_COL(C) [a##C] "v"(a[C])
    asm("s_nop 1\n\t" QOCX_ACTION16_MAC("s0", 0) QOCX_ACTION16_MAC("s1", 1) QOCX_ACTION16_MAC("s2", 2)
            QOCX_ACTION16_MAC("s3", 3) QOCX_ACTION16_MAC("s0", 4) QOCX_ACTION16_MAC("s1", 5)
                QOCX_ACTION16_MAC("s2", 6) QOCX_ACTION16_MAC("s3", 7) QOCX_ACTION16_MAC("s0", 8)
                    QOCX_ACTION16_MAC("s1", 9) QOCX_ACTION16_MAC("s2", 10) QOCX_ACTION16_MAC("s3", 11)
                        QOCX_ACTION16_MAC("s0", 12) QOCX_ACTION16_MAC("s1", 13) QOCX_ACTION16_MAC("s2", 14)
                            QOCX_ACTION16_MAC("s3", 15)
        : [s0] "+v"(s0), [s1] "+v"(s1), [s2] "+v"(s2), [s3] "+v"(s3)
        : [x] "v"(x), QOCX_ACTION16_COL(0), QOCX_ACTION16_COL(1), QOCX_ACTION16_COL(2), QOCX_ACTION16_COL(3),
          QOCX_ACTION16_COL(4), QOCX_ACTION16_COL(5), QOCX_ACTION16_COL(6), QOCX_ACTION16_COL(7),
          QOCX_ACTION16_COL(8), QOCX_ACTION16_COL(9), QOCX_ACTION16_COL(10), QOCX_ACTION16_COL(11),
          QOCX_ACTION16_COL(12), QOCX_ACTION16_COL(13), QOCX_ACTION16_COL(14), QOCX_ACTION16_COL(15));
#undef QOCX_ACTION16_COL
#undef QOCX_ACTION16_MAC
    return (s0 + s1) + (s2 + s3);
}

// [p0, p1, p2, p3] on the rows of 16 lanes -> [p0 + p2, p0 + p2, p1 + p3, p1 + p3] (see the head of the file)
__device__ __forceinline__ double sum_split(double p) {
    const unsigned lo = (unsigned)__double2loint(p), hi = (unsigned)__double2hiint(p);
    auto a = __builtin_amdgcn_permlane16_swap(lo, lo, false, false);
    auto b = __builtin_amdgcn_permlane16_swap(hi, hi, false, false);
    auto e = __builtin_amdgcn_permlane32_swap(a[0], a[1], false, false);
    auto f = __builtin_amdgcn_permlane32_swap(b[0], b[1], false, false);
    return make_f64((int)e[0], (int)f[0]) + make_f64((int)e[1], (int)f[1]);
}

// The sweeps of one seed on one wave: the contract of action_sweep_kernel (qocx_action.hip).
// LDS: the vector where the cost code reads it ([16] complex), then the images of H0 and of the controls
// KR .. KR + near - 1, every lane's own 16 doubles ([1 + near][8][64] pairs: a lane reads back what it wrote).
// (four waves to a SIMD: at most 128 registers)
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(4, 4))) void action16_sweep_kernel(
    ActionArgs args, int near) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double2* turn = reinterpret_cast<double2*>(smem);
    double2* lds_g = turn + NP;
    const SweepArgs& sw = args.sw;
    const int b = blockIdx.x;
    const int lane = lane_id(), l = lane & 15, q = lane >> 4;
    const int part = q >> 1;             // 0: the lane holds a real part, 1: an imaginary part
    const bool holder = (q & 1) == 0;    // the rows 0 and 2 store
    const int slot = 2 * l + part;       // the lane's double in a vector of 16 complex numbers
    const int nsteps = sw.nsteps, K = args.K, m_max = args.m_max;
    const int jb = sw.j_begin, je = sw.j_end;
    const double dt = args.dt;
    __builtin_amdgcn_s_setprio(3);  // the serial chain of the evaluation goes first on its SIMD

    // The lane's row of -i dt (x + i y) = dt y - i dt x: re (rows 0, 3), im (row 1), -im (row 2). Element
    // (l, c) of a column-major image sits at (c / 4) 64 + (c % 4) 16 + l.
    const double fac = q == 1 ? -dt : dt;
    const bool take_y = q == 0 || q == 3;
    auto entry = [&](const double2* img, int c) __attribute__((always_inline)) {
        const double2 e = img[(c >> 2) * 64 + (c & 3) * NP + l];
        return fac * (take_y ? e.y : e.x);
    };
    double g[KR][NP];
#pragma unroll
    for (int c = 0; c < NP; c += 2)
        lds_g[(c / 2) * 64 + lane] = make_double2(entry(args.h0_rimg, c), entry(args.h0_rimg, c + 1));
#pragma unroll
    for (int k = 0; k < KR; ++k)
#pragma unroll
        for (int c = 0; c < NP; ++c) g[k][c] = k < K ? entry(args.g_rimg + (size_t)k * MAT, c) : 0.0;
    for (int kk = 0; kk < near; ++kk)
#pragma unroll
        for (int c = 0; c < NP; c += 2) {
            const double2* img = args.g_rimg + (size_t)(KR + kk) * MAT;
            lds_g[((1 + kk) * 8 + c / 2) * 64 + lane] = make_double2(entry(img, c), entry(img, c + 1));
        }

    const ScalarInts words = (ScalarInts)(sw.s_arr + (size_t)b * nsteps);
    const ScalarDoubles u_b = (ScalarDoubles)(args.ustep + (size_t)b * nsteps * K);
    // What a step reads first: its word and the controls held in registers, asked for a step ahead
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
    double a[NP];
    auto build = [&](int step, const StepHead& s) __attribute__((always_inline)) {
        // (the controls of the images in LDS: asked for together, ahead of everything else the step builds -
        // one round trip through the scalar cache, not one per control; an index past K - 1 reads K - 1)
        double uk[KL];
#pragma unroll
        for (int kk = 0; kk < KL; ++kk) uk[kk] = u_b[(size_t)step * K + min(KR + kk, K - 1)];
        // (an image from LDS: its eight reads asked for before the first is used)
        auto image = [&](int slot, double2 (&e)[8]) __attribute__((always_inline)) {
#pragma unroll
            for (int c2 = 0; c2 < 8; ++c2) e[c2] = lds_g[(slot * 8 + c2) * 64 + lane];
            asm volatile("" ::: "memory");
        };
        {
            double2 e[8];
            image(0, e);
#pragma unroll
            for (int c2 = 0; c2 < 8; ++c2) {
                a[2 * c2] = e[c2].x;
                a[2 * c2 + 1] = e[c2].y;
            }
        }
#pragma unroll
        for (int k = 0; k < KR; ++k)
            if (k < K) {
#pragma unroll
                for (int c = 0; c < NP; ++c) a[c] = fma(s.u[k], g[k][c], a[c]);
            }
#pragma unroll
        for (int kk = 0; kk < KL; ++kk)
            if (kk < near) {
                double2 e[8];
                image(1 + kk, e);
#pragma unroll
                for (int c2 = 0; c2 < 8; ++c2) {
                    a[2 * c2] = fma(uk[kk], e[c2].x, a[2 * c2]);
                    a[2 * c2 + 1] = fma(uk[kk], e[c2].y, a[2 * c2 + 1]);
                }
            }
        for (int k = KR + near; k < K; ++k) {
            const double uk = u_b[(size_t)step * K + k];
            const double2* img = args.g_rimg + (size_t)k * MAT;
#pragma unroll
            for (int c = 0; c < NP; ++c) a[c] = fma(uk, entry(img, c), a[c]);
        }
    };
    // One step: the vector v, in split form, becomes sum_p (sign a)^p / p! v; the terms 0 .. m - 1 go to
    // `keep`. False: the degree is outside the buffers.
    double v = 0;
    int count = 0;  // lane l: steps at degree l
    auto step_apply = [&](int step, const StepHead& s, double sign, double2* keep_base)
                          __attribute__((always_inline)) {
        const int m = step_degree(__builtin_amdgcn_readfirstlane(s.word));
        if (m < 1 || m > m_max) return false;
        build(step, s);
        double* keep = keep_base ? reinterpret_cast<double*>(keep_base + ((size_t)b * nsteps + step) * m_max * NP)
                                 : nullptr;
        count += (lane == m) ? 1 : 0;
        double sum = v;
        for (int p = 1; p <= m; ++p) {
            const double f = sign * inv_p(p);
            if (keep != nullptr && holder) keep[(size_t)(p - 1) * 2 * NP + slot] = v;
            v = f * sum_split(dpp_rowdot16(v, a));
            sum += v;
        }
        v = sum;
        return true;
    };
    auto refuse = [&]() {  // never clamped: the host runs the evaluation again on the Pade route
        if (lane == 0) atomicOr(sw.status, 8);
    };
    auto load = [&](const double2* vec) { return reinterpret_cast<const double*>(vec)[slot]; };
    auto store = [&](double2* vec) {
        if (holder) reinterpret_cast<double*>(vec)[slot] = v;
    };

    // ---- forward sweep ----------------------------------------------------------------------
    if (sw.phase & 1) {
        v = load(jb == 0 ? sw.psi0 : args.carry_f + (size_t)b * NP);
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
            reinterpret_cast<double*>(turn)[slot] = v;  // (both holders of a number hold the same value: all store)
            wave_sync();
            const double cost = eval_costs<1>(sw, false, true, turn, nullptr, q, l);
            if (sw.unit_adjoint && sw.want_grad) unit_adjoint_scales<1>(sw, turn, b, q, l);
            store(sw.final_out + (size_t)b * NP);
            if (lane == 0) sw.cost_out[b] = cost;
        } else {
            store(args.carry_f + (size_t)b * NP);
        }
    }
    if (!(sw.phase & 2)) return;

    // ---- adjoint sweep: the back-propagated target (unit adjoint) ------------------------------
    wave_sync();
    if (je == nsteps) {
        unit_adjoint_seed<1>(sw, turn, 0, 1, q, l);
        wave_sync();
        v = reinterpret_cast<const double*>(turn)[slot];
    } else {
        v = load(sw.lam_buf + (size_t)b * NP);
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
    if (jb > 0) store(sw.lam_buf + (size_t)b * NP);
}

// All rho_i = sum_{l < M - i} c_il v_l of a step at degree M, for ONE entry: the M terms in registers (one
// load each, all in flight together), the coefficients compile-time constants. The even l and the odd l each
// in increasing l from zero, added once (the order of qocx_action.hip). rho_i goes to row M - 1 - i of `rows`.
template <int M>
__device__ __forceinline__ void rho_rows(const double2* terms, double2* rows) {
    constexpr CoefTable coef;
    double2 v[M];
#pragma unroll
    for (int l = 0; l < M; ++l) v[l] = terms[(size_t)l * NP];
#pragma unroll
    for (int i = 0; i < M; ++i) {
        double er = 0, ei = 0, orr = 0, oi = 0;
#pragma unroll
        for (int l = 0; l < M - i; l += 2) {
            er = fma(coef.c[i * MMAX + l], v[l].x, er);
            ei = fma(coef.c[i * MMAX + l], v[l].y, ei);
            if (l + 1 < M - i) {
                orr = fma(coef.c[i * MMAX + l + 1], v[l + 1].x, orr);
                oi = fma(coef.c[i * MMAX + l + 1], v[l + 1].y, oi);
            }
        }
        rows[(M - 1 - i) * NP] = make_double2(er + orr, ei + oi);
        if constexpr (M >= 16) asm volatile("" ::: "memory");  // (one rho_i at a time: the scalar registers)
    }
}
__device__ __forceinline__ void rho_rows_dispatch(int m, const double2* terms, double2* rows) {
    static_assert(MMAX == 18, "one case per degree");
    switch (m) {
#define QOCX_ACTION16_RHO(M) case M: rho_rows<M>(terms, rows); break;
        QOCX_ACTION16_RHO(1) QOCX_ACTION16_RHO(2) QOCX_ACTION16_RHO(3) QOCX_ACTION16_RHO(4) QOCX_ACTION16_RHO(5)
        QOCX_ACTION16_RHO(6) QOCX_ACTION16_RHO(7) QOCX_ACTION16_RHO(8) QOCX_ACTION16_RHO(9) QOCX_ACTION16_RHO(10)
        QOCX_ACTION16_RHO(11) QOCX_ACTION16_RHO(12) QOCX_ACTION16_RHO(13) QOCX_ACTION16_RHO(14)
        QOCX_ACTION16_RHO(15) QOCX_ACTION16_RHO(16) QOCX_ACTION16_RHO(17) QOCX_ACTION16_RHO(18)
#undef QOCX_ACTION16_RHO
    }
}

// One wave per (step, seed), split in quarters: lane (q, l) holds abar at row l and the columns q, 4 + q,
// 8 + q, 12 + q - where the E_k image has them for it (lane (q, l) of fragment cc: row l, column 4 cc + q),
// four complex numbers. LDS: rho_(m-1) .. rho_0 [m][16].
//   1. All rho_i of the step for the entry lane & 15 (the four rows of 16 lanes form and write the same
//      numbers), then a wave-level fence: a lane reads entries other lanes wrote.
//   2. Per term one read of w_i[l] from memory, four of rho_i from LDS, 16 multiply-adds.
//   3. gamma_k = sum conj(abar) E_k, every control's two sums by the tree of wave_sum: a fixed order, no atomics.
// (Against four steps per wave, a step per row of 16 lanes with the broadcast of rho inside the multiply-adds:
// the same 16 multiply-adds per term and step, but one build per degree serves a wave only if its four steps
// share the degree, which the step table does not promise.)
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(5, 5))) void action16_grad_kernel(
    ActionGradArgs args) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double2* rows = reinterpret_cast<double2*>(smem);
    const int step = args.step0 + blockIdx.x, b = blockIdx.y;
    const int lane = lane_id(), l = lane & 15, q = lane >> 4;
    const int K = args.K;
    const size_t idx = (size_t)b * args.nsteps + step;
    const int m = step_degree(__builtin_amdgcn_readfirstlane(args.s_arr[idx]));
    if (m < 1 || m > args.m_max) return;  // (the sweeps have raised the status bit)
    const double2* vf = args.kv_f + idx * args.m_max * NP;
    const double2* wb = args.kv_b + idx * args.m_max * NP;
    rho_rows_dispatch(m, vf + l, rows + l);
    wave_sync();
    double abr[4], abi[4];
#pragma unroll
    for (int cc = 0; cc < 4; ++cc) {
        abr[cc] = 0;
        abi[cc] = 0;
    }
    double2 w = wb[l];
    for (int i = 0; i < m; ++i) {
        const double2 wn = wb[(size_t)min(i + 1, m - 1) * NP + l];  // (asked for a term ahead)
        const double2* rho = rows + (m - 1 - i) * NP + q;
#pragma unroll
        for (int cc = 0; cc < 4; ++cc) {
            const double2 r = rho[4 * cc];
            abr[cc] = fma(w.y, r.y, fma(w.x, r.x, abr[cc]));
            abi[cc] = fma(-w.x, r.y, fma(w.y, r.x, abi[cc]));
        }
        w = wn;
    }
    double2* out = reinterpret_cast<double2*>(args.gstep) + idx * K;
    for (int k = 0; k < K; ++k) {
        const double2* img = args.e_img + (size_t)k * MAT;
        double re = 0, im = 0;
#pragma unroll
        for (int cc = 0; cc < 4; ++cc) {
            const double2 e = img[cc * 64 + lane];
            re = fma(abi[cc], e.y, fma(abr[cc], e.x, re));
            im = fma(abi[cc], -e.x, fma(abr[cc], e.y, im));
        }
        re = wave_sum(re);
        im = wave_sum(im);
        if (lane == 0) out[k] = make_double2(re, im);
    }
}

}  // namespace action16

void launch_action16_sweep(const ActionArgs& a, int batch, hipStream_t st) {
    if (batch <= 0 || a.sw.j_end <= a.sw.j_begin) return;
    const int near = std::min(std::max(a.K - action16::KR, 0), action16::KL);
    const size_t lds = (size_t)(action16::NP + (1 + near) * 8 * 64) * sizeof(double2);
    hipLaunchKernelGGL(action16::action16_sweep_kernel, dim3(batch), dim3(64), lds, st, a, near);
}

void launch_action16_grad(const ActionGradArgs& a, int nsteps, int batch, hipStream_t st) {
    if (batch <= 0 || nsteps <= 0) return;
    hipLaunchKernelGGL(action16::action16_grad_kernel, dim3(nsteps, batch), dim3(64),
                       (size_t)a.m_max * action16::NP * sizeof(double2), st, a);
}

}  // namespace qocx
