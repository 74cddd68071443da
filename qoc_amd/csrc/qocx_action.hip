// qocx_action.hip - the matrix-free route of ONE state per seed, Hermitian H, 17 <= n <= 32: the sweeps
// apply exp(a_j), a_j = -i dt H(u_mid), to their vector by the truncated Taylor series (Al-Mohy &
// Higham 2011, qocx_action.h) instead of solving with the factors of a Pade denominator. Nothing is
// factored and no matrix is stored: n^2 work per Taylor term, m terms per step, against the n^3 of a
// Pade step that only ever served one vector.
//
//   forward   v_0 = psi,     v_p = a v_(p-1) / p,   psi'   = sum_{p=0..m} v_p      (keeps v_0 .. v_(m-1))
//   adjoint   w_0 = lambda', w_p = -a w_(p-1) / p,  lambda = sum_{p=0..m} w_p      (a^H = -a; keeps w_0 .. w_(m-1))
//   generator cotangent   abar = sum_{i<m} w_i rho_i^H,  rho_i = sum_{l<m-i} c_il v_l,  c_il = i! l! / (i + l + 1)!
//   - the exact reverse rule of psi' = T_m(a) psi: d(a^p)/p! in direction E is sum_{i+l=p-1} a^i E a^l / p!,
//   and a^i / i!, a^l / l! applied to lambda', psi are w_i (up to (-1)^i (-1)^i = 1 through a^H = -a), v_l.
//   step gradient   gamma_k = sum conj(abar) (.) (-i dt G_k), a complex pair per (step, k) as K3 leaves
//   it under the unit adjoint (KrylovArgs::gstep): the adjoint runs on the target and the scatter
//   kernel applies the cost's scalar.
//
// The degree m of a step comes from the step table (bits 24..29 of its entry), decided from the same
// bound as the Pade order. A step's arithmetic depends on nothing but its inputs, so results are bit
// identical however the steps are cut into launches.
#include "qocx_action_sweep.h"

namespace qocx {

namespace action {

template <int NB, int KR>
__global__ __launch_bounds__(64) void action_sweep_kernel(ActionArgs args) {
    __shared__ __attribute__((aligned(16))) double2 turn[Geo<NB>::NP];  // the vector where the cost code reads / writes it
    action_sweep_body<NB, KR, false>(args, turn);
}

// K == 2, the headline's: the same sweeps with the control count a constant
template <int NB>
__global__ __launch_bounds__(64) void action_sweep_exact_kernel(ActionArgs args) {
    __shared__ __attribute__((aligned(16))) double2 turn[Geo<NB>::NP];
    action_sweep_body<NB, 2, true>(args, turn);
}

// The rank-1 update of one Taylor term, abar += w rho^H, on the lane's 16 columns: 64 multiply-adds with the
// broadcast of rho INSIDE them, as dpp_cmac16 has it for the sweeps. rho is in the spread form of the gradient
// kernel below - lane c of every row of 16 lanes holds the entry 2 c + h of its lane group h - and column cc
// of the lane's block is the entry 2 cc + h. Per column, in the order of
//   abr = fma(w.y, rho.y, fma(w.x, rho.x, abr)),  abi = fma(-w.x, rho.y, fma(w.y, rho.x, abi))
// with the factors of a product exchanged and the sign of the last one on rho (the same product bit for
// bit); two columns in turn, so that three instructions lie between two writes of one accumulator.
__device__ __forceinline__ void dpp_rank1_16(double (&abr)[16], double (&abi)[16], double wx, double wy, double rx,
                                             double ry) {
#define QOCX_ACTION_R1(C, D)                                                                               \
    "v_fmac_f64_dpp %[r" #C "], %[rx], %[wx] row_newbcast:" #C " row_mask:0xf bank_mask:0xf\n\t"            \
    "v_fmac_f64_dpp %[i" #C "], %[rx], %[wy] row_newbcast:" #C " row_mask:0xf bank_mask:0xf\n\t"            \
    "v_fmac_f64_dpp %[r" #D "], %[rx], %[wx] row_newbcast:" #D " row_mask:0xf bank_mask:0xf\n\t"            \
    "v_fmac_f64_dpp %[i" #D "], %[rx], %[wy] row_newbcast:" #D " row_mask:0xf bank_mask:0xf\n\t"            \
    "v_fmac_f64_dpp %[r" #C "], %[ry], %[wy] row_newbcast:" #C " row_mask:0xf bank_mask:0xf\n\t"            \
    "v_fmac_f64_dpp %[i" #C "], -%[ry], %[wx] row_newbcast:" #C " row_mask:0xf bank_mask:0xf\n\t"           \
    "v_fmac_f64_dpp %[r" #D "], %[ry], %[wy] row_newbcast:" #D " row_mask:0xf bank_mask:0xf\n\t"            \
    "v_fmac_f64_dpp %[i" #D "], -%[ry], %[wx] row_newbcast:" #D " row_mask:0xf bank_mask:0xf\n\t"
#define QOCX_ACTION_ACC(C) [r##C] "+v"(abr[C]), [i##C] "+v"(abi[C])
    // (volatile, "memory": what the caller asked for before the block - the next term's rho and w - is asked
    // for before it, and waited for behind it)
    asm volatile("s_nop 1\n\t" QOCX_ACTION_R1(0, 1) QOCX_ACTION_R1(2, 3) QOCX_ACTION_R1(4, 5) QOCX_ACTION_R1(6, 7)
                     QOCX_ACTION_R1(8, 9) QOCX_ACTION_R1(10, 11) QOCX_ACTION_R1(12, 13) QOCX_ACTION_R1(14, 15)
        : QOCX_ACTION_ACC(0), QOCX_ACTION_ACC(1), QOCX_ACTION_ACC(2), QOCX_ACTION_ACC(3), QOCX_ACTION_ACC(4),
          QOCX_ACTION_ACC(5), QOCX_ACTION_ACC(6), QOCX_ACTION_ACC(7), QOCX_ACTION_ACC(8), QOCX_ACTION_ACC(9),
          QOCX_ACTION_ACC(10), QOCX_ACTION_ACC(11), QOCX_ACTION_ACC(12), QOCX_ACTION_ACC(13), QOCX_ACTION_ACC(14),
          QOCX_ACTION_ACC(15)
        : [wx] "v"(wx), [wy] "v"(wy), [rx] "v"(rx), [ry] "v"(ry)
        : "memory");
#undef QOCX_ACTION_ACC
#undef QOCX_ACTION_R1
}

// N sums over the wave at once, each by the tree of wave_sum (qocx_wave.h) - the same additions in the same
// order, so the same bits -, stage by stage across the N values: one tree's instructions fill the wait
// states of the others' exchanges, as sum_spread2 does for a pair.
// (the exchanges below read every lane from a lane of its row: nothing of the destination is kept, and said
// so, the compiler does not copy the value into it first)
template <int CTRL>
__device__ __forceinline__ double dpp_f64_all(double v) {
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xf, 0xf, true);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xf, 0xf, true);
    return make_f64(lo, hi);
}
template <int N>
__device__ __forceinline__ void wave_sums(double (&v)[N]) {
#pragma unroll
    for (int q = 0; q < N; ++q) v[q] = v[q] + dpp_f64_all<0xB1>(v[q]);
#pragma unroll
    for (int q = 0; q < N; ++q) v[q] = v[q] + dpp_f64_all<0x4E>(v[q]);
#pragma unroll
    for (int q = 0; q < N; ++q) v[q] = v[q] + dpp_f64_all<0x141>(v[q]);
#pragma unroll
    for (int q = 0; q < N; ++q) v[q] = v[q] + dpp_f64_all<0x140>(v[q]);
    double r[N][4];
#pragma unroll
    for (int q = 0; q < N; ++q)
#pragma unroll
        for (int row = 0; row < 4; ++row) r[q][row] = readlane_f64(v[q], 16 * row);
#pragma unroll
    for (int q = 0; q < N; ++q) v[q] = (r[q][0] + r[q][1]) + (r[q][2] + r[q][3]);
}

// All rho_i = sum_{l < M - i} c_il v_l of a step at degree M, for ONE entry: the M terms v_l[entry] in
// registers (one load each, all in flight together), the coefficients compile-time constants, every loop
// unrolled. Both partial sums of the entry, the even l and the odd l, each in increasing l from zero, added
// once - the association the two lane groups had when each summed its half and they exchanged. rho_i goes to
// row M - 1 - i of `rows` (LDS, the lane's own column: it is the lane that reads it back).
template <int M, int NP>
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
        // (the largest builds one rho_i at a time: all their coefficients at once do not fit the scalar registers)
        if constexpr (M >= 16) asm volatile("" ::: "memory");
    }
}
// (the degree is the wave's: a scalar branch to the build of its degree)
template <int NP>
__device__ __forceinline__ void rho_rows_dispatch(int m, const double2* terms, double2* rows) {
    static_assert(MMAX == 18, "one case per degree");
    switch (m) {
#define QOCX_ACTION_RHO(M) case M: rho_rows<M, NP>(terms, rows); break;
        QOCX_ACTION_RHO(1) QOCX_ACTION_RHO(2) QOCX_ACTION_RHO(3) QOCX_ACTION_RHO(4) QOCX_ACTION_RHO(5)
        QOCX_ACTION_RHO(6) QOCX_ACTION_RHO(7) QOCX_ACTION_RHO(8) QOCX_ACTION_RHO(9) QOCX_ACTION_RHO(10)
        QOCX_ACTION_RHO(11) QOCX_ACTION_RHO(12) QOCX_ACTION_RHO(13) QOCX_ACTION_RHO(14) QOCX_ACTION_RHO(15)
        QOCX_ACTION_RHO(16) QOCX_ACTION_RHO(17) QOCX_ACTION_RHO(18)
#undef QOCX_ACTION_RHO
    }
}

// One wave per (step, seed). LDS: rho_(m-1) .. rho_0 [m_max][NP] and nothing else, every lane writing and
// reading its own column - the place the m rho_i wait in while the accumulators have the registers.
//   1. All rho_i of the step, before any of them is used (rho_rows): the terms v_l of the lane's entry come
//      straight from memory into registers, in one round trip. The entry is 2 (lane & 15) + (lane >> 5): the
//      spread form dpp_rank1_16 broadcasts from. Two lanes hold an entry; they write the same values to the
//      same addresses in the same instructions, and no lane touches another entry's column: no barrier.
//   2. The rank-1 loop: per term ONE read of rho_i from LDS and one of w_i from memory, both asked for a
//      term ahead, and the 64 multiply-adds.
//   3. The contraction with E_k = -i dt G_k, read as the image the problem setter built (ActionGradArgs::
//      e_img: (p, q) = (dt G.y, -dt G.x), the products the kernel used to form per step), two controls at a
//      time: their four sums reduced together, one store per control.
// Built for five waves to a SIMD (96 registers: two waves fit beside a sweep wave) with the image read in
// batches of four - measured against four waves (batches of 4 and 8), three (16), and against rank-1 updates
// that read rho from LDS into plain multiply-adds (six waves spill).
template <int NB>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(5, 5))) void action_grad_kernel(
    ActionGradArgs args) {
    typedef Geo<NB> G;
    constexpr int NP = G::NP, CPL = G::CPL, H = G::H, GB = 4;
    static_assert(H == 2 && CPL == 16, "one block of 16 columns per lane group");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double2* vl = reinterpret_cast<double2*>(smem);
    const int step = args.step0 + blockIdx.x, b = blockIdx.y;
    const int lane = lane_id(), i = lane % NP, h = lane / NP;
    const int j = 2 * (lane & 15) + h;  // the entry of rho this lane forms and broadcasts
    const int K = args.K;
    const size_t idx = (size_t)b * args.nsteps + step;
    const int m = step_degree(__builtin_amdgcn_readfirstlane(args.s_arr[idx]));
    if (m < 1 || m > args.m_max) return;  // (the sweeps have raised the status bit)
    const double2* vf = args.kv_f + idx * args.m_max * NP;
    const double2* wb = args.kv_b + idx * args.m_max * NP;
    double2 w = wb[i];
    // (every term of the lane's entry asked for at once, straight into registers: the sweeps wrote them,
    // they come from L2 or further. The accumulators of the rank-1 loop are not alive yet.)
    rho_rows_dispatch<NP>(m, vf + j, vl + j);
    // (a lane reads back the column it wrote, in program order: no exchange between lanes, no barrier)
    double abr[CPL], abi[CPL];
#pragma unroll
    for (int cc = 0; cc < CPL; ++cc) {
        abr[cc] = 0;
        abi[cc] = 0;
    }
    // (two terms per turn, each in registers of its own: no copy stands between a read and its use, so a
    // term's operands are waited for behind the other term's multiply-adds. A read past the last term
    // reads the last term again and is not used.)
    double2 rho = vl[(m - 1) * NP + j];
    int ii = 0;
    for (; ii + 1 < m; ii += 2) {
        const double2 w1 = (wb + (size_t)(ii + 1) * NP)[(unsigned)i];
        const double2 rho1 = vl[(m - 2 - ii) * NP + j];
        dpp_rank1_16(abr, abi, w.x, w.y, rho.x, rho.y);
        w = (wb + (size_t)min(ii + 2, m - 1) * NP)[(unsigned)i];
        rho = vl[max(m - 3 - ii, 0) * NP + j];
        dpp_rank1_16(abr, abi, w1.x, w1.y, rho1.x, rho1.y);
    }
    if (ii < m) dpp_rank1_16(abr, abi, w.x, w.y, rho.x, rho.y);
    // gamma_k = sum conj(abar) E_k (krylov_grad_body, unit adjoint):
    //   re = fma(abi, q, fma(abr, p, re)),  im = fma(abi, -p, fma(abr, q, im))
    auto contract = [&](int k0, auto count) __attribute__((always_inline)) {
        constexpr int KK = decltype(count)::value;
        double s[2 * KK];
#pragma unroll
        for (int q = 0; q < 2 * KK; ++q) s[q] = 0;
#pragma unroll
        for (int kk = 0; kk < KK; ++kk) {
            const double2* img = args.e_img + (size_t)(k0 + kk) * G::MAT;  // (one address for the wave)
#pragma unroll
            for (int c0 = 0; c0 < CPL; c0 += GB) {
                double2 e[GB];  // the fragments of a batch asked for before the first is used
#pragma unroll
                for (int cc = 0; cc < GB; ++cc) e[cc] = (img + c0 * 64)[(unsigned)(cc * 64 + lane)];
                asm volatile("" ::: "memory");  // (no load of the next batch moves up between these)
#pragma unroll
                for (int cc = 0; cc < GB; ++cc) {
                    s[2 * kk] = fma(abi[c0 + cc], e[cc].y, fma(abr[c0 + cc], e[cc].x, s[2 * kk]));
                    s[2 * kk + 1] = fma(abi[c0 + cc], -e[cc].x, fma(abr[c0 + cc], e[cc].y, s[2 * kk + 1]));
                }
            }
        }
        wave_sums(s);
        if (lane == 0) {
            double2* out = reinterpret_cast<double2*>(args.gstep) + idx * K + k0;
#pragma unroll
            for (int kk = 0; kk < KK; ++kk) out[kk] = make_double2(s[2 * kk], s[2 * kk + 1]);
        }
    };
    int k = 0;
    for (; k + 1 < K; k += 2) contract(k, std::integral_constant<int, 2>());
    if (k < K) contract(k, std::integral_constant<int, 1>());
}

}  // namespace action

int action_grad_lds_bytes(int m_max) { return (m_max + 2) * Geo<2>::NP * (int)sizeof(double2); }

void launch_action_sweep(const ActionArgs& a, int batch, hipStream_t st) {
    if (batch <= 0 || a.sw.j_end <= a.sw.j_begin) return;
    if (a.K == 2)
        hipLaunchKernelGGL((action::action_sweep_exact_kernel<2>), dim3(batch), dim3(64), 0, st, a);
    else
        hipLaunchKernelGGL((action::action_sweep_kernel<2, 2>), dim3(batch), dim3(64), 0, st, a);
}

void launch_action_grad(const ActionGradArgs& a, int nsteps, int batch, hipStream_t st) {
    if (batch <= 0 || nsteps <= 0) return;
    // (its own LDS size: the rows of the terms alone, rho_i overwrites them)
    hipLaunchKernelGGL((action::action_grad_kernel<2>), dim3(nsteps, batch), dim3(64),
                       a.m_max * Geo<2>::NP * (int)sizeof(double2), st, a);
}

}  // namespace qocx
