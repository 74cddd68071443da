// qocx_action_core.h - what the matrix-free kernels of 17 <= n <= 32 share (qocx_action.hip: one state
// per seed; qocx_action_states.hip: two to four): the tables of 1 / p and of the reverse rule's
// coefficients, the four-column multiply-add with the broadcast inside, the spread of a vector over the
// rows of 16 lanes - and the spread form in which the one-state sweeps keep their vector from term to term,
// with the exchange that sums the lane groups' partial products into it.
#ifndef QOCX_ACTION_CORE_H
#define QOCX_ACTION_CORE_H

#include "qocx_sweep_common.h"
#include "qocx_action.h"

namespace qocx {

namespace action {

constexpr int MMAX = QOCX_ACTION_MAX_DEGREE;

struct InvTable {  // 1 / p
    double v[MMAX + 2];
    constexpr InvTable() : v{} {
        for (int p = 1; p < MMAX + 2; ++p) v[p] = 1.0 / (double)p;
    }
};
struct CoefTable {  // c_il = i! l! / (i + l + 1)! = c_(i,l-1) l / (i + l + 1), c_i0 = 1 / (i + 1)
    double c[MMAX * MMAX];
    constexpr CoefTable() : c{} {
        for (int i = 0; i < MMAX; ++i) {
            double v = 1.0 / (double)(i + 1);
            c[i * MMAX] = v;
            for (int l = 1; l < MMAX; ++l) {
                v = v * (double)l / (double)(i + l + 1);
                c[i * MMAX + l] = v;
            }
        }
    }
};
__device__ __constant__ const InvTable INV_P = InvTable();
__device__ __constant__ const CoefTable COEF = CoefTable();

// Four columns K0 .. K0 + 3 of y += a x with the broadcast of x INSIDE the multiply-add (v_fmac_f64_dpp
// row_newbcast, as the triangular solves of qocx_sweep_core.h): lane k of every row of 16 lanes holds
// x[column k of the lane's block], so a column costs four instructions and no trip through LDS. Two
// accumulator pairs in turn. (s_nop: a DPP operand may not be read in the two cycles after the VALU
// instruction that wrote it, and the compiler does not look into the block.)
template <int K0>
__device__ __forceinline__ void dpp_cmac4(double& r0, double& i0, double& r1, double& i1, double xr, double xi,
                                          double a0r, double a0i, double a1r, double a1i, double a2r,
                                          double a2i, double a3r, double a3i) {
#define QOCX_ACTION_CMAC(R, I, AR, AI, BC)                                                        \
    "v_fmac_f64_dpp %[" R "], %[xr], %[" AR "] row_newbcast:%[" BC "] row_mask:0xf bank_mask:0xf\n\t"  \
    "v_fmac_f64_dpp %[" I "], %[xi], %[" AR "] row_newbcast:%[" BC "] row_mask:0xf bank_mask:0xf\n\t"  \
    "v_fmac_f64_dpp %[" R "], -%[xi], %[" AI "] row_newbcast:%[" BC "] row_mask:0xf bank_mask:0xf\n\t" \
    "v_fmac_f64_dpp %[" I "], %[xr], %[" AI "] row_newbcast:%[" BC "] row_mask:0xf bank_mask:0xf\n\t"
    asm("s_nop 1\n\t" QOCX_ACTION_CMAC("r0", "i0", "a0r", "a0i", "k0") QOCX_ACTION_CMAC("r1", "i1", "a1r", "a1i", "k1")
            QOCX_ACTION_CMAC("r0", "i0", "a2r", "a2i", "k2") QOCX_ACTION_CMAC("r1", "i1", "a3r", "a3i", "k3")
        : [r0] "+v"(r0), [i0] "+v"(i0), [r1] "+v"(r1), [i1] "+v"(i1)
        : [xr] "v"(xr), [xi] "v"(xi), [a0r] "v"(a0r), [a0i] "v"(a0i), [a1r] "v"(a1r), [a1i] "v"(a1i),
          [a2r] "v"(a2r), [a2i] "v"(a2i), [a3r] "v"(a3r), [a3i] "v"(a3i), [k0] "i"(K0), [k1] "i"(K0 + 1),
          [k2] "i"(K0 + 2), [k3] "i"(K0 + 3));
#undef QOCX_ACTION_CMAC
}

// x on the rows of 16 lanes a lane group multiplies with: lane group 0 (lanes 0 .. 31) the entries
// 0 .. 15 in both of its rows, lane group 1 the entries 16 .. 31. In: lane (h, i) holds x[i].
__device__ __forceinline__ double spread_halves(double v, int h) {
    const unsigned lo = (unsigned)__double2loint(v), hi = (unsigned)__double2hiint(v);
    // (swap of a register with itself: [0] the even rows in every row pair, [1] the odd rows)
    auto a = __builtin_amdgcn_permlane16_swap(lo, lo, false, false);
    auto b = __builtin_amdgcn_permlane16_swap(hi, hi, false, false);
    return h == 0 ? make_f64((int)a[0], (int)b[0]) : make_f64((int)a[1], (int)b[1]);
}

// SPREAD FORM of a vector of 32 entries on one wave (the sweeps of qocx_action.hip keep theirs in it): lane
// L holds the entry 16 (L >> 5) + (L & 15) - the rows 0 and 1 of 16 lanes x[0 .. 15], the rows 2 and 3
// x[16 .. 31], which is what spread_halves makes and what the multiply-adds above broadcast from. Every
// entry has two holders; the one with (L & 16) == 0 stores it.
__device__ __forceinline__ int spread_index(int lane) { return 16 * (lane >> 5) + (lane & 15); }
__device__ __forceinline__ bool spread_holder(int lane) { return (lane & 16) == 0; }

// The sum over the two lane groups of the partial products p of a matrix-vector product (lane (h, i): row
// i, the columns of lane group h), delivered in spread form. The rows of 16 lanes hold [p0, p1, p2, p3]:
//   permlane16_swap of p with its copy   X = [p0, p0, p2, p2], Y = [p1, p1, p3, p3]
//   permlane32_swap of X and Y           X = [p0, p0, p1, p1], Y = [p2, p2, p3, p3]
// and X + Y is p(0, i) + p(1, i) at both holders of entry i: the two addends of sum_groups<2>, so the same
// bits, without the trip back to "lane (h, i) holds x[i]" that the next product would undo at once. A pair
// of values (re, im) at a time, so that one chain's instructions fill the wait states of the other's swaps.
__device__ __forceinline__ void sum_spread2(double pr, double pi, double& yr, double& yi) {
    const unsigned rl = (unsigned)__double2loint(pr), rh = (unsigned)__double2hiint(pr);
    const unsigned il = (unsigned)__double2loint(pi), ih = (unsigned)__double2hiint(pi);
    auto a = __builtin_amdgcn_permlane16_swap(rl, rl, false, false);
    auto b = __builtin_amdgcn_permlane16_swap(rh, rh, false, false);
    auto c = __builtin_amdgcn_permlane16_swap(il, il, false, false);
    auto d = __builtin_amdgcn_permlane16_swap(ih, ih, false, false);
    auto e = __builtin_amdgcn_permlane32_swap(a[0], a[1], false, false);
    auto f = __builtin_amdgcn_permlane32_swap(b[0], b[1], false, false);
    auto g = __builtin_amdgcn_permlane32_swap(c[0], c[1], false, false);
    auto k = __builtin_amdgcn_permlane32_swap(d[0], d[1], false, false);
    yr = make_f64((int)e[0], (int)f[0]) + make_f64((int)e[1], (int)f[1]);
    yi = make_f64((int)g[0], (int)k[0]) + make_f64((int)g[1], (int)k[1]);
}

}  // namespace action

}  // namespace qocx

#endif
