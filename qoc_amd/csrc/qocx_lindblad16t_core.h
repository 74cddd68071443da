// qocx_lindblad16t_core.h - what the kernel of qocx_lindblad16t.hip is made of: the geometry of sixteen
// waves on a 64 x 64 image, the LDS layout, operand fragments read from C-dumps in memory, the products,
// the density costs and the right-hand side.
#ifndef QOCX_LINDBLAD16T_CORE_H
#define QOCX_LINDBLAD16T_CORE_H

#include "qocx_lindblad4t_core.h"  // (the tableau in constant memory: lindblad4t::RK)

namespace qocx {

namespace lindblad16t {

using namespace tilewave;
using lindblad4t::RK;

// 33 <= n <= 64: sixteen waves, wave w owns tile (w & 3, w >> 2) of every 64 x 64 matrix
struct G64T {
    static constexpr int NP = 64, IMG = 64, WAVES = 16, NTW = 1;
    static __device__ __forceinline__ int ti(int i, int w) { return w & 3; }
    static __device__ __forceinline__ int tj(int w) { return w >> 2; }
};

typedef G64T G;
typedef Tile<G> T;
typedef Wave<G> W;  // (store / load / cimg; its products keep whole fragment columns in registers: not used)
typedef Dim<G> D;

constexpr int STAGES = QOCX_RK_STAGES;
constexpr int MAT = D::IMAT;  // complex elements of a C-dump
constexpr int MAX_OPS = LINDBLAD_TILE16_MAX_OPS;  // the operators are read from memory: the engine's limit

// LDS matrices (pitch 65): the argument of the right-hand side, and one temporary - t_i = gamma_i L_i Y of
// the operator at hand, then the stage value of the control-cotangent products. Behind them the partial
// sums of a reduction [parity][wave] and of the control cotangents [wave][2][8].
enum { M_ARG = 0, M_T = 1, M_COUNT = 2 };
constexpr int RED_OFF = M_COUNT * D::MBYTES;
constexpr int GRED_OFF = RED_OFF + 2 * G::WAVES * 16;
constexpr int LDS_BYTES = GRED_OFF + G::WAVES * 2 * QOCX_LINDBLAD_MAX_K * 8;
static_assert(LDS_BYTES <= 160 * 1024, "one seed per CU");

// Per-seed scratch (C-dumps): [S] densities, [S] cotangents, [STAGES] k_j / Ybar_j, [STAGES] stage values
// recomputed from a checkpoint, the six generator images of the sub-interval at hand, the cotangent under
// construction. (qocx_lindblad16t.hip: lindblad16t_scratch_elems)
enum { GEN_LA = 0, GEN_LAH, GEN_LD, GEN_LDH, GEN_RA, GEN_RAH, GEN_COUNT };
constexpr int SCRATCH_EXTRA = 2 * STAGES + GEN_COUNT + 1;

struct Ctx {
    const LindbladArgs& a;
    W wv;
    double2* red;
    double* gred;
    int parity;
    int kt;     // tiles along k of a product: ceil(n / 16); everything behind is padding
    unsigned dump_off, fa_off, fb_off;  // byte offsets of the lane: its tile in a dump, its fragments (frag_a / frag_b)
    bool live;  // this wave's tile holds elements of the matrix (else: padding only, its products are zero)

    // Every access to memory is a uniform base plus a 32-bit byte offset of the lane plus a constant: the
    // form the load and store instructions take as it stands (base in scalar registers), so no per-lane
    // 64-bit address is ever formed - hoisted out of the loops, those were what spilled.
    // (the empty asm makes the lane's offset opaque at every use, so base + offset is formed where it is used;
    // `fixed`, a constant, goes into the instruction's immediate)
    static __device__ __forceinline__ double2 ldg(const double2* base, unsigned lane_bytes, int fixed) {
        asm volatile("" : "+v"(lane_bytes));
        return *reinterpret_cast<const double2*>(reinterpret_cast<const char*>(base) + fixed + (size_t)lane_bytes);
    }
    static __device__ __forceinline__ void stg(double2* base, unsigned lane_bytes, int fixed, double2 v) {
        asm volatile("" : "+v"(lane_bytes));
        *reinterpret_cast<double2*>(reinterpret_cast<char*>(base) + fixed + (size_t)lane_bytes) = v;
    }
    // component r of this wave's tile in a C-dump: element cimg(0, r) = cimg(0, 0) + 64 r
    __device__ __forceinline__ T load_dump(const double2* d) const {
        T t;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const double2 e = ldg(d, dump_off, r * 1024);
            t.re[0][r] = e.x;
            t.im[0][r] = e.y;
        }
        return t;
    }
    __device__ __forceinline__ void store_dump(const T& t, double2* d) const {
#pragma unroll
        for (int r = 0; r < 4; ++r) stg(d, dump_off, r * 1024, make_double2(t.re[0][r], t.im[0][r]));
    }
    // the sum over the workgroup of a complex scalar, in every lane (one barrier): the sixteen waves'
    // partial sums in one fixed order
    __device__ __forceinline__ void block_sum(double& re, double& im) {
        re = wave_sum(re);
        im = wave_sum(im);
        double2* slot = red + parity * G::WAVES;
        parity ^= 1;
        if (wv.lane == 0) slot[wv.w] = make_double2(re, im);
        __syncthreads();
        re = 0;
        im = 0;
#pragma unroll
        for (int w = 0; w < G::WAVES; ++w) {
            const double2 s = slot[w];
            re += s.x;
            im += s.y;
        }
    }
    // tr(X^H Y): this wave's share
    static __device__ __forceinline__ void frob_part(const T& x, const T& y, double& re, double& im) {
        re = 0;
        im = 0;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            re += x.re[0][r] * y.re[0][r] + x.im[0][r] * y.im[0][r];
            im += x.re[0][r] * y.im[0][r] - x.im[0][r] * y.re[0][r];
        }
    }
    static __device__ __forceinline__ void add_scaled(T& l, double zr, double zi, const T& t) {
        l.re[0] += zr * t.re[0] - zi * t.im[0];
        l.im[0] += zr * t.im[0] + zi * t.re[0];
    }

    // Density costs on the S densities in `dens` (dumps in memory); optionally adds the cotangents into
    // `lam` (qoc/standard/costs/targetdensityinfidelity.py:41-69, forbiddensities.py:53-85): as costs() of
    // qocx_lindblad4t_core.h, the traces summed over the sixteen tiles.
    __device__ __forceinline__ double costs(bool step_pass, bool final_pass, const double2* dens, double2* lam) {
        const int S = a.S, n = a.n;
        double total = 0;
        for (int ci = 0; ci < a.cost_count; ++ci) {
            const DevCost c = a.costs[ci];
            const bool on = c.step_cost ? step_pass : final_pass;
            if (!on) continue;
            const double2* pool = a.cost_matrices + (size_t)c.vec_offset * MAT;
            if (c.kind == QOCX_DEV_COST_TARGET_DENSITY) {
                double fid = 0;
                for (int s = 0; s < S; ++s) {
                    const T t = load_dump(pool + (size_t)s * MAT);
                    const T rho = load_dump(dens + (size_t)s * MAT);
                    double zr, zi;
                    frob_part(t, rho, zr, zi);
                    block_sum(zr, zi);
                    const double mag = sqrt(zr * zr + zi * zi);
                    fid += mag;
                    if (lam != nullptr && mag > 0) {
                        const double f = -c.scale / ((double)S * n * mag);
                        T l = load_dump(lam + (size_t)s * MAT);
                        add_scaled(l, f * zr, f * zi, t);
                        store_dump(l, lam + (size_t)s * MAT);
                    }
                }
                total += c.scale * (1.0 - fid / ((double)S * n));
            } else {  // QOCX_DEV_COST_FORBID_DENSITY
                int base = 0;
                double acc = 0;
                for (int s = 0; s < S; ++s) {
                    const int fs = a.cost_counts[c.cnt_offset + s];
                    // (one matrix at a time beside the density: the cotangent is read, added to and written
                    // back per forbidden matrix instead of being carried in registers)
                    for (int f = 0; f < fs; ++f) {
                        const T t = load_dump(pool + (size_t)(base + f) * MAT);
                        double zr, zi;
                        frob_part(t, load_dump(dens + (size_t)s * MAT), zr, zi);
                        block_sum(zr, zi);
                        zr /= n;
                        zi /= n;
                        acc += (zr * zr + zi * zi) / fs;
                        if (lam != nullptr) {
                            const double g = 2.0 * c.scale / ((double)fs * n);
                            T l = load_dump(lam + (size_t)s * MAT);
                            add_scaled(l, g * zr, g * zi, t);
                            store_dump(l, lam + (size_t)s * MAT);
                        }
                    }
                    base += fs;
                }
                total += c.scale * acc;
            }
        }
        return total;
    }

    // ---- operand fragments of v_mfma_f64_16x16x4_f64: lane (q, c) supplies A[16 ti + c][4 kk + q] and
    // B[4 kk + q][16 tj + c].
    // From a C-dump in memory: element (4 kk + q, 16 t + c) of the dumped matrix is component kk & 3 of tile
    // (kk >> 2, t) in lane 16 q + c, at ((kk >> 2) 16 + (kk & 3) + 4 t) 64 + lane - the B fragment of k-step kk
    // and column tile t is 64 consecutive elements, one coalesced KiB. The A fragment of a matrix M is the
    // conjugate of the same read from the dump of M^H, so every matrix that is a left operand has the dump
    // of its conjugate transpose beside it.
    // k-step kk = 4 k4 + u: k4 moves the uniform base, u is a constant of the unrolled loop.
    __device__ __forceinline__ double2 frag_a(const double2* dump, int k4, int u) const {  // row tile ti
        return ldg(dump + (size_t)k4 * 1024, fa_off, u * 1024);
    }
    __device__ __forceinline__ double2 frag_b(const double2* dump, int k4, int u) const {  // column tile tj
        return ldg(dump + (size_t)k4 * 1024, fb_off, u * 1024);
    }
    static __device__ __forceinline__ double2 conj2(double2 v) { return make_double2(v.x, -v.y); }
    // from an LDS matrix
    __device__ __forceinline__ double2 lds_a(const double2* m, int k4, int u) const {
        return m[(16 * wv.ti(0) + wv.c) * D::PM + wv.q + 16 * k4 + 4 * u];
    }
    __device__ __forceinline__ double2 lds_b(const double2* m, int k4, int u) const {
        return m[wv.q * D::PM + 16 * wv.tj() + wv.c + (16 * k4 + 4 * u) * D::PM];
    }
    __device__ __forceinline__ double2 lds_ah(const double2* m, int k4, int u) const {  // A = M^H
        return conj2(m[wv.q * D::PM + 16 * wv.ti(0) + wv.c + (16 * k4 + 4 * u) * D::PM]);
    }
    __device__ __forceinline__ double2 lds_bh(const double2* m, int k4, int u) const {  // B = M^H
        return conj2(m[(16 * wv.tj() + wv.c) * D::PM + wv.q + 16 * k4 + 4 * u]);
    }

    // acc += sign * A B, this wave's tile, the fragments of k-step 4 k4 + u from fa(k4, u), fb(k4, u);
    // three real products per complex one. The k-loop stays rolled in fours: operand fragments of a whole
    // 64-column would be 128 registers, all a wave has here.
    template <class FA, class FB>
    __device__ __forceinline__ void mm(T& acc, double sign, FA fa, FB fb) const {
        d4 t1 = {0, 0, 0, 0}, t2 = {0, 0, 0, 0}, t3 = {0, 0, 0, 0};
#pragma unroll 1
        for (int k4 = 0; k4 < kt; ++k4) {
            double2 x[4], y[4];  // the four k-steps' fragments are asked for before the first is used
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                x[u] = fa(k4, u);
                y[u] = fb(k4, u);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                t1 = mfma_f64(x[u].x, y[u].x, t1);
                t2 = mfma_f64(x[u].y, y[u].y, t2);
                t3 = mfma_f64(x[u].x + x[u].y, y[u].x + y[u].y, t3);
            }
        }
        acc.re[0] += sign * (t1 - t2);
        acc.im[0] += sign * (t3 - t1 - t2);
    }

    // The generators of a sub-interval, linear in the stage's position c (the controls are linear in time
    // between knots): left(c) = LA + c LD, right(c) = RA - c LD with LA = A0L + sum u_a Gp_k,
    // RA = A0R - sum u_a Gp_k, LD = sum (u_b - u_a) Gp_k; their conjugate transposes are the generators of
    // the adjoint stage and the left-operand images of the forward one. Six dumps in the seed's scratch,
    // every wave its tile; a workgroup barrier before (the last products have read the old ones) and after.
    __device__ __forceinline__ void form_generators(const SubStep& ss, const double* ctl, double2* gen) const {
        __syncthreads();
        // one image at a time (six tiles at once are 96 registers): base + sum_k (fa u_a + fd (u_b - u_a)) G_k
        auto form = [&](const double2* base, const double2* gk, double fa, double fd, int which) {
            T t = tile_zero<G>();
            if (base != nullptr) t = load_dump(base);
            const int K = a.K;
#pragma unroll 1
            for (int k = 0; k < K; ++k) {
                const double ua = ss.wa1 * ctl[(size_t)ss.ia1 * K + k] + ss.wa2 * ctl[(size_t)ss.ia2 * K + k];
                const double ub = ss.wb1 * ctl[(size_t)ss.ib1 * K + k] + ss.wb2 * ctl[(size_t)ss.ib2 * K + k];
                tile_axpy<G>(t, fa * ua + fd * (ub - ua), load_dump(gk + (size_t)k * MAT));
            }
            store_dump(t, gen + (size_t)which * MAT);
        };
        form(a.a0l_cimg, a.gp_cimg, 1.0, 0.0, GEN_LA);
        form(a.a0ld_cimg, a.gpd_cimg, 1.0, 0.0, GEN_LAH);
        form(nullptr, a.gp_cimg, 0.0, 1.0, GEN_LD);
        form(nullptr, a.gpd_cimg, 0.0, 1.0, GEN_LDH);
        form(a.a0r_cimg, a.gp_cimg, -1.0, 0.0, GEN_RA);
        form(a.a0rd_cimg, a.gpd_cimg, -1.0, 0.0, GEN_RAH);
        __syncthreads();
    }

    // out = left(c) y + y right(c) + sum_i gamma_i L_i y L_i^H (ADJ: the generators' conjugate transposes
    // and L_i^H y L_i). y goes to M_ARG and stays there; the generators and the operators come from memory
    // as fragments; t_i = gamma_i L_i y goes through M_T, one operator at a time: two workgroup barriers
    // for the argument, two more per operator behind the first.
    template <bool ADJ>
    __device__ __forceinline__ T rhs(const T& y, const double2* gen, double c) const {
        const int nops = a.nops;
        const double2* arg = wv.mat(M_ARG);
        const double2* tm = wv.mat(M_T);
        __syncthreads();  // the products of the stage before have read M_ARG and M_T
        wv.store(y, M_ARG);
        __syncthreads();
        T acc = tile_zero<G>();
        if (live) {
            // left operand M = left(c) (ADJ: left(c)^H): the conjugate of the dump of M^H
            const double2* pa = gen + (size_t)(ADJ ? GEN_LA : GEN_LAH) * MAT;
            const double2* pd = gen + (size_t)(ADJ ? GEN_LD : GEN_LDH) * MAT;
            mm(acc, 1.0,
               [&](int k4, int u) {
                   const double2 x = frag_a(pa, k4, u), v = frag_a(pd, k4, u);
                   return make_double2(fma(c, v.x, x.x), -fma(c, v.y, x.y));
               },
               [&](int k4, int u) { return lds_b(arg, k4, u); });
            const double2* qa = gen + (size_t)(ADJ ? GEN_RAH : GEN_RA) * MAT;
            const double2* qd = gen + (size_t)(ADJ ? GEN_LDH : GEN_LD) * MAT;
            mm(acc, 1.0, [&](int k4, int u) { return lds_a(arg, k4, u); },
               [&](int k4, int u) {
                   const double2 x = frag_b(qa, k4, u), v = frag_b(qd, k4, u);
                   return make_double2(fma(-c, v.x, x.x), fma(-c, v.y, x.y));
               });
        }
#pragma unroll 1
        for (int i = 0; i < nops; ++i) {
            // [nops] dumps of L_i, then [nops] of L_i^H
            const double2* op = a.op_cimg + (size_t)i * MAT;
            const double2* oph = a.op_cimg + (size_t)(nops + i) * MAT;
            T t = tile_zero<G>();
            if (live) {
                const double2* left = ADJ ? op : oph;  // left operand L_i (ADJ: L_i^H), from the other one's dump
                mm(t, a.gammas[i], [&](int k4, int u) { return conj2(frag_a(left, k4, u)); },
                   [&](int k4, int u) { return lds_b(arg, k4, u); });
            }
            if (i > 0) __syncthreads();  // t_(i-1) has been read
            wv.store(t, M_T);
            __syncthreads();
            if (live) {
                const double2* right = ADJ ? op : oph;  // right operand L_i^H (ADJ: L_i)
                mm(acc, 1.0, [&](int k4, int u) { return lds_a(tm, k4, u); },
                   [&](int k4, int u) { return frag_b(right, k4, u); });
            }
        }
        return acc;
    }
};

}  // namespace lindblad16t

}  // namespace qocx

#endif  // QOCX_LINDBLAD16T_CORE_H
