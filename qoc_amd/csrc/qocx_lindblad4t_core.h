// qocx_lindblad4t_core.h - what the tile-per-wave Lindblad kernels share (qocx_lindblad4t.hip: the kernels
// every run without per-member rates launches; qocx_lindblad4t_rates.hip: the same body behind a member
// table): the LDS layout, the tableau, the per-wave context with the costs and the right-hand side. The
// kernel's body itself is qocx_lindblad4t_body.inc.
#ifndef QOCX_LINDBLAD4T_CORE_H
#define QOCX_LINDBLAD4T_CORE_H

#include "qocx_device.h"
#include "qocx_lindblad_route.h"
#include "qocx_tilewave.h"
#include "dop853_tableau.h"

namespace qocx {

namespace lindblad4t {

using namespace tilewave;

typedef G32 G;
typedef Tile<G> T;
typedef Wave<G> W;
typedef Dim<G> D;

constexpr int STAGES = QOCX_RK_STAGES;
constexpr int MAT = D::IMAT;  // complex elements of a C-dump
constexpr int MAX_OPS = LINDBLAD_TILE4_MAX_OPS;  // (the route sends no launch with more)

// LDS matrices (pitch 33): the argument of the right-hand side, the two generators at the stage's
// time (then t_0, t_1), the operators, the stage value of the control-cotangent products; behind them
// the partial sums of a reduction
// (Hermitian problems: M_GR carries X = A_L Y to the wave that needs its mirror tile, t_1 has M_T1H)
enum { M_ARG = 0, M_GL, M_GR, M_YS, M_T1H, M_OP0, M_COUNT = M_OP0 + MAX_OPS, M_T0 = M_GL, M_T1 = M_GR, M_XS = M_GR };
constexpr int RED_OFF = M_COUNT * D::MBYTES;
constexpr int LDS_BYTES = RED_OFF + 2 * 4 * 16;  // [parity][wave] of a complex scalar
static_assert(LDS_BYTES <= 160 * 1024, "one seed per CU");

// the Butcher tableau in constant memory (runtime-indexed by the rolled stage loops)
struct TableauInit {
    double a[STAGES * STAGES], b[STAGES], c[STAGES];
    constexpr TableauInit() : a(), b(), c() {
        for (int i = 0; i < STAGES; ++i) {
            b[i] = QOCX_RK_B[i];
            c[i] = QOCX_RK_C[i];
            for (int j = 0; j < STAGES; ++j) a[i * STAGES + j] = QOCX_RK_A[i][j];
        }
    }
};
__device__ __constant__ const TableauInit RK = TableauInit{};

struct Ctx {
    const LindbladArgs& a;
    W wv;
    double2* red;
    int parity;

    __device__ __forceinline__ T load_dump(const double2* d) const {
        T t;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const double2 e = d[wv.cimg(0, r)];
            t.re[0][r] = e.x;
            t.im[0][r] = e.y;
        }
        return t;
    }
    __device__ __forceinline__ void store_dump(const T& t, double2* d) const {
#pragma unroll
        for (int r = 0; r < 4; ++r) d[wv.cimg(0, r)] = make_double2(t.re[0][r], t.im[0][r]);
    }
    // the sum over the workgroup of a complex scalar, in every lane (one barrier)
    __device__ __forceinline__ void block_sum(double& re, double& im) {
        re = wave_sum(re);
        im = wave_sum(im);
        double2* slot = red + parity * 4;
        parity ^= 1;
        if (wv.lane == 0) slot[wv.w] = make_double2(re, im);
        __syncthreads();
        const double2 s0 = slot[0], s1 = slot[1], s2 = slot[2], s3 = slot[3];
        re = (s0.x + s1.x) + (s2.x + s3.x);
        im = (s0.y + s1.y) + (s2.y + s3.y);
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

    // Density costs on the S densities in `dens` (HBM dumps); optionally adds the cotangents into
    // `lam` (qoc/standard/costs/targetdensityinfidelity.py:41-69, forbiddensities.py:53-85): as
    // density_costs of qocx_lindblad.hip, the traces summed over the four tiles.
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
                    const T rho = load_dump(dens + (size_t)s * MAT);
                    T l = tile_zero<G>();
                    if (lam != nullptr) l = load_dump(lam + (size_t)s * MAT);
                    for (int f = 0; f < fs; ++f) {
                        const T t = load_dump(pool + (size_t)(base + f) * MAT);
                        double zr, zi;
                        frob_part(t, rho, zr, zi);
                        block_sum(zr, zi);
                        zr /= n;
                        zi /= n;
                        acc += (zr * zr + zi * zi) / fs;
                        if (lam != nullptr) {
                            const double g = 2.0 * c.scale / ((double)fs * n);
                            add_scaled(l, g * zr, g * zi, t);
                        }
                    }
                    if (lam != nullptr) store_dump(l, lam + (size_t)s * MAT);
                    base += fs;
                }
                total += c.scale * acc;
            }
        }
        return total;
    }

    // the generators of a sub-interval, linear in the stage's position c (the controls are linear in
    // time between knots): left(c) = la + c ld, right(c) = ra - c ld
    struct Gen {
        T la, ld, ra;
    };
    __device__ __forceinline__ Gen generators(const SubStep& ss, const double* ctl, bool adjoint) const {
        Gen g;
        g.la = load_dump(adjoint ? a.a0ld_cimg : a.a0l_cimg);
        g.ra = load_dump(adjoint ? a.a0rd_cimg : a.a0r_cimg);
        g.ld = tile_zero<G>();
        const int K = a.K;
        for (int k = 0; k < K; ++k) {
            const double ua = ss.wa1 * ctl[(size_t)ss.ia1 * K + k] + ss.wa2 * ctl[(size_t)ss.ia2 * K + k];
            const double ub = ss.wb1 * ctl[(size_t)ss.ib1 * K + k] + ss.wb2 * ctl[(size_t)ss.ib2 * K + k];
            const T gk = load_dump((adjoint ? a.gpd_cimg : a.gp_cimg) + (size_t)k * MAT);
            tile_axpy<G>(g.la, ua, gk);
            tile_axpy<G>(g.ra, -ua, gk);
            tile_axpy<G>(g.ld, ub - ua, gk);
        }
        return g;
    }

    // out = left(c) y + y right(c) + sum_i gamma_i L_i y L_i^H (ADJ: L_i^H y L_i; the generators are
    // then the conjugate transposes already). The operators go in pairs: t_i = gamma_i L_i y into the
    // slots of the generators, a barrier, t_i L_i^H - three workgroup barriers for up to two operators,
    // five for up to four (one more in the forward stage); y stays in M_ARG afterwards.
    // HERM (host-checked: y Hermitian, right = left^H): y right = (left y)^H - one product less, the
    // mirror tile of X = left y comes from its owner through LDS.
    // `stage` = sub-interval index * STAGES + stage index: selects the time samples of a time-dependent
    // Hamiltonian (a0_tab: A0L, A0R, A0L^H, A0R^H per stage; gp_tab: Gp, Gp^H, Gp^T per stage and
    // control) and of time-dependent lindblad_data (op_tab, gamma_tab) when the host supplied them
    // (qocx_lindblad.hip: build_generator, rhs_split); such problems take the general stages.
    template <bool ADJ, bool HERM>
    __device__ __forceinline__ T rhs(const T& y, const Gen& g, double c, const SubStep& ss, const double* ctl,
                                     size_t stage) const {
        const int nops = a.nops;
        const double* gam = a.gammas;
        T gl, gr;
        if (!HERM && a.a0_tab != nullptr) {
            const double2* t = a.a0_tab + stage * 4 * MAT;
            gl = load_dump(t + (ADJ ? 2 : 0) * (size_t)MAT);
            gr = load_dump(t + (ADJ ? 3 : 1) * (size_t)MAT);
            const int K = a.K;
            for (int k = 0; k < K; ++k) {
                const double ua = ss.wa1 * ctl[(size_t)ss.ia1 * K + k] + ss.wa2 * ctl[(size_t)ss.ia2 * K + k];
                const double ub = ss.wb1 * ctl[(size_t)ss.ib1 * K + k] + ss.wb2 * ctl[(size_t)ss.ib2 * K + k];
                const double u = (1.0 - c) * ua + c * ub;  // u(t) is linear inside a sub-interval
                const T gk = a.gp_tab != nullptr ? load_dump(a.gp_tab + ((stage * K + k) * 3 + (ADJ ? 1 : 0)) * MAT)
                                                 : load_dump((ADJ ? a.gpd_cimg : a.gp_cimg) + (size_t)k * MAT);
                tile_axpy<G>(gl, u, gk);
                tile_axpy<G>(gr, -u, gk);
            }
        } else {
            gl = g.la;
            tile_axpy<G>(gl, c, g.ld);
            if (!HERM) {
                gr = g.ra;
                tile_axpy<G>(gr, -c, g.ld);
            }
        }
        // (the last products of the previous stage read t_i from the generators' slots - and the
        // operators; the adjoint stage ends with a barrier of its own)
        if (!ADJ) __syncthreads();
        if (!HERM && a.op_tab != nullptr) {  // this stage's L_i(t), gamma_i(t)
            for (int i = 0; i < nops; ++i) wv.store(load_dump(a.op_tab + (stage * nops + i) * MAT), M_OP0 + i);
            gam = a.gamma_tab + stage * nops;
        }
        wv.store(y, M_ARG);
        wv.store(gl, M_GL);
        if (!HERM) wv.store(gr, M_GR);
        __syncthreads();
        T acc = tile_zero<G>();
        wv.template mm<false, false>(acc, M_GL, M_ARG, 1.0);
        int first = 0;  // the first operator of the pair loop below
        if (HERM) {
            wv.store(acc, M_XS);
            T t0 = tile_zero<G>();
            if (nops > 0) wv.template mm<ADJ, false>(t0, M_OP0, M_ARG, gam[0]);
            if (nops > 1) {
                T t1 = tile_zero<G>();
                wv.template mm<ADJ, false>(t1, M_OP0 + 1, M_ARG, gam[1]);
                wv.store(t1, M_T1H);
            }
            __syncthreads();  // X complete; the generator has been read: t_0 takes its place
            tile_axpy<G>(acc, 1.0, wv.load_adjoint(M_XS));
            if (nops == 0) return acc;
            wv.store(t0, M_T0);
            __syncthreads();
            wv.template mm<false, !ADJ>(acc, M_T0, M_OP0, 1.0);
            if (nops > 1) wv.template mm<false, !ADJ>(acc, M_T1H, M_OP0 + 1, 1.0);
            first = 2;
        } else {
            wv.template mm<false, false>(acc, M_ARG, M_GR, 1.0);
        }
        const int second_slot = HERM ? M_T1H : M_T1;
#pragma unroll 1
        for (int i = first; i < nops; i += 2) {
            __syncthreads();  // the generators (the previous pair's t_i) have been read
            {
                T t = tile_zero<G>();
                wv.template mm<ADJ, false>(t, M_OP0 + i, M_ARG, gam[i]);
                wv.store(t, M_T0);
            }
            if (i + 1 < nops) {
                T t = tile_zero<G>();
                wv.template mm<ADJ, false>(t, M_OP0 + i + 1, M_ARG, gam[i + 1]);
                wv.store(t, second_slot);
            }
            __syncthreads();
            wv.template mm<false, !ADJ>(acc, M_T0, M_OP0 + i, 1.0);
            if (i + 1 < nops) wv.template mm<false, !ADJ>(acc, second_slot, M_OP0 + i + 1, 1.0);
        }
        return acc;
    }
};

}  // namespace lindblad4t

}  // namespace qocx

#endif  // QOCX_LINDBLAD4T_CORE_H
