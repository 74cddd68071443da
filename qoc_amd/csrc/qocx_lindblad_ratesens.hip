// qocx_lindblad_ratesens.hip - rate sensitivities of a two-sided Lindblad evaluation: the derivative of a
// seed's cost with respect to the factor c_l of its l-th dissipation rate (rate = c_l gamma_l), the exact
// one of the discrete scheme on its frozen grid (tests/lindblad_sweep_model.py restates it in NumPy):
//
//   dE/dc_l = sum over sub-intervals q, stages i, densities s of
//             Re( conj(c_s) tr( kbar_{i,s}^H  gamma_l ( L_l Y_{i,s} L_l^H - 1/2 (M_l Y_{i,s} + Y_{i,s} M_l) ) ) )
//
// with Y_i the forward stage values (ystages), kbar_i the stage cotangents of the unit adjoint (kbstages;
// the true cotangent is c_s kbar_i with the scalar c_s = lam_scale[b][s], as in the combine kernels),
// gamma_l the PROBLEM's own rate, L_l its operator and M_l = L_l^H L_l (a host-built dump). A sibling of
// lindblad_combine_kernel (qocx_lindblad.hip) and of its tile-per-wave form (qocx_lindblad4t.hip): it
// reads what they read, right after them, before the next piece reuses the stage buffers.
//
// The traces are formed as
//   tr(kbar^H (M Y + Y M)) = <M, Z>,        Z = Y kbar^H + kbar^H Y   (one Z per stage, shared by the l)
//   tr(kbar^H L Y L^H)     = <L^H kbar, Y L^H>   (n <= 16)   = <kbar, (L Y) L^H>   (n > 16)
// with <A, B> = sum conj(A_ij) B_ij; every product runs on v_mfma_f64_16x16x4_f64 through the helpers of
// the stage loops (LB<1> at n <= 16: one wave, the left operand in a planar LDS slot; tilewave::Wave at
// 17 <= n <= 32: four waves, a tile each, both operands in LDS).
//
// Summation order. One partial per (item, sub-interval, l):
//   partial = 0; for stage i = 0 .. 11: for density s = 0 .. S - 1: partial += term(i, s)
// where term(i, s) is a sum over the matrix elements in the fixed tree of wave_sum (n <= 16), or
// accumulated per lane in that loop order and summed over the workgroup once, in the fixed tree of
// block_sum (n > 16). The reduce kernel then adds the partials of an item over the sub-intervals
// q = 0, 1, ... ascending, from +0.0. Nothing depends on the launch (piece sizes, streams, batch).
#include "qocx_lindblad_core.h"
#include "qocx_lindblad4t_core.h"

namespace qocx {

constexpr int RATESENS_MAX_OPS = 4;  // (a two-sided evaluation has at most four operators)

namespace {

// n <= 16: one wave per (sub-interval, item)
__global__ __launch_bounds__(64) void lindblad_ratesens_kernel(LindbladArgs a, RateSensArgs rs) {
    typedef LB<1, false, false> I;
    typedef I::Mat Mat;
    __shared__ __attribute__((aligned(16))) char smem[2 * I::SLOT_BYTES];
    // slot_k: kbar, then the operator L_l; slot_y: Y
    const Slot slot_k = I::slot_at(smem), slot_y = I::slot_at(smem + I::SLOT_BYTES);
    const int q = blockIdx.x, b = blockIdx.y, S = a.S, nsub = a.nsub, L = rs.nops;
    double acc[RATESENS_MAX_OPS];
#pragma unroll
    for (int l = 0; l < RATESENS_MAX_OPS; ++l) acc[l] = 0;
    for (int i = 0; i < STAGES; ++i)
        for (int s = 0; s < S; ++s) {
            const double2 cs = a.lam_scale[(size_t)b * S + s];
            const size_t at = (((((size_t)b * nsub + q) * S + s) * STAGES) + i) * I::MAT;
            Mat y, kb, kbd, z;
            I::dump_load(y, a.ystages + at);
            I::dump_load(kb, a.kbstages + at);
            wave_sync();  // (the slots of the previous term have been read)
            cmat_to_lds<1>(kb, slot_k.re, slot_k.im);
            cmat_to_lds<1>(y, slot_y.re, slot_y.im);
            wave_sync();
            I::load_adjoint(kbd, slot_k);
            I::mat_zero(z);
            I::template gemm<true>(z, slot_k, y);     // kbar^H Y
            I::template gemm<false>(z, slot_y, kbd);  // + Y kbar^H
#pragma unroll
            for (int l = 0; l < RATESENS_MAX_OPS; ++l)
                if (l < L) {
                    Mat m, op, oph, left, right;
                    double t2r, t2i, t1r, t1i;
                    I::dump_load(m, rs.ldl_cimg + (size_t)l * I::MAT);
                    I::frob_inner(m, z, t2r, t2i);  // tr(M Z), M = M^H
                    I::dump_load(op, a.op_cimg + (size_t)l * I::MAT);
                    wave_sync();  // kbar's slot (then the previous operator's) has been read
                    cmat_to_lds<1>(op, slot_k.re, slot_k.im);
                    wave_sync();
                    I::load_adjoint(oph, slot_k);
                    I::mat_zero(right);
                    I::template gemm<false>(right, slot_y, oph);  // Y L^H
                    I::mat_zero(left);
                    I::template gemm<true>(left, slot_k, kb);     // L^H kbar
                    I::frob_inner(left, right, t1r, t1i);         // tr(kbar^H L Y L^H)
                    const double vr = t1r - 0.5 * t2r, vi = t1i - 0.5 * t2i;
                    acc[l] += rs.gammas[l] * fma(cs.y, vi, cs.x * vr);  // Re(conj(c) v)
                }
        }
    if (lane_id() == 0)
#pragma unroll
        for (int l = 0; l < RATESENS_MAX_OPS; ++l)
            if (l < L) rs.partials[((size_t)b * nsub + q) * L + l] = acc[l];
}

// thread (b, l): the partials of item b over its sub-intervals, ascending
__global__ __launch_bounds__(64) void lindblad_ratesens_reduce_kernel(RateSensArgs rs, int nsub, int batch) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x, L = rs.nops;
    if (e >= batch * L) return;
    const int b = e / L, l = e % L;
    double sum = 0.0;
    for (int q = 0; q < nsub; ++q) sum = sum + rs.partials[((size_t)b * nsub + q) * L + l];
    rs.out[(size_t)b * L + l] = sum;
}

}  // namespace

namespace lindblad4t {

// 17 <= n <= 32: four waves per (sub-interval, item), wave w the tile (w & 1, w >> 1) of every matrix.
// LDS matrices: 0 = Y, 1 = kbar (then L_l Y), 2 = L_l.
__global__ __launch_bounds__(256) void lindblad4t_ratesens_kernel(LindbladArgs a, RateSensArgs rs) {
    __shared__ __attribute__((aligned(16))) char smem[3 * D::MBYTES + 2 * 4 * 16];
    Ctx cx{a, make_wave<G>(smem, false), reinterpret_cast<double2*>(smem + 3 * D::MBYTES), 0};
    const W& wv = cx.wv;
    const int q = blockIdx.x, b = blockIdx.y, S = a.S, nsub = a.nsub, L = rs.nops;
    double acc[RATESENS_MAX_OPS];
#pragma unroll
    for (int l = 0; l < RATESENS_MAX_OPS; ++l) acc[l] = 0;
#pragma unroll 1
    for (int i = 0; i < STAGES; ++i)
#pragma unroll 1
        for (int s = 0; s < S; ++s) {
            const double2 cs = a.lam_scale[(size_t)b * S + s];
            const size_t at = (((((size_t)b * nsub + q) * S + s) * STAGES) + i) * MAT;
            const T kb = cx.load_dump(a.kbstages + at);
            wv.store(cx.load_dump(a.ystages + at), 0);
            wv.store(kb, 1);
            __syncthreads();
            T z = tile_zero<G>();
            wv.template mm<false, true>(z, 0, 1, 1.0);  // Y kbar^H
            wv.template mm<true, false>(z, 1, 0, 1.0);  // + kbar^H Y
#pragma unroll
            for (int l = 0; l < RATESENS_MAX_OPS; ++l)
                if (l < L) {
                    double t2r, t2i, t1r, t1i;
                    Ctx::frob_part(cx.load_dump(rs.ldl_cimg + (size_t)l * MAT), z, t2r, t2i);  // tr(M Z): a share
                    __syncthreads();  // matrices 1 and 2 have been read
                    wv.store(cx.load_dump(a.op_cimg + (size_t)l * MAT), 2);
                    __syncthreads();
                    T u = tile_zero<G>();
                    wv.template mm<false, false>(u, 2, 0, 1.0);  // L Y
                    wv.store(u, 1);
                    __syncthreads();
                    T v = tile_zero<G>();
                    wv.template mm<false, true>(v, 1, 2, 1.0);  // (L Y) L^H
                    Ctx::frob_part(kb, v, t1r, t1i);            // tr(kbar^H L Y L^H): a share
                    const double vr = t1r - 0.5 * t2r, vi = t1i - 0.5 * t2i;
                    acc[l] += rs.gammas[l] * fma(cs.y, vi, cs.x * vr);  // Re(conj(c) v)
                }
            __syncthreads();  // the three matrices are free again
        }
#pragma unroll
    for (int l = 0; l < RATESENS_MAX_OPS; ++l)
        if (l < L) {
            double x = acc[l], unused = 0;
            cx.block_sum(x, unused);
            if (wv.tid == 0) rs.partials[((size_t)b * nsub + q) * L + l] = x;
        }
}

}  // namespace lindblad4t

// The partials of `batch` items of one piece and their sums rs.out [batch][L], on `st`. The caller has
// checked 1 <= rs.nops <= 4 and that the piece ran two-sided (ystages, kbstages, lam_scale are its own).
void launch_lindblad_ratesens(const LindbladArgs& a, const RateSensArgs& rs, int batch, hipStream_t st) {
    if (batch <= 0 || a.nsub <= 0 || rs.nops < 1 || rs.nops > RATESENS_MAX_OPS) return;
    if (a.n > 16)
        hipLaunchKernelGGL(lindblad4t::lindblad4t_ratesens_kernel, dim3(a.nsub, batch), dim3(256), 0, st, a, rs);
    else
        hipLaunchKernelGGL(lindblad_ratesens_kernel, dim3(a.nsub, batch), dim3(64), 0, st, a, rs);
    const int total = batch * rs.nops;
    hipLaunchKernelGGL(lindblad_ratesens_reduce_kernel, dim3((total + 63) / 64), dim3(64), 0, st, rs, a.nsub, batch);
}

}  // namespace qocx
