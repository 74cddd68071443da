// qocx_action_eff.hip - the matrix-free route (qocx_action.hip) on EFFECTIVE controls (qocx_effctl.hip; knob
// "action_eff" = 1): M4 on a time-independent system and Hamiltonians quadratic in the controls have a step
// generator a_j = -i dt (H0 + sum_e v_e(j) G^_e) that is linear in Ke effective controls over an augmented
// operator set - a plain Hermitian problem with one row of Ke controls per step, which is what the
// matrix-free sweeps and gradient kernels consume. Here:
//   effective_table_kernel  one thread per (seed, step): the Ke effective controls of the step into veff
//     (the bits the controls kernels of qocx_effctl.hip write: one definition, qocx_effctl.h) and the step
//     word with the Taylor degree from |dt| (||H0|| + sum_e |v_e| ||G^_e||) in the 1-norm and over the
//     spectral bounds. One launch in place of the controls kernel and a table launch; the sweeps read veff
//     as their step controls, nothing copies it.
//   action_eff_sweep_kernel<KE>  the sweeps of 17 <= n <= 32 (qocx_action_sweep.h) with the control count a
//     constant and all KE operator images in registers beside H0: the streamed build reads KE - 2 images
//     of 16 KB per step and direction.
#include <type_traits>
#include "qocx_effctl.h"
#include "qocx_action_sweep.h"

namespace qocx {

namespace action_eff {

// the step word in the layout of step_table_kernel (qocx_kernels.hip): the Pade order and the squaring count of
// the same 1-norm bound ride along, though no kernel of this route reads them (the dominance bit stays clear:
// nothing is factored)
__device__ __forceinline__ void write_step_word(const EffTableArgs& t, size_t w, int Ke, const double* v) {
    double bound = t.h0_norm, bound2 = t.h0_norm2;
    for (int e = 0; e < Ke; ++e) {
        const double ve = fabs(v[e]);
        bound = fma(ve, t.norm1[e], bound);
        bound2 = fma(ve, t.norm2[e], bound2);
    }
    bound *= fabs(t.dt);
    bound2 *= fabs(t.dt);
    int sq = 0, order = 13;
    if (!(bound < 1e300)) {  // inf / nan
        atomicOr(t.status, 2);
    } else {
        order = pade_order_for(bound, 0);
        if (order == 13) {
            double th = QOCX_THETA13;
            while (bound > th && sq < 30) {
                th *= 2.0;
                ++sq;
            }
        }
    }
    const int degree = action_degree_rule(bound, bound2, t.degree_rule) << QOCX_STEP_DEGREE_SHIFT;
    t.s_arr[w] = step_entry(sq, order) | degree;
}

// KIND: EffKind below. The arguments of the kind's controls kernel, and the table's.
enum EffKind { M4_LINEAR = 1, QUADRATIC = 2 };
template <int KIND, bool SCALED = false>
__global__ __launch_bounds__(256) void effective_table_kernel(
    std::conditional_t<KIND == M4_LINEAR, M4LinArgs, QuadArgs> args, EffTableArgs t) {
    static_assert(KIND == QUADRATIC || !SCALED, "term scales belong to quadratic terms");
    const size_t w = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= args.total) return;
    if constexpr (KIND == M4_LINEAR) {
        QOCX_M4LIN_EFFECTIVE(args, w)
    } else {
        QOCX_QUAD_EFFECTIVE(args, w, SCALED)
    }
    // (read back what this thread has just stored: the values the sweeps will read)
    write_step_word(t, w, args.Ke, args.veff + w * args.Ke);
}

// All KE operator images in registers (KE = 5: M4 with two controls, the headline's control count)
template <int KE>
__global__ __launch_bounds__(64) void action_eff_sweep_kernel(ActionArgs args) {
    __shared__ __attribute__((aligned(16))) double2 turn[Geo<2>::NP];
    action::action_sweep_body<2, KE, true>(args, turn);
}

}  // namespace action_eff

template <class Kernel, class Args>
static void launch_table(Kernel kernel, const Args& a, const EffTableArgs& t, hipStream_t st) {
    if (a.total == 0) return;
    hipLaunchKernelGGL(kernel, dim3((unsigned)((a.total + 255) / 256)), dim3(256), 0, st, a, t);
}
void launch_m4lin_table(const M4LinArgs& a, const EffTableArgs& t, hipStream_t st) {
    launch_table(action_eff::effective_table_kernel<action_eff::M4_LINEAR>, a, t, st);
}
void launch_quad_table(const QuadArgs& a, const EffTableArgs& t, hipStream_t st) {
    if (a.term_scales != nullptr) launch_table((action_eff::effective_table_kernel<action_eff::QUADRATIC, true>), a, t, st);
    else launch_table((action_eff::effective_table_kernel<action_eff::QUADRATIC, false>), a, t, st);
}

bool action_eff_exact_supports(int Ke) { return Ke == 5; }
void launch_action_eff_sweep(const ActionArgs& a, int batch, hipStream_t st) {
    if (batch <= 0 || a.sw.j_end <= a.sw.j_begin) return;
    hipLaunchKernelGGL((action_eff::action_eff_sweep_kernel<5>), dim3(batch), dim3(64), 0, st, a);
}

}  // namespace qocx
