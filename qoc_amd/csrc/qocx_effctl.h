// qocx_effctl.h - the effective controls of ONE step (EffCtlArgs, qocx_device.h), the one definition behind
// the controls kernels of qocx_effctl.hip and the step table of qocx_action_eff.hip: whichever of them
// writes veff writes the same bits.
#ifndef QOCX_EFFCTL_H
#define QOCX_EFFCTL_H

#include "qocx_device.h"
#include "qocx_wave.h"

namespace qocx {

// The two bodies are macros, not functions: the controls kernels expand them where their statements stood,
// and compile to the instructions they had before the step table shared them.
//
// M4-linear: v_k, w_k, z_kl of work item w = (seed b, step) into row w of veff.
// mathmethods.py:96-122 with a(t) = -i (H0 + sum u_k(t) G_k).
#define QOCX_M4LIN_EFFECTIVE(args, w)                                                                          \
    const int step = (int)(w % args.nsteps), K = args.K;                                                       \
    const size_t b = w / args.nsteps;                                                                          \
    const double* ctl_b = args.controls + b * args.nc * K;                                                     \
    const StepInterp s1 = args.interp[(size_t)step * 2], s2 = args.interp[(size_t)step * 2 + 1];               \
    double u1[QOCX_M4LIN_MAX_K], u2[QOCX_M4LIN_MAX_K];                                                         \
    double* v = args.veff + w * args.Ke;                                                                       \
    for (int k = 0; k < K; ++k) {                                                                              \
        u1[k] = control_at(ctl_b, s1, K, k);                                                                   \
        u2[k] = control_at(ctl_b, s2, K, k);                                                                   \
        v[k] = 0.5 * (u1[k] + u2[k]);                                                                          \
        v[K + k] = args.f0dt * (u2[k] - u1[k]);                                                                \
    }                                                                                                          \
    int e = 2 * K;                                                                                             \
    for (int k = 0; k < K; ++k)                                                                                \
        for (int l = k + 1; l < K; ++l) v[e++] = args.f0dt * (u2[k] * u1[l] - u2[l] * u1[k]);

// Quadratic: w = [r_k(t_mid), r_kq(t_mid) r_lq(t_mid)] of work item w = (item b of the chunk, step) into row w
// of veff. SCALED (a constant expression): the product times the term scale of the item's member.
// (control_at again rather than a local array indexed by the pair: no scratch, same bits)
#define QOCX_QUAD_EFFECTIVE(args, w, SCALED)                                                                   \
    const int step = (int)(w % args.nsteps), K = args.K;                                                       \
    const size_t b = w / args.nsteps;                                                                          \
    const double* ctl_b = args.controls + b * args.nc * K;                                                     \
    const StepInterp si = args.interp[step];                                                                   \
    double* v = args.veff + w * args.Ke;                                                                       \
    for (int k = 0; k < K; ++k) v[k] = control_at(ctl_b, si, K, k);                                            \
    const double* cm = nullptr; /* the item's member's term scales */                                          \
    (void)cm;                                                                                                  \
    if constexpr (SCALED) cm = args.term_scales + ((args.item0 + b) % (size_t)args.M) * (size_t)args.count;    \
    for (int q = 0; q < args.count; ++q) {                                                                     \
        const double rr =                                                                                      \
            control_at(ctl_b, si, K, args.pairs[2 * q]) * control_at(ctl_b, si, K, args.pairs[2 * q + 1]);     \
        if constexpr (SCALED) v[K + q] = cm[q] * rr;                                                           \
        else v[K + q] = rr;                                                                                    \
    }

// The step table of the matrix-free route on effective controls (qocx_action_eff.hip)
struct EffTableArgs {
    double dt;                 // the bounds are |dt| (h0_norm + sum_e |v_e| norm[e])
    double h0_norm, h0_norm2;  // ||H0||_1 and the bound of ||H0||_2
    const double* norm1;       // [Ke] ||G^_e||_1 of the augmented operators (device memory)
    const double* norm2;       // [Ke] the bounds of ||G^_e||_2, never above norm1
    int degree_rule;           // knob "action_degree" (qocx_action.h: action_degree_rule)
    int* s_arr;                // out: [B][nsteps] the step words (the Taylor degree in bits 24..29)
    int* status;               // bit 1: non-finite bound
};
void launch_m4lin_table(const M4LinArgs& a, const EffTableArgs& t, hipStream_t st);
void launch_quad_table(const QuadArgs& a, const EffTableArgs& t, hipStream_t st);
// ... and the sweeps of 17 <= n <= 32 with the control count a constant and every operator image in registers
// (a.K = 3, 4 or 5 where the build exists: action_eff_exact_supports)
bool action_eff_exact_supports(int Ke);
void launch_action_eff_sweep(const ActionArgs& a, int batch, hipStream_t st);

}  // namespace qocx

#endif
