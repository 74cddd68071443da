// qocx_action.h - the degree of the truncated Taylor series that applies exp(a) to a vector
// (qocx_action.hip), shared by the step table (qocx_kernels.hip) and the host's route decision
// (qocx_action_route.h: action_plan).
//
// A. H. Al-Mohy, N. J. Higham, "Computing the action of the matrix exponential, with an application
// to exponential integrators", SIAM J. Sci. Comput. 33 (2011): for ||a||_1 <= theta_m the degree-m
// Taylor polynomial T_m(a) equals exp(a + da) with ||da|| <= 2^-53 ||a|| - the criterion of "Pade
// order by norm" (qocx_wave.h) for another approximant. theta_m for m = 1 .. 18 as SciPy carries
// them (scipy.sparse.linalg._expm_multiply._theta, the paper's Table 3.1 to three digits).
// The generators of this route are normal, and a bound of their 2-norm admits a lower degree by the
// remainder of the series itself (action_degree_normal); a step takes the lesser (action_degree_rule).
#ifndef QOCX_ACTION_H
#define QOCX_ACTION_H

#include <hip/hip_runtime.h>

namespace qocx {

#define QOCX_ACTION_MAX_DEGREE 18
// the most states per seed the matrix-free route takes (qocx_action_states.hip: a wave per state, one per
// SIMD of a CU; knob "action_states")
#define QOCX_ACTION_MAX_STATES 4
// bits 24..29 of a step's entry in s_arr (qocx_wave.h: bits 0..7 squarings, 8..15 Pade order, 16
// dominance): the Taylor degree of the step, 1 .. 18, or 19 - the bound is above theta_18
#define QOCX_STEP_DEGREE_SHIFT 24
#define QOCX_STEP_DEGREE_MASK 0x3f

__host__ __device__ inline double action_theta(int m) {
    switch (m) {
        case 1: return 2.29e-16;
        case 2: return 2.58e-8;
        case 3: return 1.39e-5;
        case 4: return 3.40e-4;
        case 5: return 2.40e-3;
        case 6: return 9.07e-3;
        case 7: return 2.38e-2;
        case 8: return 5.00e-2;
        case 9: return 8.96e-2;
        case 10: return 1.44e-1;
        case 11: return 2.14e-1;
        case 12: return 3.00e-1;
        case 13: return 4.00e-1;
        case 14: return 5.14e-1;
        case 15: return 6.41e-1;
        case 16: return 7.81e-1;
        case 17: return 9.31e-1;
        case 18: return 1.09;
    }
    return 0.0;
}

// the least m with bound <= theta_m; QOCX_ACTION_MAX_DEGREE + 1 above theta_18 (also NaN)
__host__ __device__ inline int action_degree_for(double bound) {
    for (int m = 1; m <= QOCX_ACTION_MAX_DEGREE; ++m)
        if (bound <= action_theta(m)) return m;
    return QOCX_ACTION_MAX_DEGREE + 1;
}

// A NORMAL a (every generator of this route: a = -i dt H, H Hermitian) with ||a||_2 <= beta: the
// eigenvalues i lambda lie on the imaginary axis, |lambda| <= beta, and T_m(a) psi - exp(a) psi is, in
// the eigenbasis, the Lagrange remainder of e^(i lambda): at most beta^(m+1) / (m+1)! ||psi||. Asking
// that to be <= 2^-53 - below one rounding of the state - gives
//     theta'_m = ((m+1)! 2^-53)^(1/(m+1)),
// here each rounded DOWN to a double (theta'_m^(m+1) <= (m+1)! 2^-53 holds in exact arithmetic).
__host__ __device__ inline double action_theta_normal(int m) {
    double t = 0.0;
    switch (m) {
        case 1: t = 1.4901161193847656e-08; break;
        case 2: t = 8.733476581980375e-06; break;
        case 3: t = 0.00022719845192922352; break;
        case 4: t = 0.0016784882105346471; break;
        case 5: t = 0.006563323151782549; break;
        case 6: t = 0.01777016817886154; break;
        case 7: t = 0.038138740273514826; break;
        case 8: t = 0.06998730192918919; break;
        case 9: t = 0.11495221029281477; break;
        case 10: t = 0.17401909444156718; break;
        case 11: t = 0.24763513660365769; break;
        case 12: t = 0.3358381601514265; break;
        case 13: t = 0.43837339055193697; break;
        case 14: t = 0.5547883372015275; break;
        case 15: t = 0.6845053769594961; break;
        case 16: t = 0.8268751230769177; break;
        case 17: t = 0.9812145020859808; break;
        case 18: t = 1.1468331956329982; break;
    }
    return t;
}

// the least m with beta <= theta'_m; QOCX_ACTION_MAX_DEGREE + 1 above theta'_18 (also NaN)
__host__ __device__ inline int action_degree_normal(double beta) {
    for (int m = 1; m <= QOCX_ACTION_MAX_DEGREE; ++m)
        if (beta <= action_theta_normal(m)) return m;
    return QOCX_ACTION_MAX_DEGREE + 1;
}

// The degree of a step. bound1 >= ||a||_1 and bound2 >= ||a||_2 of its generator; rule 1 (knob
// "action_degree", default): the lesser of the two criteria - never above what the 1-norm alone asks
// for; rule 0: the 1-norm alone.
__host__ __device__ inline int action_degree_rule(double bound1, double bound2, int rule) {
    const int m1 = action_degree_for(bound1);
    if (rule == 0) return m1;
    const int m2 = action_degree_normal(bound2);
    return m2 < m1 ? m2 : m1;
}

__host__ __device__ inline int step_degree(int entry) {
    return (entry >> QOCX_STEP_DEGREE_SHIFT) & QOCX_STEP_DEGREE_MASK;
}

}  // namespace qocx

#endif
