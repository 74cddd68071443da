// qocx_action.h - the degree of the truncated Taylor series that applies exp(a) to a vector
// (qocx_action.hip), shared by the step table (qocx_kernels.hip) and the host's route decision
// (qocx_host_resident.hip).
//
// A. H. Al-Mohy, N. J. Higham, "Computing the action of the matrix exponential, with an application
// to exponential integrators", SIAM J. Sci. Comput. 33 (2011): for ||a||_1 <= theta_m the degree-m
// Taylor polynomial T_m(a) equals exp(a + da) with ||da|| <= 2^-53 ||a|| - the criterion of "Pade
// order by norm" (qocx_wave.h) for another approximant. theta_m for m = 1 .. 18 as SciPy carries
// them (scipy.sparse.linalg._expm_multiply._theta, the paper's Table 3.1 to three digits).
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

__host__ __device__ inline int step_degree(int entry) {
    return (entry >> QOCX_STEP_DEGREE_SHIFT) & QOCX_STEP_DEGREE_MASK;
}

}  // namespace qocx

#endif
