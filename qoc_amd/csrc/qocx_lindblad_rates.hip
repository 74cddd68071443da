// qocx_lindblad_rates.hip - the Lindblad engine at n <= 32 (qocx_lindblad_core.h) for an ensemble with
// per-member dissipation rates (qocx_lindblad_set_ensemble_rates): the bodies of qocx_lindblad.hip's kernels
// behind a member table. The A0 dumps and the rates are those of the workgroup's member, folded into the
// base pointers once, before run() - every read of a.a0*_cimg (the constant cache, cache_gen, the Q2 / CH
// copies) and of a.gammas (rhs, the one-wave and several-wave stage loops, substep_q2, chain_jobs) then
// finds its member's; nothing is added inside a stage. A file and a code object of its own: every run
// without rates launches, from qocx_lindblad.hip, the kernels it launched before this file existed. The
// combine kernels read neither A0 nor rates; launch_lindblad_combine serves both.
#include "qocx_lindblad_core.h"

namespace qocx {

namespace {

template <int LNB, bool GS, bool MW, bool MW4, bool STAMP = false, bool Q2 = false, bool CH = false>
__global__ __launch_bounds__(MW ? (MW4 ? 256 : 384) : 64) void lindblad_rates_kernel(LindbladArgs a,
                                                                                   LindbladMembers mem) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    mem.select(a);
    LB<LNB, GS, MW, (LNB == 1 && !GS && !MW), STAMP, MW4, Q2, CH>::run(a, smem);
}

struct LaunchRates {  // (lindblad_dispatch)
    const LindbladArgs& a;
    const LindbladMembers& mem;
    int batch;
    hipStream_t st;
    template <int LNB, bool GS, bool MW, bool MW4, bool STAMP, bool Q2, bool CH>
    void operator()(int bytes, int threads) const {
        (void)hipFuncSetAttribute(
            reinterpret_cast<const void*>(lindblad_rates_kernel<LNB, GS, MW, MW4, STAMP, Q2, CH>),
            hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
        hipLaunchKernelGGL((lindblad_rates_kernel<LNB, GS, MW, MW4, STAMP, Q2, CH>), dim3(batch), dim3(threads), bytes,
                           st, a, mem);
    }
};

}  // namespace

// (33 <= n <= 64 has no kernel with a member table: the setters refuse rates there, and so does this)
int launch_lindblad_rates(LindbladKernel kernel, bool stamped, const LindbladArgs& a, const LindbladMembers& mem,
                          int batch, hipStream_t st) {
    switch (kernel) {
    case LindbladKernel::NONE:
    case LindbladKernel::TILE16: return 1;
    case LindbladKernel::TILE4:
    case LindbladKernel::TILE4_HERM:
        launch_lindblad4t_rates(kernel == LindbladKernel::TILE4_HERM, a, mem, batch, st);
        return 0;
    default: return lindblad_dispatch(kernel, stamped, a, LaunchRates{a, mem, batch, st}) ? 0 : 1;
    }
}

}  // namespace qocx
