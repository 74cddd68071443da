// qocx_lindblad4t_rates.hip - the tile-per-wave Lindblad kernel (qocx_lindblad4t.hip, 17 <= n <= 32) for an
// ensemble with per-member dissipation rates (qocx_lindblad_set_ensemble_rates). The A0 dumps and the rates
// are those of the workgroup's member, folded into the base pointers once, before anything reads them
// (load_dump of a0l / a0r / a0ld / a0rd_cimg in Ctx::generators and `gam = a.gammas` in Ctx::rhs); nothing
// is added inside a stage. A file and a code object of its own: every run without rates launches, from
// qocx_lindblad4t.hip, the kernels it launched before this file existed. lindblad4t_combine_kernel reads
// neither A0 nor rates and serves both.
#include "qocx_lindblad4t_core.h"

namespace qocx {

namespace lindblad4t {

template <bool HERM>
__global__ __launch_bounds__(256) void lindblad4t_rates_kernel(LindbladArgs a, LindbladMembers mem) {
    mem.select(a);
#include "qocx_lindblad4t_body.inc"
}

}  // namespace lindblad4t

void launch_lindblad4t_rates(bool hermitian, const LindbladArgs& a, const LindbladMembers& mem, int batch,
                             hipStream_t st) {
    static bool attr_set = false;
    if (!attr_set) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(lindblad4t::lindblad4t_rates_kernel<false>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, lindblad4t::LDS_BYTES);
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(lindblad4t::lindblad4t_rates_kernel<true>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, lindblad4t::LDS_BYTES);
        attr_set = true;
    }
    if (hermitian)
        hipLaunchKernelGGL(lindblad4t::lindblad4t_rates_kernel<true>, dim3(batch), dim3(256), lindblad4t::LDS_BYTES, st,
                           a, mem);
    else
        hipLaunchKernelGGL(lindblad4t::lindblad4t_rates_kernel<false>, dim3(batch), dim3(256), lindblad4t::LDS_BYTES,
                           st, a, mem);
}

}  // namespace qocx
