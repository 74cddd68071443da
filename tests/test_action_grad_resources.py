"""
Resource budgets of the gradient kernel of the matrix-free route (qoc_amd/csrc/qocx_action.hip:
action_grad_kernel<2>), in the style of tests/test_action_sweep_exact_resources.py: compiled for gfx950 with the
resource remarks on, no GPU needed.

The kernel is built for FIVE waves to a SIMD: at most 96 registers - so that two of its waves also fit beside a
sweep wave -, no scratch and no spill. Its LDS is dynamic: the rows of the Taylor terms alone, [m_max][32]
double2, since every rho_i overwrites the row of the term it is the last to read. Five waves per SIMD are
twenty per CU; in 160 KiB they fit up to m_max = 16, and at the most the route allows, m_max = 18, seventeen
still do - four per SIMD, one wave more than the [m_max + 2] rows of the kernel before allowed.
"""
import os
import re

from tests.test_build_resources import find, resources, total_registers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS_PER_CU = 160 * 1024
ROW = 32 * 16  # NP double2


def test_gradient_kernel_keeps_five_waves_per_simd():
    table = resources("qocx_action.hip")
    grad = find(table, "action_grad_kernelILi2E")
    exact = find(table, "action_sweep_exact_kernelILi2E")
    assert grad["ScratchSize"] == 0 and grad["VGPRs Spill"] == 0 and grad["SGPRs Spill"] == 0, grad
    granule = lambda r: (r + 7) // 8 * 8  # noqa: E731  (allocation granularity)
    assert granule(total_registers(grad)) <= 96 and grad["Occupancy"] == 5, grad
    assert granule(total_registers(exact)) + 2 * granule(total_registers(grad)) <= 512
    assert grad["LDS Size"] == 0  # (all of it dynamic)


def test_gradient_kernel_lds_is_the_rows_of_the_terms_alone():
    with open(os.path.join(ROOT, "qoc_amd", "csrc", "qocx_action.hip")) as f:
        source = f.read()
    launch = re.search(r"action_grad_kernel<2>\), dim3\(nsteps, batch\), dim3\(64\),\s*([^,]+),", source)
    assert launch and launch.group(1).replace(" ", "") == "a.m_max*Geo<2>::NP*(int)sizeof(double2)", launch
    waves = lambda m_max: LDS_PER_CU // (m_max * ROW)  # noqa: E731
    assert waves(16) >= 20 and waves(18) == 17
