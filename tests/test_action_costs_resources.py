"""
Resource budgets of the matrix-free kernels under step costs and several costs
(qoc_amd/csrc/qocx_action_costs.hip), in the style of tests/test_action_states_resources.py: compiled for
gfx950 with the resource remarks on, no GPU needed. The sweep wave holds H0, two G_k and the step generator
in registers and must not spill, with the cost code of qocx_sweep_common.h inlined three times beside the
step; a gradient wave must fit beside it (512 registers per SIMD), three gradient waves must share a SIMD,
and the sweep's LDS - the state the cost code reads and the cotangent it adds to - must leave room for them.
"""
from tests.test_build_resources import find, resources, total_registers


def test_action_costs_kernels_keep_their_budgets():
    table = resources("qocx_action_costs.hip")
    sweep = find(table, "action_costs_sweep_kernelILi2ELi2E")
    grad = find(table, "action_costs_grad_kernelILi2E")
    for entry in (sweep, grad):
        assert entry["ScratchSize"] == 0 and entry["VGPRs Spill"] == 0 and entry["SGPRs Spill"] == 0, entry
    granule = lambda r: (r + 7) // 8 * 8  # noqa: E731  (allocation granularity)
    assert granule(total_registers(grad)) * 3 <= 512 and grad["Occupancy"] >= 3
    assert granule(total_registers(sweep)) + granule(total_registers(grad)) <= 512
    assert sweep["LDS Size"] <= 4096
