"""
Resource budgets of the matrix-free kernels for two to four states per seed
(qoc_amd/csrc/qocx_action_states.hip), in the style of tests/test_action_resources.py: compiled for
gfx950 with the resource remarks on, no GPU needed. A sweep wave holds H0, two G_k and the step
generator in registers - the workgroup's waves sit one per SIMD - and must not spill; a gradient wave
must fit beside it (512 registers per SIMD), three gradient waves must share a SIMD, and the sweep's LDS
(the final states of a seed) must leave room for them.
"""
from tests.test_build_resources import find, resources, total_registers


def test_action_states_kernels_keep_their_budgets():
    table = resources("qocx_action_states.hip")
    sweep = find(table, "action_states_sweep_kernelILi2ELi2E")
    grad = find(table, "action_states_grad_kernelILi2E")
    for entry in (sweep, grad):
        assert entry["ScratchSize"] == 0 and entry["VGPRs Spill"] == 0 and entry["SGPRs Spill"] == 0, entry
    granule = lambda r: (r + 7) // 8 * 8  # noqa: E731  (allocation granularity)
    assert granule(total_registers(grad)) * 3 <= 512 and grad["Occupancy"] >= 3
    assert granule(total_registers(sweep)) + granule(total_registers(grad)) <= 512
    assert sweep["LDS Size"] <= 4096
