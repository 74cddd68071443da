"""
The register and scratch budgets of the matrix-free kernels at n <= 16 (qoc_amd/csrc/qocx_action16.hip),
in the style of tests/test_action_resources.py: compiled for gfx950 with the resource remarks on, no GPU
needed. The sweep - one wave per seed, one control and the step generator as 16 doubles a lane each in
registers, H0 and further controls in LDS - stays within 128 registers; the gradient kernel was designed
for five waves to a SIMD (its largest degree holds 18 terms of an entry in registers at once); neither
touches scratch.
"""

from tests.test_build_resources import find, resources, total_registers


def test_action16_kernels_keep_their_budgets():
    table = resources("qocx_action16.hip")
    sweep = find(table, "action16_sweep_kernel")
    grad = find(table, "action16_grad_kernel")
    for entry in (sweep, grad):
        assert entry["VGPRs Spill"] == 0 and entry["SGPRs Spill"] == 0 and entry["ScratchSize"] == 0, entry
    granule = lambda r: (r + 7) // 8 * 8  # noqa: E731  (allocation granularity)
    assert total_registers(sweep) <= 128, sweep
    assert granule(total_registers(grad)) * 5 <= 512, grad  # five waves per SIMD
    assert grad["Occupancy"] >= 5, grad
