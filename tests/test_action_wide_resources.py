"""
Resource budgets of the wide matrix-free route's kernels (qoc_amd/csrc/qocx_action4.hip), in the style
of tests/test_action_resources.py: compiled for gfx950 with the resource remarks on, no GPU needed.

A sweep wave holds three images of 16 columns x (re, im) = 64 registers each - H0, one G_k, the step
generator - and must stay within 256 registers without a byte of scratch: two sweep waves then share a
SIMD, so the workgroups of a seed's two directions (NW <= 4 waves each, one per SIMD) share a CU and
each SIMD has a wave to issue while the other waits at the barrier of its Taylor term. Its LDS is the
vector and two sets of NW partial vectors, all of 64 entries: 16 * 64 * (1 + 2 NW) bytes <= 9216, which
leaves a CU's 160 KiB to the gradient kernel. A gradient wave keeps 32 accumulator doubles and must
stay at four waves per SIMD (<= 128 registers), again without scratch.
"""
import pytest

from tests.test_build_resources import find, resources, total_registers


@pytest.mark.parametrize("waves", [3, 4])
def test_action4_kernels_keep_their_budgets(waves):
    table = resources("qocx_action4.hip")
    sweep = find(table, "action4_sweep_kernelILi%dELi1E" % waves)
    grad = find(table, "action4_grad_kernelILi%dE" % waves)
    for entry in (sweep, grad):
        assert entry["ScratchSize"] == 0 and entry["VGPRs Spill"] == 0 and entry["SGPRs Spill"] == 0, entry
    granule = lambda r: (r + 7) // 8 * 8  # noqa: E731  (allocation granularity)
    assert granule(total_registers(sweep)) * 2 <= 512 and sweep["Occupancy"] >= 2, sweep
    assert sweep["LDS Size"] <= 16 * 64 * (1 + 2 * waves), sweep
    assert granule(total_registers(grad)) * 4 <= 512 and grad["Occupancy"] >= 4, grad
    assert grad["LDS Size"] == 0, grad  # (its LDS is sized at the launch: action4_grad_lds_bytes)
