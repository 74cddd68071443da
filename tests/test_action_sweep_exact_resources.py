"""
Resource budgets of the exact-K sweep of the matrix-free route (qoc_amd/csrc/qocx_action.hip:
action_sweep_exact_kernel<2>, the sweep of every problem with two controls - the headline's), in the style
of tests/test_action_resources.py: compiled for gfx950 with the resource remarks on, no GPU needed. It is the
same step body as action_sweep_kernel<2, 2> with the control count a constant, and it is held to the same
budgets: no scratch and no spill, a gradient wave beside it on the SIMD (512 registers), and LDS that leaves
room for the gradient waves. The generic sweep keeps its name and its budgets (test_action_resources.py).
"""
from tests.test_build_resources import find, resources, total_registers


def test_exact_sweep_keeps_the_budgets_of_the_generic_one():
    table = resources("qocx_action.hip")
    exact = find(table, "action_sweep_exact_kernelILi2E")
    generic = find(table, "action_sweep_kernelILi2ELi2E")
    grad = find(table, "action_grad_kernelILi2E")
    for entry in (exact, generic, grad):
        assert entry["ScratchSize"] == 0 and entry["VGPRs Spill"] == 0 and entry["SGPRs Spill"] == 0, entry
    granule = lambda r: (r + 7) // 8 * 8  # noqa: E731  (allocation granularity)
    assert granule(total_registers(grad)) * 3 <= 512 and grad["Occupancy"] >= 3
    for sweep in (exact, generic):
        assert granule(total_registers(sweep)) + granule(total_registers(grad)) <= 512
        assert sweep["LDS Size"] <= 2048
    # the constant control count costs no register over the generic build
    assert granule(total_registers(exact)) <= granule(total_registers(generic))
