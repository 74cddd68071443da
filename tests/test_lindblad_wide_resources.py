"""
Resource budgets of the Lindblad kernel of 33 <= n <= 64 (qoc_amd/csrc/qocx_lindblad16t.hip), in the
style of tests/test_action_wide_resources.py: compiled for gfx950 with the resource remarks on, no GPU
needed.

Sixteen waves per workgroup are four per SIMD: a wave has 128 registers, and the kernel must fit them
without a byte of scratch and without a spilled vector register (scalar registers spilled into vector
lanes are allowed, as in qocx_lindblad4t.hip). Its LDS is sized at the launch (lindblad16t_lds_bytes):
two 64 x 64 complex matrices at pitch 65 and the partial sums, within the 160 KiB of a CU.
"""
import os
import re

from tests.test_build_resources import find, resources, total_registers

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "qoc_amd", "csrc")


def test_lindblad16t_kernel_keeps_its_budget():
    entry = find(resources("qocx_lindblad16t.hip"), "lindblad16t_kernel")
    assert entry["ScratchSize"] == 0 and entry["VGPRs Spill"] == 0, entry
    assert total_registers(entry) <= 128 and entry["Occupancy"] >= 4, entry
    assert entry["LDS Size"] == 0, entry  # (dynamic: sized at the launch)


def test_lindblad16t_lds_fits_a_cu():
    """The launch's LDS as qocx_lindblad16t_core.h computes it, and the header's own static_assert."""
    matrices = 2 * 64 * 65 * 16
    reduction = 2 * 16 * 16        # [parity][wave] complex
    cotangents = 16 * 2 * 8 * 8    # [wave][2][8] doubles
    assert matrices + reduction + cotangents <= 160 * 1024
    with open(os.path.join(CSRC, "qocx_lindblad16t_core.h")) as f:
        text = f.read()
    assert re.search(r"static_assert\(LDS_BYTES <= 160 \* 1024", text)
    assert "M_COUNT * D::MBYTES" in text and "2 * G::WAVES * 16" in text
