"""The register / LDS budget the weight-gradient kernels are launched for, checked on the compiler's own resource remarks and on the plan the
dispatch reports (no GPU needed, only hipcc).

Every instantiation of csrc/conv_wgrad.hip (ten kernels, each with its deterministic twin) must come out without scratch and without spills.
The line kernels are persistent: the dispatch walks the segments with 256 CUs x R workgroups, R = the workgroups of that kernel it counts on being
resident on a CU at once. That holds only while the registers admit R workgroups (occupancy in waves per SIMD x 4 SIMDs / waves per workgroup >= R)
and R x the largest dynamic LDS a launch of the kernel can ask for fits into the CU's 160 KB. The grid cap is read from forge_conv_wgrad_plan on a
matrix case with more segments than the cap, the occupancy from the remarks; the largest LDS follows from the limits of the line kernels
(include/forge_hip.h, tests/conv_wgrad_cases.py: 32-voxel segments, |dx| <= 3, at most 9 lines, 6 with a stride-2 gathered operand)."""
import os

import pytest

import conv_wgrad_cases as wc
from resource_remarks import kernel_remarks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "forge_amd", "csrc", "conv_wgrad.hip")
LDS_PER_CU = 160 * 1024
NUM_CU, SIMDS = 256, 4
SEG, MAX_DX = 32, 3

# matrix case with more segments than the grid cap -> (mangled-name fragment of the kernel pair, floats of a staged dY row, most lines)
PERSISTENT = {
    "l_dx3": ("conv_wgrad_lines_kernelINS_11Mfma32x32x2ELi32ELi1ELi7ELi4E", 32, 9),
    "l16_c16": ("conv_wgrad_lines_kernelINS_11Mfma16x16x4ELi16ELi1ELi7ELi4E", 16, 9),
    "l16_c20": ("conv_wgrad_lines_kernelINS_11Mfma16x16x4ELi32ELi1ELi4ELi8E", 16, 9),
    "l16_s2": ("conv_wgrad_lines_kernelINS_11Mfma16x16x4ELi16ELi2ELi9ELi4E", 16, 6),
}


@pytest.fixture(scope="module")
def remarks(tmp_path_factory):
    out = kernel_remarks(SRC, tmp_path_factory.mktemp("res"), "conv_wgrad")
    if out is None:
        pytest.skip("hipcc not found")
    return out


def test_no_instantiation_uses_scratch_or_spills(remarks):
    assert len(remarks) == 20, sorted(remarks)             # ten kernels and their deterministic twins
    for name, k in remarks.items():
        assert k["ScratchSize"] == 0 and k["VGPRs Spill"] == 0 and k["SGPRs Spill"] == 0, (name, k)


@pytest.mark.parametrize("case", sorted(PERSISTENT))
def test_persistent_grid_cap_is_resident(remarks, case):
    fragment, ywidth, max_lines = PERSISTENT[case]
    c = wc.CASE[case]
    segments = c.n * c.D * c.H * ((c.W + SEG - 1) // SEG)
    for det in (0, 1):
        rc, plan = wc.query_plan(c, det)
        assert rc == 0 and (plan["family"], plan["p1"], plan["p2"], plan["nwv"]) == c.plan, wc.plan_text(plan)
        assert segments > plan["grid"] and plan["grid"] % NUM_CU == 0, (segments, wc.plan_text(plan))
        resident = plan["grid"] // NUM_CU
        twins = [k for name, k in remarks.items() if fragment in name and name.endswith("ELb%dEEEvNS_9WgradArgsENS_9LineTableE" % det)]
        assert len(twins) == 1, (fragment, sorted(remarks))
        k = twins[0]
        assert k["Occupancy"] * SIMDS // plan["nwv"] >= resident, "%s det %d: %d VGPRs + %d AGPRs, %d waves per SIMD, %d workgroups per CU planned" % (
            case, det, k["VGPRs"], k["AGPRs"], k["Occupancy"], resident)
        cit, stride = plan["p1"], plan["p2"]
        lds = (SEG * ywidth + max_lines * ((SEG - 1) * stride + 1 + 2 * MAX_DX) * cit) * 4
        assert resident * lds <= LDS_PER_CU, "%s: %d workgroups x %d bytes of LDS" % (case, resident, lds)
