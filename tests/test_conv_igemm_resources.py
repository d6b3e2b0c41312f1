"""The register / LDS budget the implicit-GEMM launches are scheduled for, checked on the compiler's own resource remarks (no GPU needed, only hipcc).

The four-point Winograd form (conv_igemm_kernel<64, 128, 8, 1, 1>, forge_wino_gemm_half) is launched with RS_STAGES x 24 KB of dynamic LDS and
is meant to run THREE workgroups per CU: that needs 6 waves per SIMD (at most 80 VGPRs), no scratch, and 3 x its LDS within the CU's 160 KB.
Tile B (<64, 128, 8, 1, 0>) keeps three 48 KB workgroups per CU (plan_conv's occupancy 3).
The two depth nests (<64, 128, 8, 1, 2>, forge_wino_gemm_dn; <64, 128, 8, 1, 3>, forge_wino_gemm_dn4) are scheduled for TWO workgroups per CU: no scratch,
at least 4 waves per SIMD, and 2 x their launched LDS (64 KB / 48 KB) within 160 KB."""
import os
import re

import pytest

from resource_remarks import kernel_remarks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "forge_amd", "csrc", "conv_igemm.hip")
LDS_PER_CU = 160 * 1024
WAVES_PER_WORKGROUP, SIMDS = 8, 4


@pytest.fixture(scope="module")
def remarks(tmp_path_factory):
    out = kernel_remarks(SRC, tmp_path_factory.mktemp("res"))
    if out is None:
        pytest.skip("hipcc not found")
    return out


def _kernel(remarks, rs):
    name = "_ZN5forge17conv_igemm_kernelILi64ELi128ELi8ELi1ELi%dEEEvNS_8ConvArgsE" % rs
    assert name in remarks, sorted(remarks)
    return remarks[name]


def _constants():
    src = open(SRC).read()
    stages = int(re.search(r"constexpr int RS_STAGES = (\d+);", src).group(1))
    bk = int(re.search(r"constexpr int BK = (\d+),", src).group(1))
    assert "const size_t lds = RS_STAGES * (64 * BK + 128 * BK) * sizeof(float);" in src      # the launcher sizes its LDS from the same constant
    return stages, (64 * bk + 128 * bk) * 4


def _launched_lds(rs):
    """Bytes of dynamic LDS of form rs, evaluated from the expression its launch line in launch_conv_tile hands to the kernel launch."""
    src = open(SRC).read()
    stages = int(re.search(r"constexpr int RS_STAGES = (\d+);", src).group(1))
    bk = int(re.search(r"constexpr int BK = (\d+),", src).group(1))
    m = re.search(r"const size_t lds = (.+?) \* sizeof\(float\); return launch_point_form<%d>\(" % rs, src)
    assert m, "launch line of form %d not found" % rs
    return eval(m.group(1), {"__builtins__": {}}, {"RS_STAGES": stages, "BK": bk}) * 4


def _resident_by_registers(k):
    return k["Occupancy"] * SIMDS // WAVES_PER_WORKGROUP


def test_four_point_form_keeps_three_workgroups_per_cu(remarks):
    k = _kernel(remarks, 1)
    stages, stage_bytes = _constants()
    assert k["ScratchSize"] == 0 and k.get("VGPRs Spill", 0) == 0 and k.get("SGPRs Spill", 0) == 0
    resident = _resident_by_registers(k)
    assert resident >= 3, "four-point form: %d VGPRs, %d waves per SIMD" % (k["VGPRs"], k["Occupancy"])
    assert resident * stages * stage_bytes <= LDS_PER_CU, "the registers admit %d workgroups, the LDS does not" % resident


def test_tile_b_keeps_three_48k_workgroups_per_cu(remarks):
    k = _kernel(remarks, 0)
    _, stage_bytes = _constants()
    assert k["ScratchSize"] == 0
    assert 2 * stage_bytes == 48 * 1024 and 3 * 2 * stage_bytes <= LDS_PER_CU
    assert _resident_by_registers(k) >= 3


@pytest.mark.parametrize("rs, name", [(2, "depth nest"), (3, "F(4, 3) depth nest")])
def test_depth_nests_keep_two_workgroups_per_cu(remarks, rs, name):
    k = _kernel(remarks, rs)
    lds = _launched_lds(rs)
    assert k["ScratchSize"] == 0 and k.get("VGPRs Spill", 0) == 0 and k.get("SGPRs Spill", 0) == 0
    assert _resident_by_registers(k) >= 2, "%s: %d VGPRs, %d waves per SIMD" % (name, k["VGPRs"], k["Occupancy"])
    assert 2 * lds <= LDS_PER_CU, "%s: two workgroups need %d bytes of LDS" % (name, 2 * lds)
