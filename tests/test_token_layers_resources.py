"""The register / LDS budget the token-layer launches are planned for, checked on the compiler's own resource remarks (no GPU needed, only hipcc).

csrc/token.hip plans (its header comment and constants): the forward, dx and LayerNorm-forward kernels are 2-wave workgroups with one 32 x 260
float tile in LDS, FOUR of them per CU (2 waves per SIMD); the dW kernel is a 4-wave workgroup without LDS, at least two per CU; the LayerNorm
backward is a 4-wave workgroup with a 32 x 257 float reduction tile, at least two per CU. No kernel may use scratch."""
import os
import re

import pytest

from resource_remarks import kernel_remarks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "forge_amd", "csrc", "token.hip")
LDS_PER_CU, SIMDS = 160 * 1024, 4
#          kernel (as in the mangled name)   waves per workgroup, workgroups per CU the launcher plans for
PLANNED = {"token_linear_fwd_kernel": (2, 4), "layer_norm_fwd_kernel": (2, 4), "token_linear_dx_kernel": (2, 4), "token_linear_dw_kernel": (4, 2),
           "layer_norm_bwd_kernel": (4, 2)}


@pytest.fixture(scope="module")
def remarks(tmp_path_factory):
    out = kernel_remarks(SRC, tmp_path_factory.mktemp("res"))
    if out is None:
        pytest.skip("hipcc not found")
    return out


def test_every_kernel_of_the_file_is_planned(remarks):
    src = open(SRC).read()
    declared = set(re.findall(r"__global__\s+__launch_bounds__\([^)]*\)\s+void\s+(\w+)\s*\(", src))
    assert declared == set(PLANNED)
    for name in PLANNED:
        assert sum(name in k for k in remarks) == 1, (name, sorted(remarks))


@pytest.mark.parametrize("name", sorted(PLANNED))
def test_no_scratch_and_the_planned_occupancy(remarks, name):
    waves, per_cu = PLANNED[name]
    k = next(v for key, v in remarks.items() if name in key)
    assert k["ScratchSize"] == 0 and k.get("VGPRs Spill", 0) == 0 and k.get("SGPRs Spill", 0) == 0, k
    by_registers = k["Occupancy"] * SIMDS // waves                              # workgroups per CU the register count admits
    assert by_registers >= per_cu, "%s: %d VGPRs + %d AGPRs, %d waves per SIMD" % (name, k["VGPRs"], k.get("AGPRs", 0), k["Occupancy"])
    assert per_cu * k["LDS Size"] <= LDS_PER_CU, "%s: %d bytes of LDS per workgroup" % (name, k["LDS Size"])


def test_the_lds_tile_is_what_the_constants_say(remarks):
    src = open(SRC).read()
    rows = int(re.search(r"constexpr int TK_ROWS = (\d+);", src).group(1))
    kc = int(re.search(r"constexpr int TK_KC = (\d+);", src).group(1))
    assert "constexpr int TK_LD = TK_KC + 4;" in src
    for name in ("token_linear_fwd_kernel", "layer_norm_fwd_kernel", "token_linear_dx_kernel"):
        k = next(v for key, v in remarks.items() if name in key)
        assert k["LDS Size"] == rows * (kc + 4) * 4 == 33280
    assert next(v for key, v in remarks.items() if "token_linear_dw_kernel" in key)["LDS Size"] == 0
