"""The register and LDS budget of the connected-component kernels, checked on the compiler's own resource remarks (no GPU needed, only hipcc):
every kernel of csrc/components.hip must come out without scratch and without spills - the union and find loops live in a handful of registers,
and a spill would put scratch traffic inside a pointer chase - and the tile kernel's LDS must be what the file's header says: one int32 parent
per voxel of a T^3 tile."""
import os
import re

import pytest

from resource_remarks import kernel_remarks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "forge_amd", "csrc", "components.hip")
KERNELS = ("cc_local", "cc_seam", "cc_flatten", "cc_scan", "cc_rank", "cc_labels", "cc_stats_init", "cc_stats", "cc_winner", "cc_select")


@pytest.fixture(scope="module")
def remarks(tmp_path_factory):
    out = kernel_remarks(SRC, tmp_path_factory.mktemp("res"))
    if out is None:
        pytest.skip("hipcc not found")
    return out


def kernel(remarks, short):
    (k,) = [v for name, v in remarks.items() if re.search(r"\d%sE" % short, name)]          # the mangled name: <length><name>E
    return k


def test_every_kernel_without_scratch_or_spills(remarks):
    assert len(remarks) == len(KERNELS), sorted(remarks)
    for short in KERNELS:
        k = kernel(remarks, short)
        print("components_resources %-14s %3d VGPRs %2d AGPRs, occupancy %d, LDS %5d bytes, scratch %d, spills %d / %d" % (
            short, k["VGPRs"], k["AGPRs"], k["Occupancy"], k["LDS Size"], k["ScratchSize"], k["VGPRs Spill"], k["SGPRs Spill"]))
        assert k["ScratchSize"] == 0 and k["VGPRs Spill"] == 0 and k["SGPRs Spill"] == 0, (short, k)
        assert k["Occupancy"] == 8, (short, k)


def test_tile_kernel_lds_is_what_the_header_says(remarks):
    from forge_amd import ops
    T = ops.components_tile()
    head = open(SRC).read().split("#include", 1)[0]
    m = re.search(r"cc_local\s+(\d+) VGPR, (\d+) B LDS", head)
    assert m, "the header comment of components.hip must record cc_local's VGPRs and LDS"
    k = kernel(remarks, "cc_local")
    assert k["LDS Size"] == int(m.group(2)) == 4 * T ** 3
    assert kernel(remarks, "cc_seam")["LDS Size"] == 0
