"""The register budget of the winding-number kernel, checked on the compiler's own resource remarks (no GPU needed, only hipcc): every kernel
of csrc/winding.hip must come out without scratch and without spills - the sum keeps its query, a float64 total and a face record in registers
for 10^9 and more (query, face) pairs, and a spill there would sit in its inner loop - with the tile of records as its only LDS, and with
room for at least 4 waves per SIMD: the loop hides its square roots and its reciprocal behind other waves."""
import os

import pytest

from resource_remarks import kernel_remarks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "forge_amd", "csrc", "winding.hip")
KERNELS = ("winding_kernel",)                      # the staging kernel is tridist.hip's: tests/test_tridist_resources.py
RECORD_BYTES = 48                                  # a | b | c | n: 12 floats per face (section g3b: the workspace)


@pytest.fixture(scope="module")
def remarks(tmp_path_factory):
    out = kernel_remarks(SRC, tmp_path_factory.mktemp("res"))
    if out is None:
        pytest.skip("hipcc not found")
    return out


def test_every_kernel_without_scratch_or_spills(remarks):
    assert len(remarks) == len(KERNELS) and all(any(k in name for name in remarks) for k in KERNELS), sorted(remarks)
    for name, k in sorted(remarks.items()):
        print("winding_resources %-70s %3d VGPRs %2d AGPRs, occupancy %d, LDS %5d bytes, scratch %d, spills %d / %d" % (
            name, k["VGPRs"], k["AGPRs"], k["Occupancy"], k["LDS Size"], k["ScratchSize"], k["VGPRs Spill"], k["SGPRs Spill"]))
        assert k["ScratchSize"] == 0 and k["VGPRs Spill"] == 0 and k["SGPRs Spill"] == 0, (name, k)
        assert k["Occupancy"] >= 4, (name, k)


def test_the_tile_of_records_is_the_only_lds(remarks):
    """One record per face of a tile of forge_nn_tile_faces(), and the workspace holds the same record per face row as forge_nn_triangles'."""
    from forge_amd import _lib
    (k,) = [v for name, v in remarks.items() if "winding_kernel" in name]
    assert k["LDS Size"] == RECORD_BYTES * _lib.lib().forge_nn_tile_faces()
    assert _lib.size_query("forge_winding_workspace_bytes", 3, 100, 0) == 3 * 100 * RECORD_BYTES + 16
    assert _lib.size_query("forge_winding_workspace_bytes", 3, 100, 1) == 100 * RECORD_BYTES + 16
