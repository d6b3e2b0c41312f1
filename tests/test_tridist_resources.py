"""The register budget of the point-to-triangle kernels, checked on the compiler's own resource remarks (no GPU needed, only hipcc): every
kernel of csrc/tridist.hip must come out without scratch and without spills - the search keeps its query, the running minimum and a face
record in registers for 10^9 and more (query, face) pairs, and a spill there would sit in its inner loop."""
import os

import pytest

from resource_remarks import kernel_remarks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "forge_amd", "csrc", "tridist.hip")
KERNELS = ("tri_stage_kernel", "nn_triangles_kernel")
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
        print("tridist_resources %-70s %3d VGPRs %2d AGPRs, occupancy %d, LDS %5d bytes, scratch %d, spills %d / %d" % (
            name, k["VGPRs"], k["AGPRs"], k["Occupancy"], k["LDS Size"], k["ScratchSize"], k["VGPRs Spill"], k["SGPRs Spill"]))
        assert k["ScratchSize"] == 0 and k["VGPRs Spill"] == 0 and k["SGPRs Spill"] == 0, (name, k)


def test_the_tile_of_records_is_the_only_lds_of_the_search(remarks):
    """One record per face of a tile of forge_nn_tile_faces(), and the workspace holds the same record per face row."""
    from forge_amd import _lib
    (k,) = [v for name, v in remarks.items() if "nn_triangles_kernel" in name]
    assert k["LDS Size"] == RECORD_BYTES * _lib.lib().forge_nn_tile_faces()
    (s,) = [v for name, v in remarks.items() if "tri_stage_kernel" in name]
    assert s["LDS Size"] == 0
    assert _lib.size_query("forge_nn_triangles_workspace_bytes", 3, 100, 0) == 3 * 100 * RECORD_BYTES + 16
    assert _lib.size_query("forge_nn_triangles_workspace_bytes", 3, 100, 1) == 100 * RECORD_BYTES + 16
