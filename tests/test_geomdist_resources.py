"""The register budget of the surface-metric kernels, checked on the compiler's own resource remarks (no GPU needed, only hipcc): every kernel
of csrc/geomdist.hip must come out without scratch and without spills - the nearest-neighbour search keeps its queries, the running minimum and a
group of references in registers for 10^10 pairs, and a spill there would sit in its inner loop."""
import os

import pytest

from resource_remarks import kernel_remarks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "forge_amd", "csrc", "geomdist.hip")
KERNELS = ("surface_scan_kernel", "surface_sample_kernel", "nn_points_kernel", "geom_partial_kernel", "geom_finalize_kernel")


@pytest.fixture(scope="module")
def remarks(tmp_path_factory):
    out = kernel_remarks(SRC, tmp_path_factory.mktemp("res"))
    if out is None:
        pytest.skip("hipcc not found")
    return out


def test_every_kernel_without_scratch_or_spills(remarks):
    assert len(remarks) == len(KERNELS) and all(any(k in name for name in remarks) for k in KERNELS), sorted(remarks)
    for name, k in sorted(remarks.items()):
        print("geomdist_resources %-70s %3d VGPRs %2d AGPRs, occupancy %d, LDS %5d bytes, scratch %d, spills %d / %d" % (
            name, k["VGPRs"], k["AGPRs"], k["Occupancy"], k["LDS Size"], k["ScratchSize"], k["VGPRs Spill"], k["SGPRs Spill"]))
        assert k["ScratchSize"] == 0 and k["VGPRs Spill"] == 0 and k["SGPRs Spill"] == 0, (name, k)


def test_nn_tile_is_the_only_lds_of_the_search(remarks):
    """Three planes of forge_nn_tile_points() floats: the occupancy of the search is bounded by registers, not by LDS."""
    from forge_amd import _lib
    (k,) = [v for name, v in remarks.items() if "nn_points_kernel" in name]
    assert k["LDS Size"] == 3 * 4 * _lib.lib().forge_nn_tile_points()
    assert k["Occupancy"] >= 4
