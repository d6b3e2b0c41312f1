"""The register budget of the alignment kernels, checked on the compiler's own resource remarks (no GPU needed, only hipcc): every kernel of
csrc/align.hip must come out without scratch and without spills - the moments pass holds 21 float64 accumulators per thread, the solve holds a 3x3
SVD in registers, and an array of either that went to scratch would turn the pass from bandwidth into latency."""
import os

import pytest

from resource_remarks import kernel_remarks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "forge_amd", "csrc", "align.hip")
KERNELS = ("align_moments_kernel", "align_solve_kernel", "align_select_kernel")


@pytest.fixture(scope="module")
def remarks(tmp_path_factory):
    out = kernel_remarks(SRC, tmp_path_factory.mktemp("res"), name_filter="_kernel")
    if out is None:
        pytest.skip("hipcc not found")
    return out


def test_every_kernel_without_scratch_or_spills(remarks):
    assert len(remarks) == len(KERNELS) and all(any(k in name for name in remarks) for k in KERNELS), sorted(remarks)
    for name, k in sorted(remarks.items()):
        print("align_resources %-60s %3d VGPRs %2d AGPRs, occupancy %d, LDS %5d bytes, scratch %d, spills %d / %d" % (
            name, k["VGPRs"], k["AGPRs"], k["Occupancy"], k["LDS Size"], k["ScratchSize"], k["VGPRs Spill"], k["SGPRs Spill"]))
        assert k["ScratchSize"] == 0 and k["VGPRs Spill"] == 0 and k["SGPRs Spill"] == 0, (name, k)


def test_the_moments_pass_reduces_through_one_lds_array(remarks):
    """256 doubles, reused for the 21 sums: the fixed tree of geom_common.h."""
    (k,) = [v for name, v in remarks.items() if "align_moments_kernel" in name]
    assert k["LDS Size"] == 256 * 8
