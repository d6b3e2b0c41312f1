"""The register / LDS budget of the direct convolutions, checked on the compiler's own resource remarks (no GPU needed, only hipcc).

csrc/conv_direct.hip instantiates 12 (Cin, Cout) pairs x {forward, data gradient, atomic weight gradient, deterministic weight gradient}. The
weight-gradient kernel keeps wg_taps x Cout x Cin (up to 64) partial sums plus its batched float4 loads in registers: every instantiation must come
out without scratch and without spills, and with the static LDS the source implies - DMAX_W floats of weights for the forward / data gradient,
4 waves x NACC partial sums for the weight gradient."""
import os

import pytest

import direct_cases as dc
from resource_remarks import kernel_remarks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "forge_amd", "csrc", "conv_direct.hip")
DMAX_W = 64 * 4 * 16


@pytest.fixture(scope="module")
def remarks(tmp_path_factory):
    out = kernel_remarks(SRC, tmp_path_factory.mktemp("res"), "conv_direct")
    if out is None:
        pytest.skip("hipcc not found")
    return out


def _kernels():
    """{mangled name: (what, Cin, Cout, static LDS bytes)} of the 48 instantiations."""
    want = {}
    for ci, co in dc.PAIRS:
        for dgrad in (0, 1):
            want["_ZN5forge18conv_direct_kernelILi%dELi%dELb%dEEEvNS_10DirectArgsE" % (ci // 4, co, dgrad)] = ("dgrad" if dgrad else "fwd", ci, co, DMAX_W * 4)
        for det in (0, 1):
            want["_ZN5forge24conv_direct_wgrad_kernelILi%dELi%dELb%dEEEvNS_10DirectArgsE" % (ci // 4, co, det)] = (
                "wgrad det" if det else "wgrad", ci, co, 4 * dc.wg_taps(ci, co) * co * ci * 4)
    return want


def test_all_48_instantiations_without_scratch_or_spills(remarks):
    want = _kernels()
    assert len(want) == 48 and set(remarks) == set(want), sorted(set(remarks) ^ set(want))
    for name, (what, ci, co, lds) in sorted(want.items(), key=lambda kv: kv[1]):
        k = remarks[name]
        print("conv_direct_resources %-9s Cin %2d Cout %d: %3d VGPRs %2d AGPRs, occupancy %d, LDS %5d bytes, scratch %d, spills %d / %d" % (
            what, ci, co, k["VGPRs"], k["AGPRs"], k["Occupancy"], k["LDS Size"], k["ScratchSize"], k["VGPRs Spill"], k["SGPRs Spill"]))
        assert k["ScratchSize"] == 0 and k["VGPRs Spill"] == 0 and k["SGPRs Spill"] == 0, (what, ci, co, k)
        assert k["LDS Size"] == lds, (what, ci, co, k["LDS Size"], lds)
