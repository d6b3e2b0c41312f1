"""The four-point Winograd GEMM (forge_wino_gemm_half) keeps its results bit for bit under its own schedule: a prefetch cursor that walks over the
point switches, the row stage's first plane stored before the fourth point runs, and depth taps that are zero for a whole workgroup not walked.

Every case compares the 8 planes against the row-combined 16 point products of forge_wino_gemm - the same fp32 operations in the same order, so
torch.equal - on outputs prefilled with NaN (an element that is not written, or written from a stage that had not landed, does not compare equal)."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _check(n, D, Ht, Wt, C1, C2, Cout, kd=3, seed=11):
    from forge_amd import convops as co
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(seed)
    R = n * D * Ht * Wt
    V1 = torch.randn(16, R, C1, device=dev, generator=g)
    V2 = torch.randn(16, R, C2, device=dev, generator=g) if C2 else None
    U = torch.randn(16, kd, Cout, C1 + C2, device=dev, generator=g) * 0.05
    Mm = torch.full((16, R, Cout), float("nan"), device=dev)
    Mm8 = torch.full((8, R, Cout), float("nan"), device=dev)
    co.wino_gemm(V1, C1, V2, C2, U, Mm, n, D, Ht, Wt, Cout, half=False)
    co.wino_gemm(V1, C1, V2, C2, U, Mm8, n, D, Ht, Wt, Cout, half=True)
    torch.cuda.synchronize()
    assert not torch.isnan(Mm).any()
    s0 = (Mm[0:4] + Mm[4:8]) + Mm[8:12]                              # rows of A^T M over the point index i (p = 4 i + j)
    s1 = (Mm[4:8] - Mm[8:12]) - Mm[12:16]
    assert torch.equal(Mm8[0:4], s0), "plane i' = 0 differs"
    assert torch.equal(Mm8[4:8], s1), "plane i' = 1 differs"


@pytest.mark.parametrize("D", [1, 2, 3, 32])
def test_whole_tiles_in_one_depth_plane(D):
    """Ht x Wt = 256: every 64-row tile lies in one depth plane. D = 1: both outer taps are skipped by every workgroup; D = 2: one by each;
    D = 3: the middle plane walks all three; D = 32: the shape of the step."""
    _check(1, D, 16, 16, 128, 0, 128)


def test_tiles_straddle_planes_and_batch_elements():
    """Ht x Wt = 240, two batch elements: tiles cross depth planes and scenes - no tap may be skipped there, and taps must not cross scenes."""
    _check(2, 3, 16, 15, 64, 0, 128)
    _check(2, 1, 16, 15, 64, 0, 128)


@pytest.mark.parametrize("Cin", [32, 64])
@pytest.mark.parametrize("D", [1, 4])
def test_fewer_k_steps_per_point_than_the_prefetch_depth(Cin, D):
    """Cin = 32 / 64: one or two K-steps per tap, at D = 1 per POINT - the point switch happens in the prefetch of every step or every other step."""
    _check(1, D, 16, 16, Cin, 0, 128)


def test_one_depth_tap_2d_form():
    _check(3, 1, 16, 16, 32, 0, 128, kd=1)
    _check(1, 5, 16, 16, 64, 32, 256, kd=1)


@pytest.mark.parametrize("shape", [(1, 3, 13, 11, 64, 0, 96), (2, 2, 9, 7, 32, 0, 160), (1, 32, 16, 16, 64, 0, 200)])
def test_ragged_rows_and_columns(shape):
    """R not a multiple of 64 (rows beyond M must not be stored: the planes are contiguous, a stray row would land in the next plane) and Cout not a
    multiple of 128 / 32 (a stray column would land in the next row)."""
    _check(*shape)


@pytest.mark.parametrize("shape", [(1, 32, 16, 16, 128, 128, 256), (1, 1, 16, 16, 32, 32, 128), (2, 3, 16, 15, 32, 64, 128)])
def test_two_operands(shape):
    """The channel concatenation [V1 | V2] (the ConvGRU's [x | h]): the K loop changes operand inside a tap."""
    _check(*shape)
