"""No GPU: which epilogue a launch of the wide implicit-GEMM kernel takes (forge_conv_igemm_epilogue, host arithmetic in csrc/conv_igemm.hip), one
condition at a time, the 2 GiB boundary of the 32-bit store offsets, the process-wide switch and its environment variable."""
import os
import subprocess
import sys

import pytest

from forge_amd import convops as co

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE = dict(M=5120, Cout=256, ldo=256, ldr=256, residual=True, ostride=1, same_grid=True, nphase=1, lift=0, ksplit=1, stats=False, epilogue=co.EPI_AFFINE_ACT)


@pytest.fixture(autouse=True)
def switch_on(built_lib):
    prev = co.STATE.conv_fast_epilogue
    co.STATE.conv_fast_epilogue = True
    yield
    co.STATE.conv_fast_epilogue = prev


def direct(**kw):
    return co.conv_epilogue_is_direct(**dict(BASE, **kw))


def test_trunk_launches_take_the_direct_store_epilogue():
    assert direct()
    assert direct(residual=False)
    assert direct(epilogue=co.EPI_BIAS, residual=False)
    assert direct(M=1, Cout=17, ldo=17, ldr=17)
    assert direct(ldo=512, ldr=512)                                   # a channel slice of a wider tensor
    assert direct(ldo=512, ldr=256)                                   # residual and output rows of different strides
    assert direct(epilogue=co.EPI_BIAS, ldr=0)                        # the plain epilogue reads no residual: ldr does not matter
    assert direct(M=16, ldo=(1 << 22) - 1, ldr=(1 << 22) - 1)         # the widest row stride whose dropped rows cannot wrap round 2^32


@pytest.mark.parametrize("kw", [dict(ksplit=2), dict(ostride=2), dict(same_grid=False), dict(nphase=4), dict(nphase=8), dict(lift=2), dict(lift=32),
                                dict(stats=True, epilogue=co.EPI_BIAS), dict(epilogue=co.EPI_GRU_GATES), dict(epilogue=co.EPI_GRU_OUT),
                                dict(ldo=255), dict(ldr=255), dict(ldo=1 << 22, M=16), dict(ldr=1 << 22, M=16), dict(Cout=16, ldo=16, ldr=16)],
                         ids=lambda kw: ",".join("%s=%s" % i for i in kw.items()))
def test_each_condition_alone_keeps_the_general_epilogue(kw):
    assert direct()                                                   # the rest of the launch qualifies
    assert not direct(**kw)


def _rows_at_limit(ld, Cout):
    """Largest M with ((M - 1) ld + Cout) 4 < 2^31."""
    M = ((1 << 29) - 1 - Cout) // ld + 1
    assert ((M - 1) * ld + Cout) * 4 < (1 << 31) <= (M * ld + Cout) * 4
    return M


@pytest.mark.parametrize("ld,Cout", [(64, 64), (256, 256), (264, 256), (2048, 130)])
def test_two_gib_boundary_of_the_output(ld, Cout):
    M = _rows_at_limit(ld, Cout)
    assert direct(M=M, Cout=Cout, ldo=ld, ldr=ld, residual=False)
    assert not direct(M=M + 1, Cout=Cout, ldo=ld, ldr=ld, residual=False)
    assert not direct(M=(1 << 31) - 1, Cout=Cout, ldo=ld, ldr=ld, residual=False)


def test_two_gib_boundary_exactly():
    # ((M - 1) ldo + Cout) 4 == 2^31 - 4 and == 2^31: ldo = Cout = 32
    M = (1 << 29) // 32
    assert ((M - 1) * 32 + 32) * 4 == 1 << 31
    assert not direct(M=M, Cout=32, ldo=32, ldr=32, residual=False)
    assert direct(M=M - 1, Cout=32, ldo=32, ldr=32, residual=False)
    assert ((M - 1) * 32 + 31) * 4 == (1 << 31) - 4
    assert direct(M=M, Cout=31, ldo=32, ldr=32, residual=False)


def test_two_gib_boundary_of_the_residual():
    M = _rows_at_limit(512, 256)
    assert direct(M=M, ldo=256, ldr=512)
    assert not direct(M=M + 1, ldo=256, ldr=512)
    assert direct(M=M + 1, ldo=256, ldr=512, residual=False)          # without a residual its stride does not count
    assert direct(M=M + 1, ldo=256, ldr=512, epilogue=co.EPI_BIAS)    # nor under the plain epilogue, which does not read it


def test_switch_sends_every_launch_to_the_general_epilogue():
    co.STATE.conv_fast_epilogue = False
    assert not direct() and not direct(residual=False, epilogue=co.EPI_BIAS)
    co.STATE.conv_fast_epilogue = True
    assert direct()


@pytest.mark.parametrize("env,want", [(None, True), ("0", False)])
def test_environment_variable_sets_the_default(env, want):
    e = dict(os.environ)
    e.pop("FORGE_CONV_FAST_EPILOGUE", None)
    if env is not None:
        e["FORGE_CONV_FAST_EPILOGUE"] = env
    code = ("from forge_amd import convops as co; "
            "print(int(co.STATE.conv_fast_epilogue), int(co.conv_epilogue_is_direct(5120, 256, 256, 256, True, epilogue=1)))")
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=e, stdout=subprocess.PIPE, text=True, check=True).stdout.split()
    assert out == [str(int(want))] * 2
