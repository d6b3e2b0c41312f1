"""Deterministic mode without a GPU: the switch's semantics, the host-only workspace queries of the _det entry points, and the dispatch
(with the library mocked) - forge_amd/determinism.py, include/forge_hip.h "Deterministic mode"."""
import ctypes

import pytest
import torch

import forge_amd
from forge_amd import _lib, convops as co, determinism


@pytest.fixture(autouse=True)
def _restore():
    prev, flag, warn = determinism.get_deterministic_setting(), torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    yield
    determinism.set_deterministic(prev)
    torch.use_deterministic_algorithms(flag, warn_only=warn)


def test_none_follows_torch_flag_including_warn_only():
    forge_amd.set_deterministic(None)
    torch.use_deterministic_algorithms(False)
    assert forge_amd.is_deterministic() is False
    torch.use_deterministic_algorithms(True, warn_only=True)
    assert forge_amd.is_deterministic() is True
    torch.use_deterministic_algorithms(True)
    assert forge_amd.is_deterministic() is True
    forge_amd.set_deterministic(False)                      # an explicit setting wins over torch's flag
    assert forge_amd.is_deterministic() is False
    torch.use_deterministic_algorithms(False)
    forge_amd.set_deterministic(True)
    assert forge_amd.is_deterministic() is True


def test_context_manager_restores_previous_mode_even_after_an_exception():
    forge_amd.set_deterministic(False)
    with forge_amd.deterministic(True):
        assert forge_amd.is_deterministic()
        with forge_amd.deterministic(None):
            assert determinism.get_deterministic_setting() is None
        assert determinism.get_deterministic_setting() is True
    assert determinism.get_deterministic_setting() is False
    with pytest.raises(ZeroDivisionError):
        with forge_amd.deterministic(True):
            1 / 0
    assert determinism.get_deterministic_setting() is False and not forge_amd.is_deterministic()
    with pytest.raises(TypeError):
        forge_amd.set_deterministic(1)


def _taps(taps):
    return (ctypes.c_int * (3 * len(taps)))(*[v for t in taps for v in t])


T27 = [tuple(t) for t in co.TAPS_3x3x3]


def test_det_ws_bytes_queries_are_host_only_pure_and_checked():
    L = _lib.lib()
    t27 = _taps(T27)
    good = [
        (L.forge_conv_wgrad_det_ws_bytes, (128, 128, 4, 32, 32, 32, 1, 32, 32, 32, 128, t27, 27)),   # tiles, two inputs
        (L.forge_conv_wgrad_det_ws_bytes, (64, 0, 1, 16, 16, 16, 1, 16, 16, 16, 64, t27, 27)),       # tiles, small M
        (L.forge_conv_wgrad_det_ws_bytes, (32, 0, 4, 64, 64, 64, 1, 64, 64, 64, 16, t27, 27)),       # lines16
        (L.forge_conv_wgrad_det_ws_bytes, (32, 0, 4, 64, 64, 64, 1, 64, 64, 64, 32, t27, 27)),       # lines
        (L.forge_wino_wgrad_det_ws_bytes, (128, 0, 4, 32, 16, 16, 256, 3)),
        (L.forge_wino_wgrad_det_ws_bytes, (256, 0, 5, 1, 8, 8, 256, 1)),
        (L.forge_conv_direct_wgrad_det_ws_bytes, (4, 64, 64, 64, 8, 1, 27)),
        (L.forge_rotate_bwd_det_ws_bytes, (20, 128, 32, 32, 32)),
        (L.forge_rotate_bwd_slots_det_ws_bytes, (20, 128, 32, 32, 32)),
    ]
    for fn, args in good:
        a, b = fn(*args), fn(*args)
        assert a == b and a > 0 and a % 16 == 0, (fn, args, a)
        assert a <= 64 << 20 or fn in (L.forge_rotate_bwd_det_ws_bytes, L.forge_rotate_bwd_slots_det_ws_bytes), a     # the slab cap
    assert L.forge_rotate_bwd_det_ws_bytes(20, 128, 32, 32, 32) == 20 * 512 * 12 * 4           # [n][blocks][12] partials
    bad = [
        (L.forge_conv_wgrad_det_ws_bytes, (3, 0, 4, 32, 32, 32, 1, 32, 32, 32, 128, t27, 27)),       # C1 not a multiple of 4
        (L.forge_conv_wgrad_det_ws_bytes, (64, 0, 0, 32, 32, 32, 1, 32, 32, 32, 128, t27, 27)),      # n = 0
        (L.forge_conv_wgrad_det_ws_bytes, (64, 0, 1, 32, 32, 32, 1, 32, 32, 32, 128, None, 27)),     # no tap table
        (L.forge_conv_wgrad_det_ws_bytes, (64, 32, 1, 32, 32, 32, 1, 32, 32, 32, 128, t27, 27)),     # two inputs, C1 % 128 != 0
        (L.forge_wino_wgrad_det_ws_bytes, (128, 0, 4, 32, 16, 16, 256, 2)),                          # kd not 1 / 3
        (L.forge_conv_direct_wgrad_det_ws_bytes, (1, 8, 8, 8, 32, 1, 27)),                            # Cin outside 4 / 8 / 16
        (L.forge_rotate_bwd_det_ws_bytes, (1, 6, 8, 8, 8)),                                           # C % 4 != 0
        (L.forge_rotate_bwd_slots_det_ws_bytes, (0, 8, 8, 8, 8)),
    ]
    for fn, args in bad:
        assert fn(*args) < 0, (fn, args)


def test_conv_wgrad_det_ws_bytes_depends_on_shape_only():
    """The plan is a function of the shape: strides / batch strides of the operands do not enter the query, and the same shape gives the same
    bytes whatever was queried before."""
    L = _lib.lib()
    t27 = _taps(T27)
    a = L.forge_conv_wgrad_det_ws_bytes(128, 0, 2, 16, 32, 32, 1, 16, 32, 32, 128, t27, 27)
    L.forge_conv_wgrad_det_ws_bytes(32, 0, 4, 64, 64, 64, 1, 64, 64, 64, 16, t27, 27)
    assert L.forge_conv_wgrad_det_ws_bytes(128, 0, 2, 16, 32, 32, 1, 16, 32, 32, 128, t27, 27) == a


class _FakeLib:
    """Records every call; entry points return 0, the workspace queries 256 bytes."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, args))
            return 256 if name.endswith("_ws_bytes") else 0
        return fn


@pytest.mark.parametrize("mode", [False, True])
def test_dispatch_calls_det_entry_only_in_deterministic_mode(monkeypatch, mode):
    fake = _FakeLib()
    monkeypatch.setattr(_lib, "lib", lambda: fake)
    monkeypatch.setattr(_lib, "current_stream", lambda: None)
    dy = torch.zeros(1, 4, 4, 4, 16)
    x = torch.zeros(1, 4, 4, 4, 32)
    dw = torch.zeros(27, 16, 32)
    with forge_amd.deterministic(mode):
        co.conv_wgrad(dy, x, 32, None, 0, dw, (1, 4, 4, 4), (4, 4, 4), 16, T27)
        determinism.launch("forge_rotate_bwd", (None,) * 11, (1, 4, 4, 4, 4), "cpu")
    names = [c[0] for c in fake.calls]
    if mode:
        assert names == ["forge_conv_wgrad_det_ws_bytes", "forge_conv_wgrad_det", "forge_rotate_bwd_det_ws_bytes", "forge_rotate_bwd_det"]
        det_args = fake.calls[1][1]
        assert det_args[-4] == 1 and det_args[-2] == 256                 # accumulate = 1 (the += contract of every call site), ws_bytes
    else:
        assert names == ["forge_conv_wgrad", "forge_rotate_bwd"]


def test_dispatch_follows_torch_flag(monkeypatch):
    fake = _FakeLib()
    monkeypatch.setattr(_lib, "lib", lambda: fake)
    monkeypatch.setattr(_lib, "current_stream", lambda: None)
    forge_amd.set_deterministic(None)
    torch.use_deterministic_algorithms(True, warn_only=True)
    determinism.launch("forge_wino_wgrad", (None,) * 16, (128, 0, 1, 1, 1, 1, 64, 1), "cpu")
    torch.use_deterministic_algorithms(False)
    determinism.launch("forge_wino_wgrad", (None,) * 16, (128, 0, 1, 1, 1, 1, 64, 1), "cpu")
    assert [c[0] for c in fake.calls] == ["forge_wino_wgrad_det_ws_bytes", "forge_wino_wgrad_det", "forge_wino_wgrad"]


def test_dispatch_raises_on_rejected_shape(monkeypatch):
    class Neg(_FakeLib):
        def __getattr__(self, name):
            if name == "forge_last_error":
                return lambda: b"bad dims"
            return (lambda *a: -2) if name.endswith("_ws_bytes") else super().__getattr__(name)
    monkeypatch.setattr(_lib, "lib", lambda: Neg())
    monkeypatch.setattr(_lib, "current_stream", lambda: None)
    with forge_amd.deterministic(True):
        with pytest.raises(RuntimeError, match="rejected"):
            determinism.launch("forge_rotate_bwd", (None,) * 11, (1, 6, 4, 4, 4), "cpu")
