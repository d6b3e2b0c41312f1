"""Deterministic mode: bitwise-reproducible weight and pose gradients.

Most backward kernels of this library are deterministic by construction (gathers, fixed-order float64 partials). The exceptions add
partial sums with hardware fp32 atomics, whose order changes from run to run: forge_conv_wgrad, forge_wino_wgrad, forge_conv_direct_wgrad
and the pose gradient of forge_rotate_bwd(_slots). Each has a `_det` counterpart in the C-ABI that stores partial sums into slabs of a
workspace and sums them in a fixed order (include/forge_hip.h, "Deterministic mode"). This module holds the switch and routes launches.

    forge_amd.set_deterministic(True | False | None)   None (the default): follow torch.are_deterministic_algorithms_enabled(),
                                                       which is also True under torch.use_deterministic_algorithms(True, warn_only=True)
    forge_amd.is_deterministic()                       the effective mode
    with forge_amd.deterministic(True): ...            restores the previous setting on exit, also after an exception

The mode is read when an op launches. A graph captured by GraphedForward / GraphedStep / the refinement loop replays the launches it
recorded, so it keeps the mode that was active at capture.
"""
import contextlib

import torch

from . import _lib

_setting = None          # True / False / None (follow torch's flag); process-wide, like torch's own switch


def set_deterministic(mode):
    """True: the deterministic kernels; False: the default (atomic) kernels; None: follow torch.are_deterministic_algorithms_enabled()."""
    global _setting
    if mode is not None and not isinstance(mode, bool):
        raise TypeError("set_deterministic expects True, False or None, got %r" % (mode,))
    _setting = mode


def get_deterministic_setting():
    """The raw setting (True / False / None), as set_deterministic() took it."""
    return _setting


def is_deterministic():
    """The effective mode: the explicit setting, or torch's deterministic-algorithms flag when the setting is None."""
    if _setting is None:
        return bool(torch.are_deterministic_algorithms_enabled())
    return _setting


@contextlib.contextmanager
def deterministic(mode=True):
    """Context manager: set_deterministic(mode) inside the block, the previous setting restored on exit."""
    prev = _setting
    set_deterministic(mode)
    try:
        yield
    finally:
        set_deterministic(prev)


def launch(name, args, ws_query, device):
    """Launch `forge_<name>`(*args, stream) - or, in deterministic mode, `forge_<name>_det`(*args, accumulate = 1, ws, ws_bytes, stream) with
    a workspace of `forge_<name>_det_ws_bytes`(*ws_query) bytes from torch's allocator on the current stream. accumulate = 1 keeps the
    default entry's contract at every call site (the output is a zero-filled or partially accumulated gradient: out = prior + S), and a
    chain of launches into one output stays ordered on the one stream. Raises on a rejected call; never falls back."""
    L = _lib.lib()
    st = _lib.current_stream()
    if not is_deterministic():
        _lib.check(getattr(L, name)(*args, st), name)
        return
    nbytes = int(getattr(L, name + "_det_ws_bytes")(*ws_query))
    if nbytes < 0:
        raise RuntimeError("forge_amd: %s_det_ws_bytes rejected the shape (code %d): %s"
                           % (name, nbytes, L.forge_last_error().decode("utf-8", "replace")))
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=device)
    _lib.check(getattr(L, name + "_det")(*args, 1, _lib.ptr(ws), nbytes, st), name + "_det")
