"""What the raw-ctypes GPU tests of the depth nests share (test_gpu_wino_depth_nest.py, test_gpu_wino_depth_nest4.py): canary-patterned output buffers
with guard rows, NaN-padded operands, the run-twice check. No fixtures here: those stay in the test files."""
import ctypes

import torch

import conv_igemm_cases as cc

F32, NAN = torch.float32, float("nan")
FWD = 1e-5                    # test_gpu_convgru_matrix.py's forward bound (relative to max |reference|)
EINVAL = -1


def emitter(tag):
    """print-a-row function of one matrix record (profiles/*_matrix.txt under -s): every line starts with `tag`."""
    return lambda line: print(tag + " " + line)


def P(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


class OutBuf:
    """planes x rows x ld floats inside a CANARY-filled allocation with guard rows on both sides; every element of the body is named."""

    def __init__(self, dev, planes, rows, ld):
        self.shape, self.G = (planes, rows, ld), 4 * ld
        self.t = torch.full((2 * self.G + planes * rows * ld,), cc.CANARY, dtype=torch.int32, device=dev)

    def ptr(self):
        return ctypes.c_void_p(self.t.data_ptr() + 4 * self.G)

    def fetch(self, what):
        torch.cuda.synchronize()
        raw = self.t.cpu()
        assert (raw[:self.G] == cc.CANARY).all() and (raw[-self.G:] == cc.CANARY).all(), (what, "guard rows were written")
        body = raw[self.G:-self.G].view(F32).reshape(self.shape).clone()
        assert torch.isfinite(body).all(), (what, "a named element is not finite")
        return body


def twice(fn, buf, what):
    outs = []
    for _ in range(2):
        buf.t.fill_(cc.CANARY)
        fn()
        outs.append(buf.fetch(what))
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32)), (what, "two runs differ")
    return outs[0]


def padded(t, dev, guard=4096):
    """t on the device between NaN guards (operand padding): the tensor view of the middle."""
    flat = torch.full((t.numel() + 2 * guard,), NAN, dtype=F32)
    flat[guard:guard + t.numel()] = t.reshape(-1)
    return flat.to(dev)[guard:guard + t.numel()].view(t.shape)
