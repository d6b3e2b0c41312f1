"""`--dump-outputs DIR`: what the timed path returned in its last timed step, as DIR/<name>.npy (float32, or float64 where the path computes
float64), so that two builds can be compared output for output. The inputs are seeded (weights, samples, synthetic volumes), so the same
arguments give the same inputs run to run. At most MAX_BYTES in all: past that every array is written as a fixed, seeded sample of its
flattened elements (the same indices for the same shape), each array its share of the budget in proportion to its size."""
import os

import numpy as np
import torch

MAX_BYTES = 60 << 20                     # 63 MB of array data: the .npy headers stay inside 64 MB
SAMPLE_SEED = 0


def host_copy(named):
    """{name: tensor} -> {name: host tensor}. Call it right after the timed region: graph replays overwrite their static outputs."""
    out = {}
    for k, v in named.items():
        v = v.detach()
        out[k] = v.to("cpu", torch.float64 if v.dtype == torch.float64 else torch.float32)
    return out


def dump_outputs(path, named):
    """Write {name: host tensor} as `path`/<name>.npy; returns {name: {shape, dtype, sampled elements or None}} for the full record."""
    os.makedirs(path, exist_ok=True)
    total = sum(v.numel() * v.element_size() for v in named.values())
    info = {}
    for k, v in named.items():
        a, sampled = v.reshape(-1), None
        if total > MAX_BYTES:
            n = max(1, int(a.numel() * (MAX_BYTES / total)))
            g = torch.Generator().manual_seed(SAMPLE_SEED)
            idx = torch.randperm(a.numel(), generator=g)[:n].sort().values
            a, sampled = a[idx], n
        else:
            a = v
        np.save(os.path.join(path, k + ".npy"), a.contiguous().numpy())
        info[k] = {"shape": list(v.shape), "dtype": str(a.numpy().dtype), "sampled_elements": sampled}
    return {"dir": path, "arrays": info}
