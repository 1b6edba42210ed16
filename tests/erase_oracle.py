"""Host oracles of random erasing, shared by tests/test_random_erasing_cpu.py and
tests/test_gpu_random_erasing.py: the "pixel" fill of csrc/patchify.hip ``erase_normal`` in numpy (float64,
and the same formula in float32 as the yardstick of a kernel checked against float64), built on the hash
replica of tests/test_drop_path_cpu.py, and the erase formula one sample at a time."""
import numpy as np
import torch

from tests import test_drop_path_cpu as H

ERASE_SITE = 1 << 23
TWO_PI_F32 = np.float32(6.2831853)


def uniforms(seed: int, n: int):
    """(u1, u2) float64 [n] of elements 0 .. n - 1 at counter value ``seed``: u1 in (0, 1], u2 in [0, 1), both
    multiples of 2^-24 and hence exact in float32 too."""
    sd = H.site_seed(seed, ERASE_SITE)
    e = np.arange(n, dtype=np.uint64)
    h1 = H.rng_hash(sd, np.uint64(2) * e)
    h2 = H.rng_hash(sd, np.uint64(2) * e + np.uint64(1))
    u1 = ((h1 >> np.uint64(8)) + np.uint64(1)).astype(np.float64) * 2.0 ** -24
    u2 = (h2 >> np.uint64(8)).astype(np.float64) * 2.0 ** -24
    return u1, u2


def normal64(u1, u2):
    """The fill formula in float64 (with the kernel's float32 constant for 2 pi)."""
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(np.float64(TWO_PI_F32) * u2)


def normal32(u1, u2):
    """The same formula with every operation in float32: the yardstick."""
    u1, u2 = u1.astype(np.float32), u2.astype(np.float32)
    return np.sqrt(np.float32(-2.0) * np.log(u1)) * np.cos(TWO_PI_F32 * u2)


def loop_erase(x, plan, fill=None):
    """The erase formula one sample at a time, with slices (CPU fp32). ``fill``: the "pixel" values, a tensor of
    the batch's shape; a "const" plan carries its value."""
    out = x.clone()
    C = x.shape[1]
    for b in range(x.shape[0]):
        x0, y0, x1, y1 = plan.box[b].tolist()
        if plan.mode == "pixel":
            out[b, :, y0:y1, x0:x1] = fill[b, :, y0:y1, x0:x1]
        else:
            for c, v in enumerate(plan.channel_values(C)):
                out[b, c, y0:y1, x0:x1] = v
    return out
