"""Float64 reference of the optimizer path (csrc/optim.hip, ``cast_f32_bf16``): plain tensor code that
imports without a GPU or the extension, and is itself checked against ``torch.optim.Adam`` / ``AdamW``
in float64 on the CPU (tests/test_optim.py).

A group row is one ``[8]`` row of the kernels' table (csrc/kernels.h ``AdamGroup``):
lr, beta1, beta2, eps, weight_decay, bc1 = 1 - beta1^t, bc2_sqrt = sqrt(1 - beta2^t), decoupled."""
from __future__ import annotations

import math
from typing import Sequence, Tuple

import numpy as np
import torch

BETAS = ((0.9, 0.999), (0.8, 0.95), (0.0, 0.5))


def group_row(lr, betas, eps, wd, step, decoupled) -> list:
    """One table row in Python doubles (the values torch.optim derives for step ``step``)."""
    b1, b2 = betas
    return [lr, b1, b2, eps, wd, 1.0 - b1 ** step, math.sqrt(1.0 - b2 ** step), bool(decoupled)]


def table_f32(rows: Sequence[Sequence]) -> np.ndarray:
    """Rows as the kernels take them (csrc/kernels.h AdamGroup): float32 [G, 10], the [8] row with the
    decoupled flag as integer bits in column 7, then 1 - beta1 and 1 - beta2 rounded from the double."""
    arr = np.zeros((len(rows), 10), dtype=np.float32)
    for i, r in enumerate(rows):
        arr[i, :7] = [float(x) for x in r[:7]]
        arr[i, 8:] = [1.0 - float(r[1]), 1.0 - float(r[2])]
    arr.view(np.int32)[:, 7] = [int(bool(r[7])) for r in rows]
    return arr


def row_values(row):
    """(lr, b1, b2, eps, wd, bc1, bc2_sqrt, decoupled, 1 - b1, 1 - b2) of a row. An [8] row of Python
    doubles gives 1 - beta in double. A float32 table row is read as the kernel reads it: fp32 values
    widened exactly, the flag from its integer bits, 1 - beta from columns 8 and 9."""
    if isinstance(row, torch.Tensor):
        row = row.detach().cpu().numpy()
    if isinstance(row, np.ndarray) and row.dtype == np.float32:
        assert row.shape == (10,)
        dec = bool(np.ascontiguousarray(row).view(np.int32)[7] != 0)
        return tuple(float(x) for x in row[:7]) + (dec, float(row[8]), float(row[9]))
    return tuple(float(x) for x in row[:7]) + (bool(row[7]), 1.0 - float(row[1]), 1.0 - float(row[2]))


def adam_step64(p, g, m, v, group_row, gscale=1.0):
    """One Adam / AdamW step in float64 on (fp32) inputs; returns float64 (p, m, v)."""
    lr, b1, b2, eps, wd, bc1, bc2_sqrt, decoupled, omb1, omb2 = row_values(group_row)
    p, m, v = p.double().clone(), m.double().clone(), v.double().clone()
    gr = g.double() * float(gscale)
    if decoupled:
        p = p * (1.0 - lr * wd)
    elif wd != 0.0:
        gr = gr + wd * p
    m = b1 * m + omb1 * gr
    v = b2 * v + omb2 * gr * gr
    denom = v.sqrt() / bc2_sqrt + eps
    p = p - (lr / bc1) * m / denom
    return p, m, v


def norm64(flat: torch.Tensor) -> float:
    """L2 norm of a flat buffer accumulated in float64."""
    return float(flat.double().square().sum().sqrt())


def expand_segments(seg_start: Sequence[int], seg_group: Sequence[int], n: int) -> torch.Tensor:
    """Per-element group index (int64 [n], -1 frozen) of a segment table whose first segment starts
    at 0: segment i covers [seg_start[i], seg_start[i + 1]), the last one runs to n."""
    starts = [int(s) for s in seg_start]
    assert starts and starts[0] == 0 and starts == sorted(starts) and starts[-1] < n
    lens = torch.tensor([b - a for a, b in zip(starts, starts[1:] + [n])], dtype=torch.int64)
    return torch.repeat_interleave(torch.tensor([int(x) for x in seg_group], dtype=torch.int64), lens)


def bf16_rne_bits(x: torch.Tensor) -> torch.Tensor:
    """bfloat16 bit patterns (int32 in 0 .. 65535) of an fp32 tensor, round to nearest even, by integer
    arithmetic on the fp32 bits only. NaN stays NaN (the quiet bit is set, the payload's top bits kept)."""
    assert x.dtype == torch.float32
    b = x.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    nan = ((b & 0x7F800000) == 0x7F800000) & ((b & 0x007FFFFF) != 0)
    r = (b + 0x7FFF + ((b >> 16) & 1)) >> 16
    return torch.where(nan, (b >> 16) | 0x40, r).to(torch.int32)


def bf16_bits(t: torch.Tensor) -> torch.Tensor:
    """Bit patterns (int32 in 0 .. 65535) of a bfloat16 tensor."""
    assert t.dtype == torch.bfloat16
    return t.contiguous().view(torch.int16).to(torch.int32) & 0xFFFF


def bf16_is_nan(bits: torch.Tensor) -> torch.Tensor:
    return ((bits & 0x7F80) == 0x7F80) & ((bits & 0x007F) != 0)


def adam_inputs(n: int, gen: torch.Generator, device="cpu"):
    """The input recipe of the optimizer checks: parameters randn * 0.05."""
    return torch.randn(n, generator=gen, device=device) * 0.05


def adam_grad(n: int, gen: torch.Generator, device="cpu") -> torch.Tensor:
    """Gradients with magnitudes log-uniform over 1e-6 .. 1e2, random signs, every 97th exactly zero."""
    mag = torch.pow(10.0, torch.rand(n, generator=gen, device=device) * 8.0 - 6.0)
    sign = (torch.rand(n, generator=gen, device=device) < 0.5).float() * 2.0 - 1.0
    g = mag * sign
    g[::97] = 0.0
    return g


def cast_planted_values() -> torch.Tensor:
    """fp32 values at the edges of the bf16 rounding: exact ties on even and odd upper halves in both
    signs, one bit below and above a tie, +-0, +-Inf, NaN, the largest finite value (rounds to Inf)
    and the smallest normal. No subnormals."""
    bits = []
    # odd, even, odd, even upper halves; the first value is a tie that rounds up (truncation differs)
    for hi in (0x3F81, 0x3F80, 0x4049, 0x404A):
        for sign in (0, 0x8000):
            for lo in (0x8000, 0x7FFF, 0x8001):
                bits.append(((hi | sign) << 16) | lo)
    bits += [0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0x7F800001, 0xFFC12345,
             0x7F7FFFFF, 0xFF7FFFFF, 0x00800000, 0x80800000]
    a = np.array(bits, dtype=np.uint32).view(np.float32)
    return torch.from_numpy(a.copy())
