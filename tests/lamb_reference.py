"""Float64 reference of the LAMB step (csrc/lamb.hip, optim/lamb.py) on one parameter tensor: plain
tensor code that imports without a GPU or the extension. Rows, gradients and inputs are those of
tests/optim_reference.py."""
from __future__ import annotations

import torch

from tests.optim_reference import adam_grad, adam_inputs, row_values  # noqa: F401  (the LAMB tests' recipe too)


def lamb_step64(p, g, m, v, row, adapt, gscale=1.0):
    """One LAMB step of one tensor in float64 on (fp32) inputs. ``row``: a group row as ``row_values``
    takes it (its decoupled word is not read); ``adapt``: the group takes the trust ratio (weight decay
    non-zero or always_adapt). Returns float64 (p, m, v) and the floats (||w||, ||u||, r)."""
    lr, b1, b2, eps, wd, bc1, bc2_sqrt, _, omb1, omb2 = row_values(row)
    p, m, v = p.double().clone(), m.double().clone(), v.double().clone()
    gr = g.double() * float(gscale)
    m = b1 * m + omb1 * gr
    v = b2 * v + omb2 * gr * gr
    u = (m / bc1) / (v.sqrt() / bc2_sqrt + eps)
    if wd != 0.0:
        u = u + wd * p
    wn, un = float(p.square().sum().sqrt()), float(u.square().sum().sqrt())
    r = wn / un if (adapt and wn > 0.0 and un > 0.0) else 1.0
    p = p - lr * r * u
    return p, m, v, wn, un, r


EPS32 = 2.0 ** -24  # one fp32 rounding, relative
# ||w|| of a tensor as csrc/lamb.hip sums it: a thread adds at most 16 squares in sequence (16 additions and the
# squares' own roundings, one per addend), the wave's butterfly adds 6 levels, the four waves 2 more: at
# most 25 roundings on a sum of non-negative terms, 25 * 2^-24 = 1.5e-6 relative on the sum and half of that,
# 0.75e-6, on the norm; the chunk sums are added in double and the root is rounded once. Stated as 1e-6.
W_BOUND = 1e-6


def lamb_rounding_floors(p, g, m, v, row, adapt, gscale=1.0):
    """What fp32 arithmetic alone may cost one LAMB step of one tensor, worked out from the operation
    counts of the formula and the inputs, never from a result: elementwise absolute bounds (float64
    tensors) on the errors of m, v, u and p_after - p_before of any fp32 evaluation against
    ``lamb_step64``, and the relative bounds of the trust row that follow from them.

    With e = 2^-24 and gr = g * gscale (one rounding when gscale != 1; a row of Python doubles adds one
    rounding for every fp32 table value an expression reads):
      m = b1 m0 + (1 - b1) gr    two products and a sum: 3 e (|b1 m0| + |(1 - b1) gr|), the terms may cancel
      v = b2 v0 + (1 - b2) gr gr three products and a sum of non-negative terms: 4 e v (gr twice: + 2 e)
      a = (m / bc1) / (sqrt(v) / bc2_sqrt + eps): m's relative error, half of v's, and five operations
      u = a + wd p               one fma: e (|a| + |wd p|)
      p -= (lr r) u              r's own bound, the product lr r and the fma: e |p_after|
    ||u|| is summed as ||w|| is (W_BOUND) from u's fp32 values: + ||bound of u|| / ||u||; r is their
    quotient rounded once. Returns (bounds dict dp / m / v, (W_BOUND, u_bound, r_bound))."""
    import numpy as np

    lr, b1, b2, eps, wd, bc1, bc2_sqrt, _, omb1, omb2 = row_values(row)
    t = 0 if (isinstance(row, np.ndarray) and row.dtype == np.float32) else 1  # table values rounded to fp32
    s = 0 if float(gscale) == 1.0 else 1
    p0, m0, v0 = p.double(), m.double(), v.double()
    gr = g.double() * float(gscale)
    pr, mr, vr, wn, un, r = lamb_step64(p, g, m, v, row, adapt, gscale)
    f_m = (3 + s + 2 * t) * EPS32 * (b1 * m0.abs() + omb1 * gr.abs())
    f_v = (4 + 2 * s + 2 * t) * EPS32 * vr
    a = (mr / bc1) / (vr.sqrt() / bc2_sqrt + eps)
    zero = torch.zeros_like(a)
    rel_a = torch.where(mr != 0, f_m / mr.abs(), zero) + torch.where(vr != 0, 0.5 * f_v / vr, zero) + (5 + 3 * t) * EPS32
    f_u = a.abs() * rel_a + ((1 + t) * EPS32 * (a.abs() + abs(wd) * p0.abs()) if wd != 0.0 else 0.0)
    u = a + wd * p0 if wd != 0.0 else a
    u_bound = W_BOUND + (float(f_u.square().sum().sqrt()) / un if un > 0.0 else 0.0)
    r_bound = (W_BOUND + u_bound + EPS32) if r != 1.0 else 0.0
    f_dp = lr * r * f_u + lr * r * u.abs() * (r_bound + (1 + t) * EPS32) + EPS32 * pr.abs()
    return {"dp": f_dp, "m": f_m, "v": f_v}, (W_BOUND, u_bound, r_bound)


def floor_metrics(bound: torch.Tensor, ref: torch.Tensor):
    """An elementwise bound in the two metrics of ``errs64`` against ``ref``: (rel-L2, max)."""
    b, r = bound.double().reshape(-1), ref.double().reshape(-1)
    rn, rm = float(r.norm()), float(r.abs().max())
    if rn == 0.0:
        return float(b.norm()), float(b.max())
    return float(b.norm()) / rn, float(b.max()) / rm
