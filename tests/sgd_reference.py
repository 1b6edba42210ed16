"""Float64 numpy reference of the SGD step (csrc/sgd.hip, optim/sgd.py) and what fp32 arithmetic alone may
cost it: plain array code that imports without a GPU or the extension, itself held to float64
``torch.optim.SGD`` on the CPU (tests/test_sgd_cpu.py).

Per element, ``c`` the clip coefficient::

    g' = g * c
    g' = g' + wd * p                          (wd != 0)
    buf = momentum * buf + g'                 (momentum != 0; buf starts at zero)
    d  = g' + momentum * buf if nesterov else buf       (d = g' where momentum == 0)
    p  = p - lr * d
"""
from __future__ import annotations

import numpy as np

EPS32 = 2.0 ** -24  # one fp32 rounding, relative


def _f64(x) -> np.ndarray:
    if hasattr(x, "detach"):
        x = x.detach().cpu().numpy()
    return np.asarray(x, dtype=np.float64)


def sgd_step64(p, g, buf, lr, momentum=0.0, wd=0.0, nesterov=False, gscale=1.0):
    """One step in float64 on (fp32 or fp64) arrays or tensors. Returns float64 numpy ``(p, buf)``; with
    ``momentum == 0`` the buffer comes back as it went in (it is not part of the step)."""
    p, g, buf = _f64(p), _f64(g), _f64(buf)
    gr = g * float(gscale)
    if wd != 0.0:
        gr = gr + float(wd) * p
    if momentum != 0.0:
        buf = float(momentum) * buf + gr
        d = gr + float(momentum) * buf if nesterov else buf
    else:
        buf = buf.copy()
        d = gr
    return p - float(lr) * d, buf


def sgd_rounding_floors(p, g, buf, lr, momentum=0.0, wd=0.0, nesterov=False, gscale=1.0):
    """What fp32 arithmetic alone may cost one step, from the operation counts of the formula and the inputs,
    never from a result: elementwise absolute bounds (float64 arrays) on the errors of ``p_after - p_before``
    and of ``buf`` of any fp32 evaluation (each operation rounded once, fused or not) against ``sgd_step64``
    fed the same fp32 hyper-parameters. With e = 2^-24, to first order:

      gr = g c                  one product when c != 1:                s e |gr|
      g' = gr + wd p            (wd != 0) a product and a sum:          + e |wd p| + e |g'|
      buf = mom buf0 + g'       a product and a sum, and g''s error:    f_g + e |mom buf0| + e |buf|
      d = g' + mom buf          (Nesterov) the same, buf's error scaled: f_g + mom f_buf + e |mom buf| + e |d|
      p = p0 - lr d             a product and a sum, d's error scaled:  lr f_d + e |lr d| + e |p|

    A fused multiply-add saves the product's rounding and stays inside. Returns ``{"dp": ..., "buf": ...}``
    (``buf`` all zeros where ``momentum == 0``: the buffer must not change at all)."""
    p0, g, b0 = _f64(p), _f64(g), _f64(buf)
    lr, mom, wd = float(lr), float(momentum), float(wd)
    s = 0.0 if float(gscale) == 1.0 else 1.0
    gr = g * float(gscale)
    f_g = s * EPS32 * np.abs(gr)
    gp = gr
    if wd != 0.0:
        gp = gr + wd * p0
        f_g = f_g + EPS32 * (np.abs(wd * p0) + np.abs(gp))
    if mom != 0.0:
        b = mom * b0 + gp
        f_b = f_g + EPS32 * (np.abs(mom * b0) + np.abs(b))
        if nesterov:
            d = gp + mom * b
            f_d = f_g + mom * f_b + EPS32 * (np.abs(mom * b) + np.abs(d))
        else:
            d, f_d = b, f_b
    else:
        d, f_d, f_b = gp, f_g, np.zeros_like(p0)
    pn = p0 - lr * d
    f_dp = lr * f_d + EPS32 * (np.abs(lr * d) + np.abs(pn))
    return {"dp": f_dp, "buf": f_b}


def errs64(out, ref):
    """(rel-L2, max error / max |ref|) of one array against a float64 reference; absolute for an all-zero one."""
    o, r = _f64(out).reshape(-1), _f64(ref).reshape(-1)
    d = o - r
    rn, rm = float(np.linalg.norm(r)), float(np.abs(r).max()) if r.size else 0.0
    if rn == 0.0:
        return float(np.linalg.norm(d)), float(np.abs(d).max()) if d.size else 0.0
    return float(np.linalg.norm(d)) / rn, float(np.abs(d).max()) / rm


def floor_metrics(bound, ref):
    """An elementwise bound in the two metrics of ``errs64`` against ``ref``: (rel-L2, max)."""
    b, r = _f64(bound).reshape(-1), _f64(ref).reshape(-1)
    rn, rm = float(np.linalg.norm(r)), float(np.abs(r).max()) if r.size else 0.0
    if rn == 0.0:
        return float(np.linalg.norm(b)), float(b.max()) if b.size else 0.0
    return float(np.linalg.norm(b)) / rn, float(b.max()) / rm
