"""Numerics checks of every HIP kernel against a plain PyTorch fp32 reference of the same op.

Each check returns ``(name, metrics, limits)``: ``metrics`` maps a measured quantity to its value,
``limits`` the same keys to the largest value that passes. Error metrics are per tensor:

* ``l2``  = ||out - ref||_2 / ||ref||_2   (relative L2 over the whole tensor),
* ``max`` = max|out - ref| / max|ref|     (max error relative to the tensor's largest value),

worst over the tensors a check compares; boolean properties (masks agree, other rows stay zero,
...) are 0 / 1 metrics with limit 0. The limits are about 2x the errors measured on MI355X for that
check (``python tests/kernel_checks.py`` prints every measured value; so does the pytest summary).
Used by tests/test_gpu_kernels.py (pytest -m gpu).
"""
from __future__ import annotations

import math
import os
import sys
from typing import Callable, Dict, List, Tuple

import torch
import torch.nn.functional as F

sys.path.insert(0, os.environ.get("PVR_PKG_ROOT") or os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pytorch_vit_paper_replication_amd import _ext  # noqa: E402
from pytorch_vit_paper_replication_amd.ops import gemm as G  # noqa: E402

DEV = "cuda"
Result = Tuple[str, Dict[str, float], Dict[str, float]]


def errs(out: torch.Tensor, ref: torch.Tensor) -> Tuple[float, float]:
    """(relative L2, max error / max |ref|) of one tensor."""
    o, r = out.float().reshape(-1), ref.float().reshape(-1)
    d = o - r
    rn = r.norm().item()
    rm = r.abs().max().item() if r.numel() else 0.0
    if rn == 0.0:  # an all-zero reference: absolute errors
        return d.norm().item(), (d.abs().max().item() if d.numel() else 0.0)
    return d.norm().item() / rn, d.abs().max().item() / rm


def worst(*pairs: Tuple[torch.Tensor, torch.Tensor]) -> Dict[str, float]:
    l2 = mx = 0.0
    for o, r in pairs:
        a, b = errs(o, r)
        l2, mx = max(l2, a), max(mx, b)
    return {"l2": l2, "max": mx}


def lim(l2: float, mx: float, **flags: float) -> Dict[str, float]:
    d = {"l2": l2, "max": mx}
    d.update(flags)
    return d


def passed(metrics: Dict[str, float], limits: Dict[str, float]) -> bool:
    return all(metrics[k] <= limits[k] for k in limits)


def fmt_metrics(metrics: Dict[str, float], limits: Dict[str, float]) -> str:
    return " ".join(f"{k}={metrics[k]:.2e}/{limits[k]:.1e}" for k in limits)


def bf(x):
    return x.to(torch.bfloat16)


def rnd(*shape, scale=1.0):
    return (torch.randn(*shape, device=DEV) * scale)


class tile:
    """Context: force one GEMM tile config (gemm.FORCE_TILE test hook)."""

    def __init__(self, t):
        self.t = t

    def __enter__(self):
        self.old = G.FORCE_TILE
        G.FORCE_TILE = self.t

    def __exit__(self, *exc):
        G.FORCE_TILE = self.old


def rate_limit(p: float, n: int) -> float:
    """5 sigma of a Bernoulli(p) rate estimated from n draws (the mask-rate tolerance)."""
    return 5.0 * math.sqrt(max(p * (1 - p), 1e-12) / max(n, 1))


# ----------------------------------------------------------------------------- GEMM
def check_gemm_fwd(M, N, K, t=0, bias=True, resid=False) -> Result:
    x, w = bf(rnd(M, K)), bf(rnd(N, K, scale=0.05))
    b = rnd(N) if bias else None
    r = bf(rnd(M, N)) if resid else None
    with tile(t):
        y = G.linear_fwd(x, w, b, resid=r)
    ref = x.float() @ w.float().t()
    if b is not None:
        ref = ref + b
    if r is not None:
        ref = ref + r.float()
    return (f"gemm_fwd M{M} N{N} K{K} t{t} b{int(bias)} r{int(resid)}", worst((y, ref)), lim(3.5e-3, 7e-3))


def check_gemm_gelu(M, N, K, t=0):
    x, w, b = bf(rnd(M, K)), bf(rnd(N, K, scale=0.05)), rnd(N)
    u = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
    with tile(t):
        h = G.linear_fwd(x, w, b, gelu_aux=u)
    prod = x.float() @ w.float().t()
    if t == 15:  # tile 15 hands the product to its epilogue waves in bf16 (autocast Linear rounding)
        prod = prod.bfloat16().float()
    uref = (prod + b).requires_grad_(True)
    gp = torch.autograd.grad(F.gelu(uref), uref, torch.ones_like(uref))[0]
    # tile 15: a bf16 ulp of max deviation on top (the rounded product and the rounded outputs can
    # land on opposite sides of the reference)
    return (f"gemm_gelu M{M} N{N} K{K} t{t}", worst((u, gp), (h, F.gelu(uref.detach()))), lim(4e-3, 7e-3 if t != 15 else 1.6e-2))


def check_gemm_gelu_dropout(M, N, K, tiles=(12, 13), l2_lim=1e-3):
    """GELU + dropout + aux epilogue: identical masks and values across GEMM structures (tile 15
    rounds the pre-activation to bf16 before the GELU, as an autocast Linear output is: ``l2_lim``
    then allows that rounding, the fp32-reference tolerance of check_gemm_gelu)."""
    x, w, b = bf(rnd(M, K)), bf(rnd(N, K, scale=0.05)), rnd(N)
    seed = torch.tensor([777], dtype=torch.int64, device=DEV)
    outs = []
    for t in tiles:
        with tile(t):
            u = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
            h = G.linear_fwd(x, w, b, gelu_aux=u, drop=(seed, 5 << 32, 0.1))
            outs.append((h, u))
    h0, u0 = outs[0]
    same_mask = all(torch.equal(h0 == 0, h1 == 0) and torch.equal(u0 == 0, u1 == 0) for h1, u1 in outs[1:])
    rate = (u0 == 0).float().mean().item()
    m = worst(*[pair for h1, u1 in outs[1:] for pair in ((h1, h0), (u1, u0))])
    m.update(mask_differs=float(not same_mask), rate_dev=abs(rate - 0.1))
    return (f"gemm_gelu+dropout M{M} N{N} K{K} tiles{tiles} (drop rate {rate:.4f})", m,
            lim(l2_lim, 8e-3 if 15 not in tiles else 1.6e-2, mask_differs=0, rate_dev=rate_limit(0.1, M * N)))  # same values (1-ulp flips tolerated)


def check_gemm_gelu_drop_paths(M=3000, N=768, p=0.1):
    """GELU + dropout epilogue: the keep mask is one function of (seed, element index), the same for
    short and long K loops (K 256 / 1024) in the one-tile (12) and persistent (13) kernels. u = 1 + bias
    (inputs of ones, weights 1/K) keeps every kept output away from 0, so h == 0 is exactly the drop
    mask."""
    seed = torch.tensor([31337], dtype=torch.int64, device=DEV)
    b = rnd(N, scale=0.1)
    masks, names = [], []
    for K in (256, 1024):
        x, w = bf(torch.ones(M, K, device=DEV)), bf(torch.full((N, K), 1.0 / K, device=DEV))
        for t in (12, 13, 15):
            with tile(t):
                u = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
                h = G.linear_fwd(x, w, b, gelu_aux=u, drop=(seed, 11 << 32, p))
            masks.append(h == 0)
            names.append((K, t))
    differs = sum(int((mk != masks[0]).sum()) for mk in masks[1:])
    rate = masks[0].float().mean().item()
    m = {"mask_differs": float(differs), "rate_dev": abs(rate - p)}
    return (f"gemm_gelu drop mask: K 256 vs K 1024, tiles 12 / 13 / 15 (rate {rate:.4f})", m,
            {"mask_differs": 0, "rate_dev": rate_limit(p, M * N)})


def check_gemm_dgelu_tiles(M=5000, N=3072, K=768):
    """dGELU dgrad + bias-gradient column sums on the one-tile (12) and persistent (13) ping-pong
    kernels (the persistent one is the default at ViT sizes since round 5) vs fp32."""
    dy, w, g = bf(rnd(M, K)), bf(rnd(K, N, scale=0.05)), bf(rnd(M, N))
    wt = w.t().contiguous()
    ref = (dy.float() @ w.float()) * g.float()
    m = {}
    for t in (12, 13):
        with tile(t):
            cs = torch.zeros(N, device=DEV)
            out = G.linear_dgrad(dy, w, dgelu_aux=g, wt=wt, colsum=cs)
        l2, mx = errs(out, ref)
        l2c, _ = errs(cs, ref.sum(0))
        m.update({f"t{t}_l2": l2, f"t{t}_max": mx, f"t{t}_colsum_l2": l2c})
    return (f"gemm dGELU dgrad + colsum M{M} N{N} K{K}, tiles 12 / 13 vs fp32", m,
            {"t12_l2": 3.5e-3, "t12_max": 7e-3, "t12_colsum_l2": 1.5e-6, "t13_l2": 3.5e-3, "t13_max": 7e-3, "t13_colsum_l2": 1.5e-6})


def check_gemm_small_splitk(M, N, K, resid=False, gelu=False):
    """Serving-size forward GEMM (few output tiles): split-K fp32 partials + the reduction pass with
    bias / exact GELU / residual, vs a PyTorch fp32 reference."""
    S = G._small_splitk(M, N, K)
    x, w, b = bf(rnd(M, K)), bf(rnd(N, K, scale=0.05)), rnd(N)
    r = bf(rnd(M, N)) if resid else None
    y = G.linear_fwd(x, w, b, resid=r, gelu=gelu)
    ref = x.float() @ w.float().t() + b
    if gelu:
        ref = F.gelu(ref)
    if resid:
        ref = ref + r.float()
    m = worst((y, ref))
    m["not_split"] = float(S < 2)
    return (f"gemm small-M split-K M{M} N{N} K{K} S{S} resid{int(resid)} gelu{int(gelu)}", m, lim(3.5e-3, 7e-3, not_split=0))


def check_gemm_patch_embed_epilogue(B=20, n_p=196, D=768, K=768, p=0.1):
    """Patch-embedding GEMM epilogue (rows remapped past each image's CLS row, + position embedding,
    + dropout on the token index) on the ping-pong kernel (tile 12) vs the 128x128 kernel (tile 0):
    same values, same dropout mask, CLS rows untouched."""
    ntok = n_p + 1
    x, w, b = bf(rnd(B * n_p, K)), bf(rnd(D, K, scale=0.05)), rnd(D)
    pos = rnd(ntok, D)
    seed = torch.tensor([2024], dtype=torch.int64, device=DEV)
    outs = []
    for t in (0, 12):
        with tile(t):
            out = torch.full((B * ntok, D), 7.0, dtype=torch.bfloat16, device=DEV)
            G.linear_fwd(x, w, b, addend=pos, addend_period=ntok, row_remap=(n_p, ntok, 1), drop=(seed, 0, p), out=out)
            outs.append(out)
    a, c = outs
    cls = torch.arange(B, device=DEV) * ntok
    cls_ok = bool((a[cls] == 7.0).all().item() and (c[cls] == 7.0).all().item())
    same_mask = torch.equal(a == 0, c == 0)
    rate = (c == 0).float().mean().item()
    m = worst((c, a))
    m.update(cls_or_mask_bad=float(not (cls_ok and same_mask)), rate_dev=abs(rate - p * n_p / ntok))
    return (f"patch-embed GEMM epilogue tile 12 vs tile 0 (mask {same_mask}, CLS rows {cls_ok})", m,
            lim(1e-3, 8e-3, cls_or_mask_bad=0, rate_dev=rate_limit(p, B * n_p * D)))


class gemm_tail:
    """Context: split-K tail of the last dispatch round on / off (ext.set_gemm_tail)."""

    def __init__(self, on: bool):
        self.on = on

    def __enter__(self):
        _ext.ext().set_gemm_tail(self.on)

    def __exit__(self, *exc):
        _ext.ext().set_gemm_tail(True)


def check_gemm_tail_split(M=50432, N=768, K=768, kind="resid_drop", p=0.1):
    """Split-K tail (the leftover tiles of the last dispatch round as K-parts, fp32 partial tiles
    handed to the last part through an agent-scope release / acquire) on the ping-pong kernel vs the
    same GEMM with one workgroup per tile: same dropout masks, values within fp32 reassociation
    (bf16 1-ulp flips), bitwise identical across two runs (fixed summation order), and vs fp32.
    kind: resid_drop (fc2 forward), gelu (fc1 forward + aux), dgelu (dGELU dgrad + column sum),
    patch (position-embedding addend, row remap, dropout)."""
    seed = torch.tensor([4242], dtype=torch.int64, device=DEV)
    drop = (seed, 9 << 32, p)
    if kind == "dgelu":
        dy, w, g = bf(rnd(M, K)), bf(rnd(K, N, scale=0.05)), bf(rnd(M, N))
        wt = w.t().contiguous()

        def run():
            cs = torch.zeros(N, device=DEV)
            out = G.linear_dgrad(dy, w, dgelu_aux=g, wt=wt, colsum=cs)
            return out, cs
        ref = (dy.float() @ w.float()) * g.float()
        refs = (ref, ref.sum(0))
    else:
        x, w, b = bf(rnd(M, K)), bf(rnd(N, K, scale=0.05)), rnd(N)
        if kind == "gelu":
            def run():
                u = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
                h = G.linear_fwd(x, w, b, gelu_aux=u, drop=drop)
                return h, u
        elif kind == "patch":
            n_p = 196
            ntok = n_p + 1
            Bimg = M // n_p
            x = x[:Bimg * n_p]
            pos = rnd(ntok, N)

            def run():
                out = torch.full((Bimg * ntok, N), 7.0, dtype=torch.bfloat16, device=DEV)
                G.linear_fwd(x, w, b, addend=pos, addend_period=ntok, row_remap=(n_p, ntok, 1), drop=drop, out=out)
                return (out,)
        else:
            r = bf(rnd(M, N))

            def run():
                return (G.linear_fwd(x, w, b, resid=r, drop=drop),)
        refs = None
    # dropped elements: 0 without a residual, exactly the residual with one (out = resid + 0)
    dropped = (lambda t: t == r) if kind == "resid_drop" else (lambda t: t == 0)
    old_units, G.DGRAD_TAIL_UNITS = G.DGRAD_TAIL_UNITS, 0  # the backward's split-round limit off: split here
    try:
        with tile(12):
            with gemm_tail(False):
                base = run()
            a = run()
            c = run()
    finally:
        G.DGRAD_TAIL_UNITS = old_units
    m = worst(*zip(a, base))
    # (the dGELU column sum accumulates with float atomics: its order, hence its last bits, vary run
    # to run with or without the split; determinism is checked on the GEMM outputs)
    m["nondeterministic"] = float(not all(torch.equal(u, v) for u, v in zip(a[:1] if kind == "dgelu" else a, c)))
    # with a residual, a kept element whose value is below half a bf16 ulp of the residual also reads
    # as "dropped", and fp32 reassociation can flip such a borderline element: a tiny tolerance there
    # without one, a kept output whose pre-activation sits at ~0 (or a GELU of a very negative one) can
    # round to exactly 0 in one summation order and not the other (seen: u ~ -1e-7): such flips are not
    # mask differences, which would zero O(1) values
    flip = dropped(a[0]) != dropped(base[0])
    if kind != "resid_drop":
        flip &= torch.maximum(a[0].float().abs(), base[0].float().abs()) > 1e-3
    diff = flip.float().mean().item() if kind != "dgelu" else 0.0
    m["mask_differs"] = diff if kind == "resid_drop" else float(diff > 0)
    if refs is not None:
        l2, mx = errs(a[0], refs[0])
        l2c, mxc = errs(a[1], refs[1])
        m.update(ref_l2=l2, ref_max=mx, colsum_l2=l2c)
        lims = lim(1e-3, 8e-3, nondeterministic=0, mask_differs=0, ref_l2=3.5e-3, ref_max=7e-3, colsum_l2=1.5e-6)
    else:
        lims = lim(1e-3, 8e-3, nondeterministic=0, mask_differs=2e-6 if kind == "resid_drop" else 0)
    tiles = math.ceil(M / 256) * math.ceil(N / 256)
    S = _ext.ext().gemm_tail_split(M, N, K, 2)
    m["not_split"] = float(S < 2)
    lims["not_split"] = 0
    return (f"gemm split-K tail {kind} M{M} N{N} K{K} ({tiles} tiles, {S} K-parts) vs one workgroup per tile", m, lims)


def check_gemm_tail_split_fp8(M=65792, N=1280, K=5120):
    """The split-K tail on the fp8 (e4m3) forward GEMM (ViT-H/14 fc2 shape: 1285 tiles = 5 rounds + 5)."""
    from pytorch_vit_paper_replication_amd.ops import fp8 as F8

    x, w, b, r = bf(rnd(M, K)), bf(rnd(N, K, scale=0.05)), rnd(N), bf(rnd(M, N))
    xq, xs, _ = _fp8_operand(x)
    wq, ws, _ = _fp8_operand(w)

    def run():
        return F8.linear_fwd_fp8(xq, xs, wq, ws, b, resid=r)
    with gemm_tail(False):
        base = run()
    a, c = run(), run()
    m = worst((a, base))
    m["nondeterministic"] = float(not torch.equal(a, c))
    S = _ext.ext().gemm_tail_split(M, N, K, 1)
    m["not_split"] = float(S < 2)
    return (f"gemm_fp8 split-K tail M{M} N{N} K{K} ({S} K-parts) vs one workgroup per tile", m,
            lim(1e-3, 8e-3, nondeterministic=0, not_split=0))


def check_gemm_dgrad(M, N, K, t=0, transposed=False):
    dy, w = bf(rnd(M, N)), bf(rnd(N, K, scale=0.05))
    with tile(t):
        dx = G.linear_dgrad(dy, w, wt=w.t().contiguous() if transposed else None)
    return (f"gemm_dgrad M{M} N{N} K{K} t{t} wt{int(transposed)}", worst((dx, dy.float() @ w.float())), lim(3.5e-3, 7e-3))


def check_gemm_dgelu(M, N, K, transposed=False, t=None):
    """dGELU dgrad epilogue and its fused column sum (the fc1 bias gradient, fp32 from the fp32
    accumulator, before bf16 rounding)."""
    dy, w, g = bf(rnd(M, N)), bf(rnd(N, K, scale=0.05)), bf(rnd(M, K))
    cs = torch.zeros(K, device=DEV)
    # with W^T the tile comes from the selection (forced through the test hook), else from `tile=`
    with tile(t if transposed else None):
        dx = G.linear_dgrad(dy, w, dgelu_aux=g, wt=w.t().contiguous() if transposed else None, tile=t, colsum=cs)
    ref = (dy.float() @ w.float()) * g.float()
    m = worst((dx, ref))
    l2c, mxc = errs(cs, ref.sum(0))
    m.update(colsum_l2=l2c, colsum_max=mxc)
    return (f"gemm_dgelu M{M} N{N} K{K} wt{int(transposed)} t{t}", m, lim(3.5e-3, 7e-3, colsum_l2=1.5e-6, colsum_max=1.5e-6))


def check_gemm_wgrad(T, N, K, t=0):
    dy, x = bf(rnd(T, N)), bf(rnd(T, K))
    out = torch.zeros(N, K, device=DEV)
    with tile(t):
        G.linear_wgrad(dy, x, out)
        G.linear_wgrad(dy, x, out)  # accumulates
    ref = 2 * (dy.float().t() @ x.float())
    return (f"gemm_wgrad T{T} N{N} K{K} t{t}", worst((out, ref)), lim(1e-6, 4e-6))


def check_gemm_wgrad_fixup(T, N, K):
    """Weight gradient with the in-launch split-K reduction (each split adds 1/S of its tile, the
    slabs summed in a fixed order): vs the fp32 product, accumulating into a non-zero out, bitwise
    repeatable, no spin timeout; and vs the separate-reduce-pass path."""
    ext = _ext.ext()
    dy, x = bf(rnd(T, N)), bf(rnd(T, K))
    init = rnd(N, K)
    outs = []
    prev = G.SPLITK_FIXUP
    for fix in (True, True, False):
        G.SPLITK_FIXUP = fix
        try:
            out = init.clone()
            with tile(12):
                G.linear_wgrad(dy, x, out)
            outs.append(out)
        finally:
            G.SPLITK_FIXUP = prev
    torch.cuda.synchronize()
    timeouts = ext.splitk_timeouts(dy, True)
    ref = init + dy.float().t() @ x.float()
    m = worst((outs[0], ref), (outs[0], outs[2]))
    m.update(repeat_differs=float(not torch.equal(outs[0], outs[1])), timeouts=float(timeouts))
    # fp32 sums over 12k-50k tokens: the accumulation error of either order grows past the short-T 1e-6
    return (f"gemm_wgrad in-launch split-K T{T} N{N} K{K}", m, lim(3e-6, 1e-5, repeat_differs=0, timeouts=0))


def check_gemm_dropout(M=512, N=256, K=128, p=0.1, t=None):
    x, w = bf(torch.ones(M, K, device=DEV)), bf(torch.full((N, K), 1.0 / K, device=DEV))
    seed = torch.tensor([12345], dtype=torch.int64, device=DEV)
    with tile(t):
        y = G.linear_fwd(x, w, None, drop=(seed, 7 << 32, p))
    keep = (y.float() != 0)
    rate = 1 - keep.float().mean().item()
    scale_dev = abs(y.float()[keep].mean().item() - 1.0 / (1 - p))
    # backward mask (colsum kernel) must zero exactly the same elements
    dz = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
    db = torch.zeros(N, device=DEV)
    G.bias_grad(bf(torch.ones(M, N, device=DEV)), db, drop=(seed, 7 << 32, p), dz=dz)
    same = torch.equal(dz.float() != 0, keep)
    m = {"rate_dev": abs(rate - p), "scale_dev": scale_dev, "bwd_mask_differs": float(not same)}
    return (f"dropout rate/scale/fwd-bwd mask tile{t} (rate {rate:.4f})", m,
            {"rate_dev": rate_limit(p, M * N), "scale_dev": 3.5e-3, "bwd_mask_differs": 0})  # bf16 rounding of the scale


# ----------------------------------------------------------------------------- patch embedding / layout
def check_im2col(B, C, H, P):
    ext = _ext.ext()
    img = rnd(B, C, H, H)
    kc = C * P * P
    kp = (kc + 63) // 64 * 64
    g = H // P
    out = torch.empty(B * g * g, kp, dtype=torch.bfloat16, device=DEV)
    ext.im2col(img, out, P, kp)
    ref = img.reshape(B, C, g, P, g, P).permute(0, 2, 4, 1, 3, 5).reshape(B * g * g, kc)
    ref = F.pad(ref, (0, kp - kc))
    return (f"im2col B{B} C{C} H{H} P{P}", worst((out, bf(ref))), lim(0, 0))


def check_patch_bwd(B, ntok, D, p=0.1):
    """Patch-embedding backward (dropout mask from the shared counter hash) vs torch sums."""
    ext = _ext.ext()
    dE = bf(rnd(B * ntok, D))
    seed = torch.tensor([4242], dtype=torch.int64, device=DEV)
    off = 3 << 32
    mask = torch.empty_like(dE)  # mask from the column-sum kernel on ones (same hash)
    ext.colsum(bf(torch.ones(B * ntok, D, device=DEV)), B * ntok, D, None, mask, seed, off, p)
    thr = min(int(round(p * 65536)), 65535)
    dpre = dE.float() * (mask.float() != 0).float() * (65536.0 / (65536.0 - thr))  # the kernels' exact fp32 scale
    gpos, gcls, gb = torch.zeros(ntok, D, device=DEV), torch.zeros(D, device=DEV), torch.zeros(D, device=DEV)
    dconv = torch.empty(B * (ntok - 1), D, dtype=torch.bfloat16, device=DEV)
    ext.patch_bwd(dE, B, ntok, D, gpos.view(-1), gcls, dconv, gb, seed, off, p)
    d3 = dpre.view(B, ntok, D)
    sums = worst((gpos, d3.sum(0)), (gcls, d3[:, 0].sum(0)), (gb, d3[:, 1:].sum((0, 1))))
    dc = worst((dconv, d3[:, 1:].reshape(-1, D)))
    m = {"sums_l2": sums["l2"], "sums_max": sums["max"], "dconv_l2": dc["l2"], "dconv_max": dc["max"]}
    return (f"patch_bwd B{B} ntok{ntok} D{D} p{p}", m, {"sums_l2": 5e-6, "sums_max": 2e-5, "dconv_l2": 3.5e-3, "dconv_max": 7e-3})


def check_patch_wgrad_narrow(T, D=1280, kc=588):
    """Patch-embedding weight gradient with K padded to the tile (kc = C*P*P -> kp): the split-K
    reduction writes the first kc columns straight into the [D, kc] gradient (accumulating), and
    pad_cols_bf16 builds the zero-padded bf16 weight the forward GEMM reads."""
    ext = _ext.ext()
    kp = (kc + 63) // 64 * 64
    dy = bf(rnd(T, D))
    x = bf(F.pad(rnd(T, kc), (0, kp - kc)))
    g0 = rnd(D, kc)
    gw = g0.clone()
    G.linear_wgrad(dy, x, gw)
    ref = g0 + dy.float().t() @ x[:, :kc].float()
    w = bf(rnd(D, kc))
    wp = torch.full((D, kp), float("nan"), dtype=torch.bfloat16, device=DEV)
    ext.pad_cols_bf16(w, wp)
    pad_ok = torch.equal(wp[:, :kc], w) and bool((wp[:, kc:] == 0).all())
    m = worst((gw, ref))
    m["pad_wrong"] = float(not pad_ok)
    return (f"patch wgrad narrow T{T} D{D} kc{kc}->kp{kp}", m, lim(1e-6, 4e-6, pad_wrong=0))


def check_transpose_batched():
    ext = _ext.ext()
    shapes = [(128, 192), (100, 70), (768, 2304)]
    src = torch.cat([bf(rnd(r * c)) for r, c in shapes])
    dst = torch.zeros_like(src)
    meta, so, tiles = [], 0, 0
    for r, c in shapes:
        meta.append([so, so, r, c, tiles])
        so += r * c
        tiles += ((r + 63) // 64) * ((c + 63) // 64)
    ext.transpose_batched(src, dst, torch.tensor(meta, dtype=torch.int64, device=DEV), tiles)
    pairs, so = [], 0
    for r, c in shapes:
        pairs.append((dst[so:so + r * c].view(c, r), src[so:so + r * c].view(r, c).t()))
        so += r * c
    return ("transpose_batched (full and edge tiles)", worst(*pairs), lim(0, 0))


# ----------------------------------------------------------------------------- LayerNorm
def check_layernorm(T, D):
    ext = _ext.ext()
    x = bf(rnd(T, D) * 2 + 0.5)
    w, b = rnd(D) * 0.5 + 1, rnd(D) * 0.1
    y, mean, rstd = ext.layernorm_fwd(x, w, b, 1e-5, T, D)
    xr = x.float().requires_grad_(True)
    wr, br = w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    ref = F.layer_norm(xr, (D,), wr, br, 1e-5)
    dy = bf(rnd(T, D))
    dres = bf(rnd(T, D))
    ref.backward(dy.float())
    dx = torch.empty_like(x)
    dw = torch.zeros(D, device=DEV)
    db = torch.zeros(D, device=DEV)
    ext.layernorm_bwd(dy, D, x, D, mean, rstd, w, dres, D, dx, D, dw, db, T)
    act = worst((y, ref), (dx, xr.grad + dres.float()))
    par = worst((dw, wr.grad), (db, br.grad))
    m = {"l2": act["l2"], "max": act["max"], "dwdb_l2": par["l2"], "dwdb_max": par["max"]}
    return (f"layernorm T{T} D{D}", m, lim(3.5e-3, 6e-3, dwdb_l2=1e-6, dwdb_max=2e-6))


def check_layernorm_linked(T, D, p=0.1):
    """LayerNorm backward with everything the encoder block fuses into it: residual gradient,
    dgamma/dbeta, the producing layer's dropout backward (dz) and its bias gradient (column sums of
    dz). dz's mask must be the colsum kernel's mask for the same (seed, offset) — one hash everywhere."""
    ext = _ext.ext()
    x = bf(rnd(T, D) * 2 + 0.5)
    w, b = rnd(D) * 0.5 + 1, rnd(D) * 0.1
    y, mean, rstd = ext.layernorm_fwd(x, w, b, 1e-5, T, D)
    xr = x.float().requires_grad_(True)
    wr, br = w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    ref = F.layer_norm(xr, (D,), wr, br, 1e-5)
    dy, dres = bf(rnd(T, D)), bf(rnd(T, D))
    ref.backward(dy.float())
    seed = torch.tensor([31337], dtype=torch.int64, device=DEV)
    off = 11 << 32
    dx, dz = torch.empty_like(x), torch.empty_like(x)
    dw, db, dsum = (torch.zeros(D, device=DEV) for _ in range(3))
    ext.layernorm_bwd(dy, D, x, D, mean, rstd, w, dres, D, dx, D, dw, db, T, dsum, dz, seed, off, p)
    dx_ref = xr.grad + dres.float()
    keep = torch.empty_like(x)
    G.bias_grad(bf(torch.ones(T, D, device=DEV)), torch.zeros(D, device=DEV), drop=(seed, off, p), dz=keep)
    keep = keep.float() != 0
    thr = min(int(round(p * 65536)), 65535)
    dz_ref = torch.where(keep, dx_ref * (65536.0 / (65536.0 - thr)), torch.zeros_like(dx_ref))  # fp32, exact scale
    act = worst((dx, dx_ref), (dz, dz_ref))
    par = worst((dw, wr.grad), (db, br.grad), (dsum, dz_ref.sum(0)))
    rate = 1 - keep.float().mean().item()
    m = {"l2": act["l2"], "max": act["max"], "sums_l2": par["l2"], "sums_max": par["max"], "rate_dev": abs(rate - p)}
    return (f"layernorm bwd + dropout dz + dsum T{T} D{D} (rate {rate:.3f})", m,
            lim(3.5e-3, 7e-3, sums_l2=5e-6, sums_max=2e-5, rate_dev=rate_limit(p, T * D)))


# ----------------------------------------------------------------------------- attention
def _mix32(x):
    """rng_mix32 of csrc/common.h on int64 tensors holding uint32 values (or on Python ints)."""
    M = 0xFFFFFFFF

    def mul(v, c):  # (v * c) mod 2^32 without overflowing int64
        return (v * (c & 0xFFFF) + (((v * (c >> 16)) & 0xFFFF) << 16)) & M

    x = x ^ (x >> 16)
    x = mul(x, 0x7FEB352D)
    x = x ^ (x >> 15)
    x = mul(x, 0x846CA68B)
    x = x ^ (x >> 16)
    return x


def attn_keep_mask(seed: int, off: int, BH: int, N: int, p: float) -> torch.Tensor:
    """The attention-dropout keep mask [BH, N, N] the HIP kernels draw (csrc/attention.hip AttnDrop),
    regenerated in PyTorch from the same counter hash."""
    M = 0xFFFFFFFF
    s64 = (seed + off) & ((1 << 64) - 1)
    key0 = _mix32((s64 & M) ^ _mix32(((s64 >> 32) + 0x9E3779B9) & M))
    thr = min(int(round(p * 65536)), 65535)
    bh = torch.arange(BH, device=DEV, dtype=torch.int64)
    keys = _mix32(torch.full_like(bh, key0) ^ ((0x9E3779B9 * (bh + 1)) & M))  # [BH]
    npad = (N + 3) & ~3
    q = torch.arange(N, device=DEV, dtype=torch.int64)
    idx = (q[:, None] * npad + q[None, :])  # [N, N]
    h = _mix32((idx[None] >> 1) ^ keys[:, None, None])
    half = torch.where((idx[None] & 1) == 1, h >> 16, h & 0xFFFF)
    return half >= thr


def _attn_ref(qkv, B, N, H, keep=None, p=0.0):
    D = qkv.shape[1] // 3
    dh = D // H
    q, k, v = qkv.float().view(B, N, 3, H, dh).permute(2, 0, 3, 1, 4)
    s = (q @ k.transpose(-1, -2)) / math.sqrt(dh)
    lse = torch.logsumexp(s, -1)
    pr = torch.softmax(s, -1)
    if keep is not None:
        thr = min(int(round(p * 65536)), 65535)
        pr = pr * keep.view(B, H, N, N).float() * (65536.0 / (65536.0 - thr))
    o = pr @ v
    return o.transpose(1, 2).reshape(B * N, D), lse.reshape(B * H, N)


def check_attn_fwd(B, N, H, dh=64):
    ext = _ext.ext()
    D = H * dh
    qkv = bf(rnd(B * N, 3 * D))
    o, lse = ext.attn_fwd(qkv, B, N, H, 1.0 / math.sqrt(dh))
    oref, lref = _attn_ref(qkv, B, N, H)
    m = worst((o, oref))
    m["lse_l2"], m["lse_max"] = errs(lse, lref)
    # N < 8: a handful of lse values, each one fp32 dot product whose cancellation near 0 makes the
    # relative l2 of so few terms wobble with the data (1.7e-7 seen at N = 1)
    return (f"attn_fwd B{B} N{N} H{H} dh{dh}", m, lim(4.5e-3, 6e-3, lse_l2=1.5e-7 if N >= 8 else 3e-7, lse_max=3e-7))


def check_attn_fwd_head_qf(B, N, H):
    """Whole-head forward (dh 64, N <= 256) with 2 query fragments per wave (the A/B form) vs 1 (the
    default): per query the same MFMA sequence, so bitwise equal outputs; and vs fp32."""
    ext = _ext.ext()
    D = H * 64
    qkv = bf(rnd(B * N, 3 * D))
    try:
        ext.set_attn_fwd_head_qf(1)
        o1, l1 = ext.attn_fwd(qkv, B, N, H, 0.125)
        ext.set_attn_fwd_head_qf(2)
        o2, l2 = ext.attn_fwd(qkv, B, N, H, 0.125)
    finally:
        ext.set_attn_fwd_head_qf(1)
    oref, lref = _attn_ref(qkv, B, N, H)
    m = worst((o2, oref))
    m["lse_l2"], m["lse_max"] = errs(l2, lref)
    m["qf_differs"] = float(not (torch.equal(o1, o2) and torch.equal(l1, l2)))
    return (f"attn_fwd whole-head QF 2 vs 1, B{B} N{N} H{H}", m, lim(4.5e-3, 6e-3, lse_l2=1.5e-7, lse_max=3e-7, qf_differs=0))


def check_attn_bwd(B, N, H, dh=64, fused_bias=False):
    """dQ|dK|dV (and the fused in_proj bias gradient) vs autograd of the fp32 reference."""
    ext = _ext.ext()
    D = H * dh
    qkv = bf(rnd(B * N, 3 * D))
    o, lse = ext.attn_fwd(qkv, B, N, H, 1.0 / math.sqrt(dh))
    do = bf(rnd(B * N, D))
    dbias = torch.zeros(3 * D, device=DEV) if fused_bias else None
    dqkv = ext.attn_bwd(do, qkv, o, lse, B, N, H, 1.0 / math.sqrt(dh), dbias)
    qr = qkv.float().requires_grad_(True)
    oref, _ = _attn_ref(qr, B, N, H)
    oref.backward(do.float())
    m = worst((dqkv, qr.grad))
    if fused_bias:
        m["dbias_l2"], m["dbias_max"] = errs(dbias, qr.grad.sum(0))
    return (f"attn_bwd B{B} N{N} H{H} dh{dh} dbias{int(fused_bias)}", m,
            lim(5e-3, 1e-2, **({"dbias_l2": 1.6e-3, "dbias_max": 1e-3} if fused_bias else {})))


def check_attn_bwd_det(B, N, H, dh=64, fused_bias=False):
    """Deterministic mode on a multi-key-block shape with neither the lastkey nor the tail-split slab
    path (N = 677 = 2 x 256 + 165): per-key-block f32 dQ slabs summed in a fixed order instead of f32
    atomics. Two backward calls are bitwise equal, and dQ|dK|dV (and the bias gradient) match the fp32
    reference as in check_attn_bwd."""
    ext = _ext.ext()
    D = H * dh
    sc = 1.0 / math.sqrt(dh)
    qkv = bf(rnd(B * N, 3 * D))
    o, lse = ext.attn_fwd(qkv, B, N, H, sc)
    do = bf(rnd(B * N, D))
    was = ext.deterministic()
    ext.set_deterministic(True)
    try:
        outs = []
        for _ in range(2):
            dbias = torch.zeros(3 * D, device=DEV) if fused_bias else None
            outs.append((ext.attn_bwd(do, qkv, o, lse, B, N, H, sc, dbias), dbias))
    finally:
        ext.set_deterministic(was)
    (d0, b0), (d1, b1) = outs
    qr = qkv.float().requires_grad_(True)
    oref, _ = _attn_ref(qr, B, N, H)
    oref.backward(do.float())
    m = worst((d0, qr.grad))
    m["not_bitwise_repeatable"] = float(not (torch.equal(d0, d1) and (not fused_bias or torch.equal(b0, b1))))
    if fused_bias:
        m["dbias_l2"], m["dbias_max"] = errs(b0, qr.grad.sum(0))
    return (f"attn_bwd deterministic ordered dQ slabs B{B} N{N} H{H} dh{dh} dbias{int(fused_bias)}", m,
            lim(5e-3, 1e-2, not_bitwise_repeatable=0, **({"dbias_l2": 1.6e-3, "dbias_max": 1e-3} if fused_bias else {})))


def check_attn_bwd_q8(B, N, H, dh=64, p=0.0, fmt=1):
    """The attention backward's own fp8 copy of dQKV (fp8 recipe, grad slot 3; fmt 1 e5m2, 0 e4m3) vs
    quantizing its bf16 dQKV: same bytes up to the double rounding bf16 -> fp8 (the kernel rounds the
    fp32 value once), i.e. at most one fp8 step apart on a tiny fraction of elements; the amax record
    is max |dQKV|."""
    ext = _ext.ext()
    D = H * dh
    sc = 1.0 / math.sqrt(dh)
    qkv = bf(rnd(B * N, 3 * D))
    seed = torch.tensor([4321], dtype=torch.int64, device=DEV) if p > 0 else None
    o, lse = ext.attn_fwd(qkv, B, N, H, sc, seed, 5 << 32, p)
    do = bf(rnd(B * N, D))
    qs = torch.tensor([3000.0 if fmt else 20.0], device=DEV)
    amax = torch.zeros(1, dtype=torch.int32, device=DEV)
    q8 = torch.full((B * N, 3 * D), 0xAB, dtype=torch.uint8, device=DEV)
    dqkv = ext.attn_bwd(do, qkv, o, lse, B, N, H, sc, None, None, seed, 5 << 32, p, q_out=q8, q_scale=qs, q_amax=amax,
                        q_fmt=fmt)
    f8t, fmax = (torch.float8_e5m2, 57344) if fmt else (torch.float8_e4m3fn, 448)
    got = q8.view(f8t).float()
    ref = (dqkv.float() * qs).clamp(-fmax, fmax).to(f8t).float()
    # one fp8 step at the reference magnitude: 2 / 3 mantissa bits, the subnormal spacing (2^-16 / 2^-9) below
    step = torch.clamp(ref.abs() * (0.25 if fmt else 0.125), min=2.0 ** -16 if fmt else 2.0 ** -9)
    far = ((got - ref).abs() > step * 1.01).float().mean().item()
    diff = (got != ref).float().mean().item()
    am = amax.view(torch.float32).item()
    am_ref = dqkv.float().abs().max().item()
    m = {"beyond_one_step": far, "differ_frac": diff, "amax_rel": abs(am - am_ref) / am_ref}
    # differ_frac: bf16 keeps 6 bits past e5m2's 2, so ~1/64 of the bf16 values sit exactly on an e5m2
    # rounding midpoint and about half of those round the other way than the fp32 value (1.0e-2 measured)
    # (e4m3 keeps 5 bits fewer than bf16: ~1/32 of the values on a midpoint, differ_frac ~2x e5m2's)
    return (f"attn_bwd {'e5m2' if fmt else 'e4m3'} dQKV copy B{B} N{N} H{H} dh{dh} p{p}", m,
            {"beyond_one_step": 0, "differ_frac": 2.5e-2 if fmt else 4.5e-2, "amax_rel": 8e-3})


def check_attn_dropout(B, N, H, dh=64, p=0.1):
    """Attention-probability dropout: the forward's mask is the counter hash regenerated in PyTorch
    (rate ~ p), O and dQ|dK|dV match the fp32 reference under THAT mask (so forward and backward
    draw the same bits), and p = 0 with a seed is bit-identical to no dropout."""
    ext = _ext.ext()
    D = H * dh
    sc = 1.0 / math.sqrt(dh)
    qkv = bf(rnd(B * N, 3 * D))
    seed_val, off = 987654321, 77 << 32
    seed = torch.tensor([seed_val], dtype=torch.int64, device=DEV)
    o, lse = ext.attn_fwd(qkv, B, N, H, sc, seed, off, p)
    do = bf(rnd(B * N, D))
    dqkv = ext.attn_bwd(do, qkv, o, lse, B, N, H, sc, None, None, seed, off, p)
    keep = attn_keep_mask(seed_val, off, B * H, N, p)
    qr = qkv.float().requires_grad_(True)
    oref, lref = _attn_ref(qr, B, N, H, keep, p)
    oref.backward(do.float())
    m = worst((o, oref), (dqkv, qr.grad))
    rate = 1 - keep.float().mean().item()
    o0, l0 = ext.attn_fwd(qkv, B, N, H, sc)
    o1, l1 = ext.attn_fwd(qkv, B, N, H, sc, seed, off, 0.0)
    m.update(rate_dev=abs(rate - p), lse_l2=errs(lse, lref)[0],
             p0_not_identical=float(not (torch.equal(o0, o1) and torch.equal(l0, l1))))
    return (f"attn dropout p{p} B{B} N{N} H{H} dh{dh} (rate {rate:.4f})", m,
            lim(5e-3, 1e-2, rate_dev=rate_limit(p, B * H * N * N), lse_l2=1.5e-7, p0_not_identical=0))


# ----------------------------------------------------------------------------- fp8
def check_fp8_format(fmt=0):
    """Our quantizer must produce OCP fp8 (torch float8_e4m3fn / float8_e5m2 decode of the bytes)."""
    ext = _ext.ext()
    x = bf(rnd(64, 256) * 3)
    qs = torch.tensor([7.0], device=DEV)
    am = torch.zeros(1, dtype=torch.int32, device=DEV)
    y = torch.empty(64, 256, dtype=torch.uint8, device=DEV)
    ext.fp8_quant(x, y, qs, am, fmt)
    tdt = torch.float8_e4m3fn if fmt == 0 else torch.float8_e5m2
    fmax = 448.0 if fmt == 0 else 57344.0
    ref = (x.float().cpu() * 7.0).clamp(-fmax, fmax).to(tdt)
    got = y.cpu().view(tdt)
    mism = (got.float() != ref.float()).float().mean().item()
    amax_bad = float(abs(am.view(torch.float32).item() - x.float().abs().max().item()) >= 1e-6)
    dq_bad = float(not torch.equal(ext.fp8_dequant(y, None, fmt).cpu(), got.float()))
    return (f"fp8 quant format fmt{fmt}", {"byte_mismatch": mism, "amax_bad": amax_bad, "dequant_bad": dq_bad},
            {"byte_mismatch": 0.0, "amax_bad": 0, "dequant_bad": 0})


def check_fp8_strided(fmt=1):
    """Strided rows (row index math) and dense rows (flat offsets) quantize to the same bytes."""
    ext = _ext.ext()
    big = bf(rnd(96, 512) * 2)
    x = big[:, 128:384]  # ldx 512, cols 256
    qs = torch.tensor([5.0], device=DEV)
    am1, am2 = (torch.zeros(1, dtype=torch.int32, device=DEV) for _ in range(2))
    y1, y2 = (torch.empty(96, 256, dtype=torch.uint8, device=DEV) for _ in range(2))
    ext.fp8_quant(x, y1, qs, am1, fmt)
    ext.fp8_quant(x.contiguous(), y2, qs, am2, fmt)
    m = {"byte_mismatch": (y1 != y2).float().mean().item(), "amax_differs": float(am1.item() != am2.item())}
    return (f"fp8 quant strided == dense fmt{fmt}", m, {"byte_mismatch": 0.0, "amax_differs": 0})


def check_fp8_weight_batch():
    """The per-step multi-tensor weight refresh gives the bytes / scales of per-weight current scaling."""
    from pytorch_vit_paper_replication_amd.ops import fp8 as F8

    st = F8.Fp8State(1, DEV)
    ws = [bf(rnd(256, 384, scale=0.05)), bf(rnd(384, 256, scale=0.2)), bf(rnd(64, 1024, scale=3.0))]
    for i, w in enumerate(ws):
        st.weight(w, i, 1)  # first generation: per-weight path, records the set
    for w in ws:
        w.mul_(1.7).add_(0.01)  # the optimizer's update of the bf16 shadows (same storage)
    mism = sc = 0.0
    for i, w in enumerate(ws):
        q, ds = st.weight(w, i, 2)  # first call runs the batched refresh of all three
        meta = F8.Fp8Meta(1, DEV, history=1)
        qr, dsr = meta.quantize(w, 0, current=True)
        mism = max(mism, (q != qr).float().mean().item())
        sc = max(sc, abs(ds.item() - dsr.item()) / dsr.item())
    m = {"byte_mismatch": mism, "scale_rel": sc, "not_batched": float(st._batch_gen != 2)}
    return ("fp8 batched weight refresh == per-weight quantization", m, {"byte_mismatch": 0.0, "scale_rel": 1e-7, "not_batched": 0})


def _fp8_operand(x, fmt=0):
    from pytorch_vit_paper_replication_amd.ops import fp8 as F8

    meta = F8.Fp8Meta(1, DEV, history=1, fmt=fmt)
    q, ds = meta.quantize(x, 0, current=True)
    deq = _ext.ext().fp8_dequant(q.contiguous(), ds, fmt)
    return q, ds, deq


def check_gemm_fp8(M, N, K, resid=False, gelu=False):
    """fp8 forward GEMM vs the exact product of the same quantized operands (the kernel's own error:
    l2 / max), and vs the unquantized bf16 operands (the e4m3 rounding included: bf16_l2)."""
    from pytorch_vit_paper_replication_amd.ops import fp8 as F8

    x, w = bf(rnd(M, K)), bf(rnd(N, K, scale=0.05))
    b = rnd(N)
    r = bf(rnd(M, N)) if resid else None
    xq, xs, xd = _fp8_operand(x)
    wq, ws, wd = _fp8_operand(w)
    u = torch.empty(M, N, dtype=torch.bfloat16, device=DEV) if gelu else None
    y = F8.linear_fwd_fp8(xq, xs, wq, ws, b, resid=r, gelu_aux=u)

    def ref_of(a, bm):
        ref = a @ bm.t() + b
        if gelu:
            ref = F.gelu(ref)
        return ref + r.float() if r is not None else ref

    m = worst((y, ref_of(xd, wd)))
    m["bf16_l2"] = errs(y, ref_of(x.float(), w.float()))[0]
    return (f"gemm_fp8 e4m3 M{M} N{N} K{K} r{int(resid)} g{int(gelu)}", m, lim(3.5e-3, 6e-3, bf16_l2=6.5e-2))


def check_gemm_fp8_persistent(M=16384, N=4096, K=384):
    """The persistent fp8 ping-pong (tile 13 form, >= 4 output tiles per CU) against the one-tile-per-
    workgroup kernel (ext.set_fp8_persistent(0)) on the same operands: bias and the GELU epilogue
    with dropout, derivative and the e4m3 copy + amax (the residual and dGELU epilogues run one tile
    per workgroup in both modes). Same MFMA order and the same epilogue code, so every output must be
    bit-identical."""
    from pytorch_vit_paper_replication_amd.ops import fp8 as F8

    ext = _ext.ext()
    x, w = bf(rnd(M, K)), bf(rnd(N, K, scale=0.05))
    xq, xs, _ = _fp8_operand(x)
    wq, ws, _ = _fp8_operand(w)
    b = rnd(N)
    r = bf(rnd(M, N))
    seed = torch.tensor([77], dtype=torch.int64, device=DEV)

    def run(mode):
        ext.set_fp8_persistent(mode)
        try:
            meta = F8.Fp8Meta(1, DEV, history=1, fmt=F8.E4M3)
            meta.calibrated[0] = True
            meta.qscale.fill_(40.0)
            meta.dscale.copy_(1.0 / meta.qscale)
            aux = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
            y0 = F8.linear_fwd_fp8(xq, xs, wq, ws, b)
            y1 = F8.linear_fwd_fp8(xq, xs, wq, ws, b, resid=r)
            y2, (q, _) = F8.linear_fwd_fp8(xq, xs, wq, ws, b, gelu_aux=aux, drop=(seed, 5 << 32, 0.1), quant=meta.producer(0))
            # dGELU dgrad: e5m2 gradient x e4m3 W^T rows, derivative factor, column sums, e5m2 copy
            m5 = F8.Fp8Meta(1, DEV, history=1, fmt=F8.E5M2)
            m5.calibrated[0] = True
            m5.qscale.fill_(3.0)
            m5.dscale.copy_(1.0 / m5.qscale)
            cs = torch.zeros(N, device=DEV)
            y3, (q3, _) = F8.linear_dgrad_fp8(gq, gs, wq, ws, dgelu_aux=aux, colsum=cs, quant=m5.producer(0))
            torch.cuda.synchronize()
            return [y0, y1, y2, aux, q, meta.amax.clone(), y3, q3, m5.amax.clone()], cs
        finally:
            ext.set_fp8_persistent(1)

    gq, gs, _ = _fp8_operand(bf(rnd(M, K, scale=0.01)), 1)
    (ref, cs0), (got, cs1) = run(0), run(1)
    ndiff = sum(int((a.view(torch.uint8) != c.view(torch.uint8)).sum().item()) if a.dtype != torch.int32 else int((a != c).sum().item())
                for a, c in zip(ref, got))
    m = {"differing_bytes": float(ndiff), "nonfinite": float(not torch.isfinite(got[2].float()).all().item()),
         "colsum_rel": errs(cs1, cs0)[0]}
    return (f"gemm_fp8 persistent vs one-tile kernel M{M} N{N} K{K} (bias / resid / GELU+drop+e4m3 / dGELU+colsum+e5m2)", m,
            {"differing_bytes": 0, "nonfinite": 0, "colsum_rel": 1e-5})  # column sums: f32 atomics, any order


def _fp8_code_dist(q: torch.Tensor, ref: torch.Tensor) -> float:
    """Largest distance between two fp8 byte tensors in representable steps (sign-magnitude codes:
    adjacent magnitudes are one step apart; a sign flip counts the steps through zero)."""
    a, b = q.to(torch.int32), ref.to(torch.int32)
    sa = torch.where(a & 0x80 != 0, -(a & 0x7F), a & 0x7F)
    sb = torch.where(b & 0x80 != 0, -(b & 0x7F), b & 0x7F)
    return (sa - sb).abs().max().item()


def check_gemm_fp8_producer(M, N, K, dgelu=False):
    """Producer-side quantization: the fp8 GEMM's GELU (e4m3) / dGELU (e5m2) epilogue writes the
    output's fp8 copy with a slot's scale and records its amax. Against the quantize pass over the
    bf16 output with the same scale: decoded values (differences only where the epilogue rounds the
    fp32 value and the pass the bf16 one: at most one fp8 step), the amax (bf16 rounding of the
    output at most), and the bf16 output itself is bit-identical to the GEMM without the copy."""
    from pytorch_vit_paper_replication_amd.ops import fp8 as F8

    ext = _ext.ext()
    x, w = bf(rnd(M, K)), bf(rnd(N, K, scale=0.05))
    xq, xs, _ = _fp8_operand(x, 1 if dgelu else 0)  # dgrad: e5m2 gradient operand
    wq, ws, _ = _fp8_operand(w)
    fmt = F8.E5M2 if dgelu else F8.E4M3
    meta = F8.Fp8Meta(1, DEV, history=1, fmt=fmt)
    meta.calibrated[0] = True
    meta.qscale.fill_(3.0 if dgelu else 40.0)
    meta.dscale.copy_(1.0 / meta.qscale)
    aux = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
    if dgelu:
        aux.copy_(bf(torch.rand(M, N, device=DEV) * 1.1))
        plain = F8.linear_dgrad_fp8(xq, xs, wq, ws, dgelu_aux=aux)
        y, (q, ds) = F8.linear_dgrad_fp8(xq, xs, wq, ws, dgelu_aux=aux, quant=meta.producer(0))
    else:
        b = rnd(N)
        plain = F8.linear_fwd_fp8(xq, xs, wq, ws, b, gelu_aux=aux)
        y, (q, ds) = F8.linear_fwd_fp8(xq, xs, wq, ws, b, gelu_aux=aux, quant=meta.producer(0))
    ref = torch.empty(M, N, dtype=torch.uint8, device=DEV)
    scratch = torch.zeros(1, dtype=torch.int32, device=DEV)
    ext.fp8_quant(y, ref, meta.qscale[0:1], scratch, fmt)
    amax = meta.amax.view(torch.float32)[0].item()
    m = {"fp8_steps": _fp8_code_dist(q, ref), "mismatch_frac": (q != ref).float().mean().item(),
         "amax_rel": abs(amax - y.float().abs().max().item()) / y.float().abs().max().item(),
         "bf16_not_identical": float(not torch.equal(y, plain))}
    return (f"gemm_fp8 producer quant {'dgelu e5m2' if dgelu else 'gelu e4m3'} M{M} N{N} K{K}", m,
            {"fp8_steps": 1, "mismatch_frac": 0.05, "amax_rel": 4e-3, "bf16_not_identical": 0})


def check_layernorm_fwd_q8(T=3000, D=1280):
    """LayerNorm forward with the fused e4m3 copy: y, mean, rstd bit-identical to the plain forward;
    the copy within one fp8 step of quantizing y (fp32 vs bf16-rounded input) and amax = max|y|."""
    from pytorch_vit_paper_replication_amd.ops import fp8 as F8

    ext = _ext.ext()
    x = bf(rnd(T, D) * 2 + 0.5)
    w, b = rnd(D) * 0.5 + 1.0, rnd(D) * 0.1
    meta = F8.Fp8Meta(1, DEV, history=1, fmt=F8.E4M3)
    meta.calibrated[0] = True
    meta.qscale.fill_(60.0)
    meta.dscale.copy_(1.0 / meta.qscale)
    y0, m0, r0 = ext.layernorm_fwd(x, w, b, 1e-6, T, D)
    y, m1, r1, (q, ds) = F8.layernorm_fwd_q8(x, w, b, 1e-6, meta.producer(0))
    ref = torch.empty(T, D, dtype=torch.uint8, device=DEV)
    ext.fp8_quant(y, ref, meta.qscale[0:1], torch.zeros(1, dtype=torch.int32, device=DEV), 0)
    amax = meta.amax.view(torch.float32)[0].item()
    m = {"fp8_steps": _fp8_code_dist(q, ref), "mismatch_frac": (q != ref).float().mean().item(),
         "amax_rel": abs(amax - y.float().abs().max().item()) / y.float().abs().max().item(),
         "ln_not_identical": float(not (torch.equal(y, y0) and torch.equal(m0, m1) and torch.equal(r0, r1)))}
    return (f"layernorm_fwd_q8 T{T} D{D}", m, {"fp8_steps": 1, "mismatch_frac": 0.05, "amax_rel": 4e-3, "ln_not_identical": 0})


def check_layernorm_bwd_q8(T=3000, D=1280, linked=False, p=0.1, fmt=1):
    """LayerNorm backward with the fused e5m2 copy of the gradient it writes last (dz with the linked
    dropout backward, else dx): dx / dz / dgamma / dbeta / dsum bit-identical to the plain backward
    (f32 atomics aside: the same kernel order), the copy within one fp8 step of quantizing the bf16
    output with the same scale, and amax = max|output| (to bf16 rounding)."""
    from pytorch_vit_paper_replication_amd.ops import fp8 as F8

    ext = _ext.ext()
    x = bf(rnd(T, D) * 2 + 0.5)
    w, b = rnd(D) * 0.5 + 1, rnd(D) * 0.1
    _, mean, rstd = ext.layernorm_fwd(x, w, b, 1e-5, T, D)
    dy, dres = bf(rnd(T, D)), bf(rnd(T, D))
    meta = F8.Fp8Meta(1, DEV, history=1, fmt=fmt)
    meta.calibrated[0] = True
    meta.qscale.fill_(2.0)
    meta.dscale.copy_(1.0 / meta.qscale)
    seed = torch.tensor([4242], dtype=torch.int64, device=DEV)
    outs = []
    for quant in (False, True):
        dx, dz = torch.empty_like(x), (torch.empty_like(x) if linked else None)
        dw, db, ds = (torch.zeros(D, device=DEV) for _ in range(3))
        kw = dict(dsum=ds, dz=dz, seed=seed if linked else None, seed_offset=3 << 32, drop_p=p if linked else 0.0)
        q = None
        if quant:
            q = torch.empty(T, D, dtype=torch.uint8, device=DEV)
            kw.update(q_out=q, q_scale=meta.qscale[0:1], q_amax=meta.amax[0:1], q_fmt=fmt)
        ext.layernorm_bwd(dy, D, x, D, mean, rstd, w, dres, D, dx, D, dw, db, T, **kw)
        outs.append((dx, dz, dw, db, ds, q))
    (dx0, dz0, dw0, db0, ds0, _), (dx1, dz1, dw1, db1, ds1, q) = outs
    y = dz1 if linked else dx1
    ref = torch.empty(T, D, dtype=torch.uint8, device=DEV)
    ext.fp8_quant(y, ref, meta.qscale[0:1], torch.zeros(1, dtype=torch.int32, device=DEV), fmt)
    amax = meta.amax.view(torch.float32)[0].item()
    same = torch.equal(dx0, dx1) and (not linked or torch.equal(dz0, dz1))
    sums = max(errs(dw1, dw0)[0], errs(db1, db0)[0], errs(ds1, ds0)[0])
    m = {"fp8_steps": _fp8_code_dist(q, ref), "mismatch_frac": (q != ref).float().mean().item(),
         "amax_rel": abs(amax - y.float().abs().max().item()) / y.float().abs().max().item(),
         "grad_not_identical": float(not same), "sums_l2": sums}
    return (f"layernorm_bwd_q8 {'e5m2' if fmt else 'e4m3'} T{T} D{D} linked{int(linked)}", m,
            {"fp8_steps": 1, "mismatch_frac": 0.05, "amax_rel": 8e-3, "grad_not_identical": 0, "sums_l2": 1e-6})  # amax: bf16 rounding <= 2^-8


def check_colsum_q8(T=4000, N=3840, fmt=1):
    """Column sums (the in_proj bias gradient over all of dQKV) fused with dQKV's e5m2 copy: the sums
    as the plain column-sum pass, the copy as the quantize pass with the same scale (the inputs are
    the bf16 values themselves, so the bytes should agree), amax = max|dy|."""
    from pytorch_vit_paper_replication_amd.ops import fp8 as F8

    ext = _ext.ext()
    dy = bf(rnd(T, N) * 0.3)
    meta = F8.Fp8Meta(1, DEV, history=1, fmt=fmt)
    meta.calibrated[0] = True
    meta.qscale.fill_(8.0)
    meta.dscale.copy_(1.0 / meta.qscale)
    db0, db1 = torch.zeros(N, device=DEV), torch.zeros(N, device=DEV)
    G.bias_grad(dy, db0)
    q, ds = G.bias_grad(dy, db1, quant=meta.producer(0))
    ref = torch.empty(T, N, dtype=torch.uint8, device=DEV)
    ext.fp8_quant(dy, ref, meta.qscale[0:1], torch.zeros(1, dtype=torch.int32, device=DEV), fmt)
    amax = meta.amax.view(torch.float32)[0].item()
    m = {"fp8_steps": _fp8_code_dist(q, ref), "mismatch_frac": (q != ref).float().mean().item(),
         "amax_rel": abs(amax - dy.float().abs().max().item()) / dy.float().abs().max().item(),
         "colsum_l2": errs(db1, db0)[0], "colsum_vs_fp32_l2": errs(db1, dy.float().sum(0))[0]}
    return (f"colsum + {'e5m2' if fmt else 'e4m3'} copy T{T} N{N}", m,
            {"fp8_steps": 1, "mismatch_frac": 1e-3, "amax_rel": 1e-6, "colsum_l2": 1e-6, "colsum_vs_fp32_l2": 1e-5})


def check_attn_fwd_q8(B=2, N=257, H=4, dh=80):
    """Attention forward with the fused e4m3 output copy: O / lse bit-identical to the plain forward,
    the copy within one fp8 step of quantizing O, amax = max|O| (up to O's bf16 rounding)."""
    from pytorch_vit_paper_replication_amd.ops import fp8 as F8

    ext = _ext.ext()
    D = H * dh
    qkv = bf(rnd(B * N, 3 * D) * 2)
    sc = 1.0 / math.sqrt(dh)
    meta = F8.Fp8Meta(1, DEV, history=1, fmt=F8.E4M3)
    meta.calibrated[0] = True
    meta.qscale.fill_(300.0)
    meta.dscale.copy_(1.0 / meta.qscale)
    o0, l0 = ext.attn_fwd(qkv, B, N, H, sc)
    q = torch.empty(B * N, D, dtype=torch.uint8, device=DEV)
    o1, l1 = ext.attn_fwd(qkv, B, N, H, sc, None, 0, 0.0, q, meta.qscale[0:1], meta.amax[0:1])
    ref = torch.empty(B * N, D, dtype=torch.uint8, device=DEV)
    ext.fp8_quant(o1, ref, meta.qscale[0:1], torch.zeros(1, dtype=torch.int32, device=DEV), 0)
    amax = meta.amax.view(torch.float32)[0].item()
    m = {"fp8_steps": _fp8_code_dist(q, ref), "mismatch_frac": (q != ref).float().mean().item(),
         "amax_rel": abs(amax - o1.float().abs().max().item()) / o1.float().abs().max().item(),
         "not_identical": float(not (torch.equal(o0, o1) and torch.equal(l0, l1)))}
    lim_ = {"fp8_steps": 1, "mismatch_frac": 0.05, "amax_rel": 4e-3, "not_identical": 0}
    if dh == 64 and N <= 256:  # the plain call takes the whole-head kernel, the copy the generic one
        del m["not_identical"], lim_["not_identical"]
        m["o_vs_head_kernel_l2"] = errs(o1, o0)[0]
        lim_["o_vs_head_kernel_l2"] = 5e-3
    return (f"attn_fwd_q8 B{B} N{N} H{H} dh{dh}", m, lim_)


def check_fp8_transpose(T=1000, C=1280, fmt=1):
    """The fp8 weight gradient's transposed operand from the row-major fp8 copy (byte transpose) must be
    byte-identical to the transposing quantize pass over the bf16 tensor with the same scale, zero
    padding of the token dim included."""
    from pytorch_vit_paper_replication_amd.ops import fp8 as F8

    ext = _ext.ext()
    x = bf(rnd(T, C))
    meta = F8.Fp8Meta(1, DEV, history=1, fmt=fmt)
    q, _ = meta.quantize(x, 0)
    Tp = (T + 127) // 128 * 128
    a = torch.full((C, Tp), 7, dtype=torch.uint8, device=DEV)
    b = torch.full((C, Tp), 9, dtype=torch.uint8, device=DEV)
    ext.fp8_transpose(q, a)
    ext.fp8_quant_t(x, b, meta.qscale[0:1], fmt)
    return (f"fp8_transpose T{T} C{C} fmt{fmt}", {"bytes_differ": float((a != b).sum().item())}, {"bytes_differ": 0})


def check_wgrad_fp8_mn(T, N, K, gfmt=1):
    """fp8 weight gradient read straight from the row-major fp8 copies (mn-contiguous operands,
    ds_read_b64_tr_b8 fragments) vs the byte-transposed copies through the k-contiguous GEMM (the same
    fp8 operands: equal up to fp32 summation order) and vs the exact product of the dequantized
    operands; token counts that are not multiples of 128 exercise the split tails."""
    from pytorch_vit_paper_replication_amd.ops import fp8 as F8

    ext = _ext.ext()
    dy, x = bf(rnd(T, N)), bf(rnd(T, K))
    gm, am = F8.Fp8Meta(1, DEV, history=1, fmt=gfmt), F8.Fp8Meta(1, DEV, history=1, fmt=F8.E4M3)
    dy8, _ = gm.quantize(dy, 0)
    x8, _ = am.quantize(x, 0)
    out_mn = torch.zeros(N, K, device=DEV)
    out_t = torch.zeros(N, K, device=DEV)
    F8.linear_wgrad_fp8(dy, gm, 0, x, am, 0, out_mn, dy8, x8)
    F8.WGRAD_MN = False
    try:
        F8.linear_wgrad_fp8(dy, gm, 0, x, am, 0, out_t, dy8, x8)
    finally:
        F8.WGRAD_MN = True
    dyd = ext.fp8_dequant(dy8.contiguous(), gm.dscale[0:1], gfmt)
    xd = ext.fp8_dequant(x8.contiguous(), am.dscale[0:1], 0)
    m = worst((out_mn, dyd.t() @ xd))
    m["vs_transposed_l2"] = errs(out_mn, out_t)[0]
    return (f"wgrad fp8 mn-contiguous {'e5m2' if gfmt else 'e4m3'} T{T} N{N} K{K}", m, lim(2.5e-5, 5e-5, vs_transposed_l2=1e-6))


def check_wgrad_fp8(T, N, K, gfmt=1):
    """dW = dequant(dy^T (e5m2) . x (e4m3)) from the transposed quantize passes + split-K fp8 GEMM,
    against the exact product of the same quantized operands and against bf16."""
    from pytorch_vit_paper_replication_amd.ops import fp8 as F8

    dy, x = bf(rnd(T, N)), bf(rnd(T, K))
    gm, am = F8.Fp8Meta(1, DEV, history=1, fmt=gfmt), F8.Fp8Meta(1, DEV, history=1, fmt=F8.E4M3)
    _, gs = gm.quantize(dy, 0, current=True)
    _, xs = am.quantize(x, 0, current=True)
    out = torch.zeros(N, K, device=DEV)
    F8.linear_wgrad_fp8(dy, gm, 0, x, am, 0, out)
    ext = _ext.ext()  # reference from the same fp8 values (non-transposed quantize, dequantized)
    q1 = torch.empty(T, N, dtype=torch.uint8, device=DEV)
    q2 = torch.empty(T, K, dtype=torch.uint8, device=DEV)
    ext.fp8_quant(dy, q1, gm.qscale[0:1], gm.amax[0:1], gfmt)
    ext.fp8_quant(x, q2, am.qscale[0:1], am.amax[0:1], F8.E4M3)
    dyd = ext.fp8_dequant(q1, gs, gfmt).view(T, N)
    xd = ext.fp8_dequant(q2, xs, F8.E4M3).view(T, K)
    m = worst((out, dyd.t() @ xd))
    m["bf16_l2"] = errs(out, dy.float().t() @ x.float())[0]
    return (f"wgrad_fp8 {'e5m2' if gfmt else 'e4m3'}^T x e4m3 T{T} N{N} K{K}", m, lim(2.5e-5, 4e-5, bf16_l2=1.2e-1))


def check_dgrad_fp8(M, N, K, gfmt=1):
    """dX = dequant(g (e5m2) . W (e4m3)) with the dGELU epilogue and the fused bias-grad column sum."""
    from pytorch_vit_paper_replication_amd.ops import fp8 as F8

    g, wt = bf(rnd(M, N)), bf(rnd(K, N, scale=0.05))
    aux = bf(rnd(M, K))
    gq, gs, gd = _fp8_operand(g, gfmt)
    wq, ws, wd = _fp8_operand(wt, 0)
    cs = torch.zeros(K, device=DEV)
    y = F8.linear_dgrad_fp8(gq, gs, wq, ws, dgelu_aux=aux, colsum=cs, g_fmt=gfmt)
    ref = (gd @ wd.t()) * aux.float()
    m = worst((y, ref))
    m["colsum_l2"], m["colsum_max"] = errs(cs, ref.sum(0))
    return (f"dgrad_fp8 {'e5m2' if gfmt else 'e4m3'} x e4m3 dGELU M{M} N{N} K{K}", m, lim(3.5e-3, 5e-3, colsum_l2=2.5e-5, colsum_max=3e-5))


_FP8_CFG = dict(image_size=64, patch_size=16, num_transformer_layer=2, num_heads=2, embedding_dim=256, mlp_size=512,
                num_classes=10, mlp_dropout=0.0, embedding_dropout=0.0)


def _reference_logits(model, x):
    os.environ["PVR_DISABLE_FUSED"] = "1"
    try:
        return model(x)
    finally:
        os.environ["PVR_DISABLE_FUSED"] = "0"


def _train_losses(m, x, y, steps=6):
    from pytorch_vit_paper_replication_amd.ops.fused_vit import cross_entropy
    from pytorch_vit_paper_replication_amd.optim import FusedAdam

    opt = FusedAdam(m.parameters(), lr=1e-3)
    losses = []
    for _ in range(steps):
        loss = cross_entropy(m(x), y)
        opt.zero_grad()
        loss.backward()
        opt.step(clip_norm=1.0)
        losses.append(loss.item())
    ok = losses[-1] < losses[0] and all(math.isfinite(v) for v in losses)
    return losses, ok


def check_vit_fp8(B=4):
    """fp8-forward ViT logits vs the fp32 PyTorch model; training with it decreases the loss."""
    from pytorch_vit_paper_replication_amd.models import ViT

    torch.manual_seed(0)
    mf = ViT(**_FP8_CFG).to(DEV).enable_fp8(wgrad=False)
    mr = ViT(**_FP8_CFG).to(DEV)
    mr.load_state_dict(mf.state_dict())
    x = torch.rand(B * 4, 3, 64, 64, device=DEV)
    y = torch.randint(0, 10, (B * 4,), device=DEV)
    lf = mf(x)
    assert mf._fp8 is not None, "fp8 path did not engage"
    m = worst((lf, _reference_logits(mr, x)))
    losses, ok = _train_losses(mf, x, y)
    m["loss_not_falling"] = float(not ok)
    return (f"vit fp8 fwd vs fp32, loss {losses[0]:.3f}->{losses[-1]:.3f}", m, lim(8.5e-2, 1e-1, loss_not_falling=0))


def check_vit_fp8_bf16_skip(B=4, steps=4, image=64, images=None):
    """fp8 training with the bf16 copies that only fp8 consumers read left unwritten (xn1, xn2, h in
    the forward, dU and the linked dz in the backward, once their weight gradients run in fp8 from
    the e4m3 / e5m2 copies). Those unwritten tensors are filled with NaN (POISON_SKIPPED), so a
    reader of any of them would make the gradients non-finite. From the same state (one calibrating
    step), the second step's gradients must equal those of the same step with every bf16 copy
    written (a no-op DGRAD_TAP turns the skips off) up to f32-atomic reordering; a few more steps
    must stay finite and close (the fp8 quantization amplifies reordered low bits into whole fp8
    steps, so trajectories drift slightly between any two runs with different kernel timing)."""
    from pytorch_vit_paper_replication_amd.models import ViT
    from pytorch_vit_paper_replication_amd.ops import fused_vit
    from pytorch_vit_paper_replication_amd.ops.fused_vit import cross_entropy
    from pytorch_vit_paper_replication_amd.optim import FusedAdam

    res = []
    for skip in (True, False):
        torch.manual_seed(0)
        m = ViT(**dict(_FP8_CFG, mlp_dropout=0.1, image_size=image)).to(DEV).enable_fp8(wgrad=False)
        opt = FusedAdam(m.parameters(), lr=1e-3)
        nimg = images or B * 64
        x = torch.rand(nimg, 3, image, image, device=DEV)
        y = torch.randint(0, 10, (nimg,), device=DEV)
        fused_vit.DGRAD_TAP = None if skip else (lambda which, t: None)
        fused_vit.POISON_SKIPPED = skip
        try:
            losses, g2 = [], None
            for i in range(steps):
                loss = cross_entropy(m(x), y)
                opt.zero_grad()
                loss.backward()
                if i == 1:  # first step with the skips active, from an identical state
                    g2 = m._pvr_store.grad_flat.detach().clone()
                opt.step(clip_norm=1.0)
                losses.append(loss.item())
        finally:
            fused_vit.DGRAD_TAP = None
            fused_vit.POISON_SKIPPED = False
        res.append((losses, g2, m._pvr_store.flat.detach().clone()))
    (l0, g0, p0), (l1, g1, p1) = res
    m = {"grad_l2": errs(g0, g1)[0], "nonfinite": float(not (torch.isfinite(g0).all().item() and torch.isfinite(p0).all().item()
                                                          and all(math.isfinite(v) for v in l0))),
         "loss_diff": max(abs(a - b) for a, b in zip(l0, l1)), "param_l2": errs(p0, p1)[0]}
    return (f"vit fp8 bf16-copy skips (NaN-poisoned) vs all copies written, {image} px, {steps} steps (loss {l0[0]:.3f}->{l0[-1]:.3f})", m,
            # measured grad_l2 2.9e-8 / 2.4e-8; loss_diff 4.1e-3 in one run (lr 1e-3: the drift over 4 steps
            # depends on the kernel timing of the two runs, the step-2 gradients are the exact comparison)
            {"grad_l2": 1e-6, "nonfinite": 0, "loss_diff": 1e-2, "param_l2": 1e-3})


def check_vit_fp8_default_producers(images=64, steps=8):
    """The default fp8 recipe (fp8 forward + dgrad, bf16 weight gradients): once the slots are
    calibrated, every e5m2 gradient operand of the fp8 dgrad GEMMs comes from its producer kernel
    (LayerNorm backward, dGELU epilogue, bias-gradient pass, attention backward for dQKV) - no separate
    quantize pass runs in a steady-state step - and training stays finite with a falling loss."""
    from pytorch_vit_paper_replication_amd.models import ViT
    from pytorch_vit_paper_replication_amd.ops.fused_vit import cross_entropy
    from pytorch_vit_paper_replication_amd.optim import FusedAdam

    torch.manual_seed(0)
    m = ViT(**_FP8_CFG).to(DEV).enable_fp8(wgrad=False)
    x = torch.rand(images, 3, 64, 64, device=DEV)
    y = torch.randint(0, 10, (images,), device=DEV)
    opt = FusedAdam(m.parameters(), lr=1e-3)
    calls = []
    losses = []
    for i in range(steps):
        st = m._fp8  # created by the first forward
        orig = st.grad_quant if st is not None else None
        if i == steps - 1:  # steady state: count the quantize passes of the last step
            st.grad_quant = lambda g, block, which: calls.append((block, which)) or orig(g, block, which)
        try:
            loss = cross_entropy(m(x), y)
            opt.zero_grad()
            loss.backward()
            opt.step(clip_norm=1.0)
        finally:
            if st is not None:
                st.__dict__.pop("grad_quant", None)  # back to the class method
        losses.append(loss.item())
    met = {"quantize_passes": float(len(calls)), "nonfinite": float(not all(math.isfinite(v) for v in losses)),
           "loss_not_falling": float(not losses[-1] < losses[0])}
    return (f"vit fp8 default recipe (bf16 wgrad): steady-state quantize passes {sorted(set(calls))}, "
            f"loss {losses[0]:.3f}->{losses[-1]:.3f}", met, {"quantize_passes": 0, "nonfinite": 0, "loss_not_falling": 0})


def check_vit_fp8_dgrad(B=4):
    """fp8 dgrad GEMMs (enable_fp8(dgrad=True): fp8 gradients, e4m3 by default, x e4m3 W^T) against the bf16 dgrads of the
    same fp8-forward model, PER dgrad output tensor (fc2 / fc1 / out-proj / qkv of every block, tapped
    straight from the backward) on identical calibrated forward passes; then training with them must
    decrease the loss. Per-tensor errors are printed into the test log."""
    from pytorch_vit_paper_replication_amd.models import ViT
    from pytorch_vit_paper_replication_amd.ops import fused_vit
    from pytorch_vit_paper_replication_amd.ops.fused_vit import cross_entropy

    torch.manual_seed(0)
    m = ViT(**_FP8_CFG).to(DEV).enable_fp8(dgrad=True, wgrad=False)
    x = torch.rand(B * 64, 3, 64, 64, device=DEV)
    y = torch.randint(0, 10, (B * 64,), device=DEV)

    def run(dgrad_fp8: bool):
        m.enable_fp8(dgrad=dgrad_fp8, wgrad=False)  # same history / margin: keeps the calibrated scaling state
        out = []
        fused_vit.DGRAD_TAP = lambda which, t: out.append((which, t.float().clone()))
        try:
            m.zero_grad(set_to_none=False)
            cross_entropy(m(x), y).backward()
        finally:
            fused_vit.DGRAD_TAP = None
        return out

    run(True)  # calibrates every activation / gradient slot (histories hold this input's amax)
    ref = run(False)
    f8 = run(True)
    names = ["fc2", "fc1", "out", "qkv"]
    per = []
    for i, ((w, r), (w2, t)) in enumerate(zip(ref, f8)):
        assert w == w2
        per.append((f"b{_FP8_CFG['num_transformer_layer'] - 1 - i // 4}.{names[w]}", errs(t, r)[0]))
    print("fp8 dgrad per-tensor rel-L2 vs bf16 dgrad: " + ", ".join(f"{n} {e:.3e}" for n, e in per))
    m.enable_fp8(dgrad=True, wgrad=False)
    losses, ok = _train_losses(m, x, y)
    met = {"l2": max(e for _, e in per), "loss_not_falling": float(not ok or len(per) != 4 * _FP8_CFG["num_transformer_layer"])}
    return (f"vit fp8 dgrad per-tensor vs bf16 dgrad, loss {losses[0]:.3f}->{losses[-1]:.3f}", met,
            {"l2": 1.9e-1, "loss_not_falling": 0})


def check_vit_fp8_wgrad(B=4):
    """fp8 weight-gradient GEMMs (enable_fp8(wgrad=True): fp8 dy^T, e4m3 by default, x e4m3 x^T) against the bf16 weight
    gradients of the same fp8 model (identical calibrated passes, fp8 dgrads in both), per encoder
    GEMM weight; then training with them must decrease the loss. Errors printed into the test log."""
    from pytorch_vit_paper_replication_amd.models import ViT
    from pytorch_vit_paper_replication_amd.ops.fused_vit import cross_entropy

    torch.manual_seed(0)
    m = ViT(**_FP8_CFG).to(DEV).enable_fp8(dgrad=True, wgrad=True)
    x = torch.rand(B * 64, 3, 64, 64, device=DEV)
    y = torch.randint(0, 10, (B * 64,), device=DEV)
    names = [n for n, p in m.named_parameters() if p.dim() == 2 and "encoder" in n]

    def run(wgrad_fp8: bool):
        m.enable_fp8(dgrad=True, wgrad=wgrad_fp8)  # keeps the calibrated scaling state
        m.zero_grad(set_to_none=False)
        cross_entropy(m(x), y).backward()
        torch.cuda.synchronize()
        return {n: p.grad.float().clone() for n, p in m.named_parameters() if n in names}

    run(True)  # calibrates every slot; weight gradients of this first pass are bf16
    ref = run(False)
    f8 = run(True)
    per = [(n, errs(f8[n], ref[n])[0]) for n in names]
    print("fp8 wgrad per-tensor rel-L2 vs bf16 wgrad: " + ", ".join(f"{n.split('.')[-2]}.{n.split('.')[-1]} {e:.3e}" for n, e in per))
    m.enable_fp8(dgrad=True, wgrad=True)
    losses, ok = _train_losses(m, x, y)
    met = {"l2": max(e for _, e in per), "loss_not_falling": float(not ok or len(per) != 4 * _FP8_CFG["num_transformer_layer"])}
    return (f"vit fp8 wgrad per-tensor vs bf16 wgrad, loss {losses[0]:.3f}->{losses[-1]:.3f}", met,
            {"l2": 1.6e-1, "loss_not_falling": 0})


def check_vit_fp8_grad_formats(B=4):
    """e4m3 vs e5m2 gradients in the fp8 dgrad / wgrad GEMMs (enable_fp8(grad_fmt=...)): every encoder
    parameter gradient of the fully fp8 backward against the bf16-backward gradients of the same
    fp8-forward model (identical calibrated passes). e4m3's extra mantissa bit must lower the mean
    per-tensor error (the captured-operand study, profiles/r6/mx_study, measured -40 % on the weight
    gradients), and training with e4m3 gradients must decrease the loss."""
    from pytorch_vit_paper_replication_amd.models import ViT
    from pytorch_vit_paper_replication_amd.ops.fused_vit import cross_entropy

    torch.manual_seed(0)
    m = ViT(**_FP8_CFG).to(DEV)
    x = torch.rand(B * 64, 3, 64, 64, device=DEV)
    y = torch.randint(0, 10, (B * 64,), device=DEV)
    names = [n for n, p in m.named_parameters() if "encoder" in n]

    def grads(dgrad: bool, fmt: str):
        m.enable_fp8(dgrad=dgrad, wgrad=dgrad, grad_fmt=fmt)  # a new format: fresh scaling state
        for _ in range(2):  # the first pass calibrates every slot (its weight gradients are bf16)
            m.zero_grad(set_to_none=False)
            cross_entropy(m(x), y).backward()
        torch.cuda.synchronize()
        assert m._fp8 is not None and m._fp8.grad.fmt == (0 if fmt == "e4m3" else 1)
        return {n: p.grad.float().clone() for n, p in m.named_parameters() if n in names}

    ref = grads(False, "e5m2")
    e5 = grads(True, "e5m2")
    e4 = grads(True, "e4m3")
    err5 = [errs(e5[n], ref[n])[0] for n in names]
    err4 = [errs(e4[n], ref[n])[0] for n in names]
    mean5, mean4 = sum(err5) / len(err5), sum(err4) / len(err4)
    print(f"fp8 gradient formats, mean per-tensor rel-L2 vs bf16 backward: e5m2 {mean5:.3e}, e4m3 {mean4:.3e} "
          f"(ratio {mean4 / mean5:.2f})")
    m.enable_fp8(dgrad=True, wgrad=True, grad_fmt="e4m3")
    losses, ok = _train_losses(m, x, y)
    met = {"e4m3_over_e5m2": mean4 / mean5, "e4m3_max_l2": max(err4), "loss_not_falling": float(not ok)}
    return (f"vit fp8 e4m3 vs e5m2 gradients: mean rel-L2 {mean4:.2e} vs {mean5:.2e}, e4m3 loss {losses[0]:.3f}->{losses[-1]:.3f}",
            met, {"e4m3_over_e5m2": 0.9, "e4m3_max_l2": 1.6e-1, "loss_not_falling": 0})


def check_fp8_nonfinite_recovery(B=2):
    """One step whose gradients overflow (an Inf fed into the backward) must not poison the
    delayed-scaling histories: that step is skipped by FusedAdam, and the NEXT step's scales, dgrad
    outputs, loss and gradients are finite again."""
    from pytorch_vit_paper_replication_amd.models import ViT
    from pytorch_vit_paper_replication_amd.ops import fused_vit
    from pytorch_vit_paper_replication_amd.ops.fused_vit import cross_entropy
    from pytorch_vit_paper_replication_amd.optim import FusedAdam

    torch.manual_seed(0)
    m = ViT(**_FP8_CFG).to(DEV).enable_fp8(dgrad=True, wgrad=True)
    opt = FusedAdam(m.parameters(), lr=1e-3)
    x = torch.rand(B * 64, 3, 64, 64, device=DEV)
    y = torch.randint(0, 10, (B * 64,), device=DEV)

    def step(poison: bool):
        taps = []
        fused_vit.DGRAD_TAP = lambda which, t: taps.append(bool(torch.isfinite(t).all().item()))
        try:
            loss = cross_entropy(m(x), y)
            if poison:  # an overflowing loss scale: the whole backward sees Inf
                loss = loss * float("inf")
            opt.zero_grad()
            loss.backward()
            opt.step(clip_norm=1.0)
        finally:
            fused_vit.DGRAD_TAP = None
        torch.cuda.synchronize()
        return loss.item(), taps

    step(False)
    w0 = m._pvr_store.flat.clone()
    _, taps_bad = step(True)
    skipped = torch.equal(w0, m._pvr_store.flat)
    st = m._fp8
    scales_ok = all(bool(torch.isfinite(t).all().item()) and bool((t > 0).all().item())
                    for t in (st.grad.qscale, st.grad.dscale, st.act.qscale, st.act.dscale))
    scales_ok = scales_ok and bool(torch.isfinite(st.grad.hist).all().item())
    loss2, taps2 = step(False)
    g_ok = bool(torch.isfinite(m._pvr_store.grad_flat).all().item())
    met = {"not_skipped": float(not skipped), "scales_bad": float(not scales_ok),
           "next_step_nonfinite": float(not (math.isfinite(loss2) and all(taps2) and g_ok)),
           "poison_not_seen": float(all(taps_bad))}
    return ("fp8 Inf-gradient step skipped, scales and next step finite", met, {k: 0 for k in met})


# ----------------------------------------------------------------------------- head / loss / optimizer
def check_xent(B, C):
    ext = _ext.ext()
    logits = rnd(B, C) * 3
    y = torch.randint(0, C, (B,), device=DEV)
    dl = torch.empty_like(logits)
    corr = torch.empty(B, dtype=torch.int32, device=DEV)
    mean = torch.empty(1, device=DEV)
    rows = ext.xent(logits, y, dl, corr, 1.0 / B, mean)
    lr = logits.clone().requires_grad_(True)
    ref = F.cross_entropy(lr, y)
    ref.backward()
    m = worst((rows.mean(), ref), (mean[0], ref), (dl, lr.grad))
    m["acc_flags_bad"] = float(not torch.equal(corr.bool(), logits.argmax(1) == y))
    return (f"xent B{B} C{C}", m, lim(5e-7, 5e-7, acc_flags_bad=0))  # fp32 vs fp32: a few ulps (2.0e-7 seen)


def check_head(B=37, N=5, D=192, C=1000, frozen_w=False):
    """Classifier head kernels (final LayerNorm of the CLS rows + fp32 Linear, csrc/head.hip) vs
    PyTorch fp32 autograd: logits, dW, db, dgamma, dbeta, d(tokens) (CLS rows; all other rows 0).
    frozen_w: no dW (classifier weight frozen) while the bias still trains: db must be written."""
    ext = _ext.ext()
    tok = bf(rnd(B * N, D))
    gam, bet = 1 + 0.1 * rnd(D), 0.1 * rnd(D)
    W, b = rnd(C, D, scale=0.05), rnd(C)
    logits, xhat, rstd = ext.head_fwd(tok, B, N, gam, bet, 1e-5, W, b)
    t = tok.float().view(B, N, D).requires_grad_(True)
    gr, br, Wr, bbr = (x.clone().requires_grad_(True) for x in (gam, bet, W, b))
    ref = F.linear(F.layer_norm(t[:, 0], (D,), gr, br, 1e-5), Wr, bbr)
    dl = rnd(B, C)
    ref.backward(dl)
    dW, db, dg, dbt = (torch.zeros_like(x) for x in (W, b, gam, bet))
    dtok = ext.head_bwd(dl.contiguous(), xhat, rstd, gam, bet, W, B, N, None if frozen_w else dW, db, dg, dbt)
    dt = dtok.float().view(B, N, D)
    pairs = [(logits, ref), (db, bbr.grad), (dg, gr.grad), (dbt, br.grad)] + ([] if frozen_w else [(dW, Wr.grad)])
    m = worst(*pairs)
    m["dtok_l2"], m["dtok_max"] = errs(dt[:, 0], t.grad[:, 0])  # bf16 output rows
    m["other_rows_nonzero"] = float(not bool((dt[:, 1:] == 0).all().item()))
    return (f"head fwd/bwd B{B} N{N} D{D} C{C}{' (weight frozen, bias trained)' if frozen_w else ''}", m, lim(1.5e-6, 2e-6, dtok_l2=3.5e-3, dtok_max=5e-3, other_rows_nonzero=0))


def _adam_pair(cfg, freeze=None):
    from pytorch_vit_paper_replication_amd.models import ViT

    torch.manual_seed(0)
    m1, m2 = ViT(**cfg).to(DEV), ViT(**cfg).to(DEV)
    m2.load_state_dict(m1.state_dict())
    if freeze:
        for m in (m1, m2):
            freeze(m).requires_grad_(False)
    return m1, m2


def _adam_steps(m1, m2):
    from pytorch_vit_paper_replication_amd.optim import FusedAdam, param_groups_weight_decay

    o1 = FusedAdam(param_groups_weight_decay(m1, 0.03), lr=1e-2)
    o2 = torch.optim.Adam(param_groups_weight_decay(m2, 0.03), lr=1e-2)
    for it in range(3):
        for p1, p2 in zip(m1.parameters(), m2.parameters()):
            if not p1.requires_grad:
                continue
            g = torch.randn_like(p1) * (it + 1)
            p1.grad.copy_(g)
            p2.grad = g.clone()
        o1.step(clip_norm=1.0)
        torch.nn.utils.clip_grad_norm_([p for p in m2.parameters() if p.requires_grad], 1.0)
        o2.step()
    return o1, worst(*zip(m1.parameters(), m2.parameters()))


def check_adam():
    from pytorch_vit_paper_replication_amd.runtime.param_store import get_store

    m1, m2 = _adam_pair(dict(image_size=32, patch_size=16, num_transformer_layer=1, num_heads=2, embedding_dim=128,
                             mlp_size=256, num_classes=10))
    st = get_store(m1, torch.device(DEV))
    _, m = _adam_steps(m1, m2)
    m["shadow_l2"] = max(errs(st.bf16(p), p)[0] for p in m1.parameters())  # bf16 shadow = rounding of the master
    return ("fused adam+clip vs torch.optim.Adam", m, lim(1.5e-5, 1e-4, shadow_l2=3.5e-3))


def check_adam_transposed():
    """Adam writing the transposed bf16 shadow (adam_t_kernel): parameters vs torch.optim.Adam, and
    every registered W^T view bit-equal to the transpose of the updated bf16 shadow."""
    from pytorch_vit_paper_replication_amd.runtime.param_store import get_store

    cfg = dict(image_size=32, patch_size=16, num_transformer_layer=2, num_heads=2, embedding_dim=128, mlp_size=256, num_classes=10)
    m1, m2 = _adam_pair(cfg, freeze=lambda m: m.transformer_encoder[1].mlp_block.mlp[0].weight)  # a frozen registered weight
    st = get_store(m1, torch.device(DEV))
    ws = [w for blk in m1.transformer_encoder for w in blk.fused_params()[2:12:2] if w.dim() == 2]
    st.register_transposed(ws)
    st.ensure_transposed()
    o1, m = _adam_steps(m1, m2)
    m["not_fused"] = float(not (o1._tmeta_key is not None and not st._t_dirty))
    m["wt_inexact"] = float(not all(torch.equal(st.bf16_t(w), st.bf16(w).t()) for w in ws))
    return ("fused adam + W^T shadow vs torch.optim.Adam", m, lim(1.5e-5, 1e-4, not_fused=0, wt_inexact=0))


# ----------------------------------------------------------------------------- optimizer kernels on raw buffers
# csrc/optim.hip and cast_f32_bf16 through ext.grad_norm / ext.adam / ext.adam_t / ext.cast_f32_bf16, against the
# float64 reference of tests/optim_reference.py (itself checked against torch in float64 on the CPU), at
# the sizes where every grid-stride loop takes its second trip.
#
# Adam limits: the same single step is computed by fp32 torch.optim.Adam / AdamW (single-tensor, fed the
# same fp32 g * gscale) and measured against the same float64 reference; the kernel may be 4x worse on
# each metric: both evaluate the same dozen fp32 operations in another association, so a factor of a few
# is rounding and an order of magnitude is a defect. Each step starts from the kernel's own fp32 state,
# so errors do not accumulate. Metrics are taken per step and per param group; the reported value of a
# metric is that of the step and group where kernel / limit is largest (a NaN counts as largest); the
# check's name carries the yardstick's values there.
def errs64(out: torch.Tensor, ref: torch.Tensor) -> Tuple[float, float]:
    """``errs`` in float64: a float64 reference is not rounded to fp32 before the subtraction."""
    o, r = out.double().reshape(-1), ref.double().reshape(-1)
    d = o - r
    rn, rm = r.norm().item(), r.abs().max().item()
    if rn == 0.0:
        return d.norm().item(), d.abs().max().item()
    return d.norm().item() / rn, d.abs().max().item() / rm


ADAM_STEPS = (1, 2, 1000)
# (lr, betas, eps, weight decay, decoupled): lr 10x apart, so an element updated with another group's row
# is a gross error; coupled, decoupled and no decay; the betas of tests/optim_reference.py
ADAM_SPECS = ((1e-2, (0.9, 0.999), 1e-8, 0.03, False), (1e-3, (0.8, 0.95), 1e-6, 0.1, True), (1e-4, (0.0, 0.5), 1e-5, 0.0, False))
SENTINEL = 7.0


def _adam_rows(G):
    """Table rows of the three specs: the last row, the middle and row 0 of a larger table."""
    return (0, 1, 2) if G == 3 else (G - 1, G // 2, 0)


def _adam_table(step, G=3, zero_lr=None):
    """float32 [G, 10] table of ``step``; rows no segment names hold lr 1e3. zero_lr: spec whose lr is 0."""
    from tests import optim_reference as R

    rows = [R.group_row(1e3, (0.5, 0.5), 1.0, 0.5, step, False) for _ in range(G)]
    for k, (lr, betas, eps, wd, dec) in enumerate(ADAM_SPECS):
        rows[_adam_rows(G)[k]] = R.group_row(0.0 if zero_lr == k else lr, betas, eps, wd, step, dec)
    return R.table_f32(rows)


def _torch_adam_step32(p, g_scaled, m, v, row, step, betas):
    """The yardstick: one fp32 torch.optim.Adam / AdamW step (single-tensor) from the given state.
    ``betas``: the exact (double) betas the row was built from, so torch's own 1 - beta and bias
    corrections are those of the row; lr, eps and the decay are the row's fp32 values."""
    from tests import optim_reference as R

    lr, _, _, eps, wd, _, _, dec, _, _ = R.row_values(row)
    b1, b2 = betas
    tp = torch.nn.Parameter(p.clone())
    tp.grad = g_scaled.clone()
    opt = (torch.optim.AdamW if dec else torch.optim.Adam)([tp], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd, foreach=False)
    opt.state[tp] = {"step": torch.tensor(float(step - 1)), "exp_avg": m.clone(), "exp_avg_sq": v.clone()}
    opt.step()
    return tp.detach(), opt.state[tp]["exp_avg"], opt.state[tp]["exp_avg_sq"]


def _adam_driver(name, launch, bufs, elem_group, G, gscale=1.0, ema_pair=None) -> Result:
    """Three launches (table rows of steps 1, 2, 1000) on fresh gradients, each compared with the
    float64 step from the kernel's own state before it. ``bufs``: p, g, m, v and optionally shadow, ema
    (flat, layout of p); ``elem_group``: table row per element, -1 where nothing may change (frozen
    segments, gaps). ``launch(table_np)`` runs the kernel in place."""
    from tests import optim_reference as R

    p, g, m, v = bufs["p"], bufs["g"], bufs["m"], bufs["v"]
    n = p.numel()
    upd = elem_group >= 0
    idxs = {int(gi): (elem_group == gi).nonzero().squeeze(1) for gi in torch.unique(elem_group[upd]).tolist()}
    best, flags = {}, {"frozen_changed": 0.0}
    if "shadow" in bufs:
        flags["shadow_not_rne"] = 0.0
    if "ema" in bufs:
        flags["ema_off_bound"] = 0.0
    for step in ADAM_STEPS:
        tab = _adam_table(step, G)
        g.copy_(torch.where(upd, R.adam_grad(n, None, DEV), torch.full_like(g, SENTINEL)))
        before = {k: t.clone() for k, t in bufs.items()}
        launch(tab)
        torch.cuda.synchronize()
        # per param group (the lr are 10x apart and the segments of very different size: pooled, the
        # large decoupled segment would carry the norm and dilute an error confined to another group)
        for gi, idx in idxs.items():
            p0, g0, m0, v0 = (before[k][idx] for k in ("p", "g", "m", "v"))
            pr, mr, vr = R.adam_step64(p0, g0, m0, v0, tab[gi], gscale)
            py, my, vy = _torch_adam_step32(p0, g0 * gscale, m0, v0, tab[gi], step, ADAM_SPECS[_adam_rows(G).index(gi)][1])
            base = p0.double()
            for key, k_t, r_t, y_t in zip(("dp", "m", "v"), (p[idx].double() - base, m[idx], v[idx]), (pr - base, mr, vr),
                                          (py.double() - base, my, vy)):
                for suffix, kv, yv in zip(("l2", "max"), errs64(k_t, r_t), errs64(y_t, r_t)):
                    ratio = 0.0 if kv == 0.0 else (math.inf if yv == 0.0 else kv / (4.0 * yv))
                    old = best.get(f"{key}_{suffix}")
                    if old is None or (old[0] == old[0] and not ratio <= old[0]):  # a NaN is taken and kept
                        best[f"{key}_{suffix}"] = (ratio, kv, yv)
        for k, t in bufs.items():  # frozen segments and gaps: bit-unchanged (g everywhere)
            keep = torch.ones_like(upd) if k == "g" else ~upd
            flags["frozen_changed"] += float(not torch.equal(t[keep], before[k][keep]))
        if "shadow" in bufs:
            flags["shadow_not_rne"] += float(not torch.equal(R.bf16_bits(bufs["shadow"])[upd], R.bf16_rne_bits(p)[upd]))
        if "ema" in bufs:
            from tests.test_gpu_model_ema import _check_update

            try:
                _check_update(bufs["ema"], before["ema"], p, ema_pair, upd, f"{name} step {step}")
            except AssertionError:
                flags["ema_off_bound"] += 1.0
    metrics = {k: b[1] for k, b in best.items()}
    limits = {k: 4.0 * b[2] for k, b in best.items()}
    metrics.update(flags)
    limits.update({k: 0 for k in flags})
    yard_txt = " ".join(f"{k} {best[k][2]:.1e}" for k in ("dp_l2", "dp_max", "m_l2", "v_l2"))
    return (f"{name} [fp32 torch: {yard_txt}]", metrics, limits)


def _adam_flag_runs(launch, bufs, elem_group, G, metrics, limits):
    """A flagged non-finite step is skipped (every buffer bit-unchanged) or, with skip_nonfinite off,
    taken; a group with lr 0 leaves its parameters bit-unchanged while its moments move."""
    from tests import optim_reference as R

    upd = elem_group >= 0
    bad = torch.tensor([float("inf"), 0.5, 1.0], device=DEV)
    outs = [k for k in bufs if k != "g"]
    bufs["g"].copy_(torch.where(upd, R.adam_grad(upd.numel(), None, DEV), torch.full_like(bufs["g"], SENTINEL)))
    before = {k: bufs[k].clone() for k in outs}
    launch(_adam_table(3, G), clip=bad, skip=True)
    torch.cuda.synchronize()
    metrics["skipped_step_wrote"] = float(sum(not torch.equal(bufs[k], before[k]) for k in outs))
    launch(_adam_table(3, G), clip=bad, skip=False)
    torch.cuda.synchronize()
    metrics["unskipped_step_idle"] = float(sum(torch.equal(bufs[k][upd], before[k][upd]) for k in outs))
    row = _adam_rows(G)[1]
    idx = (elem_group == row).nonzero().squeeze(1)
    before = {k: bufs[k][idx].clone() for k in ("p", "m", "v")}
    launch(_adam_table(4, G, zero_lr=1))
    torch.cuda.synchronize()
    metrics["lr0_moved_p"] = float(not torch.equal(bufs["p"][idx], before["p"]))
    metrics["lr0_froze_moments"] = float(torch.equal(bufs["m"][idx], before["m"]) or torch.equal(bufs["v"][idx], before["v"]))
    limits.update(skipped_step_wrote=0, unskipped_step_idle=0, lr0_moved_p=0, lr0_froze_moments=0)


def _adam_bufs(n, upd, shadow=True, ema=False):
    from tests import optim_reference as R

    sent = torch.full((n,), SENTINEL, device=DEV)
    bufs = {"p": torch.where(upd, R.adam_inputs(n, None, DEV), sent), "g": sent.clone(),
            "m": torch.where(upd, torch.zeros_like(sent), sent), "v": torch.where(upd, torch.zeros_like(sent), sent)}
    if shadow:
        bufs["shadow"] = sent.to(torch.bfloat16)
    if ema:
        bufs["ema"] = torch.where(upd, bufs["p"] + 0.01 * torch.randn(n, device=DEV), sent)
    return bufs


EMA_PAIR = (0.99, 1.0 - 0.99)  # rounded to fp32 as ModelEma.pair_at does


def _ema_kw(bufs):
    import numpy as np

    if "ema" not in bufs:
        return {}, None
    pair = (np.float32(EMA_PAIR[0]), np.float32(EMA_PAIR[1]))
    return dict(ema=bufs["ema"], ema_pair=torch.from_numpy(np.array(pair, dtype=np.float32))), pair


ADAM_N = 4 * (8192 * 256 + 3 * 256 + 5)  # 8,391,700: adam_kernel's 8192 x 256 float4 and a second trip


def adam_kernel_layout(tiny=False):
    """(n, seg_start, spec per segment, -1 frozen). Large: a 4-element segment, a large one, a frozen one in
    the middle, a boundary 512 elements into the second grid-stride trip, a frozen segment at the end."""
    if tiny:
        return 8, [0], [1]
    n = ADAM_N
    return n, [0, 4, 5_000_000, 5_000_400, 8_388_608 + 512, n - 200], [0, 1, -1, 2, 0, -1]


def check_adam_kernel(table="host", G=3, clip=False, shadow=True, ema=False, tiny=False) -> Result:
    """adam_kernel on raw buffers. table: "host" (rows travel in the kernel arguments, G <= 8) or "dev"."""
    from tests import optim_reference as R

    ext = _ext.ext()
    n, starts, specs = adam_kernel_layout(tiny)
    rows = [(-1 if s < 0 else _adam_rows(G)[s]) for s in specs]
    elem_group = R.expand_segments(starts, rows, n).to(DEV)
    seg_start = torch.tensor(starts, dtype=torch.int64, device=DEV)
    seg_group = torch.tensor(rows, dtype=torch.int32, device=DEV)
    bufs = _adam_bufs(n, elem_group >= 0, shadow, ema)
    ema_kw, pair = _ema_kw(bufs)
    coef = 0.37
    clip_t = torch.tensor([123.0, coef, 0.0], device=DEV) if clip else None

    def launch(tab, clip=clip_t, skip=True):
        t = torch.from_numpy(tab)
        ext.adam(bufs["p"], bufs["g"], bufs["m"], bufs["v"], bufs.get("shadow"), seg_start, seg_group,
                 t if table == "host" else t.to(DEV), clip, skip, **ema_kw)

    gscale = float(clip_t[1]) if clip else 1.0
    name = (f"adam_kernel n{n} {table} table G{G}" + (f" clip coef {coef}" if clip else " no clip") + ("" if shadow else " no shadow") +
            (" +ema" if ema else ""))
    name, metrics, limits = _adam_driver(name, launch, bufs, elem_group, G, gscale, pair)
    _adam_flag_runs(launch, bufs, elem_group, G, metrics, limits)
    return name, metrics, limits


def adam_t_layout():
    """Synthetic tables of adam_t_kernel over one flat buffer with sentinel gaps. Matrices 64x128, 64x64
    (frozen) and 192x64 (R != C); flat ranges of 262,144 + 300 float4 in all (a second grid-stride trip,
    whose range lookup crosses a boundary): one right after a matrix, one of 4 elements, one frozen.
    Returns (n, nt, tmeta rows {soff, doff, R, C, first tile, spec}, fmeta rows {start, elements, spec,
    first float4}); spec -1 frozen."""
    mats = [(64, 128, 1), (64, 64, -1), (192, 64, 2)]
    total4 = 262_144 + 300
    flat = [(1000, 0), (4, 2), (400, -1), (4 * (262_144 + 100) - 1404, 1), (800, 0)]  # (elements, spec)
    assert sum(e for e, _ in flat) == 4 * total4
    order = ["m0", "f0", "gap", "m1", "f1", "gap", "m2", "gap", "f2", "gap", "f3", "f4", "gap"]
    off, doff, tiles, f4 = 64, 16, 0, 0
    trows, frows = [], []
    for item in order:
        if item == "gap":
            off += 64
        elif item[0] == "m":
            R_, C_, spec = mats[int(item[1])]
            trows.append([off, doff, R_, C_, tiles, spec])
            off += R_ * C_
            doff += R_ * C_ + 32
            tiles += (R_ // 64) * (C_ // 64)
        else:
            e, spec = flat[int(item[1])]
            frows.append([off, e, spec, f4])
            off += e
            f4 += e // 4
    return off, doff, trows, frows, tiles, f4


def check_adam_t_kernel(table="host", G=3, clip=False, ema=False) -> Result:
    ext = _ext.ext()
    n, nt, trows, frows, ntiles, flat4 = adam_t_layout()
    rowof = lambda s: -1 if s < 0 else _adam_rows(G)[s]  # noqa: E731
    elem_group = torch.full((n,), -1, dtype=torch.int64)
    for soff, _, R_, C_, _, spec in trows:
        elem_group[soff:soff + R_ * C_] = rowof(spec)
    for start, e, spec, _ in frows:
        elem_group[start:start + e] = rowof(spec)
    elem_group = elem_group.to(DEV)
    tmeta = torch.tensor([r[:5] + [rowof(r[5])] for r in trows], dtype=torch.int64, device=DEV)
    fmeta = torch.tensor([[r[0], r[1], rowof(r[2]), r[3]] for r in frows], dtype=torch.int64, device=DEV)
    bufs = _adam_bufs(n, elem_group >= 0, True, ema)
    shadow_t = torch.full((nt,), SENTINEL, dtype=torch.bfloat16, device=DEV)
    ema_kw, pair = _ema_kw(bufs)
    coef = 0.37
    clip_t = torch.tensor([123.0, coef, 0.0], device=DEV) if clip else None
    wt = {"mismatch": 0.0, "outside": 0.0}

    def launch(tab, clip=clip_t, skip=True):
        t = torch.from_numpy(tab)
        st_before = shadow_t.clone()
        ext.adam_t(bufs["p"], bufs["g"], bufs["m"], bufs["v"], bufs["shadow"], shadow_t, tmeta, ntiles, fmeta, flat4,
                   t if table == "host" else t.to(DEV), clip, skip, **ema_kw)
        torch.cuda.synchronize()
        written = torch.zeros(nt, dtype=torch.bool, device=DEV)
        for soff, doff, R_, C_, _, spec in trows:
            if spec < 0 or (skip and clip is not None and float(clip[2]) != 0.0):
                continue
            written[doff:doff + R_ * C_] = True
            w = bufs["shadow"][soff:soff + R_ * C_].view(R_, C_)
            wt["mismatch"] += float(not torch.equal(shadow_t[doff:doff + R_ * C_].view(C_, R_), w.t()))
        wt["outside"] += float(not torch.equal(shadow_t[~written], st_before[~written]))

    gscale = float(clip_t[1]) if clip else 1.0
    name = f"adam_t_kernel n{n} {table} table G{G}" + (f" clip coef {coef}" if clip else " no clip") + (" +ema" if ema else "")
    name, metrics, limits = _adam_driver(name, launch, bufs, elem_group, G, gscale, pair)
    _adam_flag_runs(launch, bufs, elem_group, G, metrics, limits)
    metrics.update(wt_not_transpose=wt["mismatch"], wt_outside_written=wt["outside"])
    limits.update(wt_not_transpose=0, wt_outside_written=0)
    return name, metrics, limits


NORM_TRIP2 = 1_048_576  # sumsq_partial_kernel: 1024 blocks x 256 float4


def check_grad_norm(n, max_norm, poison=False) -> Result:
    """grad_norm on a flat buffer of n elements. The norm's limit is derived: at most two float4 per
    thread, so the sum of squares is built from at most about 19 fp32 additions of non-negative terms
    (10 in the thread, 6 in the wave, 2 across waves, the products' roundings; the tail and the 1024
    partials are summed in double): 19 * 2^-24 = 1.1e-6 relative on the sum, half of that on the norm;
    the limit is 1e-6. poison: one Inf or NaN at element 0, at the last (tail) element or at an element
    only the second grid-stride trip reads must each raise the flag."""
    import numpy as np

    from tests import optim_reference as R

    ext = _ext.ext()
    g = torch.randn(n, device=DEV) * 3.0
    ws = torch.empty(ext.norm_partial_blocks(), device=DEV)
    out = torch.full((3,), SENTINEL, device=DEV)

    def run(buf):
        ws.fill_(float("nan"))  # stale workspace contents: every partial must be overwritten
        out.fill_(SENTINEL)
        ext.grad_norm(buf, float(max_norm), ws, out)
        torch.cuda.synchronize()
        return out.cpu().numpy().copy()

    if poison:
        where = [0, n - 1] + ([NORM_TRIP2 + 17] if n > NORM_TRIP2 + 17 else [])
        missed = 0
        for val in (float("inf"), float("-inf"), float("nan")):
            for i in where:
                gg = g.clone()
                gg[i] = val
                missed += int(run(gg)[2] != 1.0)
        return (f"grad_norm n{n} max_norm {max_norm:g}: Inf / NaN at {where}", {"flag_missed": float(missed)}, {"flag_missed": 0})
    o = run(g)
    want = R.norm64(g)
    m = {"norm_rel": abs(float(o[0]) - want) / want, "flag_set": float(o[2] != 0.0), "stale_partials": float(bool(torch.isnan(ws).any())),
         "rerun_differs": float(not np.array_equal(o.view(np.int32), run(g).view(np.int32)))}
    o0 = np.float32(o[0])
    denom = np.float32(o0 + np.float32(1e-6))
    if max_norm == 0 or denom <= np.float32(max_norm):
        m["coef_ulps"] = 0.0 if o[1] == np.float32(1.0) else math.inf  # exactly 1
    else:
        expect = np.float32(max_norm) / denom
        m["coef_ulps"] = abs(float(o[1]) - float(expect)) / float(np.spacing(expect))
    return (f"grad_norm n{n} max_norm {max_norm:g}", m, {"norm_rel": 1e-6, "coef_ulps": 1.0, "flag_set": 0, "stale_partials": 0, "rerun_differs": 0})


CAST_TRIP2 = 4_194_304  # cast_f32_bf16_kernel: 4096 blocks x 256 float4


def check_cast_f32_bf16(n) -> Result:
    """cast_f32_bf16 (ParamStore.refresh_shadow) bit for bit against the integer round-to-nearest-even of
    tests/optim_reference.py on randn plus the planted edge values (start, second trip, tail); a NaN
    may carry any payload. The element after the output stays untouched."""
    from tests import optim_reference as R

    ext = _ext.ext()
    x = torch.randn(n, device=DEV)
    planted = R.cast_planted_values().to(DEV)
    k = min(n, planted.numel())
    x[:k] = planted[:k]
    if n > CAST_TRIP2 + 8 + k:
        x[CAST_TRIP2 + 8:CAST_TRIP2 + 8 + k] = planted[:k]
    x[n - k:] = planted[planted.numel() - k:] if n > k else x[n - k:]
    out = torch.full((n + 1,), SENTINEL, dtype=torch.bfloat16, device=DEV)
    ext.cast_f32_bf16(x, out[:n])
    torch.cuda.synchronize()
    got, want = R.bf16_bits(out[:n]), R.bf16_rne_bits(x)
    nan = torch.isnan(x)
    m = {"bits_differ": float(int((got[~nan] != want[~nan]).sum())), "nan_lost": float(int((~R.bf16_is_nan(got[nan])).sum())),
         "wrote_past_n": float(float(out[n]) != SENTINEL), "ties_planted": float(int(((x.view(torch.int32) & 0xFFFF) == 0x8000).sum()) == 0)}
    return (f"cast_f32_bf16 n{n}", m, {k_: 0 for k_ in m})


# ----------------------------------------------------------------------------- whole model
def _grad_errors(mf, mr):
    """Worst per-parameter (rel-L2, max-rel) gradient error, fused model vs reference, and its name."""
    l2 = mx = 0.0
    worst_n = ""
    for (n, p1), p2 in zip(mf.named_parameters(), mr.parameters()):
        a, b = errs(p1.grad, p2.grad)
        if a > l2:
            l2, worst_n = a, n
        mx = max(mx, b)
    return l2, mx, worst_n


def check_vit_fused_vs_reference(B=4, train=False, limits=(2.1e-2, 2.8e-2, 2.5e-2, 3.6e-2), **over):
    """Whole-model forward logits and EVERY parameter gradient, fused bf16 path vs the PyTorch fp32
    model with the same weights (dropout 0)."""
    from pytorch_vit_paper_replication_amd.models import ViT

    torch.manual_seed(0)
    cfg = dict(image_size=64, patch_size=16, num_transformer_layer=2, num_heads=2, embedding_dim=128, mlp_size=256,
               num_classes=10, mlp_dropout=0.0, embedding_dropout=0.0)
    cfg.update(over)
    mf = ViT(**cfg).to(DEV)
    mr = ViT(**cfg).to(DEV)
    mr.load_state_dict(mf.state_dict())
    assert mf._fused_supported(torch.empty(1, 3, cfg["image_size"], cfg["image_size"]))
    x = torch.rand(B, 3, cfg["image_size"], cfg["image_size"], device=DEV)
    y = torch.randint(0, cfg["num_classes"], (B,), device=DEV)
    mf.train(train)
    mr.train(train)
    lf = mf(x)
    lr = _reference_logits(mr, x)
    F.cross_entropy(lf, y).backward()
    F.cross_entropy(lr, y).backward()
    l2, mx, wn = _grad_errors(mf, mr)
    fl2, fmx = errs(lf, lr)
    m = {"logits_l2": fl2, "logits_max": fmx, "grad_l2": l2, "grad_max": mx}
    D, N = cfg["embedding_dim"], (cfg["image_size"] // cfg["patch_size"]) ** 2 + 1
    return (f"vit fused vs fp32 ref B{B} D{D} N{N} L{cfg['num_transformer_layer']} (worst grad {wn})", m,
            {"logits_l2": limits[0], "logits_max": limits[1], "grad_l2": limits[2], "grad_max": limits[3]})


def check_block_full_width(B=16):
    """Full-width single encoder block (ViT-B/16 geometry: D 768, 12 heads, MLP 3072, N 197) forward +
    backward on the fused path vs fp32 autograd: logits and every parameter gradient."""
    return check_vit_fused_vs_reference(B, True, (1.3e-2, 1.4e-2, 1.5e-2, 1.9e-2), num_transformer_layer=1, image_size=224,
                                        patch_size=16, num_heads=12, embedding_dim=768, mlp_size=3072, num_classes=1000)


def check_vit_inference(B=5):
    """Inference path (eval under no_grad / inference_mode): the fc1 epilogue skips the GELU
    derivative and nothing is saved; logits must equal the grad-mode fused forward bit for bit and
    match the fp32 reference; a later training step on the same model still gets gradients."""
    from pytorch_vit_paper_replication_amd.models import ViT

    torch.manual_seed(0)
    cfg = dict(image_size=64, patch_size=16, num_transformer_layer=2, num_heads=2, embedding_dim=128, mlp_size=256,
               num_classes=10)
    m = ViT(**cfg).to(DEV).eval()
    mr = ViT(**cfg).to(DEV).eval()
    mr.load_state_dict(m.state_dict())
    x = torch.rand(B, 3, 64, 64, device=DEV)
    lg = m(x)
    with torch.no_grad():
        ln = m(x)
    with torch.inference_mode():
        li = m(x)
    with torch.no_grad():
        lr = _reference_logits(mr, x)
    same = torch.equal(lg.detach(), ln) and torch.equal(ln, li)
    m.train()
    F.cross_entropy(m(x), torch.randint(0, 10, (B,), device=DEV)).backward()
    has_grad = all(p.grad is not None and torch.isfinite(p.grad).all().item() for p in m.parameters())
    met = worst((li, lr))
    met.update(not_bit_identical=float(not same), no_grad_after=float(not has_grad))
    return ("vit inference (no_grad / inference_mode) == grad-mode logits, vs fp32 ref", met,
            lim(2.1e-2, 2.8e-2, not_bit_identical=0, no_grad_after=0))


def check_vit_fp8_inference(B=8):
    """fp8 inference (eval under inference_mode / no_grad): the fc1 GELU epilogue stores no derivative
    and the LayerNorm / attention / fc1 producers write only the e4m3 copies the next GEMM reads (no
    bf16 xn1 / o / xn2 / h: filled with NaN here, POISON_SKIPPED). Once the slots are calibrated, the logits equal
    the grad-mode fp8 forward (which writes every copy) bit for bit and stay within the fp8 forward
    error of the fp32 reference; a training step afterwards still gets finite gradients."""
    from pytorch_vit_paper_replication_amd.models import ViT
    from pytorch_vit_paper_replication_amd.ops import fused_vit

    torch.manual_seed(0)
    m = ViT(**_FP8_CFG).to(DEV).eval().enable_fp8()
    mr = ViT(**_FP8_CFG).to(DEV).eval()
    mr.load_state_dict(m.state_dict())
    x = torch.rand(B * 4, 3, 64, 64, device=DEV)  # 544 tokens: the fp8 path (>= 256)
    m(x)  # calibrates the activation slots (eval: the scales stay put afterwards)
    assert m._fp8 is not None and all(m._fp8.act.calibrated), "fp8 path did not engage / calibrate"
    lg = m(x)
    fused_vit.POISON_SKIPPED = True
    try:
        with torch.inference_mode():
            li = m(x)
        with torch.no_grad():
            ln = m(x)
    finally:
        fused_vit.POISON_SKIPPED = False
    with torch.no_grad():
        lr = _reference_logits(mr, x)
    same = torch.equal(lg.detach(), li) and torch.equal(li, ln)
    m.train()
    F.cross_entropy(m(x), torch.randint(0, 10, (B * 4,), device=DEV)).backward()
    has_grad = all(p.grad is not None and torch.isfinite(p.grad).all().item() for p in m.parameters())
    met = worst((li, lr))
    met.update(not_bit_identical=float(not same), nonfinite=float(not torch.isfinite(li).all().item()),
               no_grad_after=float(not has_grad))
    return ("vit fp8 inference (no derivative, e4m3 copies only) == grad-mode fp8 logits, vs fp32 ref", met,
            lim(8.5e-2, 1e-1, not_bit_identical=0, nonfinite=0, no_grad_after=0))


def check_vit_dropout_fused(B=4):
    """Training with every dropout on (embedding, MLP, attention probabilities p = 0.1) stays on the
    HIP path (fused forward engaged; the attention kernels draw the mask in-register): replaying the
    same device seed gives bit-identical logits and gradients (forward and backward masks are pure
    functions of the seed), a different seed different logits, and a few steps reduce the loss. With
    attn_dropout = 0 and the other dropouts 0, train-mode logits equal eval-mode logits bit for bit."""
    from pytorch_vit_paper_replication_amd.models import ViT

    torch.manual_seed(0)
    cfg = dict(image_size=64, patch_size=16, num_transformer_layer=2, num_heads=2, embedding_dim=128, mlp_size=256,
               num_classes=10, mlp_dropout=0.1, embedding_dropout=0.1, attn_dropout=0.1)
    m = ViT(**cfg).to(DEV).train()
    x = torch.rand(B, 3, 64, 64, device=DEV)
    y = torch.randint(0, 10, (B,), device=DEV)
    on_hip = m._fused_supported(x)
    m._dropout_seed(x.device)
    rng0 = m._pvr_rng.clone()
    outs = []
    for _ in range(2):
        m._pvr_rng.copy_(rng0)
        for p in m.parameters():
            p.grad = None
        lg = m(x)
        F.cross_entropy(lg, y).backward()
        outs.append((lg.detach().clone(), {n: p.grad.detach().clone() for n, p in m.named_parameters()}))
    replay_same = torch.equal(outs[0][0], outs[1][0])
    # gradients: the same masks; f32 atomics (bias / LayerNorm column sums) may reorder additions
    replay_grad = max(errs(outs[1][1][n], outs[0][1][n])[0] for n in outs[0][1])
    other = m(x).detach()  # the RNG advanced: another mask
    differs = not torch.equal(other, outs[0][0])
    losses, ok = _train_losses(m, x, y, steps=8)
    m0 = ViT(**dict(cfg, mlp_dropout=0.0, embedding_dropout=0.0, attn_dropout=0.0)).to(DEV)
    m0.load_state_dict(m.state_dict())
    p0_same = torch.equal(m0.train()(x).detach(), m0.eval()(x).detach())
    met = {"not_on_hip": float(not on_hip), "replay_differs": float(not replay_same), "replay_grad_l2": replay_grad,
           "seed_ignored": float(not differs),
           "loss_not_falling": float(not ok), "p0_not_identical": float(not p0_same)}
    return (f"vit with attention + MLP + embedding dropout on the HIP path, loss {losses[0]:.3f}->{losses[-1]:.3f}",
            met, dict({k: 0 for k in met}, replay_grad_l2=1e-5))


def all_checks() -> List[Callable[[], Result]]:
    c = []
    for t in (0, 6, 12, 13):
        c.append(lambda t=t: check_gemm_fwd(50432 // 16, 768, 768, t))
        c.append(lambda t=t: check_gemm_fwd(197 * 3, 2304, 768, t, True, True))
        c.append(lambda t=t: check_gemm_gelu(197 * 2, 3072, 768, t))
        c.append(lambda t=t: check_gemm_dgrad(197 * 2, 3072, 768, t))
        c.append(lambda t=t: check_gemm_dgrad(197 * 3, 768, 2304, t, True))
        c.append(lambda t=t: check_gemm_wgrad(197 * 5, 768, 3072, t))
    c += [
        lambda: check_gemm_fwd(777, 2304, 3072, 12, True, True),
        lambda: check_gemm_fwd(5000, 2304, 768, 13, True, True),   # persistent: several tiles per CU
        lambda: check_gemm_fwd(9000, 768, 128, 13, True, False),   # nk = 2: next-tile DMAs start at phase 3
        lambda: check_gemm_gelu(6000, 3072, 768, 13),
        # persistent, 2-3 tiles per workgroup: full tiles keep their epilogue stores in flight across
        # the tile boundary (plain / residual / GELU epilogues), the partial last row of tiles drains
        lambda: check_gemm_fwd(12608, 2304, 768, 13, True, False),
        lambda: check_gemm_fwd(12608, 2304, 768, 13, True, True),
        lambda: check_gemm_gelu(12608, 3072, 768, 13),
        lambda: check_gemm_gelu_dropout(5000, 3072, 768),
        lambda: check_gemm_dropout(3000, 768, 128, 0.1, 13),
        lambda: check_gemm_dropout(3000, 768, 1024, 0.1, 13),  # persistent, 16 K-tiles (1/K exact in bf16)
        lambda: check_gemm_dropout(3000, 768, 1024, 0.1, 12),  # one tile per workgroup, 16 K-tiles
        lambda: check_gemm_gelu_drop_paths(),
        lambda: check_gemm_dgelu_tiles(),
        # wave-specialized persistent kernel (tile 15): M / N tails, K = 256 (8 K-steps), several tiles
        # per workgroup (the epilogue of tile t - 2 beside tile t, the drain of the last two)
        lambda: check_gemm_fwd(3152, 768, 768, 15),
        lambda: check_gemm_fwd(197 * 3, 2304, 768, 15, True, True),
        lambda: check_gemm_fwd(2000, 1000, 256, 15, True, True),
        lambda: check_gemm_fwd(70000, 768, 512, 15, True, True),
        lambda: check_gemm_gelu(6000, 3072, 768, 15),
        lambda: check_gemm_gelu(50432, 3072, 768, 15),
        lambda: check_gemm_gelu_dropout(5000, 3072, 768, tiles=(13, 15), l2_lim=4e-3),
        lambda: check_gemm_dropout(3000, 768, 1024, 0.1, 15),
        lambda: check_gemm_dgelu(4096, 768, 3072, True, 15),
        lambda: check_gemm_dgelu(50432, 768, 3072, True, 15),
        lambda: check_gemm_fwd(300, 256, 64, 12, True, False),
        # split-K tail of the last dispatch round (ViT-B/16 b256 shapes: 591 tiles -> 2 rounds + 79
        # tiles as 3 K-parts; 2364 tiles -> 9 rounds + 60 tiles as 4 K-parts; 588 patch-embed tiles)
        lambda: check_gemm_tail_split(50432, 768, 3072, "resid_drop"),   # fc2 forward: 3 x 16 K-tiles
        lambda: check_gemm_tail_split(50432, 768, 2304, "resid_drop"),   # qkv dgrad K: 3 x 12 K-tiles
        lambda: check_gemm_tail_split(50432, 3072, 3072, "gelu"),        # 9 rounds + 60 tiles: 4 parts
        lambda: check_gemm_tail_split(50432, 3072, 3072, "dgelu"),
        lambda: check_gemm_tail_split(50176, 768, 3072, "patch"),
        check_gemm_tail_split_fp8,
        lambda: check_gemm_fwd(100, 64, 128, 0, True, True),
        lambda: check_gemm_dgelu(394, 768, 3072),
        lambda: check_gemm_dgelu(4096, 768, 3072, True),
        lambda: check_gemm_dgelu(4096, 768, 3072, False, 12),   # ping-pong, B = W mn-contiguous
        lambda: check_gemm_dgelu(1000, 3072, 768, False, 12),
        lambda: check_gemm_wgrad(17, 64, 128),
        lambda: check_gemm_wgrad(3000, 768, 2304, 12),
        lambda: check_gemm_wgrad_fixup(50432, 2304, 768),
        lambda: check_gemm_wgrad_fixup(12000, 768, 768),
        lambda: check_gemm_wgrad_fixup(5000, 3072, 768),
        lambda: check_gemm_wgrad_fixup(3000, 1000, 200),
        lambda: check_gemm_wgrad(1000, 304, 200, 12),
        lambda: check_gemm_dropout(),
        lambda: check_gemm_dropout(1000, 768, 128, 0.1, 12),
        lambda: check_im2col(3, 3, 224, 16),
        lambda: check_im2col(2, 3, 56, 14),
        lambda: check_patch_bwd(37, 197, 768),
        lambda: check_patch_bwd(5, 17, 1280, 0.0),
        lambda: check_patch_wgrad_narrow(8192),  # tile-12 split-K store + narrow reduction
        lambda: check_patch_wgrad_narrow(512, 256, 300),  # atomic path (temporary + narrow add)
        check_transpose_batched,
        lambda: check_layernorm(394, 768),
        lambda: check_layernorm(100, 1024),
        lambda: check_layernorm(33, 1280),
        lambda: check_layernorm(5000, 768),       # 4-column chunks, grid of resident blocks, grid-stride rows
        lambda: check_layernorm(3000, 1280),
        lambda: check_layernorm_linked(5000, 768),
        lambda: check_layernorm_linked(777, 1280),
        lambda: check_layernorm_linked(1000, 1024),
        lambda: check_attn_fwd(2, 197, 3),
        lambda: check_attn_fwd(1, 17, 2),
        lambda: check_attn_fwd(1, 577, 2),
        # whole-head forward (dh 64, N <= 256): one pair per workgroup, several pairs per
        # workgroup (B*H > CUs), N = 256 (16 waves), N = 1
        lambda: check_attn_fwd(16, 197, 12),
        lambda: check_attn_fwd(40, 197, 12),
        lambda: check_attn_fwd(3, 256, 5),
        lambda: check_attn_fwd(300, 33, 2),
        lambda: check_attn_fwd(4, 1, 3),
        lambda: check_attn_fwd(2, 400, 3),
        lambda: check_attn_fwd(2, 400, 3, 80),
        lambda: check_attn_fwd(2, 577, 3, 80),
        lambda: check_attn_bwd(2, 197, 3),       # pipelined whole-head backward
        lambda: check_attn_bwd(40, 197, 12),     # several pairs per workgroup
        lambda: check_attn_bwd(300, 197, 2),     # 600 pairs: 2-3 pairs per workgroup, pair hand-offs
        lambda: check_attn_bwd(2, 197, 3, 64, True),
        lambda: check_attn_bwd(40, 197, 12, 64, True),  # in_proj bias gradient from the pipelined kernel's partials
        lambda: check_attn_bwd(5, 193, 4),       # pipelined backward, one key in the last slice
        lambda: check_attn_bwd(3, 256, 3),       # generic kernel: 8 full key slices, no masking
        lambda: check_attn_bwd(3, 256, 3, 64, True),
        lambda: check_attn_bwd(2, 224, 3),
        lambda: check_attn_bwd(5, 129, 4),
        lambda: check_attn_bwd(97, 200, 3),
        lambda: check_attn_bwd(3, 256, 5),
        lambda: check_attn_bwd(7, 1, 3),
        lambda: check_attn_bwd(1, 17, 2),
        lambda: check_attn_bwd(1, 64, 1, 64, True),
        lambda: check_attn_bwd(1, 257, 2, 64, True),
        lambda: check_attn_bwd(1, 577, 2),
        # generic kernel with the fused in_proj bias gradient: 3 key blocks (577), a 1-key last block
        # (513 = 2 x 256 + 1), more pairs than CUs, 4 key blocks (1000 keys)
        lambda: check_attn_bwd(2, 577, 3, 64, True),
        lambda: check_attn_bwd(3, 513, 4, 64, True),
        lambda: check_attn_bwd(150, 300, 2, 64, True),
        lambda: check_attn_bwd(1, 1000, 2, 64, True),
        # again: the persistent dQ accumulator must have been re-zeroed by the tail launch's
        # conversion (577 = 2 x 256 + 65) and by the separate conversion pass (400 = 256 + 144)
        lambda: check_attn_bwd(2, 577, 3),
        lambda: check_attn_bwd(2, 400, 3),
        lambda: check_attn_bwd(2, 400, 3),
        lambda: check_attn_bwd(2, 400, 3, 80),
        lambda: check_attn_bwd(2, 577, 3, 80),
        lambda: check_attn_fwd(2, 257, 3, 80),
        lambda: check_attn_fwd(1, 33, 2, 80),
        lambda: check_attn_fwd(3, 1, 2, 80),    # tiled forward with no tile: the last key alone
        lambda: check_attn_fwd(2, 65, 2, 80),   # one full 64-key tile + the last key
        lambda: check_attn_bwd(2, 257, 3, 80),
        lambda: check_attn_bwd(2, 257, 3, 80, True),  # lastkey path + in-kernel bias partials (dh 80)
        lambda: check_attn_bwd(2, 577, 2, 64, True),  # tail split + bias partials from the tail's final dQ pass
        check_gemm_fp8_persistent,
        lambda: check_attn_bwd_q8(2, 257, 3, 80),    # e5m2 dQKV copy: lastkey path (pre-pass writes key N - 1)
        lambda: check_attn_bwd_q8(2, 577, 2, 64),    # tail split (body dK/dV, tail's final dQ pass)
        lambda: check_attn_bwd_q8(3, 197, 2, 80, 0.1),  # one key block, attention dropout
        lambda: check_attn_bwd(3, 257, 4, 64),    # N = 256 + 1: key-block body + the pre-pass's last key
        lambda: check_attn_bwd(2, 257, 2, 128),
        lambda: check_attn_bwd(1, 40, 2, 80),
        lambda: check_attn_fwd(1, 197, 2, 128),
        lambda: check_attn_bwd(1, 300, 2, 128),
        lambda: check_attn_bwd(1, 100, 2, 96),
        # attention-probability dropout: one key block, N = 197 (the ViT-B path's shape), several key
        # blocks with the dQ accumulator (400 = 256 + 144, 577 = 2 x 256 + 65 tail launch), dh 80
        lambda: check_attn_dropout(3, 197, 4),
        lambda: check_attn_dropout(2, 400, 2),
        lambda: check_attn_dropout(1, 577, 2),
        lambda: check_attn_dropout(2, 257, 2, 80, 0.2),
        lambda: check_attn_dropout(4, 33, 3, 64, 0.5),
        lambda: check_fp8_format(0),
        lambda: check_fp8_format(1),
        lambda: check_fp8_strided(0),
        lambda: check_fp8_strided(1),
        check_fp8_weight_batch,
        lambda: check_wgrad_fp8(1000, 1280, 512),
        lambda: check_wgrad_fp8(32896, 1280, 3840),
        lambda: check_gemm_fp8(3000, 768, 1280),
        lambda: check_gemm_fp8(700, 2304, 768, True, False),
        lambda: check_gemm_fp8(520, 3072, 384, False, True),
        lambda: check_dgrad_fp8(1030, 1280, 768),
        lambda: check_gemm_fp8_producer(1000, 1280, 512),
        check_layernorm_fwd_q8,
        check_fp8_transpose,
        check_attn_fwd_q8,
        lambda: check_attn_fwd_q8(3, 197, 2, 64),  # dh 64, N <= 256: the generic kernel takes the copy
        lambda: check_wgrad_fp8_mn(1000, 1280, 512),
        lambda: check_wgrad_fp8_mn(32896, 1280, 3840),
        lambda: check_wgrad_fp8_mn(300, 768, 256),
        lambda: check_fp8_transpose(257, 768, 0),
        lambda: check_layernorm_fwd_q8(50, 768),
        check_layernorm_bwd_q8,                                   # D 1280 (H/14): five 4-column chunks per lane, (MAXCH, W) = (5, 4)
        check_colsum_q8,
        lambda: check_colsum_q8(1001, 2304),
        lambda: check_layernorm_bwd_q8(2000, 768, linked=True),   # D 768: 4-column chunks + dz
        lambda: check_layernorm_bwd_q8(3000, 1280, linked=True),
        lambda: check_gemm_fp8_producer(1030, 768, 1280, True),
        check_vit_fp8,
        check_vit_fp8_dgrad,
        check_vit_fp8_default_producers,
        check_vit_fp8_wgrad,
        check_vit_fp8_bf16_skip,
        # 257 tokens: the attention backward's lastkey path writes dQKV's e5m2 copy and the in_proj bias
        # partials itself and stores no bf16 dQKV (poisoned here)
        lambda: check_vit_fp8_bf16_skip(steps=4, image=256, images=8),
        check_fp8_nonfinite_recovery,
        lambda: check_xent(8, 1000),
        lambda: check_xent(3, 3),
        check_head,
        lambda: check_head(256, 197, 768, 1000),
        lambda: check_head(37, 5, 192, 1000, frozen_w=True),
        lambda: check_head(5, 3, 1280, 10),
        check_adam,
        check_adam_transposed,
        lambda: check_vit_fused_vs_reference(4, False),
        # generic attention backward in the model (N = 257 > 224, dh 64 and dh 80): the in_proj bias
        # gradient from the dQ and dO column sums (k slice 0)
        lambda: check_vit_fused_vs_reference(2, False, image_size=256),
        lambda: check_vit_fused_vs_reference(2, False, image_size=224, patch_size=14, embedding_dim=320, num_heads=4),
        check_vit_inference,
        check_gemm_patch_embed_epilogue,
        lambda: check_gemm_small_splitk(6304, 768, 3072, resid=True),   # b32: 75 tiles
        lambda: check_gemm_small_splitk(6304, 768, 768, resid=True),
        lambda: check_gemm_small_splitk(2100, 3072, 768, gelu=True),    # 9 x 12 tiles, partial last row tile
        lambda: check_vit_fused_vs_reference(3, True),
        check_block_full_width,
        check_vit_dropout_fused,
        # ViT-H/14-like geometry: patch 14, head dim 80, D = 5 x 64
        lambda: check_vit_fused_vs_reference(2, True, (2e-2, 2e-2, 2e-2, 3e-2), image_size=56, patch_size=14, num_heads=4,
                                             embedding_dim=320, mlp_size=640),
        # round 6 additions go last: the GPU test seeds each check by its index
        lambda: check_attn_fwd_head_qf(4, 197, 12),
        lambda: check_attn_fwd_head_qf(3, 17, 2),
        lambda: check_attn_fwd_head_qf(2, 256, 4),
        # e4m3 gradients (enable_fp8(grad_fmt="e4m3")): every kernel that writes or reads a gradient copy
        lambda: check_attn_bwd_q8(2, 257, 3, 80, fmt=0),
        lambda: check_attn_bwd_q8(2, 577, 2, 64, fmt=0),
        lambda: check_attn_bwd_q8(3, 197, 2, 80, 0.1, fmt=0),
        lambda: check_layernorm_bwd_q8(fmt=0),
        lambda: check_layernorm_bwd_q8(2000, 768, linked=True, fmt=0),
        lambda: check_colsum_q8(1001, 2304, fmt=0),
        lambda: check_wgrad_fp8_mn(1000, 1280, 512, gfmt=0),
        lambda: check_wgrad_fp8_mn(300, 768, 256, gfmt=0),
        lambda: check_wgrad_fp8(1000, 1280, 512, gfmt=0),
        lambda: check_dgrad_fp8(1030, 1280, 768, gfmt=0),
        check_vit_fp8_grad_formats,
        # deterministic mode, multi-key-block shapes without the slab / lastkey paths: ordered dQ slabs
        lambda: check_attn_bwd_det(2, 677, 2),
        lambda: check_attn_bwd_det(2, 677, 3, 64, True),
        lambda: check_attn_bwd_det(1, 400, 2, 80),
        check_vit_fp8_inference,
    ]
    # optimizer kernels on raw buffers against the float64 reference (tests/optim_reference.py)
    big = NORM_TRIP2 + 4 * 100 + 3  # a second trip for the first blocks and a 3-element tail
    for n in (1, 3, 4, 5, 1023, big):
        for mn in (0.0, 1.0, 1e9):  # flag only; a clip that bites once the norm passes 1; one that never does
            c.append(lambda n=n, mn=mn: check_grad_norm(n, mn))
    for n in (5, big):
        for mn in (0.0, 1.0):
            c.append(lambda n=n, mn=mn: check_grad_norm(n, mn, poison=True))
    # norm_rel 7.5e-8 seen at the most (limit 1e-6, derived); coef, flags and the re-run exact.
    # Adam, seen on MI355X as kernel / fp32 torch on the same step (the limit is 4x torch's, per run):
    # the worst step and param group of each metric:
    #   adam_kernel   dp_l2 1.8e-7 / 1.8e-7, m_l2 4.4e-8 / 4.4e-8, v_l2 9.6e-8 / 8.7e-8, dp_max 5.3e-5 / 5.3e-5 at the
    #                 most (coupled decay, g + wd * p cancelling); n = 8: dp_l2 2.7e-6 / 2.7e-6, m_l2 2.0e-8 / 1.9e-8
    #   adam_t_kernel within the same factors of torch (the pytest summary prints each run's values)
    # every flag 0; cast_f32_bf16 bit-equal at every size.
    c += [
        lambda: check_adam_kernel("host", 3),
        lambda: check_adam_kernel("host", 8, clip=True),
        lambda: check_adam_kernel("dev", 3, clip=True, shadow=False),
        lambda: check_adam_kernel("dev", 9),                  # more rows than the kernel arguments hold
        lambda: check_adam_kernel("host", 3, clip=True, tiny=True),  # n = 8, one segment
        lambda: check_adam_kernel("host", 3, clip=True, ema=True),
        lambda: check_adam_t_kernel("host", 3),
        lambda: check_adam_t_kernel("host", 8, clip=True),
        lambda: check_adam_t_kernel("dev", 9, clip=True),
        lambda: check_adam_t_kernel("host", 3, clip=True, ema=True),
    ]
    for n in (1, 2, 3, 5, CAST_TRIP2 + 4 * 50 + 3):
        c.append(lambda n=n: check_cast_f32_bf16(n))
    return c


if __name__ == "__main__":
    torch.manual_seed(0)
    bad = 0
    for fn in all_checks():
        try:
            name, metrics, limits = fn()
            torch.cuda.synchronize()
            ok = passed(metrics, limits)
            bad += not ok
            print(f"{'OK  ' if ok else 'FAIL'} {name:80s} {fmt_metrics(metrics, limits)}", flush=True)
        except Exception as e:  # keep going: report every kernel in one GPU session
            bad += 1
            print(f"ERR  {getattr(fn, '__name__', fn)}: {type(e).__name__}: {e}", flush=True)
            if "HIP error" in str(e) or "hipError" in str(e) or "illegal" in str(e).lower():
                break
    print(f"{bad} failing checks")
    sys.exit(1 if bad else 0)
