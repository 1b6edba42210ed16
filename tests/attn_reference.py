"""Attention off the Gaussian regime: a float64 reference, a bf16-staged emulation, error figures,
input generators and a host model of the tiled forward's lazy rescale.

Nothing here touches the HIP extension, so the module imports (and tests/test_attn_reference_cpu.py
runs) without a GPU; every function takes or follows a ``device``.

Layout, as everywhere in the package: ``qkv`` is bf16 ``[B*N, 3*D]`` with head ``h`` of Q, K, V at
columns ``h*dh``, ``D + h*dh``, ``2*D + h*dh``; ``dO`` and ``O`` are ``[B*N, D]``; ``lse`` is
``[B*H, N]`` in nats; a keep mask is ``[B*H, N, N]`` (``kernel_checks.attn_keep_mask``).

* ``ref64``    the operation in float64: O, lse, dQ|dK|dV and the in_proj bias gradient. The algebra of
               ``kernel_checks._attn_ref`` and its autograd, written out.
* ``emulate``  the same operation in fp32 torch ops with the kernels' rounding points: P is rounded to
               bf16 before P.V and before dO^T.P (with dropout after the keep mask and the
               65536 / (65536 - thr) factor), the normaliser is the fp32 sum of the undropped, unrounded
               P, delta = rowsum(dO * bf16(O)), dS is rounded to bf16, O and dQ|dK|dV are rounded to
               bf16. It is the yardstick a kernel's error is held against (4 x, the project's convention
               for "the same operation in the next-best arithmetic"), not a second reference.
* ``figures``  (global relative L2, worst row error) of a pair (out, ref).
* ``make``     the seeded input regimes: gauss, sharp, shift_pos, shift_neg, ramp, uniform, onehot.
* ``lazy_rescale_model``  which (16-query group, key tile) pairs of ``attn_fwd_kernel`` move the running
               max and how large P gets against a stale one, by the rule the kernel documents.
"""
from __future__ import annotations

import math
from typing import NamedTuple, Optional, Tuple

import torch

LOG2E = 1.4426950408889634
LN2 = 0.6931471805599453
REGIMES = ("gauss", "sharp", "shift_pos", "shift_neg", "ramp", "uniform", "onehot")
RAMP_RATE = 7.0 / 64.0  # log2 units per key: a 64-key tile spans 7, under the rescale threshold of 8
RAMP_LAST = 4.0         # key N - 1 (the one that starts the online softmax) lies this far below key 0
FLOOR = 2.0 ** -9       # one bf16 half-ulp: the floor of a limit where the emulation is exact
# A float64 reference whose mean row norm is below this is zero up to its own rounding (onehot dQ and
# dK: the exact value is 0 and float64 leaves about 1e-26); its figures are absolute.
ZERO = 1e-12

# The GPU cases of tests/test_gpu_attn_regimes.py: (path, B, H, N, dh). The smallest shapes that reach
# each route of attn_fwd_launch / attn_bwd_launch / attn_bwd_generic. Kept here so that the CPU test
# proves the input conditions (onehot gaps, ramp branches) on exactly these shapes.
SHAPES = (
    ("head+pipe8", 2, 3, 197, 64), ("head+pipe8", 2, 2, 193, 64), ("head+pipe8", 2, 2, 224, 64),
    ("head+oneblock", 2, 2, 129, 64), ("head+oneblock", 2, 3, 256, 64), ("head+oneblock", 2, 2, 17, 64),
    ("tiled1+lastkey", 2, 2, 257, 64),
    ("tiled1tail+tailsplit", 2, 2, 272, 64),
    ("tiled2+tailsplit", 2, 2, 370, 64), ("tiled2+tailsplit", 2, 3, 577, 64),
    ("dqacc", 2, 2, 400, 64),
    ("dh80kt32+lastkey", 2, 2, 257, 80), ("dh80+oneblock", 2, 2, 197, 80), ("dh80tiled2", 2, 2, 577, 80),
    ("dh96", 2, 2, 100, 96), ("dh128", 2, 2, 300, 128),
)
# With the fused bias gradient N = 257 and 577 keep the lastkey / tail-split routes (the kernels write
# bias partials, attn_bwd_bpart_ok); N = 400 is the shape whose bias gradient goes with the f32 dQ
# accumulator (per-key-block bias rows summed by the host).
DBIAS_SHAPES = (("pipe8+dbias", 2, 2, 197, 64), ("tailsplit+dbias", 2, 2, 577, 64), ("lastkey+dbias", 2, 2, 257, 80),
                ("lastkey+dbias", 2, 2, 257, 64), ("dqacc+dbias", 2, 2, 400, 64))
DROP_SHAPES = (("dropout", 2, 2, 197, 64), ("dropout", 2, 2, 400, 64))
DET_SHAPE = ("detslabs", 2, 2, 400, 64)
HANDOFF_SHAPE = ("handoff", 300, 2, 197, 64)
CLS_SHAPES = (("cls", 2, 3, 197, 64), ("cls", 2, 2, 257, 80), ("cls", 2, 2, 65, 128), ("cls", 2, 2, 33, 96))


class Case(NamedTuple):
    qkv: torch.Tensor              # bf16 [B*N, 3D]
    do: torch.Tensor               # bf16 [B*N, D]
    perm: Optional[torch.Tensor]   # onehot: int64 [B*H, N], query i of a pair attends key perm[i] alone


class Result(NamedTuple):
    o: torch.Tensor      # [B*N, D]
    lse: torch.Tensor    # [B*H, N], nats
    dqkv: torch.Tensor   # [B*N, 3D]
    dbias: torch.Tensor  # [3D]: column sums of dqkv (the in_proj bias gradient)


# ----------------------------------------------------------------------------- layout helpers
def split_heads(qkv: torch.Tensor, B: int, N: int, H: int):
    """[B*N, 3D] -> Q, K, V, each [B, H, N, dh]."""
    dh = qkv.shape[1] // (3 * H)
    q, k, v = qkv.view(B, N, 3, H, dh).permute(2, 0, 3, 1, 4)
    return q, k, v


def heads(x: torch.Tensor, B: int, N: int, H: int) -> torch.Tensor:
    """[B*N, D] -> [B, H, N, dh]."""
    return x.view(B, N, H, x.shape[1] // H).permute(0, 2, 1, 3)


def merge_heads(x: torch.Tensor) -> torch.Tensor:
    """[B, H, N, dh] -> [B*N, D]."""
    B, H, N, dh = x.shape
    return x.permute(0, 2, 1, 3).reshape(B * N, H * dh)


def pack_qkv(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor) -> torch.Tensor:
    """Q, K, V [B, H, N, dh] -> [B*N, 3D]."""
    return torch.cat([merge_heads(q), merge_heads(k), merge_heads(v)], 1).contiguous()


def drop_factor(p: float) -> float:
    thr = min(int(round(p * 65536)), 65535)
    return 65536.0 / (65536.0 - thr)


def scores64(qkv: torch.Tensor, B: int, N: int, H: int) -> torch.Tensor:
    """Scaled scores in nats, float64 [B*H, N, N]."""
    q, k, _ = split_heads(qkv.double(), B, N, H)
    return ((q @ k.transpose(-1, -2)) / math.sqrt(q.shape[-1])).reshape(B * H, N, N)


# ----------------------------------------------------------------------------- float64 reference
def ref64(qkv, do, B, N, H, keep=None, p=0.0) -> Result:
    q, k, v = split_heads(qkv.double(), B, N, H)
    g = heads(do.double(), B, N, H)
    scale = 1.0 / math.sqrt(q.shape[-1])
    s = (q @ k.transpose(-1, -2)) * scale
    lse = torch.logsumexp(s, -1)
    pr = torch.exp(s - lse[..., None])
    f = None
    if keep is not None:
        f = keep.view(B, H, N, N).double() * drop_factor(p)
    pd = pr if f is None else pr * f
    o = pd @ v
    dv = pd.transpose(-1, -2) @ g
    dp = g @ v.transpose(-1, -2)
    if f is not None:
        dp = dp * f
    ds = pr * (dp - (pr * dp).sum(-1, keepdim=True))
    dq = (ds @ k) * scale
    dk = (ds.transpose(-1, -2) @ q) * scale
    dqkv = pack_qkv(dq, dk, dv)
    return Result(merge_heads(o), lse.reshape(B * H, N), dqkv, dqkv.sum(0))


# ----------------------------------------------------------------------------- bf16-staged emulation
def _bf(x: torch.Tensor) -> torch.Tensor:
    return x.to(torch.bfloat16).float()


def emulate(qkv, do, B, N, H, keep=None, p=0.0) -> Result:
    q, k, v = split_heads(qkv.float(), B, N, H)
    g = heads(do.float(), B, N, H)
    scale = 1.0 / math.sqrt(q.shape[-1])
    t = (q @ k.transpose(-1, -2)) * (scale * LOG2E)  # scores in scaled log2 units
    m = t.amax(-1, keepdim=True)
    pu = torch.exp2(t - m)
    l = pu.sum(-1, keepdim=True)  # the normaliser: undropped, unrounded
    f = None
    if keep is not None:
        f = keep.view(B, H, N, N).float() * drop_factor(p)
    o = ((_bf(pu if f is None else pu * f) @ v) / l).to(torch.bfloat16)
    lse = (m + torch.log2(l)) * LN2
    # backward, from the forward's own bf16 O and fp32 lse
    pr = torch.exp2(t - lse * LOG2E)
    pd = _bf(pr if f is None else pr * f)
    dv = pd.transpose(-1, -2) @ g
    dp = g @ v.transpose(-1, -2)
    if f is not None:
        dp = dp * f
    delta = (g * o.float()).sum(-1, keepdim=True)
    ds = _bf(pr * (dp - delta))
    dq = (ds @ k) * scale
    dk = (ds.transpose(-1, -2) @ q) * scale
    dqkv = pack_qkv(dq, dk, dv)
    # the bias gradient as the kernels form it: fp32 column sums of the unrounded dQ, no k part (the
    # rows of dS sum to zero), column sums of dO for v (the rows of P sum to one; not with dropout)
    D = dq.shape[1] * dq.shape[3]
    dbias = dqkv.sum(0)
    if f is None:
        dbias = torch.cat([dbias[:D], torch.zeros_like(dbias[:D]), do.float().sum(0)])
    return Result(merge_heads(o.float()).to(torch.bfloat16), lse.reshape(B * H, N), dqkv.to(torch.bfloat16), dbias)


# ----------------------------------------------------------------------------- figures
def figures(out: torch.Tensor, ref: torch.Tensor, dh: int) -> Tuple[float, float]:
    """(global relative L2, row figure) of ``out`` against ``ref``. Rows are token rows of one head
    slice (``dh`` consecutive columns); the row figure is
    ``max_r |out_r - ref_r| / max(|ref_r|, mean_r |ref_r|)``: an error confined to one row counts in
    full against that row unless the row is small beside the average one. With a zero
    reference (mean row norm below ZERO) both figures are absolute: the error's norm, and its largest
    row norm."""
    o, r = out.double().reshape(-1, dh), ref.double().reshape(-1, dh)
    d = o - r
    l2 = d.norm().item() / max(r.norm().item(), 1e-300)
    rows = r.norm(dim=1)
    mean = rows.mean().item() if rows.numel() else 0.0
    dr = d.norm(dim=1)
    if mean < ZERO:
        return d.norm().item(), (dr.max().item() if dr.numel() else 0.0)
    return l2, (dr / rows.clamp_min(mean)).max().item()


# ----------------------------------------------------------------------------- input regimes
def _gen(seed: int) -> torch.Generator:
    g = torch.Generator(device="cpu")
    g.manual_seed(seed)
    return g


def make(regime: str, B: int, N: int, H: int, dh: int, seed: int = 0, device="cpu") -> Case:
    """Seeded inputs of one regime (drawn on the CPU, so a CPU and a GPU test see the same bits).

    gauss      Q, K, V ~ N(0, 1): the inputs of every check in kernel_checks.
    sharp      Q, K ~ 3 N(0, 1): peaked rows, scores to about 39 nat at dh 64.
    shift_pos  Q + 4, K + 4 before the bf16 rounding: every score near +16 sqrt(dh) nat.
    shift_neg  Q - 4, K + 4: every score near -16 sqrt(dh) nat.
    ramp       Q_i = u + 0.3 noise, K_j = t_j u + 0.3 noise for a +-1 direction u per (batch, head):
               scores rise by RAMP_RATE log2 units per key over j < N - 1, key N - 1 lies RAMP_LAST below
               key 0.
    uniform    Q = 0.
    onehot     K: N distinct rows of +-4 per (batch, head); Q_i = K_perm[i]; ``perm`` is returned.
    """
    if regime not in REGIMES:
        raise ValueError(regime)
    g = _gen(seed * 1000003 + REGIMES.index(regime) * 7919 + N * 131 + dh)
    shp = (B, H, N, dh)
    q, k = torch.randn(shp, generator=g), torch.randn(shp, generator=g)
    v, do = torch.randn(shp, generator=g), torch.randn(B * N, H * dh, generator=g)
    perm = None
    if regime == "sharp":
        q, k = 3.0 * q, 3.0 * k
    elif regime == "shift_pos":
        q, k = q + 4.0, k + 4.0
    elif regime == "shift_neg":
        q, k = q - 4.0, k + 4.0
    elif regime == "ramp":
        u = torch.randint(0, 2, (B, H, 1, dh), generator=g).float() * 2 - 1
        kappa = math.sqrt(dh) * LOG2E  # log2 units of score per unit of t (|u|^2 = dh, scale = dh^-1/2)
        j = torch.arange(N, dtype=torch.float32)
        t = (RAMP_LAST + RAMP_RATE * j) / kappa
        t[N - 1] = 0.0
        q = u + 0.3 * q
        k = t.view(1, 1, N, 1) * u + 0.3 * k
    elif regime == "uniform":
        q = torch.zeros(shp)
    elif regime == "onehot":
        k = torch.randint(0, 2, shp, generator=g).float() * 8 - 4
        perm = torch.stack([torch.randperm(N, generator=_gen(seed * 7 + 11 + 31 * bh)) for bh in range(B * H)])
        q = torch.gather(k, 2, perm.view(B, H, N, 1).expand(shp))
        # an exact zero in V or dO (randn yields one about every 10^7 draws) has nothing to absorb the
        # other keys' P <= exp(-gap): O = V[perm] and dV = dO[perm^-1] bit for bit need non-zero entries
        v, do = v.bfloat16().float(), do.bfloat16().float()
        v[v == 0] = 1.0
        do[do == 0] = 1.0
    qkv = pack_qkv(q, k, v).to(torch.bfloat16).to(device)
    return Case(qkv, do.to(torch.bfloat16).to(device), None if perm is None else perm.to(device))


def gather_rows(x: torch.Tensor, idx: torch.Tensor, B: int, N: int, H: int) -> torch.Tensor:
    """x [B*N, D], idx [B*H, N] -> y with y[b, i, head h] = x[b, idx[b*H + h, i], head h]."""
    xh = heads(x, B, N, H)
    return merge_heads(torch.gather(xh, 2, idx.view(B, H, N, 1).expand(xh.shape)))


def inverse_perm(perm: torch.Tensor) -> torch.Tensor:
    inv = torch.empty_like(perm)
    ar = torch.arange(perm.shape[1], device=perm.device).expand_as(perm)
    inv.scatter_(1, perm, ar)
    return inv


def row_stats(qkv, B, N, H):
    """Per query row of the float64 softmax: (top probability, gap in nats from the best to the second
    best key, largest |score| in nats), each [B*H, N]."""
    s = scores64(qkv, B, N, H)
    top2 = s.topk(min(2, N), -1).values
    gap = top2[..., 0] - top2[..., -1]
    return torch.softmax(s, -1).amax(-1), gap, s.abs().amax(-1)


# ----------------------------------------------------------------------------- lazy-rescale rule
def lazy_rescale_model(qkv, B, N, H, KT):
    """The documented rule of ``attn_fwd_kernel``: per 16-query group and per tile of KT keys over the
    keys j < N - 1, each query's running max (scaled log2 units) starts at the score of key N - 1; a
    (group, tile) pair grows - every query's max becomes max(old, its tile max) - iff some query of
    the group has tile_max > m_run + 8, otherwise P = 2^(score - m_run) is taken against the stale
    max. Queries past N repeat row N - 1, as the kernel clamps them.

    Returns ``(grew, stale_log2p)``, both [B*H, groups, tiles]: whether the pair grew, and log2 of the
    largest P taken against a stale max (-inf where it grew)."""
    s2 = scores64(qkv, B, N, H) * LOG2E
    G = (N + 15) // 16
    idx = torch.arange(G * 16, device=s2.device).clamp_max(N - 1)
    s2 = s2[:, idx].view(-1, G, 16, N)
    m_run = s2[..., N - 1].clone()  # [BH, G, 16]
    NL = N - 1
    T = (NL + KT - 1) // KT
    grew = torch.zeros(s2.shape[0], G, T, dtype=torch.bool, device=s2.device)
    stale = torch.full((s2.shape[0], G, T), -math.inf, dtype=torch.float64, device=s2.device)
    for t in range(T):
        tmax = s2[..., t * KT:min((t + 1) * KT, NL)].amax(-1)
        over = tmax - m_run
        gr = (over > 8.0).any(-1)
        grew[:, :, t] = gr
        stale[:, :, t] = torch.where(gr, stale[:, :, t], over.amax(-1))
        m_run = torch.where(gr[..., None], torch.maximum(m_run, tmax), m_run)
    return grew, stale
