"""The row kernels off the Gaussian regime: float64 references, fp32 emulations with the kernels'
rounding points, error figures and input generators for LayerNorm (csrc/layernorm.hip), the classifier
head (csrc/head.hip), the softmax cross-entropy (csrc/xent.hip) and the GELU approximation of
csrc/common.h (``gelu_and_grad`` / ``gelu_and_grad2``).

Nothing here touches the HIP extension, so the module imports (and tests/test_rowwise_reference_cpu.py
runs) without a GPU; every function takes or follows a ``device``. Modelled on tests/attn_reference.py.

* ``ln_ref64``     LayerNorm forward and backward in float64 from the bf16 inputs: y, mean, rstd,
                   dx (with the residual gradient), dz, dgamma, dbeta and the column sums (of dz where
                   there is one, else of dx). Variants: the compact residual gradient (``dres_every``),
                   the linked dropout backward (``keep`` mask passed in, ``p``), the drop-path row scale
                   (``row_scale``, per row, as ``ext.drop_path_scale`` returns it per sample).
* ``ln_emulate``   the same in fp32 torch ops with the kernels' rounding points (see its docstring). It
                   is the yardstick a kernel's error is held against (4 x, the project's convention for
                   "the same operation in the next-best arithmetic"), not a second reference.
* ``head_ref64`` / ``head_emulate``  LayerNorm of the class rows into xhat, the fp32 Linear, and every
                   output of ``head_bwd``.
* ``xent_ref64``   ``xent`` / ``xent_soft`` rows, gradient rows, flags and batch mean in float64 from the
                   fp32 logits; the argmax is the smallest index holding the maximum, written out.
* ``gelu_ref64``   u Phi(u) and Phi(u) + u phi(u) with Phi from erfc in float64.
* ``gelu_formula64`` / ``gelu_emulate``  the formula of ``gelu_and_grad`` with the constants of common.h,
                   in float64 and in fp32 torch ops.
* ``figures``      (global relative L2, worst row error over the mean row norm) of a pair (out, ref).
* ``make_ln`` / ``make_logits`` / ``gelu_grid``  the seeded inputs.
* the ``*_SHAPES`` / ``*_DS`` tables: the cases of tests/test_gpu_rowwise_regimes.py, kept here so the CPU
  test proves the input conditions on exactly those shapes.
"""
from __future__ import annotations

import math
from typing import NamedTuple, Optional, Tuple

import torch

EPS = 1e-5
FLOOR = 2.0 ** -9   # one bf16 half-ulp: the floor of a limit where the emulation is exact
ZERO = 1e-12        # a float64 reference with a mean row norm below this is zero: absolute figures
BF16_MIN_NORMAL = 2.0 ** -126
FP32_MIN_NORMAL = 2.0 ** -126

LN_REGIMES = ("gauss", "offset", "massive", "constant", "tiny", "large", "gamma_edge", "dy_offset", "dy_sparse")
HEAD_REGIMES = ("gauss", "offset", "massive", "constant", "tiny")
LOGIT_REGIMES = ("gauss", "confident", "wrong", "shift_pos", "shift_neg", "uniform", "tie", "masked", "ignore")
SPARSE_EVERY = 5    # dy_sparse: dy is zero on all rows but 0, 5, 10, ...
MASSIVE = 300.0

# ---- the GPU cases (tests/test_gpu_rowwise_regimes.py) ---------------------------------------------
LN_T = 37           # not a multiple of 4: the last workgroup has waves past the end
# forward: MAXCH = ceil(D / 8 / 64) in 1..4, each with a full (D / 8 % 64 == 0) and a partial last chunk
#   D     8  264  512  520  768  1024  1032  1280  1536  1544  2048
#   MAXCH 1   1    1    2    2    2     3     3     3     4     4
LN_FWD_DS = (8, 264, 512, 520, 768, 1024, 1032, 1280, 1536, 1544, 2048)
# backward (MAXCH, W): D 8 (1,8) partial, 256 (1,4), 264 (1,8) partial, 512 (1,8) full, 520 (2,8) partial,
# 768 (3,4), 1024 (2,8) full, 1032 (3,8) partial, 1272 (3,8) partial, 1280 (5,4)
LN_BWD_DS = (8, 256, 264, 512, 520, 768, 1024, 1032, 1272, 1280)
LN_VARIANT_DS = (768, 1032, 1280)
LN_VARIANT_REGIMES = ("gauss", "offset", "constant", "dy_sparse")
LN_STRIDE_REGIMES = ("gauss", "offset")
HEAD_SHAPES = ((5, 3, 16, 10), (37, 5, 192, 1000), (6, 2, 1040, 17), (4, 2, 1536, 257))  # (B, N, D, C)
XENT_SHAPES = ((3, 1), (3, 3), (5, 255), (5, 256), (5, 257), (8, 1000), (2, 21843))      # (B, C)
GELU_PROBE = (300, 512, 256)  # (M, N, K) of the GELU probe GEMM
GELU_TILES = (0, 6, 12, 13, 15)


def ln_bwd_route(D: int) -> Tuple[int, int]:
    """(MAXCH, W) of pvr_layernorm_bwd's dispatch for a row length D."""
    if (D // 4) % 64 == 0 and (D // 8) % 64 != 0 and D // 4 <= 320:
        return {3: 3, 5: 5}.get(D // 256, 1), 4
    return min((D // 8 + 63) // 64, 3), 8


def ln_fwd_route(D: int) -> int:
    return min((D // 8 + 63) // 64, 4)


def drop_factor(p: float) -> float:
    thr = min(int(round(p * 65536)), 65535)
    return 65536.0 / (65536.0 - thr)


def _gen(seed: int) -> torch.Generator:
    g = torch.Generator(device="cpu")
    g.manual_seed(seed)
    return g


def _bf(x: torch.Tensor) -> torch.Tensor:
    return x.to(torch.bfloat16).float()


# ----------------------------------------------------------------------------- figures
def figures(out: torch.Tensor, ref: torch.Tensor) -> Tuple[float, float]:
    """(global relative L2, row figure) of ``out`` against ``ref``. Rows are the rows of a matrix (a
    vector is one row); the row figure is ``max_r |out_r - ref_r| / max(|ref_r|, mean_r |ref_r|)``: an
    error confined to one row counts in full against that row unless the row is small beside the
    average one. With a zero reference (mean row norm below ZERO) both figures are absolute: the
    error's norm, and its largest row norm."""
    o, r = out.double(), ref.double()
    if r.dim() < 2:
        o, r = o.reshape(1, -1), r.reshape(1, -1)
    o, r = o.reshape(r.shape[0], -1), r.reshape(r.shape[0], -1)
    d = o - r
    rows = r.norm(dim=1)
    mean = rows.mean().item() if rows.numel() else 0.0
    dr = d.norm(dim=1)
    if mean < ZERO:
        return d.norm().item(), (dr.max().item() if dr.numel() else 0.0)
    return d.norm().item() / max(r.norm().item(), 1e-300), (dr / rows.clamp_min(mean)).max().item()


# ----------------------------------------------------------------------------- LayerNorm
class LnCase(NamedTuple):
    x: torch.Tensor      # bf16 [T, D]
    dy: torch.Tensor     # bf16 [T, D]
    dres: torch.Tensor   # bf16 [T, D]
    gamma: torch.Tensor  # f32 [D]
    beta: torch.Tensor   # f32 [D]


class LnOut(NamedTuple):
    y: torch.Tensor
    pre: torch.Tensor     # y before its rounding to bf16 (what the e4m3 copy is taken from)
    mean: torch.Tensor
    rstd: torch.Tensor
    xhat: torch.Tensor
    dx: torch.Tensor
    dz: Optional[torch.Tensor]
    dgamma: torch.Tensor
    dbeta: torch.Tensor
    dsum: torch.Tensor    # column sums of dz where there is one, else of dx


def _dres_full(dres: Optional[torch.Tensor], T: int, D: int, every: int, dtype) -> torch.Tensor:
    """The residual gradient on every row: ``dres`` itself, or (``every`` > 1) the compact
    [ceil(T / every), D] tensor scattered to rows 0, every, 2 every, ... and zero elsewhere."""
    if dres is None:
        return torch.zeros(T, D, dtype=dtype)
    if every > 1:
        full = torch.zeros(T, D, dtype=dtype, device=dres.device)
        full[::every] = dres[:(T + every - 1) // every].to(dtype)
        return full
    return dres.to(dtype)


def _dz_factor(T, keep, p, row_scale, dtype, device):
    """The factor dz = f * dx, or None without a dz output: keep mask times the dropout scale, times the
    drop-path scale of the row. In the emulation the two scales are folded into one fp32 number first,
    as the kernel folds them."""
    if keep is None and row_scale is None:
        return None
    s = torch.tensor(drop_factor(p) if keep is not None else 1.0, dtype=dtype, device=device)
    f = s.expand(T, 1)
    if row_scale is not None:
        f = (s * row_scale.to(dtype)).reshape(T, 1)
    if keep is not None:
        f = f * keep.to(dtype)
    return f


def ln_ref64(x, gamma, beta, dy, dres=None, eps=EPS, *, dres_every=0, keep=None, p=0.0, row_scale=None) -> LnOut:
    T, D = x.shape
    x64, g64, b64, dy64 = x.double(), gamma.double(), beta.double(), dy.double()
    mean = x64.mean(-1, keepdim=True)
    var = ((x64 - mean) ** 2).mean(-1, keepdim=True)
    rstd = (var + eps) ** -0.5
    xhat = (x64 - mean) * rstd
    y = xhat * g64 + b64
    g = dy64 * g64
    c1, c2 = g.mean(-1, keepdim=True), (g * xhat).mean(-1, keepdim=True)
    dx = (g - c1 - xhat * c2) * rstd + _dres_full(dres, T, D, dres_every, torch.float64).to(x.device)
    f = _dz_factor(T, keep, p, row_scale, torch.float64, x.device)
    dz = None if f is None else dx * f
    return LnOut(y, y, mean[:, 0], rstd[:, 0], xhat, dx, dz, (dy64 * xhat).sum(0), dy64.sum(0), (dx if dz is None else dz).sum(0))


def ln_emulate(x, gamma, beta, dy, dres=None, eps=EPS, *, dres_every=0, keep=None, p=0.0, row_scale=None) -> LnOut:
    """The kernels' arithmetic in fp32 torch ops. x goes bf16 -> fp32; the mean is an fp32 sum divided by
    D; the variance is two-pass, about that mean; rstd = rsqrt(var + eps); y is rounded to bf16. The
    backward starts from the fp32 mean and rstd, forms g = dy gamma, c1 = sum g / D, c2 = sum g xhat / D
    and o = (g - c1 - xhat c2) rstd + dres, and rounds o to bf16 for dx. dz is the unrounded o times the
    fp32 factor (dropout scale times drop-path row scale, folded first), rounded to bf16. dgamma, dbeta and
    the column sums are fp32 sums; the sums are over the unrounded o (no dz) or the unrounded dz, except
    with a drop-path scale, where they are over the stored bf16 dz (csrc/layernorm.hip says why)."""
    T, D = x.shape
    xf, dyf = x.float(), dy.float()
    mean = xf.sum(-1, keepdim=True) / D
    d = xf - mean
    var = (d * d).sum(-1, keepdim=True) / D
    rstd = torch.rsqrt(var + eps)
    xhat = d * rstd
    pre = xhat * gamma + beta
    g = dyf * gamma
    c1, c2 = g.sum(-1, keepdim=True) / D, (g * xhat).sum(-1, keepdim=True) / D
    o = (g - c1 - xhat * c2) * rstd + _dres_full(dres, T, D, dres_every, torch.float32).to(x.device)
    f = _dz_factor(T, keep, p, row_scale, torch.float32, x.device)
    dz, summed = None, o
    if f is not None:
        summed = o * f
        dz = summed.to(torch.bfloat16)
        if row_scale is not None:
            summed = dz.float()
    return LnOut(pre.to(torch.bfloat16), pre, mean[:, 0], rstd[:, 0], xhat, o.to(torch.bfloat16), dz, (dyf * xhat).sum(0), dyf.sum(0),
                 summed.sum(0))


CONSTANT_VALUES = (0.0, 1.0, -2.5, 48.0, 2.0 ** -10, 300.0, -9984.0, 0.0078125)  # bf16 values, one per row in turn


def massive_columns(D: int) -> Tuple[int, int, int]:
    """The two columns at +-MASSIVE in every row, and the third (+MASSIVE, rows r % 3 == 0)."""
    return 1 % D, (D // 2 + 1) % D, D - 1


def make_ln(regime: str, T: int, D: int, seed: int = 0, device="cpu") -> LnCase:
    """Seeded inputs of one regime (drawn on the CPU, so a CPU and a GPU test see the same bits).

    gauss       x = 2 N(0, 1) + 0.5, gamma = 1 + 0.5 N, beta = 0.1 N, dy, dres ~ N: the inputs of
                kernel_checks.check_layernorm.
    offset      x = +-48 + N(0, 1), sign per row: a mean far above the deviation.
    massive     x ~ N(0, 1) with two fixed columns at +-300 in every row and a third at +300 in every
                third row: a residual stream with outlier channels.
    constant    every element of a row the same bf16 value (CONSTANT_VALUES in turn): var = 0.
    tiny        x = 2^-10 N: var about 1e-6, below eps.
    large       x = 2^20 N.
    gamma_edge  gauss x; gamma exactly 0 on columns 0 mod 7, negative on columns 1 mod 7, and 1e-4
                (a LayerScale-sized entry) on the block [D/2, D/2 + max(1, D/8)).
    dy_offset   gauss x; dy = 8 + N: where dy gamma - c1 cancels.
    dy_sparse   gauss x; dy zero except on rows 0, 5, 10, ...
    """
    if regime not in LN_REGIMES:
        raise ValueError(regime)
    g = _gen(seed * 1000003 + LN_REGIMES.index(regime) * 7919 + T * 131 + D)
    n = torch.randn(T, D, generator=g)
    dy, dres = torch.randn(T, D, generator=g), torch.randn(T, D, generator=g)
    gamma, beta = 1.0 + 0.5 * torch.randn(D, generator=g), 0.1 * torch.randn(D, generator=g)
    x = 2.0 * n + 0.5
    if regime == "offset":
        sign = torch.randint(0, 2, (T, 1), generator=g).float() * 2 - 1
        x = 48.0 * sign + n
    elif regime == "massive":
        x = n.clone()
        c0, c1, c2 = massive_columns(D)
        x[:, c0], x[:, c1] = MASSIVE, -MASSIVE
        x[::3, c2] = MASSIVE
    elif regime == "constant":
        v = torch.tensor([CONSTANT_VALUES[r % len(CONSTANT_VALUES)] for r in range(T)])
        x = v.view(T, 1).expand(T, D).clone()
    elif regime == "tiny":
        x = n * 2.0 ** -10
    elif regime == "large":
        x = n * 2.0 ** 20
    elif regime == "gamma_edge":
        gamma[0::7] = 0.0
        gamma[1::7] = -gamma[1::7].abs()
        gamma[D // 2:D // 2 + max(1, D // 8)] = 1e-4
    elif regime == "dy_offset":
        dy = dy + 8.0
    elif regime == "dy_sparse":
        rows = torch.arange(T) % SPARSE_EVERY != 0
        dy[rows] = 0.0
    bf = lambda t: t.to(torch.bfloat16).to(device)  # noqa: E731
    return LnCase(bf(x), bf(dy), bf(dres), gamma.to(device), beta.to(device))


# ----------------------------------------------------------------------------- classifier head
class HeadCase(NamedTuple):
    tok: torch.Tensor    # bf16 [B * N, D]
    gamma: torch.Tensor  # f32 [D]
    beta: torch.Tensor
    W: torch.Tensor      # f32 [C, D]
    bias: torch.Tensor   # f32 [C]
    dl: torch.Tensor     # f32 [B, C]


class HeadOut(NamedTuple):
    logits: torch.Tensor
    xhat: torch.Tensor
    rstd: torch.Tensor
    dW: torch.Tensor
    db: torch.Tensor
    dgamma: torch.Tensor
    dbeta: torch.Tensor
    dcls: torch.Tensor   # [B, D]: the class rows of dtok


def make_head(regime: str, B: int, N: int, D: int, C: int, seed: int = 0, device="cpu") -> HeadCase:
    """Tokens of an ``make_ln`` regime (its x on B * N rows), the parameters of kernel_checks.check_head."""
    tok = make_ln(regime, B * N, D, seed, device).x
    g = _gen(seed * 1000003 + 17 + B * 131 + C)
    gamma, beta = 1 + 0.1 * torch.randn(D, generator=g), 0.1 * torch.randn(D, generator=g)
    W, bias, dl = 0.05 * torch.randn(C, D, generator=g), torch.randn(C, generator=g), torch.randn(B, C, generator=g)
    return HeadCase(tok, *(t.to(device) for t in (gamma, beta, W, bias, dl)))


def _head(c: HeadCase, B: int, N: int, eps: float, dt, bf16_out: bool) -> HeadOut:
    D = c.tok.shape[1]
    x = c.tok.view(B, N, D)[:, 0].to(dt)
    gamma, beta, W, bias, dl = (t.to(dt) for t in (c.gamma, c.beta, c.W, c.bias, c.dl))
    mean = x.sum(-1, keepdim=True) / D
    d = x - mean
    var = (d * d).sum(-1, keepdim=True) / D
    rstd = torch.rsqrt(var + eps) if dt == torch.float32 else (var + eps) ** -0.5
    xhat = d * rstd
    xc = xhat * gamma + beta
    logits = xc @ W.t() + bias
    dy = dl @ W
    g = dy * gamma
    s1, s2 = g.sum(-1, keepdim=True) / D, (g * xhat).sum(-1, keepdim=True) / D
    dcls = rstd * (g - s1 - xhat * s2)
    if bf16_out:
        dcls = dcls.to(torch.bfloat16)
    return HeadOut(logits, xhat, rstd[:, 0], dl.t() @ xc, dl.sum(0), (dy * xhat).sum(0), dy.sum(0), dcls)


def head_ref64(c: HeadCase, B: int, N: int, eps=EPS) -> HeadOut:
    return _head(c, B, N, eps, torch.float64, False)


def head_emulate(c: HeadCase, B: int, N: int, eps=EPS) -> HeadOut:
    """fp32 torch ops from the bf16 class rows: two-pass statistics, fp32 xhat, the fp32 Linear and the
    fp32 gradients; the class rows of dtok rounded to bf16."""
    return _head(c, B, N, eps, torch.float32, True)


# ----------------------------------------------------------------------------- cross-entropy
class XentOut(NamedTuple):
    loss: torch.Tensor     # f64 [B]: 0 on rows with a label outside [0, C)
    dlogits: torch.Tensor  # f64 [B, C]
    correct: torch.Tensor  # bool [B]: first argmax == ya
    mean: torch.Tensor     # f64 []: sum of the rows / B
    valid: torch.Tensor    # bool [B]


def first_argmax(x: torch.Tensor) -> torch.Tensor:
    """The smallest index holding the row maximum, written out (torch.argmax does not promise it)."""
    C = x.shape[1]
    m = x.amax(1, keepdim=True)
    idx = torch.arange(C, device=x.device).expand_as(x)
    return torch.where(x == m, idx, torch.full_like(idx, C)).amin(1)


def xent_ref64(logits, ya, yb=None, lam=None, eps=0.0, grad_scale=1.0) -> XentOut:
    """Rows of -sum_c q_c log softmax(x)_c with q = (1 - eps)(lam onehot(ya) + (1 - lam) onehot(yb)) + eps / C
    (``xent``: yb = ya, lam = 1, eps = 0) and of (softmax - q) grad_scale, in float64 from the fp32 logits.
    A class at -inf has probability 0; with eps > 0 it makes the row loss +inf, as it is."""
    B, C = logits.shape
    x = logits.double()
    yb = ya if yb is None else yb
    lam = torch.ones(B, dtype=torch.float64, device=x.device) if lam is None else lam.double()
    valid = (ya >= 0) & (ya < C) & (yb >= 0) & (yb < C)
    a, b = ya.clamp(0, C - 1), yb.clamp(0, C - 1)
    lse = torch.logsumexp(x, 1)
    p = torch.exp(x - lse[:, None])
    q = torch.zeros_like(x)
    q.scatter_add_(1, a[:, None], lam[:, None])
    q.scatter_add_(1, b[:, None], 1.0 - lam[:, None])
    q = (1.0 - eps) * q + eps / C
    xa, xb = x.gather(1, a[:, None])[:, 0], x.gather(1, b[:, None])[:, 0]
    hard = torch.where(lam == 0, xb, torch.where(lam == 1, xa, lam * xa + (1.0 - lam) * xb))
    loss = lse - (1.0 - eps) * hard
    if eps > 0:
        loss = loss - (eps / C) * x.sum(1)
    zero = torch.zeros((), dtype=torch.float64, device=x.device)
    loss = torch.where(valid, loss, zero)
    dl = torch.where(valid[:, None], (p - q) * grad_scale, zero)
    return XentOut(loss, dl, first_argmax(logits) == ya, loss.sum() / B, valid)


def xent_roundings(C: int, eps: float = 0.0, soft: bool = False) -> Tuple[int, int]:
    """(k_loss, k_grad): the kernels' roundings, each at most 2^-24 relative, counted at the size they occur.

    The exponential sum has ceil(C / 256) serial adds per thread, 6 wave levels and 3 adds across the
    waves: n_s = ceil(C / 256) + 9 roundings relative to s (every term is positive), which enter log s
    as an absolute error. loss = (m + log s) - x[y]:
      n_s      the sum;
      2        exp of each term that matters (the product with log2 e, v_exp_f32's ulp);
      4        log s = v_log_f32(s) ln 2: two roundings at the size of log s <= |lse| + |m|, each of
               which is at most the scale max(1, max|x|, |loss|) of the bound, hence twice two;
      1        m + log s, at the size of lse;
      1        lse - x[y], at the size of the loss;
      4        the stated margin for __expf and __logf (documented as 1 ulp each on their argument
               range; the margin doubles what was counted for them above).
    xent_soft adds 4 for (1 - eps)(lam x[ya] + (1 - lam) x[yb]), and with eps > 0 the sum of the C logits,
    n_s roundings at the size C max|x| times eps / C, and 2 for eps / C and its product: (n_s + 2) eps.
    The gradient (softmax - q) grad_scale: n_s + 2 for 1 / s, 3 for the exponential (its argument's
    error d 2^-24 log2 e weighs d e^-d <= 0.37), 1 each for the product, the subtraction of q and the
    scale, and the margin 4: every one relative to a probability <= 1."""
    n_s = (C + 255) // 256 + 9
    k_loss = n_s + 2 + 4 + 1 + 1 + 4
    if soft:
        k_loss += 4 + (math.ceil((n_s + 2) * eps) if eps > 0 else 0)
    return k_loss, n_s + 2 + 3 + 3 + 4


class LogitCase(NamedTuple):
    logits: torch.Tensor  # f32 [B, C]
    labels: torch.Tensor  # int64 [B]
    other: torch.Tensor   # int64 [B]: a second label per row (xent_soft's yb), valid wherever labels is
    masked: Optional[torch.Tensor]  # bool [B, C], regime masked only


def make_logits(regime: str, B: int, C: int, seed: int = 0, device="cpu") -> LogitCase:
    """Seeded fp32 logits and int64 labels.

    gauss      3 N(0, 1), as kernel_checks.check_xent.
    confident  the label's logit 30 above the row's largest other.
    wrong      another class 30 above every logit of the row (the label where C = 1).
    shift_pos / shift_neg   +-1e4 + 3 N.
    uniform    all equal (0.75); labels 0, 1, 2, ... mod C.
    tie        (C >= 2) two classes hold the maximum exactly; the label is the higher index of the two on
               even rows, the lower on odd rows. C = 1 has no second class: its one class is the maximum.
    masked     classes c with (c + r) % 3 == 0 at -inf in row r, labels among the rest (C = 1: nothing masked).
    ignore     gauss with labels -100 on rows 0 mod 3 and C on rows 1 mod 3.
    """
    if regime not in LOGIT_REGIMES:
        raise ValueError(regime)
    g = _gen(seed * 1000003 + LOGIT_REGIMES.index(regime) * 7919 + B * 131 + C)
    x = 3.0 * torch.randn(B, C, generator=g)
    y = torch.randint(0, C, (B,), generator=g)
    other = torch.randint(0, C, (B,), generator=g)
    rows = torch.arange(B)
    masked = None
    if regime == "confident":
        x[rows, y] = x.amax(1) + 30.0
    elif regime == "wrong":
        w = (y + 1 + torch.randint(0, max(C - 1, 1), (B,), generator=g)) % C
        x[rows, w] = x.amax(1) + 30.0
    elif regime == "shift_pos":
        x = x + 1e4
    elif regime == "shift_neg":
        x = x - 1e4
    elif regime == "uniform":
        x = torch.full((B, C), 0.75)
        y = rows % C
    elif regime == "tie" and C >= 2:
        lo = torch.randint(0, C - 1, (B,), generator=g)
        hi = lo + 1 + (torch.randint(0, C, (B,), generator=g) % (C - 1 - lo))
        top = x.amax(1) + 1.0
        x[rows, lo], x[rows, hi] = top, top
        y = torch.where(rows % 2 == 0, hi, lo)
    elif regime == "masked" and C >= 2:
        masked = (torch.arange(C).view(1, C) + rows.view(B, 1)) % 3 == 0
        free = (~masked).float()
        y = torch.multinomial(free, 1, generator=g)[:, 0]
        other = torch.multinomial(free, 1, generator=g)[:, 0]
        x = x.masked_fill(masked, -math.inf)
    elif regime == "ignore":
        y = torch.where(rows % 3 == 0, torch.full_like(y, -100), torch.where(rows % 3 == 1, torch.full_like(y, C), y))
    if masked is None and regime == "masked":
        masked = torch.zeros(B, C, dtype=torch.bool)
    return LogitCase(x.to(device), y.to(device), other.to(device), None if masked is None else masked.to(device))


# ----------------------------------------------------------------------------- GELU
# the constants of gelu_and_grad (csrc/common.h), as they stand there (fp32 literals)
GELU_P = 0.23164190
GELU_A = (0.254829592, -0.284496736, 1.421413741, -1.453152027, 1.061405429)
GELU_LOG2E_HALF = 0.72134752044448170
GELU_INV_SQRT_2PI = 0.39894228040143268


def gelu_grid() -> torch.Tensor:
    """The fp32 pre-activation set: +-0, +-2^-100, 4096 points uniform in [-12, 12], every bf16 value in
    [-9, -3], +-40, +-1e4, +-1e30."""
    edge = torch.tensor([0.0, -0.0, 2.0 ** -100, -(2.0 ** -100)], dtype=torch.float32)
    lin = torch.linspace(-12.0, 12.0, 4096, dtype=torch.float64).float()
    bits = torch.arange(0xC040, 0xC110 + 1, dtype=torch.int32) << 16  # bf16 -3.0 .. -9.0
    tail = bits.view(torch.float32)
    far = torch.tensor([40.0, -40.0, 1e4, -1e4, 1e30, -1e30], dtype=torch.float32)
    return torch.cat([edge, lin, tail, far])


def gelu_ref64(u: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(u Phi(u), Phi(u) + u phi(u), Phi(u)) in float64, Phi(u) = erfc(-u / sqrt 2) / 2."""
    u = u.double()
    cdf = 0.5 * torch.special.erfc(-u / math.sqrt(2.0))
    pdf = torch.exp(-0.5 * u * u) / math.sqrt(2.0 * math.pi)
    return u * cdf, cdf + u * pdf, cdf


def _gelu_formula(u: torch.Tensor, dt) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    c = lambda v: torch.tensor(v, dtype=torch.float32).to(dt)  # noqa: E731  (the kernel's fp32 constant, then widened)
    u = u.to(dt)
    au = u.abs()
    e = torch.exp2(c(-GELU_LOG2E_HALF) * u * u)
    if dt == torch.float32:
        # the kernels' exp2 is the bare v_exp_f32, which returns 0 where the result would be an fp32
        # subnormal (|u| > 13.2); torch's exp2 returns the subnormal
        e = torch.where(e < FP32_MIN_NORMAL, torch.zeros_like(e), e)
    t = 1.0 / (c(GELU_P) * au + 1.0)
    poly = t * c(GELU_A[4]) + c(GELU_A[3])
    for a in (GELU_A[2], GELU_A[1], GELU_A[0]):
        poly = t * poly + c(a)
    half = 0.5 * t * poly * e
    cdf = torch.where(u >= 0, 1.0 - half, half)
    return u * cdf, u * c(GELU_INV_SQRT_2PI) * e + cdf, cdf


def gelu_formula64(u: torch.Tensor):
    """``gelu_and_grad`` evaluated in float64: (g, g', Phi). Abramowitz-Stegun 7.1.26 for erfc(|u| / sqrt 2),
    one exp2 and one reciprocal."""
    return _gelu_formula(u, torch.float64)


def gelu_emulate(u: torch.Tensor):
    """The same formula in fp32 torch ops, with the exponential flushed to 0 below the smallest fp32
    normal as the hardware instruction the kernels use flushes it."""
    return _gelu_formula(u.float(), torch.float32)


def gelu_probe_operands(M: int, N: int, K: int, device="cpu"):
    """The "exact operand" GEMM input: x [M, K] bf16 with a single 1.0 per row (x[i, i % K] = 1) and
    w [N, K] bf16 filled from gelu_grid() rounded to bf16, in order, repeated. x . w^T [i, n] is then
    w[n, i % K] in every GEMM kernel, whatever its accumulation order and even where the product is
    rounded to bf16 (tile 15): one product is 1 * w, every other is 0 * w = +-0. (A pre-activation of
    -0 arrives as +0: the accumulator starts at +0 and +0 + -0 = +0.)"""
    x = torch.zeros(M, K)
    r = torch.arange(M)
    x[r, r % K] = 1.0
    grid = gelu_grid().to(torch.bfloat16)
    w = grid.repeat((N * K + grid.numel() - 1) // grid.numel())[:N * K].view(N, K)
    return x.to(torch.bfloat16).to(device), w.contiguous().to(device)


def gelu_probe_product(w: torch.Tensor, M: int) -> torch.Tensor:
    """What x . w^T is for the operands above: [M, N] fp32 with entry (i, n) = w[n, i % K]."""
    K = w.shape[1]
    return w.float().t()[torch.arange(M, device=w.device) % K]
