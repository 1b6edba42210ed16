"""Colour augmentation of a raw ``uint8 [B, 3, Hs, Ws]`` batch on the device: DeiT-III's 3-Augment (one of
grayscale, solarize or Gaussian blur per image) and the brightness / contrast / saturation jitter of
``ColorJitter`` (DeiT, SimCLR, DINO, MAE).

PIL on uint8 defines the pointwise ops, because PIL is what the recipes run; every op maps a uint8 image to
a uint8 image. With ``L(r, g, b) = (19595 r + 38470 g + 7471 b + 32768) >> 16`` in integers and
``blend(d, v, f) = uint8(trunc(min(max(d + f * (v - d), 0), 255)))`` in fp32 with every operation rounded on
its own (``f = 1`` gives ``v`` and ``f = 0`` gives ``d`` exactly), a :class:`ColorPlan` gives each sample

* an ``op``: 0 none; 1 grayscale (every channel becomes ``L``); 2 solarize (``v < 128 ? v : 255 - v``);
  3 Gaussian blur with the sample's ``sigma`` in ``(0, 2]``. The blur is this project's own definition, not
  PIL's three-pass box approximation: ``R = min(6, max(1, ceil(3 sigma)))``, ``w[k] = exp(-k^2 / (2 sigma^2))``
  for ``|k| <= R`` and 0 otherwise, normalised to sum 1 in float64 and rounded once to fp32 (13 taps); a
  horizontal pass ``t = 0; for i in 0..12: t = t + w[i] * float(p[y][clamp(x + i - 6)])``, the same loop down the
  fp32 rows with the row index clamped (edge pixels are replicated), and ``uint8(min(max(floor(o + 0.5), 0), 255))``;
* then the jitter with factors ``(fb, fc, fs) >= 0`` in the sample's ``order``, an index into the
  permutations ``bcs, bsc, cbs, csb, sbc, scb``; each step's uint8 output feeds the next step:
  brightness ``blend(0, v, fb)``, saturation ``blend(L(pixel), v, fs)``, contrast ``blend(m, v, fc)`` with
  ``m = (2 S + n) // (2 n)``, ``S`` the sum of ``L`` over the ``n = Hs * Ws`` pixels of the image as it is when
  contrast runs (PIL's ``int(mean + 0.5)``).

No hue; the solarize threshold is 128; three channels only; ``Hs * Ws <= 2^24``.

The stage runs on the source batch, BEFORE the crop of ``data/device_input.py`` (the recipes run it after the
crop, at model size): pointwise ops then differ only by where the uint8 rounding falls, but contrast's mean
is taken over the whole source instead of the crop and ``sigma`` is in source pixels. Without a crop (source
size equal to model size) the order is the recipes'.

On the fused GPU path three kernels of ``csrc/color.hip`` write a new uint8 batch of the same layout, which
the patch-embedding kernel reads like the loader's (``ops.fused_vit.color_u8``). Elsewhere (CPU,
``PVR_DISABLE_FUSED=1``) :func:`color_reference` runs the same formulas as torch ops, byte for byte.
"""
from __future__ import annotations

import math
from typing import Dict, Optional, Sequence, Tuple, Union

import torch
import torch.nn.functional as F

NONE, GRAYSCALE, SOLARIZE, BLUR = 0, 1, 2, 3
ORDERS = ("bcs", "bsc", "cbs", "csb", "sbc", "scb")  # lexicographic permutations of (brightness, contrast, saturation)
TAPS = 13
SIGMA_MAX = 2.0
MAX_PIXELS = 1 << 24
ROW_WORDS = 20  # csrc/kernels.h ColorRow: op, order (int32 bits), fb, fc, fs, sigma, w[13], pad


def blur_weights(sigma: float) -> torch.Tensor:
    """The 13 fp32 taps of the module docstring for one ``sigma`` in ``(0, 2]``."""
    sigma = float(sigma)
    if not 0.0 < sigma <= SIGMA_MAX:
        raise ValueError(f"blur sigma must be in (0, {SIGMA_MAX}], got {sigma}")
    R = min(TAPS // 2, max(1, math.ceil(3.0 * sigma)))
    k = torch.arange(-(TAPS // 2), TAPS // 2 + 1, dtype=torch.float64)
    w = torch.where(k.abs() <= R, torch.exp(-(k * k) / (2.0 * sigma * sigma)), torch.zeros_like(k))
    return (w / w.sum()).to(torch.float32)


class ColorPlan:
    """A batch's colour plan (see the module docstring). Host tensors: ``op`` int32 ``[B]``, ``sigma`` float32
    ``[B]`` (read for ``op == 3`` only; ``None``: 1.0), ``factors`` float32 ``[B, 3]`` rows ``(fb, fc, fs)``
    (``None``: 1), ``order`` int32 ``[B]`` (``None``: 0), ``weights`` float32 ``[B, 13]`` (the identity tap for
    samples that are not blurred). ``rows`` is the kernels' table (``csrc/kernels.h`` ``ColorRow``), in pinned
    memory when a GPU is present. :meth:`on` uploads it (non-blocking, once per device)."""

    def __init__(self, op, sigma=None, factors=None, order=None):
        op = torch.as_tensor(op, dtype=torch.int32).reshape(-1).cpu().contiguous()
        B = op.shape[0]
        sigma = torch.ones(B) if sigma is None else sigma
        sigma = torch.as_tensor(sigma, dtype=torch.float32).reshape(-1).cpu().contiguous()
        factors = torch.ones(B, 3) if factors is None else factors
        factors = torch.as_tensor(factors, dtype=torch.float32).reshape(-1, 3).cpu().contiguous()
        order = torch.zeros(B, dtype=torch.int32) if order is None else order
        order = torch.as_tensor(order, dtype=torch.int32).reshape(-1).cpu().contiguous()
        if not (sigma.shape[0] == B and factors.shape[0] == B and order.shape[0] == B):
            raise ValueError(f"ColorPlan: op, sigma, factors and order must agree on the batch size, got {B}, "
                             f"{sigma.shape[0]}, {factors.shape[0]}, {order.shape[0]}")
        if B and not bool(((op >= NONE) & (op <= BLUR)).all()):
            raise ValueError("ColorPlan: op must be 0 (none), 1 (grayscale), 2 (solarize) or 3 (blur)")
        if B and not bool(((order >= 0) & (order < len(ORDERS))).all()):
            raise ValueError(f"ColorPlan: order must index {ORDERS}")
        if B and not bool((torch.isfinite(factors) & (factors >= 0)).all()):
            raise ValueError("ColorPlan: jitter factors must be finite and >= 0")
        weights = torch.zeros(B, TAPS, dtype=torch.float32)
        weights[:, TAPS // 2] = 1.0
        for b in (op == BLUR).nonzero().flatten().tolist():
            s = float(sigma[b])
            if not 0.0 < s <= SIGMA_MAX:  # NaN included
                raise ValueError(f"ColorPlan: sample {b} has blur sigma {s} outside (0, {SIGMA_MAX}]")
            weights[b] = blur_weights(s)
        self.op, self.sigma, self.factors, self.order, self.weights = op, sigma, factors, order, weights
        rows = torch.zeros(B, ROW_WORDS, dtype=torch.float32)
        bits = rows.view(torch.int32)
        bits[:, 0], bits[:, 1] = op, order
        rows[:, 2:5], rows[:, 5], rows[:, 6:6 + TAPS] = factors, sigma, weights
        self.rows = rows.pin_memory() if torch.cuda.is_available() else rows
        self._on: Dict[torch.device, torch.Tensor] = {}

    @property
    def batch(self) -> int:
        return self.op.shape[0]

    @classmethod
    def none(cls, batch: int) -> "ColorPlan":
        """The identity plan: op 0 and factors 1."""
        return cls(torch.zeros(batch, dtype=torch.int32))

    def on(self, device) -> torch.Tensor:
        """The table on ``device``."""
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        t = self._on.get(device)
        if t is None:
            if device.type == "cpu":
                t = self.rows
            else:
                with torch.inference_mode(False):  # kept across calls: not an inference tensor
                    t = self.rows.to(device, non_blocking=True)
            self._on[device] = t
        return t

    def check(self, batch: int) -> None:
        if self.batch != batch:
            raise ValueError(f"ColorPlan for {self.batch} samples applied to {batch} samples")

    def __repr__(self):
        n = [int((self.op == k).sum()) for k in range(4)]
        return f"ColorPlan(batch={self.batch}, none={n[0]}, grayscale={n[1]}, solarize={n[2]}, blur={n[3]})"


def _check_batch(x: torch.Tensor, what: str) -> None:
    if x.dtype != torch.uint8 or x.dim() != 4:
        raise ValueError(f"{what}: expected a uint8 [B, 3, Hs, Ws] batch, got {x.dtype} {tuple(x.shape)}")
    if x.shape[1] != 3:
        raise ValueError(f"{what}: colour augmentation takes 3 channels, got {x.shape[1]}")
    if x.shape[2] * x.shape[3] > MAX_PIXELS or x.shape[2] * x.shape[3] == 0:
        raise ValueError(f"{what}: a source of {x.shape[2]}x{x.shape[3]} pixels is outside 1 .. 2^24")


def _luma(x: torch.Tensor) -> torch.Tensor:
    """``L`` of an integer ``[B, 3, H, W]`` image: int32 ``[B, 1, H, W]``."""
    x = x.to(torch.int32)
    return (19595 * x[:, 0:1] + 38470 * x[:, 1:2] + 7471 * x[:, 2:3] + 32768) >> 16


def _blend(d: torch.Tensor, v: torch.Tensor, f: torch.Tensor) -> torch.Tensor:
    """``blend(d, v, f)`` of the module docstring: one torch op, hence one rounding, per operation."""
    v = v.to(torch.float32)
    t = v - d
    t = f * t
    t = d + t
    return t.clamp(0.0, 255.0).to(torch.uint8)


def _blur(x: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """The blur of a uint8 ``[n, 3, H, W]`` batch with fp32 taps ``w`` ``[n, 13]``: the explicit loops over
    shifted slices of the edge-padded image, multiply and add as separate ops."""
    H, W = x.shape[2], x.shape[3]
    R = TAPS // 2
    w = w.view(-1, TAPS, 1, 1, 1)
    p = F.pad(x.to(torch.float32), (R, R, 0, 0), mode="replicate")
    t = torch.zeros_like(p[..., :W])
    for i in range(TAPS):
        t = t + w[:, i] * p[..., i:i + W]
    p = F.pad(t, (0, 0, R, R), mode="replicate")
    o = torch.zeros_like(t)
    for i in range(TAPS):
        o = o + w[:, i] * p[..., i:i + H, :]
    return torch.floor(o + 0.5).clamp(0.0, 255.0).to(torch.uint8)


def color_reference(x: torch.Tensor, plan: ColorPlan) -> torch.Tensor:
    """The colour stage as plain torch ops on a uint8 ``[B, 3, Hs, Ws]`` batch on any device; returns a new
    uint8 batch. What the models run on the CPU or with ``PVR_DISABLE_FUSED=1``, and what the GPU tests
    compare the kernels against, byte for byte."""
    _check_batch(x, "color_reference")
    B, _, H, W = x.shape
    plan.check(B)
    dev = x.device

    def per_sample(t, dtype=None):
        return t.to(device=dev, dtype=dtype or t.dtype).view(B, 1, 1, 1)

    op = per_sample(plan.op)
    gray = _luma(x).to(torch.uint8).expand(B, 3, H, W)
    img = torch.where(op == GRAYSCALE, gray, x)
    img = torch.where(op == SOLARIZE, torch.where(x < 128, x, 255 - x), img)
    idx = (plan.op == BLUR).nonzero().flatten()
    if idx.numel():
        at = idx.to(dev)
        img = img.index_copy(0, at, _blur(x.index_select(0, at), plan.weights[idx].to(dev)))
    fb, fc, fs = (per_sample(plan.factors[:, k]) for k in range(3))
    zero = torch.zeros((), dtype=torch.float32, device=dev)
    n = H * W
    for k in range(3):
        step = per_sample(torch.tensor([ord(ORDERS[o][k]) for o in plan.order.tolist()], dtype=torch.int32))  # sample's k-th step
        lum = _luma(img)
        S = lum.sum(dim=(1, 2, 3), dtype=torch.int64)
        m = torch.div(2 * S + n, 2 * n, rounding_mode="floor").to(torch.float32).view(B, 1, 1, 1)
        bright = _blend(zero, img, fb)
        contrast = _blend(m, img, fc)
        satur = _blend(lum.to(torch.float32), img, fs)
        img = torch.where(step == ord("b"), bright, torch.where(step == ord("c"), contrast, satur))
    return img


def _pair(v, name: str) -> Optional[Tuple[float, float, float]]:
    if v is None:
        return None
    v = (float(v),) * 3 if isinstance(v, (int, float)) else tuple(float(a) for a in v)
    if len(v) != 3 or not all(math.isfinite(a) and a >= 0.0 for a in v):
        raise ValueError(f"ColorAugment: {name} must be one non-negative float or three (brightness, contrast, saturation), got {v}")
    return v


class ColorAugment:
    """Sampler of :class:`ColorPlan` s. ``three_augment``: with probability ``prob`` a sample gets one of
    grayscale, solarize or blur (uniformly), the blur's ``sigma`` uniform in ``sigma``; otherwise op 0.
    ``jitter`` = ``(vb, vc, vs)`` (or one value for all three; ``None``: factors of 1): each factor is uniform in
    ``[max(0, 1 - v), 1 + v]``, and the steps' order is uniform over the six permutations.

    All draws are float64, on the host, from ``generator`` (the global CPU generator when ``None``): one
    ``[B, 7]`` tensor per call whatever the settings and decisions, so the stream of draws does not depend on
    them. The generator's state is not part of any checkpoint."""

    DRAWS = 7  # apply, op, sigma, fb, fc, fs, order

    def __init__(self, three_augment: bool = True, jitter: Union[None, float, Sequence[float]] = (0.3, 0.3, 0.3),
                 sigma: Tuple[float, float] = (0.1, 2.0), prob: float = 1.0, generator: Optional[torch.Generator] = None):
        if not 0.0 <= prob <= 1.0:
            raise ValueError(f"ColorAugment: prob must be in [0, 1], got {prob}")
        if not 0.0 < sigma[0] <= sigma[1] <= SIGMA_MAX:
            raise ValueError(f"ColorAugment: sigma must be a range inside (0, {SIGMA_MAX}], got {sigma}")
        self.three_augment, self.jitter = bool(three_augment), _pair(jitter, "jitter")
        self.sigma, self.prob, self.generator = (float(sigma[0]), float(sigma[1])), float(prob), generator

    def sample(self, batch: int) -> ColorPlan:
        if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("ColorAugment draws its plan on the host every step: it cannot run inside a graph capture (a "
                               "replay would reuse one draw); pass an explicit ColorPlan or train without a graph")
        B = int(batch)
        u = torch.rand(B, self.DRAWS, generator=self.generator, dtype=torch.float64)
        op = torch.zeros(B, dtype=torch.int32)
        if self.three_augment:
            pick = (1 + (u[:, 1] * 3).long().clamp(max=2)).to(torch.int32)
            op = torch.where(u[:, 0] < self.prob, pick, op)
        sigma = (self.sigma[0] + u[:, 2] * (self.sigma[1] - self.sigma[0])).clamp(self.sigma[0], self.sigma[1])
        factors = torch.ones(B, 3, dtype=torch.float64)
        if self.jitter is not None:
            lo = torch.tensor([max(0.0, 1.0 - v) for v in self.jitter], dtype=torch.float64)
            hi = torch.tensor([1.0 + v for v in self.jitter], dtype=torch.float64)
            factors = lo + u[:, 3:6] * (hi - lo)
        order = (u[:, 6] * len(ORDERS)).long().clamp(max=len(ORDERS) - 1).to(torch.int32)
        return ColorPlan(op, sigma.to(torch.float32).clamp(max=SIGMA_MAX), factors.to(torch.float32), order)

    def __repr__(self):
        return f"ColorAugment(three_augment={self.three_augment}, jitter={self.jitter}, sigma={self.sigma}, prob={self.prob})"
