"""Random erasing (Zhong et al. 2017; the DeiT recipe trains with probability 0.25 in "pixel" mode) for a
batch on the device.

An :class:`ErasePlan` gives every sample ``s`` one half-open box ``(ex0, ey0, ex1, ey1)`` in model-image
pixels; an empty box means the sample is not erased. With ``pre(s, c, y, x)`` the fp32 pixel of sample
``s`` as the model sees it (after normalisation and the sample's own crop box on the uint8 path)::

    pre'(s, c, y, x) = fill(s, c, y, x)   if ex0[s] <= x < ex1[s] and ey0[s] <= y < ey1[s]
                       pre(s, c, y, x)    otherwise

and a batch mix (``data/batch_mix.py``) then runs on ``pre'``: erase per sample, then mix the batch, the
order of the usual recipe, so a partner's pixels come from the partner's own erased image. Labels are
untouched. ``fill`` is ``value[c]`` (mode ``"const"``; 0 is the mean colour after normalisation) or a standard
normal per element (mode ``"pixel"``).

On the fused GPU path the patch-embedding kernels do this while they gather the patch rows
(``csrc/patchify.hip``, ``ERASE`` variants): an erased pixel is not loaded, and the normal comes from the
counter hash of the dropout masks at site ``ERASE_SITE`` (``ext.erase_noise`` returns the same values).
Elsewhere (CPU, ``PVR_DISABLE_FUSED=1``) :func:`erase_reference` runs the formula as torch ops and draws
the normal from torch's RNG.
"""
from __future__ import annotations

import math
from typing import Dict, Optional, Sequence, Tuple, Union

import torch

MODES = ("pixel", "const")


class ErasePlan:
    """A batch's erase plan (see the module docstring). Host tensors: ``box`` int32 ``[B, 4]`` rows
    ``(x0, y0, x1, y1)`` (one row is repeated for the batch), ``size`` = ``(H, W)``, ``mode`` and ``value`` (a
    float, or one per channel, for ``"const"``). ``rows`` is the kernels' table (``csrc/kernels.h`` ``EraseRow``):
    the boxes, in pinned memory when a GPU is present. :meth:`on` uploads it (non-blocking, once per device)."""

    def __init__(self, box, size: Tuple[int, int], mode: str = "pixel", value: Union[float, Sequence[float]] = 0.0):
        H, W = int(size[0]), int(size[1])
        box = torch.as_tensor(box, dtype=torch.int32).reshape(-1, 4).cpu().contiguous()
        if mode not in MODES:
            raise ValueError(f"ErasePlan: mode must be one of {MODES}, got {mode!r}")
        if H <= 0 or W <= 0:
            raise ValueError(f"ErasePlan: bad size {size}")
        x0, y0, x1, y1 = box.unbind(1)
        if box.shape[0] and not bool(((x0 >= 0) & (x0 <= x1) & (x1 <= W) & (y0 >= 0) & (y0 <= y1) & (y1 <= H)).all()):
            raise ValueError(f"ErasePlan: boxes must be half-open (x0, y0, x1, y1) inside the {H}x{W} image")
        value = [float(value)] if isinstance(value, (int, float)) else [float(v) for v in value]
        if not 1 <= len(value) <= 4 or not all(math.isfinite(v) for v in value):
            raise ValueError(f"ErasePlan: value must be one finite float or one per channel (at most 4), got {value}")
        self.box, self.size, self.mode, self.value = box, (H, W), mode, tuple(value)
        self.rows = box.pin_memory() if torch.cuda.is_available() else box
        self._on: Dict[torch.device, torch.Tensor] = {}

    @property
    def batch(self) -> int:
        return self.box.shape[0]

    @property
    def erased(self) -> torch.Tensor:
        """bool ``[B]``: the samples whose box is not empty."""
        return (self.box[:, 2] > self.box[:, 0]) & (self.box[:, 3] > self.box[:, 1])

    @classmethod
    def none(cls, batch: int, size: Tuple[int, int], mode: str = "pixel", value=0.0) -> "ErasePlan":
        return cls(torch.zeros(batch, 4, dtype=torch.int32), size, mode, value)

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

    def check(self, batch: int, size: Tuple[int, int]) -> None:
        if self.batch != batch or self.size != (int(size[0]), int(size[1])):
            raise ValueError(f"ErasePlan for {self.batch} samples of {self.size[0]}x{self.size[1]} applied to {batch} samples of "
                             f"{size[0]}x{size[1]}")

    def channel_values(self, channels: int) -> Tuple[float, ...]:
        """``value`` as one float per channel."""
        if len(self.value) not in (1, channels):
            raise ValueError(f"ErasePlan: {len(self.value)} fill values for {channels} channels")
        return self.value * channels if len(self.value) == 1 else self.value

    def __repr__(self):
        return f"ErasePlan(batch={self.batch}, size={self.size}, mode={self.mode!r}, erased={int(self.erased.sum())})"


def erase_reference(x: torch.Tensor, plan: ErasePlan, fill: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The erase formula as plain torch ops on a float batch ``[B, C, H, W]`` (integer batches are cast to
    float32 first): one ``torch.where``. ``fill``: the ``"pixel"`` mode's values, a tensor of the batch's shape;
    ``None`` draws them with ``torch.randn`` on the batch's device. What the models run on the CPU or with
    ``PVR_DISABLE_FUSED=1``, and what the GPU tests compare the kernels against."""
    if x.dim() != 4:
        raise ValueError(f"erase_reference: expected [B, C, H, W], got {tuple(x.shape)}")
    if not x.is_floating_point():
        x = x.float()
    B, C, H, W = x.shape
    plan.check(B, (H, W))
    dev = x.device
    if plan.mode == "pixel":
        if fill is None:
            fill = torch.randn(x.shape, dtype=x.dtype, device=dev)
        if tuple(fill.shape) != tuple(x.shape):
            raise ValueError(f"erase_reference: fill must have the batch's shape {tuple(x.shape)}, got {tuple(fill.shape)}")
        fill = fill.to(device=dev, dtype=x.dtype)
    else:
        if fill is not None:
            raise ValueError("erase_reference: fill is the \"pixel\" mode's; a \"const\" plan carries its value")
        fill = torch.tensor(plan.channel_values(C), dtype=x.dtype, device=dev).view(1, C, 1, 1)
    box = plan.box.to(dev)
    xs = torch.arange(W, device=dev).view(1, 1, 1, W)
    ys = torch.arange(H, device=dev).view(1, 1, H, 1)
    x0, y0, x1, y1 = (box[:, i].view(B, 1, 1, 1) for i in range(4))
    inside = (xs >= x0) & (xs < x1) & (ys >= y0) & (ys < y1)
    return torch.where(inside, fill, x)


class RandomErasing:
    """Sampler of :class:`ErasePlan` s, one box per sample, by the procedure of the common implementation.

    A sample is erased with probability ``prob``. It then makes up to ``ATTEMPTS`` = 10 attempts of:
    ``area ~ U(scale) * H * W``, ``log r ~ U(log ratio)``, ``h = round(sqrt(area * r))``, ``w = round(sqrt(area / r))``;
    the first attempt with ``0 < h < H`` and ``0 < w < W`` is taken, its top-left corner uniform over the
    positions that keep the box inside the image. A sample with no accepted attempt is not erased.

    All draws are float64, on the host, from ``generator`` (the global CPU generator when ``None``): one
    ``[B, 1 + 4 * ATTEMPTS]`` tensor per call whatever the decisions, so the stream of draws does not depend
    on them. The generator's state is not part of any checkpoint. After :meth:`sample`, ``last_area`` and
    ``last_ratio`` (float64 ``[B]``, NaN where the sample is not erased) hold the accepted attempt's draws."""

    ATTEMPTS = 10

    def __init__(self, prob: float = 0.25, scale: Tuple[float, float] = (0.02, 1 / 3), ratio: Tuple[float, float] = (0.3, 3.3),
                 mode: str = "pixel", value: Union[float, Sequence[float]] = 0.0, generator: Optional[torch.Generator] = None):
        if not (0.0 <= prob <= 1.0 and 0.0 < scale[0] <= scale[1] <= 1.0 and 0.0 < ratio[0] <= ratio[1]) or mode not in MODES:
            raise ValueError(f"RandomErasing: bad prob {prob}, scale {scale}, ratio {ratio} or mode {mode!r}")
        self.prob, self.scale, self.ratio = float(prob), (float(scale[0]), float(scale[1])), (float(ratio[0]), float(ratio[1]))
        self.mode, self.value, self.generator = mode, value, generator
        self.last_area = self.last_ratio = None
        ErasePlan.none(0, (1, 1), mode, value)  # validates mode and value

    def sample(self, batch: int, height: int, width: int) -> ErasePlan:
        if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("RandomErasing draws its plan on the host every step: it cannot run inside a graph capture (a "
                               "replay would reuse one draw); pass an explicit ErasePlan or train without a graph")
        B, H, W, A = int(batch), int(height), int(width), self.ATTEMPTS
        u = torch.rand(B, 1 + 4 * A, generator=self.generator, dtype=torch.float64)
        on = u[:, 0] < self.prob
        ua, ur, uy, ux = (u[:, 1 + k::4][:, :A] for k in range(4))  # [B, A] each: area, log ratio, top, left
        area = (self.scale[0] + ua * (self.scale[1] - self.scale[0])) * (H * W)
        lo, hi = math.log(self.ratio[0]), math.log(self.ratio[1])
        r = torch.exp(lo + ur * (hi - lo))
        h = torch.round(torch.sqrt(area * r)).long()
        w = torch.round(torch.sqrt(area / r)).long()
        ok = (h > 0) & (h < H) & (w > 0) & (w < W)
        first = torch.where(ok.any(1), ok.long().argmax(1), torch.zeros(B, dtype=torch.long))[:, None]
        pick = lambda t: t.gather(1, first)[:, 0]  # noqa: E731
        hit = on & ok.any(1)
        h, w = pick(h), pick(w)
        top = (pick(uy) * (H - h + 1).double()).long().clamp(max=H - 1).minimum(H - h).clamp(min=0)
        left = (pick(ux) * (W - w + 1).double()).long().clamp(max=W - 1).minimum(W - w).clamp(min=0)
        box = torch.stack([left, top, left + w, top + h], dim=1) * hit[:, None]
        nan = torch.full((B,), float("nan"), dtype=torch.float64)
        self.last_area, self.last_ratio = torch.where(hit, pick(area), nan), torch.where(hit, pick(r), nan)
        return ErasePlan(box.to(torch.int32), (H, W), self.mode, self.value)

    def __repr__(self):
        return f"RandomErasing(prob={self.prob}, scale={self.scale}, ratio={self.ratio}, mode={self.mode!r}, value={self.value})"
