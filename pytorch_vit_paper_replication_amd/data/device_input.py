"""Device-side input preprocessing: the model takes raw ``uint8`` image batches.

The reference's input pipeline converts every image to an fp32 CHW tensor in a CPU worker
(``ToDtype(scale=True)`` / ``Normalize``) and uploads 12 bytes per pixel. With a :class:`DeviceInput`
set on the model (``ViT.set_device_input``) the loader yields ``uint8`` batches (3 bytes per pixel,
see :func:`..data.transforms.uint8_transform`) and the patch-embedding kernel ``im2col_u8`` does the
scale to [0, 1], the per-channel normalisation and, per sample, a crop box resampled to the model's
image size and an optional horizontal flip, while it gathers the patch rows.

A crop is a ``geom`` row ``(x0, y0, x1, y1)`` in source pixel-edge coordinates: ``(0, 0, Ws, Hs)`` is
the whole ``Hs x Ws`` source, ``x0 > x1`` a horizontally flipped box. Output pixel ``ox`` samples the
source at ``x0 + (ox + 0.5) * (x1 - x0) / W - 0.5`` (clamped to the image), bilinearly between the
two nearest pixels. There is NO antialiasing: a box more than ~2x the output size aliases, so
pre-shrink large sources on the host (``uint8_transform(size)`` resizes with antialiasing).
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional, Sequence, Tuple

import torch


def full_box(batch: int, src_h: int, src_w: int) -> torch.Tensor:
    """``[batch, 4]`` float32 boxes covering the whole ``src_h x src_w`` source."""
    return torch.tensor([0.0, 0.0, float(src_w), float(src_h)], dtype=torch.float32).repeat(batch, 1)


def center_box(batch: int, src_h: int, src_w: int, crop_h: float, crop_w: Optional[float] = None) -> torch.Tensor:
    """``[batch, 4]`` float32 boxes of size ``crop_h x crop_w`` (``crop_w`` defaults to ``crop_h``)
    centred in the ``src_h x src_w`` source (the device-side ``CenterCrop``)."""
    crop_w = crop_h if crop_w is None else crop_w
    if not (0 < crop_h <= src_h and 0 < crop_w <= src_w):
        raise ValueError(f"center_box: a {crop_h}x{crop_w} crop does not fit a {src_h}x{src_w} source")
    x0, y0 = (src_w - crop_w) / 2.0, (src_h - crop_h) / 2.0
    return torch.tensor([x0, y0, x0 + crop_w, y0 + crop_h], dtype=torch.float32).repeat(batch, 1)


class RandomResizedCropFlip:
    """Random-resized-crop + horizontal flip as ``geom`` boxes for the device kernel.

    Per sample: an area fraction uniform in ``scale`` and an aspect ratio (w / h) log-uniform in
    ``ratio``, up to 10 tries until the box fits the source, placed uniformly; if no try fits, the
    centred box of the source clamped to ``ratio``. With probability ``flip`` the box's x0 and x1 are
    swapped. All draws come from ``generator`` (the global CPU generator when ``None``), on the host.

    The generator's state is not part of any checkpoint: a resumed run continues with fresh draws.
    """

    TRIES = 10

    def __init__(self, scale: Tuple[float, float] = (0.08, 1.0), ratio: Tuple[float, float] = (3.0 / 4.0, 4.0 / 3.0),
                 flip: float = 0.5, generator: Optional[torch.Generator] = None):
        if not (0 < scale[0] <= scale[1] and 0 < ratio[0] <= ratio[1] and 0.0 <= flip <= 1.0):
            raise ValueError(f"RandomResizedCropFlip: bad scale {scale}, ratio {ratio} or flip {flip}")
        self.scale, self.ratio, self.flip, self.generator = tuple(scale), tuple(ratio), float(flip), generator

    def sample(self, batch: int, src_h: int, src_w: int) -> torch.Tensor:
        """``[batch, 4]`` float32 boxes ``(x0, y0, x1, y1)`` inside a ``src_h x src_w`` source."""
        g = self.generator
        u = torch.rand(batch, self.TRIES, 2, generator=g, dtype=torch.float64)
        place = torch.rand(batch, 3, generator=g, dtype=torch.float64)
        area = (self.scale[0] + u[..., 0] * (self.scale[1] - self.scale[0])) * (src_h * src_w)
        lr0, lr1 = math.log(self.ratio[0]), math.log(self.ratio[1])
        aspect = torch.exp(lr0 + u[..., 1] * (lr1 - lr0))
        w, h = torch.sqrt(area * aspect), torch.sqrt(area / aspect)
        fits = (w <= src_w) & (h <= src_h)
        first = torch.argmax(fits.to(torch.int8), dim=1, keepdim=True)  # first fitting try
        w, h = w.gather(1, first).squeeze(1), h.gather(1, first).squeeze(1)
        # fallback: the whole source, shrunk along one axis until its aspect is inside `ratio`
        in_ratio = src_w / src_h
        if in_ratio < self.ratio[0]:
            fw, fh = float(src_w), src_w / self.ratio[0]
        elif in_ratio > self.ratio[1]:
            fw, fh = src_h * self.ratio[1], float(src_h)
        else:
            fw, fh = float(src_w), float(src_h)
        ok = fits.any(dim=1)
        w = torch.where(ok, w, torch.full_like(w, fw))
        h = torch.where(ok, h, torch.full_like(h, fh))
        x0 = torch.where(ok, place[:, 0], torch.full_like(w, 0.5)) * (src_w - w)
        y0 = torch.where(ok, place[:, 1], torch.full_like(h, 0.5)) * (src_h - h)
        x1, y1 = torch.clamp(x0 + w, max=src_w), torch.clamp(y0 + h, max=src_h)
        flipped = place[:, 2] < self.flip
        box = torch.stack([torch.where(flipped, x1, x0), y0, torch.where(flipped, x0, x1), y1], dim=1)
        return box.to(torch.float32)

    def __repr__(self):
        return f"RandomResizedCropFlip(scale={self.scale}, ratio={self.ratio}, flip={self.flip})"


@dataclass
class DeviceInput:
    """What ``ViT.set_device_input`` needs to turn ``uint8`` batches into model input on the device.

    ``mean`` / ``std``: per-channel normalisation of the [0, 1]-scaled image; ``None`` means 0 / 1,
    the reference's ``default_vit_transform`` (scale only). ``augment``: a sampler of per-sample crop
    boxes (:class:`RandomResizedCropFlip`) the model draws from in training mode. ``color``: a sampler of
    per-sample colour plans (:class:`~.color_augment.ColorAugment`) the model draws from in training mode
    likewise; the colour stage runs on the source batch, before the crop.
    """

    mean: Optional[Sequence[float]] = None
    std: Optional[Sequence[float]] = None
    augment: Optional[RandomResizedCropFlip] = None
    color: Optional["ColorAugment"] = None  # noqa: F821 (data/color_augment.py)

    def mean_std(self, channels: int = 3) -> Tuple[Tuple[float, ...], Tuple[float, ...]]:
        mean = (0.0,) * channels if self.mean is None else tuple(float(m) for m in self.mean)
        std = (1.0,) * channels if self.std is None else tuple(float(s) for s in self.std)
        if len(mean) != channels or len(std) != channels:
            raise ValueError(f"DeviceInput: mean / std need {channels} values, got {mean} / {std}")
        if any(s == 0.0 for s in std):
            raise ValueError("DeviceInput: std must be non-zero")
        return mean, std


def preprocess_reference(x: torch.Tensor, mean=None, std=None, geom: Optional[torch.Tensor] = None,
                         size: Optional[Tuple[int, int]] = None, dtype=torch.float32) -> torch.Tensor:
    """The ``im2col_u8`` kernel's preprocessing as plain torch ops in the same operation order:
    ``uint8 [B, C, Hs, Ws]`` -> ``dtype [B, C, H, W]``. This is what the model runs on the CPU (or with
    ``PVR_DISABLE_FUSED=1``) and what the GPU tests compare the kernel against; ``dtype=float64``
    evaluates the same formulas in double precision.

    Every divisor is a tensor: PyTorch's GPU kernels divide by a Python scalar as a multiply with its
    reciprocal, which differs from the division in the last bit.
    """
    if x.dtype != torch.uint8 or x.dim() != 4:
        raise ValueError(f"preprocess_reference: expected a uint8 [B, C, Hs, Ws] batch, got {x.dtype} {tuple(x.shape)}")
    B, C, Hs, Ws = x.shape
    H, W = (Hs, Ws) if size is None else (int(size[0]), int(size[1]))
    dev = x.device
    m, s = DeviceInput(mean, std).mean_std(C)

    def const(v):
        return torch.tensor(v, dtype=torch.float32, device=dev).to(dtype)

    if geom is None:
        if (Hs, Ws) != (H, W):
            raise ValueError(f"preprocess_reference: a {Hs}x{Ws} source needs geom to produce {H}x{W}")
        p = x.to(dtype)
    else:
        if tuple(geom.shape) != (B, 4):
            raise ValueError(f"preprocess_reference: geom must be [{B}, 4], got {tuple(geom.shape)}")
        gm = geom.to(device=dev, dtype=dtype)

        def axis(e0, e1, n_out, n_src):
            step = (e1 - e0) / const([float(n_out)])
            o = torch.arange(n_out, device=dev, dtype=dtype) + 0.5
            sc = e0[:, None] + o[None, :] * step[:, None] - 0.5
            sc = sc.clamp(0.0, float(n_src - 1))
            f = torch.floor(sc)
            i = f.long()
            return i, (i + 1).clamp(max=n_src - 1), sc - f

        xi, xj, wx = axis(gm[:, 0], gm[:, 2], W, Ws)
        yi, yj, wy = axis(gm[:, 1], gm[:, 3], H, Hs)
        bi = torch.arange(B, device=dev)[:, None, None]

        def tap(yy, xx):  # [B, H, W, C] gather -> [B, C, H, W]
            return x[bi, :, yy[:, :, None], xx[:, None, :]].permute(0, 3, 1, 2).to(dtype)

        a, b, c, d = tap(yi, xi), tap(yi, xj), tap(yj, xi), tap(yj, xj)
        wx, wy = wx[:, None, None, :], wy[:, None, :, None]
        top = a + wx * (b - a)
        bot = c + wx * (d - c)
        p = top + wy * (bot - top)
    return (p / const([255.0]) - const(m).view(1, C, 1, 1)) / const(s).view(1, C, 1, 1)
