"""Independent oracles and shared cases for the colour-augmentation tests (data/color_augment.py).

* :func:`pil_chain`: the pointwise ops and the jitter as the recipes run them, on PIL images.
* :func:`numpy_blur`: the blur formula in numpy fp32 (``np.pad(mode="edge")``, the same ordered loop).
* :func:`pointwise_case` / :func:`blur_case`: the batches and plans the CPU and GPU tests share.
"""
import numpy as np
import torch
from PIL import Image, ImageEnhance, ImageOps

from pytorch_vit_paper_replication_amd.data.color_augment import ORDERS, ColorPlan

FIXED_FACTORS = (0.0, 0.7, 1.0, 1.3, 2.0)


def pil_chain(x: torch.Tensor, plan: ColorPlan) -> torch.Tensor:
    """uint8 ``[B, 3, H, W]`` -> the same through PIL: the op (0, 1 or 2), then ``ImageEnhance`` in the sample's order."""
    out = []
    for b in range(x.shape[0]):
        im = Image.fromarray(np.ascontiguousarray(x[b].permute(1, 2, 0).cpu().numpy()), "RGB")
        op = int(plan.op[b])
        assert op in (0, 1, 2), "PIL is the yardstick of the pointwise ops only"
        if op == 1:
            im = ImageOps.grayscale(im).convert("RGB")
        elif op == 2:
            im = ImageOps.solarize(im)  # threshold 128
        fb, fc, fs = (float(f) for f in plan.factors[b])
        for step in ORDERS[int(plan.order[b])]:
            if step == "b":
                im = ImageEnhance.Brightness(im).enhance(fb)
            elif step == "c":
                im = ImageEnhance.Contrast(im).enhance(fc)
            else:
                im = ImageEnhance.Color(im).enhance(fs)
        out.append(torch.from_numpy(np.asarray(im).copy()).permute(2, 0, 1))
    return torch.stack(out)


def numpy_blur(img: np.ndarray, w: np.ndarray) -> np.ndarray:
    """uint8 ``[3, H, W]`` and fp32 taps ``[13]`` -> the blurred uint8 image."""
    assert img.dtype == np.uint8 and w.dtype == np.float32 and w.shape == (13,)
    _, H, W = img.shape
    p = np.pad(img.astype(np.float32), ((0, 0), (0, 0), (6, 6)), mode="edge")
    t = np.zeros(img.shape, np.float32)
    for i in range(13):
        t = (t + (w[i] * p[:, :, i:i + W]).astype(np.float32)).astype(np.float32)
    p = np.pad(t, ((0, 0), (6, 6), (0, 0)), mode="edge")
    o = np.zeros(img.shape, np.float32)
    for i in range(13):
        o = (o + (w[i] * p[:, i:i + H, :]).astype(np.float32)).astype(np.float32)
    return np.clip(np.floor(o + np.float32(0.5)), 0, 255).astype(np.uint8)


def images(B: int, H: int, W: int, seed: int) -> torch.Tensor:
    """Noise, a ramp plus noise, all 0 and all 255, then noise again: uint8 ``[B, 3, H, W]``."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(0, 256, (B, 3, H, W), generator=g, dtype=torch.uint8)
    if B > 1:
        ys, xs = torch.arange(H).view(H, 1), torch.arange(W).view(1, W)
        ramp = torch.stack([(5 * xs + 0 * ys) % 256, (5 * ys + 0 * xs) % 256, (3 * (xs + ys)) % 256]).float()
        x[1] = (ramp + 12.0 * torch.randn(3, H, W, generator=g)).round().clamp(0, 255).to(torch.uint8)
    if B > 2:
        x[2] = 0
    if B > 3:
        x[3] = 255
    return x


def pointwise_case(B: int, H: int, W: int, seed: int):
    """(x, plan): ops 0 / 1 / 2 in turn, all six orders, factors from ``FIXED_FACTORS`` and seeded random ones in [0, 2]."""
    g = torch.Generator().manual_seed(seed + 1000)
    x = images(B, H, W, seed)
    op = torch.arange(B) % 3
    order = (torch.arange(B) + seed) % 6
    factors = 2.0 * torch.rand(B, 3, generator=g, dtype=torch.float64)
    fixed = torch.tensor(FIXED_FACTORS, dtype=torch.float64)
    for b in range(0, B, 2):  # every other sample: fixed factors, rotating through the list
        factors[b] = fixed[(torch.arange(3) + b + seed) % len(FIXED_FACTORS)]
    return x, ColorPlan(op, None, factors.float(), order)


def blur_case(B: int, H: int, W: int, seed: int):
    """(x, plan): every op, the blur at sigma 0.1 / 0.5 / 1.0 / 2.0, blur followed by contrast among them (so
    the luma sum reads the blurred bytes), and a blur with no jitter at all."""
    x, plan = pointwise_case(B, H, W, seed)
    op, factors = plan.op.clone(), plan.factors.clone()
    op[::2] = 3  # B = 7: samples 0, 2, 4, 6 blur, one with each sigma
    sig = torch.tensor([0.1, 0.5, 1.0, 2.0])[(torch.arange(B) // 2 + seed) % 4]
    if B > 5:
        x[[2, 5]] = x[[5, 2]]  # a noise image, not the all-0 one, under the blur
    if B > 2:
        factors[2] = torch.tensor([1.0, 1.0, 1.0])
    if B > 4:
        factors[4, 1] = 0.6  # blur, then a contrast step whatever the order
    return x, ColorPlan(op, sig, factors, plan.order)
