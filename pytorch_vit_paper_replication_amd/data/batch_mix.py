"""Mixup, CutMix and label smoothing for a batch on the device.

A :class:`MixPlan` says, per sample ``b``: a partner sample, a blend weight ``lam`` and a half-open box
``(bx0, by0, bx1, by1)`` in model-image pixels. With ``pre(s, c, y, x)`` the fp32 pixel of sample ``s``
as the model sees it (after normalisation and the sample's own crop box on the uint8 path), the mixed
pixel ``(b, c, y, x)`` is::

    pre(partner[b], c, y, x)                                  inside the box
    pre(b, c, y, x)                                           elif lam == 1   (a select)
    lam * pre(b, ...) + (1.0f - lam) * pre(partner[b], ...)   otherwise

in fp32, every operation rounded on its own. Mixup is ``lam < 1`` with an empty box, CutMix ``lam == 1``
with a box. On the fused GPU path the patch-embedding kernels do this while they gather the patch
rows (``csrc/patchify.hip``, ``MIX`` variants): CutMix moves the bytes of an unmixed batch, mixup
reads the input a second time; nothing downstream changes. Elsewhere (CPU, ``PVR_DISABLE_FUSED=1``)
:func:`mix_reference` runs the same formula as torch ops.

The labels mix with ``lam_eff = lam * (1 - box area / (H * W))``, the fraction of sample ``b`` left in
its image; ``ops.fused_vit.soft_cross_entropy`` takes the plan and a label smoothing.
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import torch


class MixPlan:
    """A batch's mix plan (see the module docstring). Host tensors:

    ``partner`` int64 ``[B]``, ``lam`` float32 ``[B]`` (pixel blend weight), ``box`` int32 ``[B, 4]`` rows
    ``(bx0, by0, bx1, by1)``, ``lam_eff`` float32 ``[B]`` (label weight), ``size`` = ``(H, W)``, and
    ``rows``, the kernels' table: int32 ``[B, 8]`` = ``partner, lam's float bits, bx0, by0, bx1, by1``, then
    ``lam_eff``'s float bits (the kernels ignore it) and 0 (``csrc/kernels.h`` ``MixRow``), in pinned memory
    when a GPU is present. :meth:`on` uploads it
    (non-blocking, once per device)."""

    def __init__(self, partner, lam, box, size: Tuple[int, int]):
        H, W = int(size[0]), int(size[1])
        partner = torch.as_tensor(partner, dtype=torch.int64).reshape(-1).cpu()
        B = partner.numel()
        lam = torch.as_tensor(lam, dtype=torch.float32).reshape(-1).cpu()
        box = torch.as_tensor(box, dtype=torch.int32).reshape(-1, 4).cpu()
        if lam.numel() == 1 and B > 1:
            lam = lam.repeat(B)
        if box.shape[0] == 1 and B > 1:
            box = box.repeat(B, 1)
        if lam.numel() != B or box.shape[0] != B or H <= 0 or W <= 0:
            raise ValueError(f"MixPlan: partner [{B}], lam [{lam.numel()}], box [{box.shape[0]}, 4], size {size} do not match")
        if B and (int(partner.min()) < 0 or int(partner.max()) >= B):
            raise ValueError(f"MixPlan: partner indices must be in [0, {B})")
        if B and not bool(((lam >= 0) & (lam <= 1)).all()):
            raise ValueError("MixPlan: lam must be in [0, 1]")
        x0, y0, x1, y1 = box.unbind(1)
        if B and not bool(((x0 >= 0) & (x0 <= x1) & (x1 <= W) & (y0 >= 0) & (y0 <= y1) & (y1 <= H)).all()):
            raise ValueError(f"MixPlan: boxes must be half-open (x0, y0, x1, y1) inside the {H}x{W} image")
        area = ((x1 - x0).double() * (y1 - y0).double()) / float(H * W)
        self.partner, self.lam, self.box, self.size = partner, lam, box, (H, W)
        self.lam_eff = (lam.double() * (1.0 - area)).to(torch.float32)
        rows = torch.zeros(B, 8, dtype=torch.int32)
        rows[:, 0] = partner.to(torch.int32)
        rows[:, 1] = lam.view(torch.int32)
        rows[:, 2:6] = box
        rows[:, 6] = self.lam_eff.view(torch.int32)
        self.rows = rows.pin_memory() if torch.cuda.is_available() else rows
        self._on: Dict[torch.device, Tuple[torch.Tensor, torch.Tensor, torch.Tensor]] = {}

    @property
    def batch(self) -> int:
        return self.partner.numel()

    @classmethod
    def identity(cls, batch: int, size: Tuple[int, int]) -> "MixPlan":
        return cls(torch.arange(batch), torch.ones(batch), torch.zeros(batch, 4, dtype=torch.int32), size)

    def on(self, device) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """``(rows, partner, lam_eff)`` on ``device``."""
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        t = self._on.get(device)
        if t is None:
            if device.type == "cpu":
                t = (self.rows, self.partner, self.lam_eff)
            else:  # one upload: the label weight rides in the table's spare word 6
                with torch.inference_mode(False):  # kept across calls: not inference tensors
                    rows = self.rows.to(device, non_blocking=True)
                    t = (rows, rows[:, 0].long(), rows[:, 6].contiguous().view(torch.float32))
            self._on[device] = t
        return t

    def check(self, batch: int, size: Tuple[int, int]) -> None:
        if self.batch != batch or self.size != (int(size[0]), int(size[1])):
            raise ValueError(f"MixPlan for {self.batch} samples of {self.size[0]}x{self.size[1]} applied to {batch} samples of "
                             f"{size[0]}x{size[1]}")

    def __repr__(self):
        return f"MixPlan(batch={self.batch}, size={self.size}, lam_eff={[round(v, 3) for v in self.lam_eff.tolist()]})"


def mix_reference(x: torch.Tensor, plan: MixPlan) -> torch.Tensor:
    """The mix formula as plain torch ops on a float batch ``[B, C, H, W]`` (integer batches are cast to
    float32 first): selects with ``torch.where``, a separate multiply, multiply and add for the blend.
    What the models run on the CPU or with ``PVR_DISABLE_FUSED=1``, and what the GPU tests compare the
    kernels against."""
    if x.dim() != 4:
        raise ValueError(f"mix_reference: expected [B, C, H, W], got {tuple(x.shape)}")
    if not x.is_floating_point():
        x = x.float()
    B, _, H, W = x.shape
    plan.check(B, (H, W))
    dev = x.device
    partner = plan.partner.to(dev)
    lam32 = plan.lam.to(dev)
    box = plan.box.to(dev)
    xp = x.index_select(0, partner)
    xs = torch.arange(W, device=dev).view(1, 1, 1, W)
    ys = torch.arange(H, device=dev).view(1, 1, H, 1)
    bx0, by0, bx1, by1 = (box[:, i].view(B, 1, 1, 1) for i in range(4))
    inside = (xs >= bx0) & (xs < bx1) & (ys >= by0) & (ys < by1)
    lam = lam32.view(B, 1, 1, 1).to(x.dtype)
    oml = (1.0 - lam32).view(B, 1, 1, 1).to(x.dtype)  # 1 - lam formed in fp32, as the kernels do
    a = lam * x
    b = oml * xp
    return torch.where(inside, xp, torch.where(lam == 1, x, a + b))


class BatchMix:
    """Sampler of :class:`MixPlan` s: mixup and / or CutMix with the usual recipe, and the label
    smoothing the loss is taken with.

    With probability ``prob`` a batch is mixed: CutMix with probability ``switch_prob`` when both
    ``mixup_alpha`` and ``cutmix_alpha`` are positive (else whichever is), ``lam ~ Beta(alpha, alpha)``.
    CutMix cuts a box of ``int(H * r) x int(W * r)`` pixels, ``r = sqrt(1 - lam)``, around a centre uniform in
    the image, clipped to it; the label weight is the area actually kept. Every sample pairs with its
    mirror in the batch (``B - 1 - b``). ``per_sample``: each sample draws its own decision, ``lam`` and box,
    and the partners are a random permutation. All draws come from ``generator`` (the global CPU
    generator when ``None``), on the host; its state is not part of any checkpoint."""

    def __init__(self, mixup_alpha: float = 0.8, cutmix_alpha: float = 1.0, prob: float = 1.0, switch_prob: float = 0.5,
                 label_smoothing: float = 0.1, per_sample: bool = False, generator: Optional[torch.Generator] = None):
        if mixup_alpha < 0 or cutmix_alpha < 0 or not (0.0 <= prob <= 1.0 and 0.0 <= switch_prob <= 1.0
                                                        and 0.0 <= label_smoothing < 1.0):
            raise ValueError(f"BatchMix: bad mixup_alpha {mixup_alpha}, cutmix_alpha {cutmix_alpha}, prob {prob}, "
                             f"switch_prob {switch_prob} or label_smoothing {label_smoothing}")
        self.mixup_alpha, self.cutmix_alpha = float(mixup_alpha), float(cutmix_alpha)
        self.prob, self.switch_prob, self.label_smoothing = float(prob), float(switch_prob), float(label_smoothing)
        self.per_sample, self.generator = bool(per_sample), generator

    def _beta(self, alpha: float, n: int) -> torch.Tensor:
        # Beta(a, a) = Ga / (Ga + Gb) of two seeded Gamma(a) draws (drawn even when unused: the stream
        # of draws does not depend on the decisions)
        conc = torch.full((2, n), max(alpha, 1e-3), dtype=torch.float64)
        g = torch._standard_gamma(conc, generator=self.generator)
        tot = g.sum(0)
        return torch.where(tot > 0, g[0] / tot.clamp_min(1e-300), torch.full_like(tot, 0.5))

    def sample(self, batch: int, height: int, width: int) -> MixPlan:
        if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("BatchMix draws its plan on the host every step: it cannot run inside a graph capture (a "
                               "replay would reuse one draw); pass an explicit MixPlan or train without a graph")
        B, H, W = int(batch), int(height), int(width)
        n = B if self.per_sample else 1
        u = torch.rand(n, 4, generator=self.generator, dtype=torch.float64)  # mix?, CutMix?, centre y, centre x
        lam_mix, lam_cut = self._beta(self.mixup_alpha, n), self._beta(self.cutmix_alpha, n)
        perm = torch.randperm(B, generator=self.generator) if self.per_sample else torch.arange(B - 1, -1, -1)
        has_mix, has_cut = self.mixup_alpha > 0, self.cutmix_alpha > 0
        on = (u[:, 0] < self.prob) & (has_mix or has_cut)
        cut = on & has_cut & ((u[:, 1] < self.switch_prob) | (not has_mix))
        mixup = on & ~cut
        r = torch.sqrt(1.0 - lam_cut)
        cut_h, cut_w = (H * r).long(), (W * r).long()
        cy, cx = (u[:, 2] * H).long().clamp(max=H - 1), (u[:, 3] * W).long().clamp(max=W - 1)
        y0, y1 = (cy - cut_h // 2).clamp(0, H), (cy + cut_h // 2).clamp(0, H)
        x0, x1 = (cx - cut_w // 2).clamp(0, W), (cx + cut_w // 2).clamp(0, W)
        box = torch.stack([x0, y0, x1, y1], dim=1) * cut[:, None]
        lam = torch.where(mixup, lam_mix, torch.ones_like(lam_mix)).to(torch.float32)
        if n != B:
            box, lam = box.expand(B, 4), lam.expand(B)
        plan = MixPlan(perm, lam, box.to(torch.int32), (H, W))
        same = plan.lam_eff == 1  # nothing of the partner is used: say so in the plan
        if bool(same.any()):
            plan = MixPlan(torch.where(same, torch.arange(B), perm), lam, box.to(torch.int32), (H, W))
        return plan

    def __repr__(self):
        return (f"BatchMix(mixup_alpha={self.mixup_alpha}, cutmix_alpha={self.cutmix_alpha}, prob={self.prob}, "
                f"switch_prob={self.switch_prob}, label_smoothing={self.label_smoothing}, per_sample={self.per_sample})")
