"""Loss modules for the engine beyond ``nn.CrossEntropyLoss``.

:class:`BinaryCrossEntropy` is the sigmoid loss of DeiT-III ("DeiT III: Revenge of the ViT", Touvron et al. 2022)
and of timm's ``--bce-loss``: every class is an independent binary problem against the one-hot, smoothed and
(under mixup / CutMix) mixed label row. On the GPU it is one fused kernel (``csrc/bce.hip``) that also hands the
engine its ``argmax == label`` flags; see :func:`~.ops.fused_vit.binary_cross_entropy`.
"""
from __future__ import annotations

from typing import Optional

import torch
from torch import nn

from .ops.fused_vit import binary_cross_entropy


class BinaryCrossEntropy(nn.Module):
    """``forward(logits [B, C], y int [B], plan=None)``: binary cross-entropy with logits against the rows
    ``(1 - smoothing) * (lam * onehot(y) + (1 - lam) * onehot(y[partner])) + smoothing / C`` (``plan``: the batch's
    :class:`~.data.batch_mix.MixPlan`; ``None``: unmixed).

    ``target_threshold`` (optional, in ``[0, 1)``): the rows are binarised, ``t = row > target_threshold`` (timm).
    ``sum_classes``: sum over the classes, then mean over the batch (timm), instead of the mean over both
    (``nn.BCEWithLogitsLoss``). Labels are class indices like ``nn.CrossEntropyLoss``'s; dense target matrices,
    ``pos_weight`` and class weights are not supported.

    As the ``loss_fn`` of :func:`~.engine.train_step` with ``batch_mix`` it receives each batch's plan, and the
    smoothing is ``batch_mix.label_smoothing`` as for cross-entropy. It synchronises nothing with the host, so it
    also serves :class:`~.runtime.graph.GraphedTrainStep`."""

    def __init__(self, smoothing: float = 0.0, target_threshold: Optional[float] = None, sum_classes: bool = False):
        super().__init__()
        if not 0.0 <= smoothing <= 1.0:
            raise ValueError(f"smoothing must be in [0, 1], got {smoothing}")
        if target_threshold is not None and not 0.0 <= target_threshold < 1.0:
            raise ValueError(f"target_threshold must be in [0, 1), got {target_threshold}")
        self.smoothing = float(smoothing)
        self.target_threshold = None if target_threshold is None else float(target_threshold)
        self.sum_classes = bool(sum_classes)

    def forward(self, logits: torch.Tensor, y: torch.Tensor, plan=None) -> torch.Tensor:
        return binary_cross_entropy(logits, y, plan, self.smoothing, self.target_threshold, self.sum_classes)

    def extra_repr(self) -> str:
        return f"smoothing={self.smoothing}, target_threshold={self.target_threshold}, sum_classes={self.sum_classes}"
