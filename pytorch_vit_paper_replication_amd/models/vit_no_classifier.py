"""ViT backbone without the classifier head (reference models/vit_no_classifier.py:172-226).

``forward`` returns the final-LayerNorm'd full token sequence ``[B, N+1, D]``; the state_dict is the
full ViT's minus ``classifier.*``. With ``set_patch_dropout(rate)`` a training forward returns the kept
tokens only, ``[B, N'+1, D]`` with ``N' = max(1, N - floor(rate * N))`` (class token first, kept patches in
raster order); eval, ``no_grad`` and ``inference_mode`` forwards return every token. The building blocks are shared with :mod:`.vit` (the reference keeps
verbatim copies; here there is one implementation).
"""
from __future__ import annotations

from typing import Optional

import torch
from torch import nn

from .. import _ext
from .vit import (MLPBlock, MultiHeadSelfAttentionBlock, PatchEmbedding, SelfAttention,  # noqa: F401
                  TransformerEncoderBlock, ViT as _FullViT)


class ViT(_FullViT):
    def __init__(self, image_size: int = 224, patch_size: int = 16, num_transformer_layer: int = 12,
                 num_heads: int = 12, embedding_dim: int = 768, mlp_size: int = 3072, attn_dropout: float = 0,
                 mlp_dropout: float = 0.1, embedding_dropout: float = 0.1):
        super().__init__(image_size=image_size, patch_size=patch_size, num_transformer_layer=num_transformer_layer,
                         num_heads=num_heads, embedding_dim=embedding_dim, mlp_size=mlp_size, attn_dropout=attn_dropout,
                         mlp_dropout=mlp_dropout, embedding_dropout=embedding_dropout, num_classes=1)
        del self.classifier
        self.config.pop("num_classes", None)

    def forward(self, x: torch.Tensor, geom: Optional[torch.Tensor] = None, mix=None, erase=None, color=None) -> torch.Tensor:
        x = self._color_stage(x, color)  # color: a ColorPlan on the raw uint8 batch, as models/vit.py
        x, pre = self._device_input(x, geom)  # uint8 batches after set_device_input (models/vit.py)
        if _ext.use_fused(x) and self._fused_supported(x, pre):
            return self._forward_fused_features(x, pre, mix, erase)
        # mix: a MixPlan, erase: an ErasePlan, as models/vit.py
        return self.forward_features(self._mix_reference(self._erase_reference(self._preprocess_reference(x, pre), erase), mix))

    def _forward_fused_features(self, x: torch.Tensor, pre=None, mix=None, erase=None) -> torch.Tensor:
        from ..ops.fused_vit import TokenLayerNormFn

        tokens, store, B, N = self._fused_encoder(x, pre, mix=mix, erase=erase)  # the full ViT's fused encoder (device checks, side-stream join)
        y = TokenLayerNormFn.apply(tokens, self.layer_norm.eps, store, self.layer_norm.weight, self.layer_norm.bias)
        return y.float().view(B, N, -1)
