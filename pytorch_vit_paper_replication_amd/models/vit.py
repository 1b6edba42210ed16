"""Vision Transformer (Dosovitskiy et al., 2020) with the reference's public surface.

API parity with the reference ``models/vit.py``:
  * ``ViT(image_size=224, patch_size=16, num_transformer_layer=12, num_heads=12, embedding_dim=768,
    mlp_size=3072, attn_dropout=0, mlp_dropout=0.1, embedding_dropout=0.1, num_classes=1000)``
    (reference models/vit.py:173-183) and ``forward(x [B,3,H,W]) -> logits [B, num_classes]``;
  * sub-blocks ``PatchEmbedding`` (:5-67), ``MultiHeadSelfAttentionBlock`` (:69-98),
    ``MLPBlock`` (:100-131), ``TransformerEncoderBlock`` (:133-169) with the same constructor
    signatures and submodule names, hence the same 152-key ``state_dict``;
  * the same initialisation, in the same RNG order (CLS/pos ``torch.rand``, Conv/Linear kaiming,
    in_proj xavier, zero MHA biases), so a seeded model is bit-identical to the reference's.

Execution: on CPU (or with ``PVR_DISABLE_FUSED=1``) every module runs plain PyTorch fp32 math
equivalent to the reference. On an MI355X the top-level ``ViT.forward`` runs the fused path: flat
parameter store with a bf16 shadow, hand-written gfx950 kernels for patch embedding, LayerNorm,
MFMA GEMMs with fused bias/GELU/dropout/residual epilogues, flash-style attention and a fused
classifier head (``ops.fused_vit``), with hand-written backward passes.
"""
from __future__ import annotations

import math
from typing import Optional, Tuple

import torch
import torch.nn.functional as F
from torch import nn

from .. import _ext


def patch_keep_count(n_p: int, rate: float) -> int:
    """Patches each sample keeps under patch dropout at ``rate``: ``max(1, n_p - floor(rate * n_p))`` (Python
    double arithmetic). ``n_p`` itself means off."""
    rate = float(rate)
    if not 0.0 <= rate < 1.0:
        raise ValueError(f"patch-dropout rate must be in [0, 1), got {rate}")
    return max(1, n_p - int(math.floor(rate * n_p)))


RESIZE_MODES = ("bicubic", "bilinear")


def resize_position_embedding(pos: torch.Tensor, new_grid: int, mode: str = "bicubic") -> torch.Tensor:
    """A position embedding ``[1, g * g + 1, D]`` (class-token row first) on a ``new_grid x new_grid`` patch grid:
    rows ``1..`` are viewed as ``[1, D, g, g]`` in fp32 and resampled with
    ``F.interpolate(grid, size=(new_grid, new_grid), mode=mode, align_corners=False)``; row 0 is copied. Returns a
    new tensor in ``pos``'s dtype (a clone for the same grid). ``ValueError`` if the rows behind the class token do
    not form a square grid.

    torchvision's own ``interpolate_embeddings`` resamples with ``align_corners=True`` (grid corners pinned); this
    one does not (pixel-centre alignment, what timm and the released ViT fine-tuning code do), so the two differ
    away from the grid's centre."""
    if mode not in RESIZE_MODES:
        raise ValueError(f"mode must be one of {RESIZE_MODES}, got {mode!r}")
    if pos.dim() != 3 or pos.shape[0] != 1 or pos.shape[1] < 2:
        raise ValueError(f"position embedding must be [1, g * g + 1, D], got {tuple(pos.shape)}")
    n, D = pos.shape[1] - 1, pos.shape[2]
    g = math.isqrt(n)
    if g * g != n:
        raise ValueError(f"{n} patch rows behind the class token do not form a square grid")
    new_grid = int(new_grid)
    if new_grid <= 0:
        raise ValueError(f"new_grid must be positive, got {new_grid}")
    if new_grid == g:
        return pos.detach().clone()
    grid = pos[:, 1:].detach().float().reshape(1, g, g, D).permute(0, 3, 1, 2)
    new = F.interpolate(grid, size=(new_grid, new_grid), mode=mode, align_corners=False)
    new = new.permute(0, 2, 3, 1).reshape(1, new_grid * new_grid, D).to(pos.dtype)
    return torch.cat((pos[:, :1].detach(), new), dim=1)


class PatchEmbedding(nn.Module):
    """Image -> [B, N+1, D] patch + CLS + position embeddings (reference models/vit.py:5-67).

    ``patch_keep`` (attribute, default 0 = off; set by :meth:`ViT.set_patch_dropout`): patch dropout. In
    training (grad mode on) each sample keeps that many of its patch tokens, in raster order, behind the
    class token: the output is ``[B, patch_keep + 1, D]``. The position embedding is added before the
    gather, the embedding dropout runs after it."""

    def __init__(self, image_size: int, color_channels: int = 3, patch_size: int = 16,
                 embedding_dropout: float = 0.1, embedding_dim: int = 768):
        super().__init__()
        self.patch_size = patch_size
        assert image_size % self.patch_size == 0, (
            f"Input image size must be divisible by patch size, image size: {image_size}, patch_size: {patch_size}")
        self.number_of_patches = int((image_size ** 2) / (patch_size ** 2))
        self.patch_and_flatten = nn.Sequential(
            nn.Conv2d(in_channels=color_channels, out_channels=embedding_dim, kernel_size=patch_size, stride=patch_size),
            nn.Flatten(start_dim=2, end_dim=3),
        )
        self.class_token = nn.Parameter(torch.rand(1, 1, embedding_dim), requires_grad=True)
        self.position_embedding = nn.Parameter(torch.rand(1, self.number_of_patches + 1, embedding_dim),
                                               requires_grad=True)
        self.dropout = nn.Dropout(p=embedding_dropout)
        self.patch_keep = 0

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        b = x.shape[0]
        cls = self.class_token.expand(b, -1, -1)
        x = self.patch_and_flatten(x).permute(0, 2, 1)
        x = torch.cat((cls, x), dim=1) + self.position_embedding
        n_keep = self.patch_keep_active()
        if n_keep:
            keep = self._draw_patch_keep(b, self.number_of_patches, n_keep, x.device).to(device=x.device, dtype=torch.int64)
            rows = torch.cat((torch.zeros(b, 1, dtype=torch.int64, device=x.device), keep + 1), dim=1)  # [0] + (keep + 1)
            x = torch.gather(x, 1, rows.unsqueeze(-1).expand(-1, -1, x.shape[-1]))
        return self.dropout(x)

    def patch_keep_active(self) -> int:
        """Patches per sample this forward keeps: ``patch_keep`` in training with grad mode on, else 0 (every
        patch: eval, ``no_grad`` and ``inference_mode`` never drop)."""
        n_keep = int(getattr(self, "patch_keep", 0))
        on = n_keep and n_keep < self.number_of_patches and self.training and torch.is_grad_enabled()
        return n_keep if on else 0

    def _draw_patch_keep(self, batch: int, n_p: int, n_keep: int, device) -> torch.Tensor:
        """The kept patch indices ``[batch, n_keep]``, ascending per sample, on the reference path: a uniform
        random subset from torch's RNG (the fused path ranks counter-hash keys instead, ``ops/fused_vit.py``
        ``patch_keep``; tests override this method to replay its table)."""
        return torch.rand(batch, n_p, device=device).argsort(dim=1)[:, :n_keep].sort(dim=1).values


class SelfAttention(nn.Module):
    """Multi-head attention with ``nn.MultiheadAttention``'s parameter layout and init.

    Parameters ``in_proj_weight [3D, D]`` (rows q;k;v), ``in_proj_bias [3D]``, ``out_proj.{weight,bias}``,
    so checkpoints interchange with the reference's ``nn.MultiheadAttention(batch_first=True)``.
    """

    def __init__(self, embed_dim: int, num_heads: int, dropout: float = 0.0, batch_first: bool = True):
        super().__init__()
        assert embed_dim % num_heads == 0, "embed_dim must be divisible by num_heads"
        self.embed_dim = embed_dim
        self.num_heads = num_heads
        self.head_dim = embed_dim // num_heads
        self.dropout = dropout
        self.batch_first = batch_first
        self.in_proj_weight = nn.Parameter(torch.empty(3 * embed_dim, embed_dim))
        self.in_proj_bias = nn.Parameter(torch.empty(3 * embed_dim))
        # created (and default-initialised) before in_proj, exactly like nn.MultiheadAttention
        self.out_proj = nn.Linear(embed_dim, embed_dim, bias=True)
        self._reset_parameters()

    def _reset_parameters(self):
        nn.init.xavier_uniform_(self.in_proj_weight)
        nn.init.constant_(self.in_proj_bias, 0.0)
        nn.init.constant_(self.out_proj.bias, 0.0)

    def forward(self, query: torch.Tensor, key: torch.Tensor, value: torch.Tensor, need_weights: bool = False,
                attn_mask: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
        if not self.batch_first:
            query, key, value = (t.transpose(0, 1) for t in (query, key, value))
        B, Nq, D = query.shape
        Nk = key.shape[1]
        H, dh = self.num_heads, self.head_dim
        w_q, w_k, w_v = self.in_proj_weight.chunk(3)
        b_q, b_k, b_v = self.in_proj_bias.chunk(3)
        if query is key and key is value:
            q, k, v = F.linear(query, self.in_proj_weight, self.in_proj_bias).chunk(3, dim=-1)
        else:
            q, k, v = F.linear(query, w_q, b_q), F.linear(key, w_k, b_k), F.linear(value, w_v, b_v)
        q = q.view(B, Nq, H, dh).transpose(1, 2)
        k = k.view(B, Nk, H, dh).transpose(1, 2)
        v = v.view(B, Nk, H, dh).transpose(1, 2)
        p = self.dropout if self.training else 0.0
        weights = None
        if need_weights:
            s = (q @ k.transpose(-2, -1)) / math.sqrt(dh)
            if attn_mask is not None:
                s = s + attn_mask
            a = torch.softmax(s, dim=-1)
            weights = a.mean(dim=1)
            a = F.dropout(a, p=p, training=p > 0)
            o = a @ v
        else:
            o = F.scaled_dot_product_attention(q, k, v, attn_mask=attn_mask, dropout_p=p)
        o = o.transpose(1, 2).reshape(B, Nq, D)
        # a functional call on out_proj's parameters, as in nn.MultiheadAttention (so module hooks and
        # torchinfo-style accounting see this layer exactly as they see the reference's MHA)
        o = F.linear(o, self.out_proj.weight, self.out_proj.bias)
        if not self.batch_first:
            o = o.transpose(0, 1)
        return o, weights


class MultiHeadSelfAttentionBlock(nn.Module):
    """LN -> MSA (reference models/vit.py:69-98); the residual is added by the caller."""

    def __init__(self, embedding_dim: int = 768, num_heads: int = 12, attn_dropout: float = 0):
        super().__init__()
        self.layer_norm = nn.LayerNorm(normalized_shape=embedding_dim)
        self.multi_head_attention = SelfAttention(embed_dim=embedding_dim, num_heads=num_heads,
                                                  dropout=attn_dropout, batch_first=True)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        normalized_x = self.layer_norm(x)
        attn_output, _ = self.multi_head_attention(query=normalized_x, key=normalized_x, value=normalized_x,
                                                   need_weights=False)
        return attn_output


class MLPBlock(nn.Module):
    """LN -> Linear -> GELU -> Dropout -> Linear -> Dropout (reference models/vit.py:100-131)."""

    def __init__(self, embedding_dim: int = 768, mlp_size: int = 3072, dropout: float = 0.1):
        super().__init__()
        self.layer_norm = nn.LayerNorm(normalized_shape=embedding_dim)
        self.mlp = nn.Sequential(
            nn.Linear(in_features=embedding_dim, out_features=mlp_size),
            nn.GELU(),
            nn.Dropout(p=dropout),
            nn.Linear(in_features=mlp_size, out_features=embedding_dim),
            nn.Dropout(p=dropout),
        )

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return self.mlp(self.layer_norm(x))


def drop_path_thr(p: float) -> int:
    """The 16-bit threshold of a drop rate, as at every dropout site of the fused kernels:
    ``min(round(p * 65536), 65535)`` (halves round up, as the host code of the kernels rounds); a sample
    is kept iff its 16-bit draw is ``>= thr``. A rate below ``2 ** -17`` has threshold 0: it never drops."""
    return min(int(math.floor(float(p) * 65536.0 + 0.5)), 65535)


def drop_path_keep_scale(p: float) -> float:
    """What a kept branch is multiplied by: ``65536 / (65536 - thr)`` (fp32 in the kernels)."""
    return 65536.0 / (65536.0 - drop_path_thr(p))


def drop_path_rates(rate: float, depth: int, schedule: str = "linear"):
    """Per-block drop-path rates: ``rate * i / (depth - 1)`` (``rate`` for a single block), or ``rate``
    for every block with ``schedule="constant"``."""
    if schedule not in ("linear", "constant"):
        raise ValueError(f"drop-path schedule must be 'linear' or 'constant', got {schedule!r}")
    rate = float(rate)
    if not 0.0 <= rate < 1.0:
        raise ValueError(f"drop-path rate must be in [0, 1), got {rate}")
    if schedule == "constant" or depth <= 1:
        return [rate] * depth
    return [rate * i / (depth - 1) for i in range(depth)]


class TransformerEncoderBlock(nn.Module):
    """x = MSA(x) + x ; x = MLP(x) + x (reference models/vit.py:133-169).

    ``drop_path`` (attribute, default 0; set by :meth:`ViT.set_drop_path`): stochastic depth. In training
    each sample drops each of the two residual branches independently with this probability, and a
    kept branch is scaled by ``drop_path_keep_scale``: ``x = x + s[b] * branch(x)``.

    ``layer_scale_1`` / ``layer_scale_2`` (parameters ``[D]``, absent by default; registered by
    :meth:`ViT.set_layer_scale`): LayerScale, ``x = x + s[b] * g1 * MSA(LN(x))``, ``x = x + s[b] * g2 * MLP(LN(x))``."""

    def __init__(self, embedding_dim: int = 768, num_heads: int = 12, attn_dropout: float = 0,
                 mlp_size: int = 3072, mlp_dropout: float = 0.1):
        super().__init__()
        self.msa_block = MultiHeadSelfAttentionBlock(embedding_dim=embedding_dim, num_heads=num_heads,
                                                     attn_dropout=attn_dropout)
        self.mlp_block = MLPBlock(embedding_dim=embedding_dim, mlp_size=mlp_size, dropout=mlp_dropout)
        self.drop_path = 0.0

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        p = self.drop_path if self.training else 0.0
        g1, g2 = getattr(self, "layer_scale_1", None), getattr(self, "layer_scale_2", None)
        if g1 is not None:  # LayerScale: each branch times its vector, before the drop-path factor and the residual add
            if p <= 0.0 or drop_path_thr(p) == 0:
                x = g1 * self.msa_block(x) + x
                return g2 * self.mlp_block(x) + x
            x = self._drop_path_scale(x, p, 0) * (g1 * self.msa_block(x)) + x
            return self._drop_path_scale(x, p, 1) * (g2 * self.mlp_block(x)) + x
        if p <= 0.0 or drop_path_thr(p) == 0:
            x = self.msa_block(x) + x
            x = self.mlp_block(x) + x
            return x
        x = self._drop_path_scale(x, p, 0) * self.msa_block(x) + x
        x = self._drop_path_scale(x, p, 1) * self.mlp_block(x) + x
        return x

    def _draw_drop_path(self, batch: int, p: float, branch: int, device) -> torch.Tensor:
        """Keep decisions (bool ``[batch]``) of one residual branch (0 attention, 1 MLP) on the reference
        path: 16-bit draws from torch's RNG against the kernels' threshold."""
        return torch.randint(0, 65536, (batch,), device=device) >= drop_path_thr(p)

    def _drop_path_scale(self, x: torch.Tensor, p: float, branch: int) -> torch.Tensor:
        """``s[b]`` as ``[B, 1, 1]`` in x's dtype: 0 for a dropped sample, else ``drop_path_keep_scale(p)``."""
        keep = self._draw_drop_path(x.shape[0], p, branch, x.device)
        return (keep.to(device=x.device, dtype=x.dtype) * drop_path_keep_scale(p)).view(-1, 1, 1)

    # fused-path helpers ---------------------------------------------------------------
    def fused_params(self):
        m, p = self.msa_block, self.mlp_block
        a = m.multi_head_attention
        ps = (m.layer_norm.weight, m.layer_norm.bias, a.in_proj_weight, a.in_proj_bias,
              a.out_proj.weight, a.out_proj.bias, p.layer_norm.weight, p.layer_norm.bias,
              p.mlp[0].weight, p.mlp[0].bias, p.mlp[3].weight, p.mlp[3].bias)
        g1 = getattr(self, "layer_scale_1", None)
        # LayerScale: the two scales follow the twelve (a block without them passes what it always passed)
        return ps if g1 is None else ps + (g1, self.layer_scale_2)

    def folded_triples(self):
        """LayerScale: ``(W, b, g)`` of the two scaled Linear layers, the out-projection with ``layer_scale_1`` and
        fc2 with ``layer_scale_2`` (empty without the option)."""
        if getattr(self, "layer_scale_1", None) is None:
            return []
        out, fc2 = self.msa_block.multi_head_attention.out_proj, self.mlp_block.mlp[3]
        return [(out.weight, out.bias, self.layer_scale_1), (fc2.weight, fc2.bias, self.layer_scale_2)]


class ViT(nn.Module):
    """ViT-Base/16 by default (reference models/vit.py:172-236)."""

    def __init__(self, image_size: int = 224, patch_size: int = 16, num_transformer_layer: int = 12,
                 num_heads: int = 12, embedding_dim: int = 768, mlp_size: int = 3072, attn_dropout: float = 0,
                 mlp_dropout: float = 0.1, embedding_dropout: float = 0.1, num_classes: int = 1000):
        super().__init__()
        self.patch_embedding_block = PatchEmbedding(image_size=image_size, patch_size=patch_size,
                                                    embedding_dim=embedding_dim, embedding_dropout=embedding_dropout)
        self.transformer_encoder = nn.Sequential(*[
            TransformerEncoderBlock(embedding_dim=embedding_dim, num_heads=num_heads, attn_dropout=attn_dropout,
                                    mlp_size=mlp_size, mlp_dropout=mlp_dropout)
            for _ in range(num_transformer_layer)])
        self.layer_norm = nn.LayerNorm(normalized_shape=embedding_dim)
        self.classifier = nn.Sequential(nn.Linear(in_features=embedding_dim, out_features=num_classes))
        self.config = dict(image_size=image_size, patch_size=patch_size, num_transformer_layer=num_transformer_layer,
                           num_heads=num_heads, embedding_dim=embedding_dim, mlp_size=mlp_size,
                           attn_dropout=attn_dropout, mlp_dropout=mlp_dropout, embedding_dropout=embedding_dropout,
                           num_classes=num_classes)

    # ------------------------------------------------------------------ reference path
    def forward_features(self, x: torch.Tensor) -> torch.Tensor:
        x = self.patch_embedding_block(x)
        x = self.transformer_encoder(x)
        return self.layer_norm(x)

    def forward(self, x: torch.Tensor, geom: Optional[torch.Tensor] = None, mix=None, erase=None, color=None) -> torch.Tensor:
        """``mix`` (optional :class:`~..data.batch_mix.MixPlan`, training or eval): mixup / CutMix of the
        batch as the model sees it, inside the patch-embedding kernels on the fused path and as
        ``data.batch_mix.mix_reference`` after the preprocessing elsewhere. ``None``: no mixing.

        ``erase`` (optional :class:`~..data.random_erasing.ErasePlan`, applied whenever it is passed, training
        or eval; nothing draws one implicitly): random erasing of each sample as the model sees it, before
        the mix, in the same kernels on the fused path (a ``"pixel"`` plan draws its noise from the step's
        value of the dropout counter) and as ``data.random_erasing.erase_reference`` between the
        preprocessing and the mix elsewhere. ``None``: no erasing.

        ``color`` (optional :class:`~..data.color_augment.ColorPlan`, applied whenever it is passed; in training
        mode the model draws one from ``DeviceInput.color`` when that is set): colour augmentation of the raw
        uint8 source batch, before everything else (the crop included), by the kernels of ``csrc/color.hip`` on
        the fused path and as ``data.color_augment.color_reference`` elsewhere. It needs a uint8 batch and
        :meth:`set_device_input`. ``None``: none."""
        x = self._color_stage(x, color)
        x, pre = self._device_input(x, geom)
        if _ext.use_fused(x) and self._fused_supported(x, pre):
            return self._forward_fused(x, pre, mix, erase)
        x = self._mix_reference(self._erase_reference(self._preprocess_reference(x, pre), erase), mix)
        x = self.forward_features(x)
        return self.classifier(x[:, 0])

    # ------------------------------------------------------------------ classifier bias
    def init_head_bias(self, value: float) -> "ViT":
        """Fill the classifier's bias with ``value`` (nothing else changes). For a sigmoid loss
        (:class:`~..losses.BinaryCrossEntropy`) the usual choice is ``-log(C)``: every class then starts at
        probability ``1 / (1 + C)`` instead of ``1 / 2``. The in-place write advances the parameter's version
        counter, which is how the flat store sees any outside write: its bf16 shadow counts as stale and is
        rebuilt before the next fused forward."""
        with torch.no_grad():
            self.classifier[0].bias.fill_(float(value))
        return self

    # ------------------------------------------------------------------ stochastic depth
    def set_drop_path(self, rate: float, schedule: str = "linear") -> "ViT":
        """Stochastic depth (drop path; Huang et al. 2016, the DeiT / ViT from-scratch recipes): in training,
        each sample drops each residual branch of block ``i`` independently with probability ``p_i`` and
        a kept branch is scaled by ``1 / (1 - p_i)``; ``p_i = rate * i / (L - 1)`` (``schedule="linear"``,
        ``p_0 = 0``; ``rate`` itself for a single block) or ``rate`` for every block (``"constant"``).
        Eval and inference never drop. ``rate = 0`` turns it off: the model then runs exactly as before.

        On the fused path the keep decisions come from the counter hash of the dropout masks (sites
        ``DROP_PATH_SITE + 2 i`` / ``+ 2 i + 1``, the step's value of the device counter), inside the
        out-projection and fc2 GEMM epilogues; elsewhere the same formula draws from torch's RNG. Not
        with :meth:`enable_fp8`. The constructor signature and ``state_dict()`` are unchanged; the rate
        is kept in ``config["drop_path"]`` (and the schedule in ``config["drop_path_schedule"]``)."""
        rates = drop_path_rates(rate, len(self.transformer_encoder), schedule)
        for blk, p in zip(self.transformer_encoder, rates):
            blk.drop_path = p
        self.config["drop_path"] = float(rate)
        self.config["drop_path_schedule"] = schedule
        return self

    def drop_path_rates(self):
        """The per-block rates in effect (all 0 without :meth:`set_drop_path`)."""
        return [float(getattr(blk, "drop_path", 0.0)) for blk in self.transformer_encoder]

    # ------------------------------------------------------------------ LayerScale
    def set_layer_scale(self, init_values: Optional[float]) -> "ViT":
        """LayerScale (Touvron et al. 2021, "Going deeper with Image Transformers"; every block of DeiT-III): a
        learnable per-channel vector on each residual branch, ``x = x + g1 * MSA(LN(x))``, ``x = x + g2 * MLP(LN(x))``.
        Registers ``layer_scale_1`` and ``layer_scale_2`` (``nn.Parameter [D]`` filled with ``init_values``; DeiT-III
        uses ``1e-4``) on every encoder block, so ``state_dict()`` grows from 152 to ``152 + 2 L`` keys; ``None``
        removes them again and the model is what it was. The constructor signature is unchanged; the value is
        kept in ``config["layer_scale"]``. 1-D parameters: ``param_groups_weight_decay`` does not decay them.

        Call it before the optimizer is built and before the first fused forward (the flat parameter store lays
        the parameters out once): with a store already covering the model it raises ``RuntimeError``.

        On the fused path the scale is folded into the branch's last Linear (the out-projection, fc2): once per
        weight change one kernel writes bf16 ``diag(g) W`` (row-major and transposed) and fp32 ``g * b``
        (``csrc/layerscale.hip``), every forward and dgrad GEMM reads those, and in the backward an unfold kernel
        turns the gradients of the folded pair into those of ``W``, ``b`` and ``g``. Dropout and drop path are
        element and row factors and commute with ``g``. Not with :meth:`enable_fp8`.
        :meth:`folded_state_dict` exports the plain model that computes the same function."""
        st = getattr(self, "_pvr_store", None)
        if st is not None and st.covers(self):
            raise RuntimeError("set_layer_scale() must run before the first fused forward and before the optimizer is "
                               "built: a ParamStore already covers this model's parameters")
        for blk in self.transformer_encoder:
            like = blk.msa_block.layer_norm.weight
            for name in ("layer_scale_1", "layer_scale_2"):
                if name in blk._parameters:
                    del blk._parameters[name]
                if init_values is not None:
                    blk.register_parameter(name, nn.Parameter(torch.full_like(like.detach(), float(init_values))))
        if init_values is None:
            self.config.pop("layer_scale", None)
        else:
            self.config["layer_scale"] = float(init_values)
        return self

    def has_layer_scale(self) -> bool:
        return any(getattr(blk, "layer_scale_1", None) is not None for blk in self.transformer_encoder)

    def folded_state_dict(self) -> dict:
        """The ``state_dict()`` of the plain model (no ``layer_scale_*`` keys: 152 for a classifier) that computes
        this model's function: each block's out-projection and fc2 hold ``g[:, None] * W`` and ``g * b``, one
        multiply in the parameters' dtype. The deployment export of a LayerScale model (detached copies);
        without the option a copy of ``state_dict()``."""
        sd = {k: v.detach().clone() for k, v in self.state_dict().items() if ".layer_scale_" not in k}
        for i, blk in enumerate(self.transformer_encoder):
            names = (f"transformer_encoder.{i}.msa_block.multi_head_attention.out_proj", f"transformer_encoder.{i}.mlp_block.mlp.3")
            for (w, b, g), name in zip(blk.folded_triples(), names):
                sd[name + ".weight"] = g.detach()[:, None] * w.detach()
                sd[name + ".bias"] = g.detach() * b.detach()
        return sd

    # ------------------------------------------------------------------ patch dropout
    def set_patch_dropout(self, rate: float) -> "ViT":
        """Patch dropout (PatchDropout, Liu et al. 2022; the token subsetting of FLIP / MAE pre-training): in
        training every sample keeps a random ``n_keep = max(1, n_p - floor(rate * n_p))`` of its ``n_p`` patch
        tokens, in raster order, behind the class token (always kept), and the encoder runs at
        ``N' = n_keep + 1`` tokens: its cost falls by about the token ratio. ``rate`` is in ``[0, 1)``;
        ``rate = 0`` (or any rate with ``n_keep == n_p``) turns it off, and the model then runs exactly as
        before. ``model.eval()``, ``no_grad`` and ``inference_mode`` forwards never drop: their outputs are
        those of the same weights without the option. The classifier-free backbone
        (``models/vit_no_classifier.py``) returns ``[B, N', D]`` in training.

        On the fused path the subset comes from the counter hash of the dropout masks (site
        ``PATCH_DROP_SITE``, the step's value of the device counter, so graph replay, resume and DDP work):
        a sample keeps the ``n_keep`` patches with the smallest ``(hash, index)`` pairs; the patchify
        kernels gather only those, the position embedding is gathered to match, the dropout masks are those
        of the compact token index, and the patch-embedding backward scatters through the inverse table
        (the position-embedding gradient is exactly zero where no sample kept a patch). Elsewhere
        :meth:`PatchEmbedding._draw_patch_keep` draws the subset from torch's RNG. Not with
        :meth:`enable_fp8`. The constructor signature and ``state_dict()`` are unchanged; the rate is kept
        in ``config["patch_dropout"]``."""
        pe = self.patch_embedding_block
        n_keep = patch_keep_count(pe.number_of_patches, rate)
        pe.patch_keep = n_keep if n_keep < pe.number_of_patches else 0
        self.config["patch_dropout"] = float(rate)
        return self

    # ------------------------------------------------------------------ resolution
    def set_image_size(self, image_size: int, mode: str = "bicubic") -> "ViT":
        """Change the model's input resolution, as the paper does between pre-training and fine-tuning: the
        patch rows of ``position_embedding`` are resampled in 2-D from the old ``g x g`` patch grid to the new
        one (:func:`resize_position_embedding`: ``F.interpolate(..., mode=mode, align_corners=False)`` on the
        fp32 ``[1, D, g, g]`` view; ``mode`` is ``"bicubic"`` or ``"bilinear"``) and the class-token row is
        copied. The parameter is replaced by one of the new shape, ``number_of_patches`` and
        ``config["image_size"]`` follow, a patch-dropout rate is re-applied to the new patch count; the
        constructor signature and the state-dict keys are unchanged. The same size is a no-op that keeps
        the parameter and its bits.

        Call it before the optimizer is built and before the first fused forward: with a ``ParamStore``
        already covering the model it raises ``RuntimeError``. ``ValueError`` for a size the patch size does
        not divide."""
        pe = self.patch_embedding_block
        P = int(pe.patch_size)
        image_size = int(image_size)
        if image_size <= 0 or image_size % P != 0:
            raise ValueError(f"image size {image_size} is not a positive multiple of the patch size {P}")
        if mode not in RESIZE_MODES:
            raise ValueError(f"mode must be one of {RESIZE_MODES}, got {mode!r}")
        g_new = image_size // P
        if g_new * g_new == pe.number_of_patches and image_size == self.config["image_size"]:
            return self
        st = getattr(self, "_pvr_store", None)
        if st is not None and st.covers(self):
            raise RuntimeError("set_image_size() must run before the first fused forward and before the optimizer is "
                               "built: a ParamStore already covers this model's parameters")
        old = pe.position_embedding
        new = resize_position_embedding(old.detach(), g_new, mode)
        pe.position_embedding = nn.Parameter(new, requires_grad=old.requires_grad)
        pe.number_of_patches = g_new * g_new
        self.config["image_size"] = image_size
        if self.config.get("patch_dropout"):
            self.set_patch_dropout(self.config["patch_dropout"])
        return self

    # ------------------------------------------------------------------ uint8 input
    def set_device_input(self, spec) -> "ViT":
        """Accept raw ``uint8 [B, 3, Hs, Ws]`` batches (contiguous or ``channels_last``): ``spec`` is a
        :class:`~..data.device_input.DeviceInput` (``None`` turns it off again). Scale to [0, 1],
        normalisation with ``spec.mean`` / ``spec.std`` and a per-sample crop box ``geom`` resampled to
        the model's image size run inside the patch-embedding kernel (``im2col_u8``) on the fused
        path, and as the same fp32 torch ops (``data.device_input.preprocess_reference``) elsewhere.

        ``forward(x, geom=None)``: an explicit ``geom`` (float32 ``[B, 4]`` rows ``(x0, y0, x1, y1)`` in
        source pixel-edge coordinates, ``x0 > x1`` = flipped) is used as given; in training mode with
        ``spec.augment`` set the model draws one box per sample from it on the host; otherwise the
        whole source is resized (nothing at all when the sizes match). The resampling is bilinear
        without antialiasing: sources more than ~2x the output size alias.

        Float inputs, and uint8 inputs without a spec, run exactly as before."""
        object.__setattr__(self, "_device_input_spec", spec)
        return self

    def _device_input(self, x: torch.Tensor, geom: Optional[torch.Tensor]):
        """``(x, pre)``: ``pre`` is None for the float path, else ``(mean, std, geom or None)`` of a
        uint8 batch to preprocess on the device (geom already there, float32 ``[B, 4]``)."""
        spec = getattr(self, "_device_input_spec", None)
        if spec is None or x.dtype != torch.uint8:
            if geom is not None:
                raise ValueError("forward(geom=...) needs a uint8 batch and set_device_input(spec)")
            return x, None
        if x.dim() != 4:
            raise ValueError(f"uint8 input must be [B, C, Hs, Ws], got {tuple(x.shape)}")
        B, C, Hs, Ws = x.shape
        S = self.config["image_size"]
        mean, std = spec.mean_std(C)
        if geom is None:
            if self.training and spec.augment is not None:
                if x.is_cuda and torch.cuda.is_current_stream_capturing():
                    raise RuntimeError("device-input augmentation draws its crop boxes on the host every step: it cannot "
                                       "run inside a graph capture (a replay would reuse one draw); pass geom explicitly "
                                       "or train without --graph")
                geom = spec.augment.sample(B, Hs, Ws)
                if x.is_cuda:
                    geom = geom.pin_memory()
            elif (Hs, Ws) != (S, S):
                from ..data.device_input import full_box

                geom = full_box(B, Hs, Ws)
        if geom is not None:
            if tuple(geom.shape) != (B, 4):
                raise ValueError(f"geom must be [{B}, 4] (x0, y0, x1, y1) rows, got {tuple(geom.shape)}")
            geom = geom.to(device=x.device, dtype=torch.float32, non_blocking=True).contiguous()
        return x, (mean, std, geom)

    def _color_stage(self, x: torch.Tensor, color) -> torch.Tensor:
        """The colour stage of ``forward(color=...)`` on the raw batch: ``x`` itself without a plan (an explicit
        one, or in training mode a draw from ``DeviceInput.color``), else a new uint8 batch of the same layout."""
        spec = getattr(self, "_device_input_spec", None)
        u8 = spec is not None and x.dtype == torch.uint8
        if color is None:
            sampler = getattr(spec, "color", None) if u8 and self.training else None
            if sampler is None:
                return x
            color = sampler.sample(x.shape[0])  # raises under a stream capture: a replay would reuse one draw
        elif not u8:
            raise ValueError("forward(color=...) needs a uint8 batch and set_device_input(spec)")
        if x.dim() != 4:
            raise ValueError(f"uint8 input must be [B, C, Hs, Ws], got {tuple(x.shape)}")
        color.check(x.shape[0])
        if _ext.use_fused(x):  # the stage does not depend on the model's shape
            from ..ops.fused_vit import color_u8

            return color_u8(x, color)
        from ..data.color_augment import color_reference

        return color_reference(x, color)

    def _preprocess_reference(self, x: torch.Tensor, pre) -> torch.Tensor:
        if pre is None:
            return x
        from ..data.device_input import preprocess_reference

        S = self.config["image_size"]
        return preprocess_reference(x, pre[0], pre[1], pre[2], (S, S))

    @staticmethod
    def _erase_reference(x: torch.Tensor, erase) -> torch.Tensor:
        if erase is None:
            return x
        from ..data.random_erasing import erase_reference

        return erase_reference(x, erase)  # "pixel" mode: the noise comes from torch's RNG here

    @staticmethod
    def _mix_reference(x: torch.Tensor, mix) -> torch.Tensor:
        if mix is None:
            return x
        from ..data.batch_mix import mix_reference

        return mix_reference(x, mix)

    # ------------------------------------------------------------------ fused path
    def _fused_supported(self, x: torch.Tensor, pre=None) -> bool:
        c = self.config
        D, H = c["embedding_dim"], c["num_heads"]
        if x.dim() != 4 or x.shape[1] != 3 or D % H != 0 or D // H not in (64, 80, 96, 128) or D % 64 != 0:
            return False
        if c["mlp_size"] % 64 != 0:
            return False
        P = c["patch_size"]
        if pre is not None:  # uint8 input: the kernel produces image_size x image_size from any source size
            return c["image_size"] % P == 0
        return x.shape[2] == x.shape[3] == c["image_size"] and x.shape[2] % P == 0

    @staticmethod
    def _rank_offset() -> int:
        # per-rank offset of the dropout counter: DDP ranks draw different masks from one base
        dist = torch.distributed
        rank = dist.get_rank() if dist.is_available() and dist.is_initialized() else 0
        return rank * 40503

    def _dropout_seed(self, device) -> torch.Tensor:
        rng = getattr(self, "_pvr_rng", None)
        if rng is not None and rng.device != device:
            with torch.inference_mode(False):  # e.g. restored on the CPU before .cuda(): keep the counter
                rng = rng.to(device)
            object.__setattr__(self, "_pvr_rng", rng)
        if rng is None:
            with torch.inference_mode(False):
                base = int(torch.randint(0, 2 ** 31 - 1, (1,)).item())
                rng = torch.tensor([base * 2654435761 + self._rank_offset()], dtype=torch.int64, device=device)
            object.__setattr__(self, "_pvr_rng", rng)
        seed = torch.empty_like(rng)
        _ext.ext().rng_next(rng, seed)  # seed = rng; rng += 1 (one device kernel, graph-replay safe)
        return seed

    def _forward_fused(self, x: torch.Tensor, pre=None, mix=None, erase=None) -> torch.Tensor:
        from ..ops.fused_vit import HeadFn

        # the head reads token 0 only: the last block may return the class-token rows alone ([B, D])
        tokens, store, B, N = self._fused_encoder(x, pre, cls_rows=True, mix=mix, erase=erase)
        head = self.classifier[0]
        return HeadFn.apply(tokens, B, N if tokens.shape[0] == B * N else 1, self.layer_norm.eps, store, self.layer_norm.weight, self.layer_norm.bias,
                            head.weight, head.bias)

    def _fused_encoder(self, x: torch.Tensor, pre=None, cls_rows: bool = False, mix=None, erase=None):
        """Patch embedding + every encoder block on the fused path: (bf16 tokens [B*N, D], store, B, N).
        Shared by this model's head and the classifier-free backbone (models/vit_no_classifier.py).
        ``cls_rows`` (a caller that reads token 0 of each image only): the last block may run on the
        class-token rows alone (ops/fused_vit.py ``CLS_LAST_BLOCK``), and ``tokens`` is then ``[B, D]``.
        ``pre`` = ``(mean, std, geom)`` of a uint8 batch (:meth:`_device_input`), None for a float one.
        ``mix``: the batch's ``MixPlan`` (None: none), applied by the patchify kernel. ``erase``: the batch's
        ``ErasePlan`` (None: none), likewise; a "pixel" plan takes the step's counter value even when nothing
        else draws from it (every dropout at 0, or an evaluation forward)."""
        from ..ops.fused_vit import (ATTN_SITE, DROP_PATH_SITE, EncoderBlockClsFn, EncoderBlockFn, PatchEmbedFn, PatchEmbedU8Fn,
                                     block_links, cls_last_block_ok, site_drop)
        from ..runtime.param_store import get_store

        c = self.config
        dev = x.device
        # (a rate whose 16-bit threshold is 0 never drops and scales by 1: such a block runs as one without)
        dp_rates = [p if self.training and drop_path_thr(p) > 0 else 0.0 for p in self.drop_path_rates()]
        if any(p > 0 for p in dp_rates) and getattr(self, "_fp8_cfg", None) is not None:
            raise NotImplementedError(
                "enable_fp8() does not combine with set_drop_path(): the fp8 gradient copies of the out-projection and "
                "fc2 dgrads would have to be taken from the drop-path-scaled gradients; turn one of the two off")
        pe = self.patch_embedding_block
        n_keep = pe.patch_keep_active()  # patch dropout: patches per sample this forward keeps (0: all)
        if n_keep and getattr(self, "_fp8_cfg", None) is not None:
            raise NotImplementedError(
                "enable_fp8() does not combine with set_patch_dropout(): the fp8 scaling state is sized by the token "
                "count, which would differ between training and evaluation; turn one of the two off")
        layer_scale = self.has_layer_scale()
        if layer_scale and getattr(self, "_fp8_cfg", None) is not None:
            raise NotImplementedError(
                "enable_fp8() does not combine with set_layer_scale(): the fp8 weight copies of the out-projection and "
                "fc2 would have to be taken from the folded weights; turn one of the two off")
        for p in self.parameters():
            if p.device != dev:
                raise RuntimeError(f"input is on {dev} but model parameters are on {p.device}")
        store = get_store(self, dev)
        store.join_side()
        store.refresh_shadow()
        if not getattr(store, "_vit_t_registered", False):
            store.register_transposed([w for blk in self.transformer_encoder for w in blk.fused_params()[2:12:2] if w.dim() == 2])
            store._vit_t_registered = True
        store.ensure_transposed()
        if layer_scale:
            # LayerScale: the folded copies of the out-projections and fc2 follow the shadows (one launch per
            # optimizer step or weight exchange, none while ``store.generation`` stands still)
            if not getattr(store, "_vit_fold_registered", False):
                store.register_folded([t for blk in self.transformer_encoder for t in blk.folded_triples()])
                store._vit_fold_registered = True
            store.fold()
        training = self.training
        grad = torch.is_grad_enabled()
        store.grad_enabled = grad  # the fused Functions' forward runs with grad mode off: tell them
        if grad:
            store.prepare_grads()
        need_seed = training and (c["mlp_dropout"] > 0 or c["embedding_dropout"] > 0 or c["attn_dropout"] > 0
                                  or any(p > 0 for p in dp_rates) or n_keep > 0)
        need_seed = need_seed or (erase is not None and erase.mode == "pixel")
        seed = self._dropout_seed(dev) if need_seed else None
        conv = pe.patch_and_flatten[0]
        if pre is None:
            tokens = PatchEmbedFn.apply(x, c["patch_size"], store, seed, pe.dropout.p, training,
                                        conv.weight, conv.bias, pe.class_token, pe.position_embedding, mix, n_keep, erase)
        else:
            mean, std, geom = pre
            tokens = PatchEmbedU8Fn.apply(x, geom, mean, std, (c["image_size"], c["image_size"]), c["patch_size"], store, seed,
                                          pe.dropout.p, training, conv.weight, conv.bias, pe.class_token,
                                          pe.position_embedding, mix, n_keep, erase)
        B = x.shape[0]
        N = (n_keep or pe.number_of_patches) + 1  # the encoder's tokens per sample
        f8 = self._fp8_state(dev, B * N)
        if f8 is not None:
            f8.begin_step(training)
        blocks = list(self.transformer_encoder)
        drops2 = [site_drop(seed, 2 + 2 * i, blk.mlp_block.mlp[4].p, training) for i, blk in enumerate(blocks)]
        # drop path: the MLP-branch site of block i rides in its link (the next block's LayerNorm backward applies it)
        dps2 = [site_drop(seed, DROP_PATH_SITE + 2 * i + 1, dp_rates[i], training) for i in range(len(blocks))]
        links = block_links(blocks, drops2, dps2)
        for i, blk in enumerate(blocks):
            ln1 = blk.msa_block.layer_norm
            ln2 = blk.mlp_block.layer_norm
            mha = blk.msa_block.multi_head_attention
            drops = (site_drop(seed, 1 + 2 * i, blk.mlp_block.mlp[2].p, training), drops2[i],
                     site_drop(seed, ATTN_SITE + i, mha.dropout, training))
            if dp_rates[i] > 0:  # rate 0: the 3-tuple of the code path without drop path
                drops = drops + (site_drop(seed, DROP_PATH_SITE + 2 * i, dp_rates[i], training), dps2[i])
            if cls_rows and i == len(blocks) - 1 and cls_last_block_ok(N, mha.num_heads, c["embedding_dim"], f8, drops[2]):
                tokens = EncoderBlockClsFn.apply(tokens, B, N, mha.num_heads, ln1.eps, ln2.eps, store, drops, links[i],
                                                 *blk.fused_params())
                break
            tokens = EncoderBlockFn.apply(tokens, B, N, mha.num_heads, ln1.eps, ln2.eps, store, drops,
                                          None if f8 is None else (f8, i), links[i], *blk.fused_params())
        return tokens, store, B, N

    # ------------------------------------------------------------------ fp8
    def enable_fp8(self, enabled: bool = True, history: int = 16, margin: int = 0, dgrad: bool = True,
                   wgrad: bool = True, grad_fmt: str = "e4m3") -> "ViT":
        """Run the encoder's GEMMs in fp8 on the fused MI355X path (ops/fp8.py), per-tensor delayed
        scaling with an amax history of ``history`` steps:

        * forward GEMMs: e4m3 activations x e4m3 weights;
        * ``dgrad=True`` (default): the backward's activation-gradient GEMMs too, e5m2 gradients x
          e4m3 transposed weights. This changes the backward numerics (``tests/kernel_checks.py``
          ``check_vit_fp8_dgrad`` pins the per-tensor error); ``dgrad=False`` keeps them bf16;
        * ``wgrad=True`` (default, with ``dgrad``): the weight-gradient GEMMs too, e5m2 gradients^T x
          e4m3 activations^T (transposed quantize passes with the same slots' scales) from the second
          step on (``check_vit_fp8_wgrad`` pins the per-tensor error, 1-8 % rel-L2 per weight
          gradient); ``wgrad=False`` keeps them bf16 (20 % of the ViT-H/14 fp8 throughput). Round 5
          made it opt-in on a 3-seed study that could not discriminate; round 6's 6-seed ViT-H/14 study
          (``profiles/r6/fp8_study/stats.md``, windowed training loss at steps 200 / 400 / 600 of a
          1000-step schedule, paired by seed) finds both fp8 variants within one bf16 standard
          deviation at every checkpoint and no significant paired difference (p 0.08-0.33), with the
          fp8 means 6-29 % above bf16's at steps 400 / 600: a trend more seeds would be needed to
          confirm or rule out;
        * ``grad_fmt``: the gradients' fp8 format in the dgrad / wgrad GEMMs, ``"e4m3"`` (default
          since round 6) or ``"e5m2"``. Round 6 measured the weight-gradient GEMM error on captured
          ViT-B/16 operands (``profiles/r6/mx_study``): the error comes from e5m2's 2-bit mantissa;
          per-32-element MX block scales change nothing. With e4m3 gradients (same per-tensor delayed
          scaling) the mean per-tensor error of all encoder gradients against the bf16 backward halves
          (0.036 vs 0.072, ``check_vit_fp8_grad_formats``), and in the 6-seed ViT-H/14 study
          (``profiles/r6/e4m3_study/stats.md``) the e4m3 run is closer to bf16 at every checkpoint (the
          one significant fp8 gap, e5m2 at step 400, p 0.008, is gone: p 0.135). The format is a
          runtime argument of every kernel that writes a gradient copy (the dgrad epilogues, LayerNorm
          backward, attention backward, column sums), so both formats run at the same speed;
        * attention, LayerNorm, the patch embedding / head GEMMs and the optimizer stay bf16 / fp32.

        The constructor signature stays the reference's; fp8 is opt-in."""
        old = getattr(self, "_fp8_cfg", None)
        if grad_fmt not in ("e5m2", "e4m3"):
            raise ValueError(f"enable_fp8: grad_fmt must be 'e5m2' or 'e4m3', got {grad_fmt!r}")
        cfg = (history, margin, bool(dgrad), bool(wgrad), grad_fmt) if enabled else None
        object.__setattr__(self, "_fp8_cfg", cfg)
        if cfg is None or old is None or old[:2] != cfg[:2] or old[4:] != cfg[4:]:
            object.__setattr__(self, "_fp8", None)  # new scaling state; only a dgrad switch keeps the histories
        return self

    def _fp8_state(self, device, tokens: int):
        cfg = getattr(self, "_fp8_cfg", None)
        if cfg is None:
            return None
        from ..ops import fp8 as F8

        c = self.config
        if not F8.supported(tokens, c["embedding_dim"], c["mlp_size"]):
            return None
        st = getattr(self, "_fp8", None)
        if st is None or st.device != device:
            old_sd = st.state_dict() if st is not None else getattr(self, "_fp8_pending", None)
            st = F8.Fp8State(c["num_transformer_layer"], device, history=cfg[0], margin=cfg[1], dgrad=cfg[2], wgrad=cfg[3],
                             grad_fmt=F8.E4M3 if cfg[4] == "e4m3" else F8.E5M2)
            if old_sd is not None:  # restored (or built) on another device: carry the scaling state over
                st.load_state_dict(old_sd)
            object.__setattr__(self, "_fp8", st)
            object.__setattr__(self, "_fp8_pending", None)
        st.dgrad = cfg[2]
        st.wgrad = cfg[3] and cfg[2]
        return st

    # ------------------------------------------------------------------ resume state
    def runtime_state_dict(self) -> dict:
        """Fused-path state outside ``state_dict()`` that a bit-exact resume needs (CPU tensors, loads
        with ``weights_only=True``): the device dropout counter (next seed of the counter-based masks)
        and the fp8 delayed-scaling state (amax histories, scales, calibration flags)."""
        out = {}
        rng = getattr(self, "_pvr_rng", None)
        if rng is not None:
            # rank-free: every DDP rank re-adds its own offset on load (rank 0 writes the checkpoint)
            out["dropout_rng"] = rng.detach().cpu().clone() - self._rank_offset()
            out["dropout_rng_rank_free"] = torch.ones(1, dtype=torch.int64)
        st = getattr(self, "_fp8", None)
        if st is not None:
            out["fp8"] = st.state_dict()
        return out

    def load_runtime_state_dict(self, sd: dict, device=None) -> None:
        """Restore :meth:`runtime_state_dict` (``device``: where the fused path will run; default the
        parameters' device). The fp8 state needs ``enable_fp8`` with the same history first."""
        dev = torch.device(device) if device is not None else next(self.parameters()).device
        if "dropout_rng" in sd:
            rng = sd["dropout_rng"].to(dtype=torch.int64).clone()
            if "dropout_rng_rank_free" in sd:
                rng += self._rank_offset()
            object.__setattr__(self, "_pvr_rng", rng.to(dev))  # moved to the forward's device on first use
        if "fp8" in sd:
            cfg = getattr(self, "_fp8_cfg", None)
            if cfg is None:
                raise RuntimeError("checkpoint holds fp8 scaling state: call enable_fp8(...) before loading it")
            if dev.type != "cuda":
                # the fused path builds its fp8 state on the forward's device: apply it there
                object.__setattr__(self, "_fp8", None)
                object.__setattr__(self, "_fp8_pending", sd["fp8"])
                return
            from ..ops import fp8 as F8

            st = getattr(self, "_fp8", None)
            if st is None or st.device != dev:
                st = F8.Fp8State(self.config["num_transformer_layer"], dev, history=cfg[0], margin=cfg[1],
                                 dgrad=cfg[2], wgrad=cfg[3], grad_fmt=F8.E4M3 if cfg[4] == "e4m3" else F8.E5M2)
                object.__setattr__(self, "_fp8", st)
            st.load_state_dict(sd["fp8"])

    def num_params(self) -> int:
        return sum(p.numel() for p in self.parameters())
