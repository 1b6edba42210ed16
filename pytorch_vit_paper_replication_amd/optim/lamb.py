"""FusedLamb: LAMB (You et al. 2019, "Large Batch Optimization for Deep Learning") on the flat parameter
store. Adam's update, rescaled per parameter tensor by the trust ratio ``||w|| / ||update||``: the
optimizer of the large-batch ViT recipes (DeiT-III), which keeps one learning rate across batch sizes
where Adam / AdamW need retuning.

Per parameter tensor ``w`` of a group at step ``t``, ``g`` the gradient after the global-norm clip::

    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    u = (m / (1 - b1^t)) / (sqrt(v) / sqrt(1 - b2^t) + eps) + wd * w
    r = ||w|| / ||u||   if (wd != 0 or always_adapt) and ||w|| > 0 and ||u|| > 0, else 1
    w = w - lr * r * u

The norms run over the whole tensor. A group with ``weight_decay == 0`` and ``always_adapt=False`` (the
bias / LayerNorm group of :func:`~.schedule.param_groups_weight_decay`) takes plain Adam steps, as in
the common implementations. No trust-ratio clipping, no ``amsgrad``, no ``maximize``.

It is a :class:`~.adam.FusedAdam`: the clip, ``ModelEma.attach``, ``graph_mode()``, the state dict
(``exp_avg``, ``exp_avg_sq``, ``step``) and checkpoints work as they do there. On the fused GPU path a step is the
two norm launches of the clip and three of csrc/lamb.hip (moments and per-chunk norm sums; per-tensor
trust ratios; the update with the bf16 shadow, W^T and the model EMA), with no host synchronisation;
``last_trust`` is then the device tensor ``[segments of the store, 3]`` of ``{||w||, ||u||, r}`` (rows of
frozen segments are never written). Elsewhere (CPU, ``PVR_DISABLE_FUSED=1``, parameters outside one
store) the same formula runs per tensor with torch ops in the parameters' dtype, and ``last_trust`` has
one row per parameter that had a gradient, in group order.
"""
from __future__ import annotations

import math
from typing import Optional

import torch

from .. import _ext
from .adam import FusedAdam

ALWAYS_ADAPT_BIT = 2  # csrc/kernels.h LAMB_ALWAYS_ADAPT


class FusedLamb(FusedAdam):
    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-6, weight_decay: float = 0.0,
                 always_adapt: bool = False, skip_nonfinite: bool = True):
        self._always_adapt_default = bool(always_adapt)
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, skip_nonfinite=skip_nonfinite)
        # LAMB's decay is part of the update the trust ratio scales: there is no decoupled variant
        self.defaults.pop("decoupled_weight_decay", None)
        self.defaults["always_adapt"] = self._always_adapt_default
        self.last_trust: Optional[torch.Tensor] = None
        self._lamb = None  # (fused tuple it was built for, chunks, seg_chunks, partial, trust)

    def add_param_group(self, param_group):
        if "decoupled_weight_decay" in param_group:
            raise ValueError("FusedLamb has no decoupled_weight_decay option: the decay is part of the update the trust ratio scales")
        super().add_param_group(param_group)
        g = self.param_groups[-1]
        g.pop("decoupled_weight_decay", None)
        g.setdefault("always_adapt", self._always_adapt_default)

    @staticmethod
    def _adapts(g) -> bool:
        return g["weight_decay"] != 0 or bool(g["always_adapt"])

    def _group_flags(self, g) -> int:
        return ALWAYS_ADAPT_BIT if g["always_adapt"] else 0

    # ------------------------------------------------------------------ fused path
    def _setup_fused(self):
        fz = super()._setup_fused()
        if fz is not None:
            self._lamb_tables(fz)  # built with the state, before any stream capture
        return fz

    def _lamb_tables(self, fz):
        """Chunk table of the norm pass, per-segment chunk ranges, the partial sums and the trust rows;
        rebuilt with the fused state (a new store, e.g. the DDP bucket re-layout, or a loaded state dict)."""
        if self._lamb is not None and self._lamb[0] is fz:
            return self._lamb[1:]
        store = fz[0]
        chunk = _ext.ext().lamb_chunk()
        mine = {id(p) for g in self.param_groups for p in g["params"]}
        chunks, seg_chunks = [], []
        for i, (p, off) in enumerate(zip(store.params, store.offsets)):
            first = len(chunks)
            if id(p) in mine and p.requires_grad:  # the segments whose seg_group is not -1
                n = (p.numel() + 3) // 4 * 4  # the store pads every segment (zeros add nothing to a norm)
                chunks.extend([off + c, min(chunk, n - c), i] for c in range(0, n, chunk))
            seg_chunks.append([first, len(chunks) - first])
        dev = store.device
        tabs = (torch.tensor(chunks, dtype=torch.int64, device=dev).reshape(-1, 3),
                torch.tensor(seg_chunks, dtype=torch.int64, device=dev).reshape(-1, 2),
                torch.zeros((len(chunks), 2), dtype=torch.float32, device=dev),
                torch.zeros((len(seg_chunks), 3), dtype=torch.float32, device=dev))
        self._lamb = (fz,) + tabs
        return tabs

    def _table_row_extra(self, store) -> dict:
        """The segment (trust row) of every weight and range: column 6 of a tile row, 4 of a flat one."""
        return {id(p): [i] for i, p in enumerate(store.params)}

    def _fused_update(self, fz, table, clip, ema_kw) -> None:
        store, m, v, seg_start, seg_group = fz[:5]
        chunks, seg_chunks, partial, trust = self._lamb_tables(fz)
        ext = _ext.ext()
        ext.lamb_moments(store.flat, store.grad_flat, m, v, chunks, seg_group, partial, table, clip, self.skip_nonfinite)
        ext.lamb_ratio(partial, seg_chunks, seg_group, trust, table, clip, self.skip_nonfinite)
        tt = self._transposed_tables(store)
        if tt is not None and tt[3] > 0:
            store.ensure_transposed()  # only if something else changed the weights since
            ext.lamb_update(store.flat, m, v, store.shadow, trust, table, clip, self.skip_nonfinite, shadow_t=store.shadow_t,
                            tmeta=tt[0], ntiles=tt[1], fmeta=tt[2], flat4=tt[3], **ema_kw)
            store.mark_shadow_fresh(transposed=True)
        else:
            ext.lamb_update(store.flat, m, v, store.shadow, trust, table, clip, self.skip_nonfinite, seg_start=seg_start,
                            seg_group=seg_group, **ema_kw)
            store.mark_shadow_fresh()
        self.last_trust = trust

    # ------------------------------------------------------------------ torch ops
    def _torch_update(self) -> None:
        rows = []
        for g in self.param_groups:
            b1, b2 = g["betas"]
            lr, eps, wd = g["lr"], g["eps"], g["weight_decay"]
            adapt = self._adapts(g)
            for p in g["params"]:
                if p.grad is None:
                    continue
                grad = p.grad
                st = self.state[p]
                if len(st) == 0 or "exp_avg" not in st:
                    st["step"] = torch.tensor(0.0)
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["step"] += 1
                t = float(st["step"])
                st["exp_avg"].lerp_(grad, 1 - b1)
                st["exp_avg_sq"].mul_(b2).addcmul_(grad, grad.conj(), value=1 - b2)
                bc1 = 1 - b1 ** t
                bc2 = 1 - b2 ** t
                denom = (st["exp_avg_sq"].sqrt() / math.sqrt(bc2)).add_(eps)
                wn = torch.linalg.vector_norm(p)
                if not adapt:  # FusedAdam's step at weight_decay 0, operation for operation
                    un = torch.linalg.vector_norm((st["exp_avg"] / bc1).div_(denom))
                    p.addcdiv_(st["exp_avg"], denom, value=-(lr / bc1))
                    r = torch.ones_like(wn)
                else:
                    u = (st["exp_avg"] / bc1).div_(denom)
                    if wd != 0:
                        u.add_(p, alpha=wd)
                    un = torch.linalg.vector_norm(u)
                    r = torch.where((wn > 0) & (un > 0), wn / un, torch.ones_like(wn))
                    p.sub_(u.mul_(lr * r))
                rows.append(torch.stack([wn, un, r]))
        self.last_trust = torch.stack([x.to(rows[0].dtype) for x in rows]) if rows else None
