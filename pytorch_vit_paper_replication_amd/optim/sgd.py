"""FusedSGD: ``torch.optim.SGD`` semantics (momentum, weight decay, Nesterov; no dampening), one HIP pass over
the flat parameter store. The paper fine-tunes every model with SGD, momentum 0.9, no weight decay, a
global-norm clip of 1 and cosine decay (:func:`~.schedule.warmup_cosine_decay`).

Per element of a group, ``c`` the clip coefficient of the step (1 without a clip)::

    g' = g * c
    g' = g' + weight_decay * p                 (only where weight_decay != 0)
    buf = momentum * buf + g'                  (only where momentum != 0; buf starts at zero, so the first
                                                step gives buf = g', torch's clone)
    d  = g' + momentum * buf  if nesterov else buf        (d = g' where momentum == 0)
    p  = p - lr * d

It is a :class:`~.adam.FusedAdam` in everything but the update: ``clip_grad_norm_``, ``step(clip_norm=)``,
``zero_grad``, ``ModelEma.attach``, ``graph_mode()`` / ``graph_prepare()`` and the pinned table ring work as
they do there. On the fused GPU path a step is the two norm launches of the clip and one of csrc/sgd.hip,
which writes the fp32 master, the momentum buffer, the bf16 shadow, the transposed bf16 shadow W^T of the
2-D encoder weights and, with a model EMA attached, the EMA, with no host synchronisation. The state is
one flat fp32 buffer (Adam keeps two: 4 bytes per parameter less); ``state[p]["momentum_buffer"]`` is a
view into it, present exactly for parameters of groups with non-zero momentum, so ``state_dict()``
interchanges with ``torch.optim.SGD``'s in both directions. The kernel neither reads nor writes the
buffer of a group with ``momentum == 0``.

Elsewhere (CPU, ``PVR_DISABLE_FUSED=1``, parameters outside one store) torch's single-tensor SGD math runs
per tensor. ``dampening != 0`` and ``maximize`` are not supported.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from .. import _ext
from .adam import GROUP_COLS, FusedAdam

NESTEROV_BIT = 4  # csrc/kernels.h SGD_NESTEROV


class FusedSGD(FusedAdam):
    def __init__(self, params, lr: float = 1e-3, momentum: float = 0.0, weight_decay: float = 0.0, nesterov: bool = False,
                 skip_nonfinite: bool = True, dampening: float = 0.0, maximize: bool = False):
        if dampening != 0 or maximize:
            raise NotImplementedError("FusedSGD supports neither dampening nor maximize")
        if lr < 0.0 or momentum < 0.0 or weight_decay < 0.0:
            raise ValueError(f"lr, momentum and weight_decay must be >= 0, got {lr}, {momentum}, {weight_decay}")
        self._sgd_defaults = dict(momentum=momentum, nesterov=bool(nesterov))
        super().__init__(params, lr=lr, weight_decay=weight_decay, skip_nonfinite=skip_nonfinite)
        for k in ("betas", "eps", "decoupled_weight_decay"):
            self.defaults.pop(k, None)
        # torch.optim.SGD's group keys, so a state dict of either loads into the other
        self.defaults.update(momentum=momentum, dampening=0, nesterov=bool(nesterov), maximize=False)
        self._sgd_tables = None  # (fused tuple they were built for, SgdTables of the segment form)
        self._sgd_ttables = None  # (FusedAdam._ttables they were built from, SgdTables of the tile form)

    def add_param_group(self, param_group):
        for k in ("betas", "eps", "decoupled_weight_decay"):
            if k in param_group:
                raise ValueError(f"FusedSGD has no {k} option")
        if param_group.get("dampening", 0) != 0 or param_group.get("maximize", False):
            raise NotImplementedError("FusedSGD supports neither dampening nor maximize")
        super().add_param_group(param_group)
        g = self.param_groups[-1]
        for k in ("betas", "eps", "decoupled_weight_decay"):
            g.pop(k, None)
        g.setdefault("momentum", self._sgd_defaults["momentum"])
        g.setdefault("nesterov", self._sgd_defaults["nesterov"])
        g.setdefault("dampening", 0)
        g.setdefault("maximize", False)
        if g["nesterov"] and g["momentum"] <= 0:
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")

    # ------------------------------------------------------------------ fused path
    def _setup_fused(self):
        params = self._all_params()
        if not params or not params[0].is_cuda or not _ext.available():
            return None
        from ..runtime.param_store import lookup_store

        store = lookup_store(params[0])
        if store is None or any(lookup_store(p) is not store for p in params):
            return None
        if not all(store.covers_param(p) for p in params):
            return None
        fz = self._fused
        if fz is not None and fz[0] is store:
            return fz
        dev = store.device
        group_of = {}
        for gi, g in enumerate(self.param_groups):
            for p in g["params"]:
                group_of[id(p)] = gi
        starts, groups = [], []
        for p, off in zip(store.params, store.offsets):
            starts.append(off)
            groups.append(group_of.get(id(p), -1) if p.requires_grad else -1)
        buf = torch.zeros(store.numel, dtype=torch.float32, device=dev)
        # carry over any existing per-tensor state (e.g. loaded from a checkpoint)
        for p, off in zip(store.params, store.offsets):
            st = self.state.get(p)
            if st and st.get("momentum_buffer") is not None:
                buf[off:off + p.numel()].copy_(st["momentum_buffer"].reshape(-1))
        for p, off in zip(store.params, store.offsets):
            gi = group_of.get(id(p))
            if gi is None:
                continue
            if self.param_groups[gi]["momentum"] != 0:
                self.state[p] = {"momentum_buffer": buf[off:off + p.numel()].view(p.shape)}
            else:
                self.state.pop(p, None)
        ws = torch.empty(_ext.ext().norm_partial_blocks(), dtype=torch.float32, device=dev)
        clip = torch.zeros(3, dtype=torch.float32, device=dev)
        seg_start = torch.tensor(starts, dtype=torch.int64)
        seg_group = torch.tensor(groups, dtype=torch.int32)
        # the same tuple shape FusedAdam keeps: (store, state, -, seg_start, seg_group, ws, clip)
        self._fused = (store, buf, None, seg_start, seg_group, ws, clip)
        # the kernel's tables, checked on the host once (csrc/bindings.cpp sgd_segments), before any capture
        self._sgd_tables = (self._fused, _ext.ext().sgd_segments(seg_start, seg_group, store.numel, dev))
        self._tmeta_key = None
        self._sgd_ttables = None
        return self._fused

    def _tile_tables(self, store):
        """The host-checked tables of the tile form, rebuilt with ``FusedAdam._transposed_tables``; None if the
        store keeps no W^T shadow."""
        tt = self._transposed_tables(store)
        if tt is None or tt[3] <= 0:
            return None
        if self._sgd_ttables is None or self._sgd_ttables[0] is not tt:
            tabs = _ext.ext().sgd_tiles(tt[0].cpu(), tt[2].cpu(), store.numel, store.shadow_t.numel(), store.device)
            self._sgd_ttables = (tt, tabs)
        return self._sgd_ttables[1]

    def graph_mode(self, enabled: bool = True, ring: int = 4) -> None:
        super().graph_mode(enabled, ring)
        if enabled:  # the tile tables' host check copies them once: before the capture, not inside it
            self._tile_tables(self._fused[0])

    def _group_array(self, step: int, arr: Optional[np.ndarray] = None) -> np.ndarray:
        """The kernels' group table (csrc/kernels.h AdamGroup rows as csrc/sgd.hip reads them): lr, the momentum in
        the beta1 column, weight_decay, the Nesterov bit in word 7; the other columns stay zero."""
        G = len(self.param_groups)
        if arr is None:
            arr = np.zeros((G, GROUP_COLS), dtype=np.float32)
        arr[:G] = 0.0
        for i, g in enumerate(self.param_groups):
            arr[i, 0] = float(g["lr"])
            arr[i, 1] = float(g["momentum"])
            arr[i, 4] = float(g["weight_decay"])
        arr.view(np.int32)[:, 7] = [self._group_flags(g) for g in self.param_groups]
        return arr

    def _group_flags(self, g) -> int:
        return NESTEROV_BIT if g["nesterov"] else 0

    def _check_groups(self) -> None:
        """Hyper-parameters changed after construction (a scheduler, user code) that the kernel cannot take."""
        for g in self.param_groups:
            if g.get("dampening", 0) != 0 or g.get("maximize", False):
                raise NotImplementedError("FusedSGD supports neither dampening nor maximize")
            if g["nesterov"] and g["momentum"] <= 0:
                raise ValueError("Nesterov momentum requires a momentum and zero dampening")

    def _fused_update(self, fz, table, clip, ema_kw) -> None:
        store, buf = fz[0], fz[1]
        ext = _ext.ext()
        self._check_groups()
        tiles = self._tile_tables(store)
        if tiles is not None:
            store.ensure_transposed()  # only if something else changed the weights since
            ext.sgd_t(store.flat, store.grad_flat, buf, store.shadow, store.shadow_t, tiles, table, clip, self.skip_nonfinite,
                      **ema_kw)
            store.mark_shadow_fresh(transposed=True)
        else:
            ext.sgd(store.flat, store.grad_flat, buf, store.shadow, self._sgd_tables[1], table, clip, self.skip_nonfinite, **ema_kw)
            store.mark_shadow_fresh()

    # ------------------------------------------------------------------ torch ops
    def _torch_update(self) -> None:
        """torch.optim.SGD's single-tensor math (dampening 0, maximize=False), operation for operation."""
        self._check_groups()
        for g in self.param_groups:
            lr, mom, wd, nesterov = g["lr"], g["momentum"], g["weight_decay"], g["nesterov"]
            for p in g["params"]:
                if p.grad is None:
                    continue
                grad = p.grad
                if wd != 0:
                    grad = grad.add(p, alpha=wd)
                if mom != 0:
                    st = self.state[p]
                    buf = st.get("momentum_buffer")
                    if buf is None:
                        buf = st["momentum_buffer"] = torch.clone(grad).detach()
                    else:
                        buf.mul_(mom).add_(grad)
                    grad = grad.add(buf, alpha=mom) if nesterov else buf
                p.add_(grad, alpha=-lr)

    def state_dict(self):
        return torch.optim.Optimizer.state_dict(self)
