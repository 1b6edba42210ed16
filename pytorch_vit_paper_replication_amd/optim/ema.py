"""ModelEma: an exponential moving average of the weights, updated inside the fused Adam pass.

    ema = ModelEma(model, decay=0.9999, warmup=False)
    ema.attach(optimizer)        # FusedAdam: step() updates the average in its own kernel
    ema.update()                 # any other optimizer / CPU / PVR_DISABLE_FUSED: torch ops, same formula
    with ema.applied():          # the model computes with the averaged weights
        ...
    ema.state_dict() / ema.load_state_dict(sd)

Every update is, per element of every trainable parameter,

    ema = decay * ema + (1 - decay) * p_new          (fp32)

with ``decay`` and ``1 - decay`` each rounded to fp32 from the double. The two-product form is exact at
both ends: ``decay = 0`` makes the average equal to the weights and ``decay = 1`` never moves it, bit for
bit. Frozen parameters (``requires_grad == False``) are not averaged; they keep their initial values.

On the fused GPU path the average is one flat fp32 buffer with the layout of the model's
``ParamStore`` (4 bytes per parameter: 0.34 GB at ViT-B/16, 2.5 GB at ViT-H/14). ``FusedAdam`` hands it
to ``adam_kernel`` / ``adam_t_kernel`` (csrc/optim.hip), where the new parameter value is in registers:
one more fp32 read and write per element, no launch. A step the kernel skips (a non-finite gradient
norm under ``skip_nonfinite``) leaves the average untouched too. The buffer is rebuilt from the
per-parameter values whenever the store or its layout changes (data-parallel training re-lays the store
out into bucket-aligned segments). Off the fused path the average is per-parameter fp32 tensors.

``warmup=True`` ramps the decay: the n-th update (n from 0) uses ``min(decay, (1 + n) / (10 + n))``.
``n`` is counted on the host, which cannot see a non-finite skip without a synchronisation, so the
counter advances on a skipped step as well.

Under data parallelism every rank holds the same all-reduced gradients, so every rank's average is the
same without communication; rank 0's goes into checkpoints.
"""
from __future__ import annotations

import contextlib
import weakref
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from .. import _ext


class ModelEma:
    def __init__(self, model: torch.nn.Module, decay: float = 0.9999, warmup: bool = False):
        if not 0.0 <= float(decay) <= 1.0:
            raise ValueError(f"decay must be in [0, 1], got {decay}")
        from ..runtime.param_store import unique_params

        self.module = getattr(model, "module", model)  # this package's DistributedDataParallel wraps .module
        self.decay = float(decay)
        self.warmup = bool(warmup)
        self.num_updates = 0
        self._names, self._params = unique_params(self.module)
        with torch.inference_mode(False), torch.no_grad():
            self._vals: Dict[int, torch.Tensor] = {id(p): p.detach().to(torch.float32, copy=True) for p in self._params}
        self._flat: Optional[torch.Tensor] = None
        self._flat_key = None
        self._optimizer = None  # weakref to the FusedAdam that updates this average in step()

    # ------------------------------------------------------------------ decay schedule
    def decay_at(self, n: int) -> float:
        return min(self.decay, (1.0 + n) / (10.0 + n)) if self.warmup else self.decay

    def pair_at(self, n: int) -> Tuple[np.float32, np.float32]:
        """(decay, 1 - decay) of update ``n``, each rounded to fp32 from the double."""
        d = self.decay_at(n)
        return np.float32(d), np.float32(1.0 - d)

    def next_pair(self) -> Tuple[np.float32, np.float32]:
        """This update's pair; advances the host counter."""
        pair = self.pair_at(self.num_updates)
        self.num_updates += 1
        return pair

    # ------------------------------------------------------------------ storage
    def _fused_store(self):
        """The ParamStore that holds exactly this model's parameters on the GPU, else None."""
        ps = self._params
        if not ps or not ps[0].is_cuda or not _ext.available():
            return None
        from ..runtime.param_store import lookup_store

        store = lookup_store(ps[0])
        if store is None or len(store.params) != len(ps):
            return None
        for p, q in zip(ps, store.params):
            if p is not q or not store.covers_param(p):
                return None
        return store

    def fused_buffer(self, store=None) -> Optional[torch.Tensor]:
        """The flat fp32 average with ``store``'s layout (None off the fused path), rebuilt from the
        per-parameter values when the store or its layout changed."""
        own = self._fused_store()
        if own is None or (store is not None and store is not own):
            return None
        store = own
        key = (weakref.ref(store), store.flat.data_ptr())  # a new layout is a new store
        if self._flat is not None and self._flat_key == key:
            return self._flat
        with torch.inference_mode(False), torch.no_grad():
            flat = torch.zeros_like(store.flat)  # the store's padding is zero and stays zero
            vals = {}
            for p, off in zip(store.params, store.offsets):
                view = flat[off:off + p.numel()].view(p.shape)
                view.copy_(self._vals[id(p)])
                vals[id(p)] = view
        self._vals, self._flat, self._flat_key = vals, flat, key
        return flat

    def _values(self):
        """Per-parameter fp32 tensors on the parameters' devices (views of the flat buffer on the fused path)."""
        if self.fused_buffer() is None:
            self._flat, self._flat_key = None, None
            with torch.inference_mode(False), torch.no_grad():
                for p in self._params:
                    v = self._vals[id(p)]
                    if v.device != p.device:
                        self._vals[id(p)] = v.to(p.device, copy=True)
                    elif v._base is not None:  # a view of a buffer that is no longer the layout: own storage
                        self._vals[id(p)] = v.clone()
        return [self._vals[id(p)] for p in self._params]

    # ------------------------------------------------------------------ optimizer
    def attach(self, optimizer) -> "ModelEma":
        """``FusedAdam``: its ``step()`` updates this average (inside the Adam kernel on the fused path,
        by :meth:`update` where it falls back to the reference math). Any other optimizer: nothing to
        hook; call :meth:`update` after its ``step()`` (``engine.train_step`` does)."""
        from .adam import FusedAdam

        self.detach()
        if isinstance(optimizer, FusedAdam):
            optimizer._ema = self
            self._optimizer = weakref.ref(optimizer)
        return self

    def detach(self) -> None:
        opt = self._optimizer() if self._optimizer is not None else None
        if opt is not None and getattr(opt, "_ema", None) is self:
            opt._ema = None
        self._optimizer = None

    def updated_by(self, optimizer) -> bool:
        """True if ``optimizer.step()`` already updates this average."""
        return self._optimizer is not None and self._optimizer() is optimizer

    @torch.no_grad()
    def update(self) -> None:
        """One update with torch ops (the kernel's formula) from the model's current weights."""
        d, w = self.next_pair()
        self._update_with(float(d), float(w))

    def _update_with(self, d: float, w: float) -> None:
        vals = self._values()
        with torch.inference_mode(False), torch.no_grad():
            ev, pv = [], []
            for p, v in zip(self._params, vals):
                if p.requires_grad:
                    ev.append(v)
                    pv.append(p.detach() if p.dtype == torch.float32 else p.detach().float())
            if not ev:
                return
            if len({(v.device, p.device) for v, p in zip(ev, pv)}) == 1:
                torch._foreach_mul_(ev, d)
                torch._foreach_add_(ev, pv, alpha=w)
            else:
                for v, p in zip(ev, pv):
                    v.mul_(d).add_(p, alpha=w)

    # ------------------------------------------------------------------ evaluation
    @contextlib.contextmanager
    def applied(self):
        """The model computes with the averaged weights inside the block (evaluation, export,
        predictions); the trained weights are back afterwards, bit for bit."""
        buf = self.fused_buffer()
        if buf is not None:
            with self._fused_store().swapped(buf):
                yield self
            return
        vals = self._values()
        saved = [p.data for p in self._params]
        try:
            for p, v in zip(self._params, vals):
                p.data = v if v.dtype == p.dtype else v.to(p.dtype)
            yield self
        finally:
            for p, s in zip(self._params, saved):
                p.data = s

    # ------------------------------------------------------------------ state
    def state_dict(self) -> Dict[str, torch.Tensor]:
        """The averaged weights under the model's own ``state_dict()`` keys, as fp32 CPU tensors with
        their own storages (``ViT(...).load_state_dict(ema.state_dict())`` works)."""
        vals = dict(zip(map(id, self._params), self._values()))
        out = {}
        for k, t in self.module.state_dict(keep_vars=True).items():
            v = vals.get(id(t), t)  # (a buffer would be stored as it is; the models here have none)
            out[k] = v.detach().to("cpu", copy=True).contiguous()
        return out

    def load_state_dict(self, sd: Dict[str, torch.Tensor]) -> None:
        missing = [n for n in self._names if n not in sd]
        if missing:
            raise KeyError(f"ModelEma.load_state_dict: missing keys {missing[:4]}{'...' if len(missing) > 4 else ''}")
        vals = self._values()
        with torch.inference_mode(False), torch.no_grad():
            for n, v in zip(self._names, vals):
                v.copy_(sd[n].reshape(v.shape))

    def reset(self) -> None:
        """Start over from the model's current weights (``num_updates`` = 0)."""
        vals = self._values()
        with torch.inference_mode(False), torch.no_grad():
            for p, v in zip(self._params, vals):
                v.copy_(p.detach())
        self.num_updates = 0
