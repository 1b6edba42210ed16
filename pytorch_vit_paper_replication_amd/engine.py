"""Training / evaluation engine with the reference API (GM/engine.py:9-211).

``train(model, train_dataloader, test_dataloader, optimizer, loss_fn, lr_scheduler, epochs, device)``
returns ``{"train_loss": [...], "train_acc": [...], "test_loss": [...], "test_acc": [...]}`` and prints
``Epoch: n | train_loss: .. | train_acc: .. | test_loss: .. | test_acc: ..`` per epoch, exactly like
the reference. Preserved semantics:
  * the scheduler steps once per batch, gradients are clipped to global norm 1.0 before the step;
  * metrics are the mean over batches of per-batch means (a partial last batch weighs like a full one);
  * the train accuracy uses argmax(softmax(logits)) (== argmax(logits)), test uses argmax(logits).

MI355X-oriented differences (no behaviour change):
  * per-batch loss/accuracy accumulate on the device; the host syncs once per epoch instead of
    twice per batch (the reference's ``.item()`` calls, GM/engine.py:54,74,121,125);
  * with :class:`~..optim.FusedAdam` the clip runs inside the optimizer (device-side coefficient,
    no sync) and ``nn.CrossEntropyLoss()`` is executed by the fused softmax-xent kernel, whose
    per-row argmax == label flags also give the accuracy (no separate argmax / eq / sum), as do those
    of the fused sigmoid-loss kernel behind :class:`~.losses.BinaryCrossEntropy`;
  * under ``torch.distributed`` metrics are all-reduced across ranks and only rank 0 prints;
  * on a GPU the next batch's host->device copy runs on a copy stream while the current step
    computes (:class:`~.data.prefetch.DevicePrefetcher`, K17) instead of a blocking ``.to(device)``.
"""
from __future__ import annotations

import contextlib
from typing import Dict, List, Optional, Tuple

import torch
from torch import nn

try:
    from tqdm.auto import tqdm
except Exception:  # pragma: no cover
    def tqdm(x, **_):
        return x

from .data.prefetch import prefetch
from .losses import BinaryCrossEntropy
from .ops import fused_vit
from .ops.fused_vit import cross_entropy, soft_cross_entropy
from .utils.profiling import range_push


def _is_dist() -> bool:
    return torch.distributed.is_available() and torch.distributed.is_initialized()


def _rank0() -> bool:
    return not _is_dist() or torch.distributed.get_rank() == 0


class _SoftLoss:
    """``soft_cross_entropy`` with a fixed label smoothing and, under ``batch_mix``, the current batch's
    plan (set per batch by ``train_step``)."""

    def __init__(self, label_smoothing: float):
        self.label_smoothing, self.plan = float(label_smoothing), None

    def __call__(self, logits, y):
        return soft_cross_entropy(logits, y, self.plan, self.label_smoothing)


class _MixedBce:
    """A :class:`~.losses.BinaryCrossEntropy` under ``batch_mix``: the module itself, called with the current
    batch's plan (set per batch by ``train_step``) and with ``batch_mix.label_smoothing`` as its smoothing,
    the rule cross-entropy has. A module that sets another non-zero smoothing of its own is refused."""

    def __init__(self, module: BinaryCrossEntropy, label_smoothing: float):
        eps = float(label_smoothing)
        if module.smoothing != 0.0 and module.smoothing != eps:
            raise ValueError(f"the loss's smoothing {module.smoothing} and batch_mix.label_smoothing {eps} differ: "
                             "under batch_mix the smoothing is batch_mix.label_smoothing")
        self.module, self.label_smoothing, self.plan = module, eps, None

    def __call__(self, logits, y):
        own, self.module.smoothing = self.module.smoothing, self.label_smoothing
        try:
            return self.module(logits, y, self.plan)
        finally:
            self.module.smoothing = own


def _fused_loss(loss_fn):
    """Use the fused kernels for a default nn.CrossEntropyLoss (same math and reduction): the
    hard-label kernel, or with ``label_smoothing > 0`` the soft-target one."""
    if isinstance(loss_fn, nn.CrossEntropyLoss) and loss_fn.weight is None and loss_fn.reduction == "mean" \
            and loss_fn.ignore_index == -100:
        if loss_fn.label_smoothing == 0.0:
            return cross_entropy
        if loss_fn.label_smoothing > 0.0:
            return _SoftLoss(loss_fn.label_smoothing)
    return loss_fn


def _mix_target(model, keyword: str = "mix"):
    """(whether the model's ``forward`` takes ``keyword`` (``mix`` or ``erase``), its image size or None): a plan
    is drawn for the image the model sees, which for a uint8 device-input batch is not the batch's own size."""
    import inspect

    inner = getattr(model, "module", model)  # DistributedDataParallel forwards keyword arguments
    takes = keyword in inspect.signature(inner.forward).parameters
    S = getattr(inner, "config", {}).get("image_size") if takes else None
    return takes, (int(S) if S else None)


def _accumulate(sums: torch.Tensor, loss: torch.Tensor, logits: torch.Tensor, y: torch.Tensor, lf) -> None:
    """sums += [batch loss, batch accuracy] on the device. With the fused cross-entropy the kernel's
    per-row argmax == label flags are summed by one small HIP kernel; otherwise argmax / eq / sum."""
    with torch.no_grad():
        fused = lf is cross_entropy or isinstance(lf, (_SoftLoss, _MixedBce, BinaryCrossEntropy))
        corr = fused_vit.last_correct if fused else None
        if corr is not None and sums.is_cuda and corr.numel() == logits.shape[0]:
            from . import _ext

            _ext.ext().metrics_accum(sums, loss.detach().float().reshape(1), corr)
            return
        acc = (logits.argmax(dim=1) == y).sum().float() / logits.shape[0]
        sums += torch.stack([loss.detach().float(), acc])


def _clip_and_step(model, optimizer, max_norm: Optional[float]) -> Optional[torch.Tensor]:
    """Clip + optimizer step; returns the pre-clip global gradient norm (a device tensor) or None."""
    from .optim.adam import FusedAdam

    if isinstance(optimizer, FusedAdam):
        optimizer.step(clip_norm=max_norm)
        return optimizer.last_grad_norm
    norm = None
    if max_norm is not None:
        norm = torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm=max_norm)
    optimizer.step()
    return norm


def _reduce_means(sums: torch.Tensor, count: int, device) -> Tuple[float, ...]:
    """sums: per-metric sums of per-batch means; returns global mean-of-batch-means."""
    vals = torch.cat([sums.double().reshape(-1), torch.tensor([float(count)], dtype=torch.float64, device=sums.device)])
    if _is_dist():
        if vals.device.type == "cpu" and torch.distributed.get_backend() == "nccl":
            vals = vals.to(device)
        torch.distributed.all_reduce(vals)
    vals = vals.cpu()
    n = max(vals[-1].item(), 1.0)
    return tuple((vals[:-1] / n).tolist())


def _set_sampler_epoch(dataloader, epoch: Optional[int]) -> None:
    """Reshuffle a DistributedSampler per epoch (otherwise every epoch repeats one permutation)."""
    sampler = getattr(dataloader, "sampler", None)
    if epoch is not None and hasattr(sampler, "set_epoch"):
        sampler.set_epoch(epoch)


def train_step(model: torch.nn.Module, dataloader, loss_fn: torch.nn.Module, optimizer: torch.optim.Optimizer,
               lr_scheduler, device, *, max_grad_norm: Optional[float] = 1.0,
               epoch: Optional[int] = None, step_logger=None, batch_mix=None, model_ema=None,
               random_erasing=None) -> Tuple[float, float]:
    """One training epoch (reference GM/engine.py:9-79). Returns (train_loss, train_acc).

    ``batch_mix`` (optional :class:`~.data.batch_mix.BatchMix`): per batch a mixup / CutMix plan is drawn
    on the host and passed to the model (``model(X, mix=plan)``; a model whose ``forward`` has no ``mix``
    parameter gets ``mix_reference(X, plan)`` instead), and the loss is ``soft_cross_entropy`` with the
    plan's label weights and ``batch_mix.label_smoothing`` in place of ``loss_fn``. A
    :class:`~.losses.BinaryCrossEntropy` ``loss_fn`` is kept instead: it is called with each batch's plan and
    with ``batch_mix.label_smoothing`` as its smoothing (another non-zero smoothing of its own raises
    ``ValueError``). The accuracy counts ``argmax == y``, the samples' own labels.

    ``random_erasing`` (optional :class:`~.data.random_erasing.RandomErasing`): per batch an erase plan is
    drawn on the host at the model's image size and passed to the model (``model(X, erase=plan)``, alone or
    next to ``mix=``: each sample is erased, then the batch is mixed; a model whose ``forward`` has no
    ``erase`` parameter gets ``erase_reference(X, plan)`` instead). Labels and loss are untouched.

    ``model_ema`` (optional :class:`~.optim.ModelEma`): attached to the optimizer on first use; a
    ``FusedAdam`` then updates the average inside its step, for any other optimizer it is updated here
    after the step.

    ``epoch`` (optional) seeds a ``DistributedSampler``'s shuffle for this epoch. ``step_logger``
    (optional :class:`~.utils.metrics.StepLogger`) gets one record per batch: step time, img/s, lr,
    loss, gradient norm and, under this package's DDP built with ``timing=True``, per-bucket
    all-reduce times — without a host synchronisation per step."""
    _set_sampler_epoch(dataloader, epoch)
    model.train()
    if batch_mix is None:
        lf = _fused_loss(loss_fn)
    elif isinstance(loss_fn, BinaryCrossEntropy):
        lf = _MixedBce(loss_fn, batch_mix.label_smoothing)
    else:
        lf = _SoftLoss(batch_mix.label_smoothing)
    takes_mix, mix_size = _mix_target(model) if batch_mix is not None else (False, None)
    takes_erase, erase_size = _mix_target(model, "erase") if random_erasing is not None else (False, None)
    sums = torch.zeros(2, dtype=torch.float32, device=device)
    nb = 0
    if model_ema is not None and not model_ema.updated_by(optimizer):
        model_ema.attach(optimizer)
    for X, y in prefetch(dataloader, device):
        if step_logger is not None:
            step_logger.begin()
        X, y = X.to(device, non_blocking=True), y.to(device, non_blocking=True)
        with range_push("forward"):  # ROCTX ranges (PVR_ROCTX=1, rocprofv3 --marker-trace)
            if batch_mix is None and random_erasing is None:
                y_pred = model(X)
            else:
                Xin, kw = X, {}
                if random_erasing is not None:  # erase each sample first, then mix the batch
                    eplan = random_erasing.sample(X.shape[0], erase_size or X.shape[-2], erase_size or X.shape[-1])
                    if takes_erase:
                        kw["erase"] = eplan
                    else:
                        from .data.random_erasing import erase_reference

                        Xin = erase_reference(Xin, eplan)
                if batch_mix is not None:
                    lf.plan = batch_mix.sample(X.shape[0], mix_size or X.shape[-2], mix_size or X.shape[-1])
                    if takes_mix:
                        kw["mix"] = lf.plan
                    else:
                        from .data.batch_mix import mix_reference

                        Xin = mix_reference(Xin, lf.plan)
                y_pred = model(Xin, **kw)
            loss = lf(y_pred, y)
        optimizer.zero_grad()
        with range_push("backward"):
            fused_vit.backward(loss)
        with range_push("optimizer"):
            norm = _clip_and_step(model, optimizer, max_grad_norm)
            if model_ema is not None and not model_ema.updated_by(optimizer):
                model_ema.update()
        lr = optimizer.param_groups[0]["lr"]
        lr_scheduler.step()
        _accumulate(sums, loss, y_pred, y, lf)
        if step_logger is not None:
            step_logger.end(batch=X.shape[0], loss=loss, grad_norm=norm, lr=lr, epoch=epoch,
                            ddp=model if hasattr(model, "pop_timing") else None)
        nb += 1
    loss_m, acc_m = _reduce_means(sums, nb, device)
    return loss_m, acc_m


def test_step(model: torch.nn.Module, dataloader, loss_fn: torch.nn.Module, device) -> Tuple[float, float]:
    """One evaluation epoch (reference GM/engine.py:81-130). Returns (test_loss, test_acc)."""
    model.eval()
    lf = _fused_loss(loss_fn)
    sums = torch.zeros(2, dtype=torch.float32, device=device)
    nb = 0
    with torch.inference_mode():
        for X, y in prefetch(dataloader, device):
            X, y = X.to(device, non_blocking=True), y.to(device, non_blocking=True)
            logits = model(X)
            loss = lf(logits, y)
            _accumulate(sums, loss, logits, y, lf)
            nb += 1
    loss_m, acc_m = _reduce_means(sums, nb, device)
    return loss_m, acc_m


def train(model: torch.nn.Module, train_dataloader, test_dataloader, optimizer: torch.optim.Optimizer,
          loss_fn: torch.nn.Module, lr_scheduler, epochs: int, device, *, max_grad_norm: Optional[float] = 1.0,
          checkpoint_dir: Optional[str] = None, metrics_path: Optional[str] = None, start_epoch: int = 0,
          results: Optional[Dict[str, List]] = None, step_metrics_path: Optional[str] = None,
          log_every: int = 50, batch_mix=None, model_ema=None, random_erasing=None) -> Dict[str, List]:
    """Train and test for ``epochs`` epochs (reference GM/engine.py:132-211).

    ``metrics_path``: one JSONL record per epoch. ``step_metrics_path``: one JSONL record per training
    step (:class:`~.utils.metrics.StepLogger`, flushed every ``log_every`` steps; rank 0 writes).

    ``batch_mix``: mixup / CutMix / label smoothing of the training batches (see :func:`train_step`);
    evaluation never mixes and keeps ``loss_fn``.

    ``random_erasing``: random erasing of the training batches (see :func:`train_step`); evaluation never
    erases.

    ``model_ema`` (optional :class:`~.optim.ModelEma`): averaged during training (see :func:`train_step`);
    the test pass runs inside ``model_ema.applied()``, so ``test_loss`` / ``test_acc`` are those of the
    averaged weights, and checkpoints carry the average.

    Resume (new, optional): ``start_epoch`` epochs are already done (``load_checkpoint(...)["epoch"]``)
    and ``results`` holds their metrics; only epochs ``start_epoch + 1 .. epochs`` run, numbered as
    in the uninterrupted run, and their metrics are appended to ``results``."""
    base = {"train_loss": [], "train_acc": [], "test_loss": [], "test_acc": []}
    results = {k: list((results or {}).get(k, [])) for k in base}
    model.to(device)
    epochs_left = range(start_epoch, epochs)
    it = tqdm(epochs_left) if _rank0() else epochs_left
    step_logger = None
    if step_metrics_path:
        from .utils.metrics import StepLogger

        world = torch.distributed.get_world_size() if _is_dist() else 1
        rank = torch.distributed.get_rank() if _is_dist() else 0
        step_logger = StepLogger(step_metrics_path, flush_every=log_every, rank=rank, world=world,
                                 device=torch.device(device))
    for epoch in it:
        train_loss, train_acc = train_step(model=model, dataloader=train_dataloader, loss_fn=loss_fn,
                                           optimizer=optimizer, lr_scheduler=lr_scheduler, device=device,
                                           max_grad_norm=max_grad_norm, epoch=epoch, step_logger=step_logger,
                                           batch_mix=batch_mix, model_ema=model_ema, random_erasing=random_erasing)
        if step_logger is not None:
            step_logger.flush()
        with model_ema.applied() if model_ema is not None else contextlib.nullcontext():
            test_loss, test_acc = test_step(model=model, dataloader=test_dataloader, loss_fn=loss_fn, device=device)
        if _rank0():
            print(f"Epoch: {epoch + 1} | "
                  f"train_loss: {train_loss:.4f} | "
                  f"train_acc: {train_acc:.4f} | "
                  f"test_loss: {test_loss:.4f} | "
                  f"test_acc: {test_acc:.4f}")
        results["train_loss"].append(train_loss)
        results["train_acc"].append(train_acc)
        results["test_loss"].append(test_loss)
        results["test_acc"].append(test_acc)
        if metrics_path and _rank0():
            from .utils.metrics import append_jsonl

            append_jsonl(metrics_path, {"epoch": epoch + 1, "train_loss": train_loss, "train_acc": train_acc,
                                        "test_loss": test_loss, "test_acc": test_acc})
        if checkpoint_dir:
            from .utils.checkpoint import save_checkpoint

            save_checkpoint(checkpoint_dir, model=model, optimizer=optimizer, lr_scheduler=lr_scheduler,
                            epoch=epoch + 1, results=results, model_ema=model_ema)
    return results
