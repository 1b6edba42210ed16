"""Command-line trainer (replaces the reference's broken GM/train.py).

Examples::

    python -m pytorch_vit_paper_replication_amd.cli.train --model vit_b16 --synthetic --epochs 2 --batch-size 64
    python -m pytorch_vit_paper_replication_amd.cli.train --model tinyvgg --train-dir data/pizza_steak_sushi/train \
        --test-dir data/pizza_steak_sushi/test --image-size 64
    torchrun --nproc-per-node 8 -m pytorch_vit_paper_replication_amd.cli.train --synthetic ...   # RCCL DP
    python -m pytorch_vit_paper_replication_amd.cli.train --model vit_h14 --synthetic --dtype fp8   # BASELINE config 5
"""
from __future__ import annotations

import argparse
import contextlib
import math

import torch


def _is_rank0() -> bool:
    d = torch.distributed
    return not (d.is_available() and d.is_initialized()) or d.get_rank() == 0


def build_parser():
    p = argparse.ArgumentParser(description="Train a ViT (or TinyVGG) with the MI355X-native engine")
    p.add_argument("--model", default="vit_b16", help="vit_b16 | vit_l16 | vit_h14 | vit_tiny_test | tinyvgg")
    p.add_argument("--image-size", type=int, default=224)
    p.add_argument("--num-classes", type=int, default=None)
    p.add_argument("--train-dir", default=None)
    p.add_argument("--test-dir", default=None)
    p.add_argument("--synthetic", action="store_true", help="synthetic ImageNet-shaped data")
    p.add_argument("--synthetic-train-len", type=int, default=512)
    p.add_argument("--synthetic-test-len", type=int, default=128)
    p.add_argument("--epochs", type=int, default=5, help="total epochs (a --resume run trains the rest)")
    p.add_argument("--batch-size", type=int, default=32)
    p.add_argument("--lr", type=float, default=1e-3, help="learning rate (LAMB recipes use about 3e-3)")
    p.add_argument("--weight-decay", type=float, default=0.03, help="weight decay (LAMB recipes use 0.02-0.05)")
    p.add_argument("--optimizer", choices=["adam", "adamw", "lamb", "sgd"], default="adam",
                   help="adam: coupled L2 decay (the reference recipe); adamw: decoupled decay; lamb: Adam's update scaled "
                        "per parameter tensor by ||w|| / ||update|| (large batches; FusedLamb only); sgd: SGD with "
                        "--momentum (the paper's fine-tuning optimizer, with --weight-decay 0 and --lr-schedule cosine)")
    p.add_argument("--momentum", type=float, default=0.9, help="with --optimizer sgd: the momentum")
    p.add_argument("--nesterov", action="store_true", help="with --optimizer sgd: Nesterov momentum")
    p.add_argument("--lr-schedule", choices=["linear", "cosine"], default="linear",
                   help="decay after the warmup: linear to 0 (the reference recipe) or cosine")
    p.add_argument("--init-from", default=None, metavar="PATH",
                   help="ViT: start from the model weights of this file (a saved model, or a checkpoint's model), nothing "
                        "else; weights trained at another --image-size get their position embedding resampled, and a "
                        "classifier of another class count is left freshly initialised")
    p.add_argument("--warmup-frac", type=float, default=0.05)
    p.add_argument("--max-grad-norm", type=float, default=1.0)
    p.add_argument("--num-workers", type=int, default=4)
    p.add_argument("--hidden-units", type=int, default=10)
    p.add_argument("--save-dir", default="models")
    p.add_argument("--save-name", default=None)
    p.add_argument("--checkpoint-dir", default=None)
    p.add_argument("--resume", default=None)
    p.add_argument("--metrics", default=None, help="append per-epoch JSONL metrics here")
    p.add_argument("--torch-optimizer", action="store_true",
                   help="use torch.optim.Adam / AdamW / SGD instead of FusedAdam / FusedSGD (there is no torch LAMB)")
    p.add_argument("--seed", type=int, default=42)
    p.add_argument("--dtype", choices=["bf16", "fp8"], default="bf16",
                   help="fp8: the encoder GEMMs in fp8 with delayed scaling (ViT.enable_fp8; GPU fused path only)")
    p.add_argument("--fp8-grad", choices=["e4m3", "e5m2"], default="e4m3", help="fp8: the gradients' format")
    p.add_argument("--fp8-bf16-wgrad", action="store_true", help="fp8: keep the weight-gradient GEMMs bf16")
    p.add_argument("--dropout", type=float, default=None,
                   help="override the MLP and embedding dropout of the ViT preset (0.1 = the reference's)")
    p.add_argument("--drop-path", type=float, default=0.0, metavar="RATE",
                   help="ViT: stochastic depth, the last block's drop rate (0: off; not with --dtype fp8)")
    p.add_argument("--drop-path-schedule", choices=["linear", "constant"], default="linear",
                   help="with --drop-path: rates rising linearly with depth from 0 to RATE, or RATE in every block")
    p.add_argument("--patch-dropout", type=float, default=0.0, metavar="RATE",
                   help="ViT: train on a random subset of each image's patch tokens, dropping this fraction "
                        "(0: off; evaluation sees every patch; not with --dtype fp8)")
    p.add_argument("--layer-scale", type=float, default=None, metavar="INIT",
                   help="ViT: LayerScale, a learnable per-channel scale on each residual branch, initialised to INIT "
                        "(DeiT-III: 1e-4; default: off; not with --dtype fp8)")
    p.add_argument("--deterministic", action="store_true",
                   help="fixed-order reductions instead of float atomics: bitwise-repeatable gradients")
    p.add_argument("--bucket-mb", type=float, default=28.0, help="DDP gradient bucket size (MiB)")
    p.add_argument("--comm-dtype", choices=["fp32", "bf16"], default="fp32", help="DDP all-reduce wire format")
    p.add_argument("--device-preprocess", action="store_true",
                   help="ViT: load uint8 images and scale / crop / resize / flip them in the patch-embedding kernel")
    p.add_argument("--augment", choices=["none", "rrc-flip"], default="none",
                   help="with --device-preprocess: random-resized-crop + horizontal flip on the device in training")
    p.add_argument("--source-size", type=int, default=None,
                   help="with --device-preprocess: side of the uint8 images the loader yields (default: --image-size)")
    p.add_argument("--three-augment", action="store_true",
                   help="with --device-preprocess: DeiT-III's 3-Augment on the device in training, one of grayscale, "
                        "solarize or Gaussian blur per image")
    p.add_argument("--color-jitter", type=float, default=0.0, metavar="V",
                   help="with --device-preprocess: brightness / contrast / saturation jitter on the device in training, "
                        "factors uniform in [max(0, 1 - V), 1 + V] (0: off; the recipes use 0.3 or 0.4)")
    p.add_argument("--mixup", type=float, default=0.0, metavar="A", help="mixup with lam ~ Beta(A, A) (0: off)")
    p.add_argument("--cutmix", type=float, default=0.0, metavar="A", help="CutMix with lam ~ Beta(A, A) (0: off)")
    p.add_argument("--mix-prob", type=float, default=1.0, help="probability that a batch is mixed")
    p.add_argument("--mix-switch-prob", type=float, default=0.5, help="with both: probability of CutMix over mixup")
    p.add_argument("--label-smoothing", type=float, default=0.0, metavar="E", help="label smoothing of the loss (0: off)")
    p.add_argument("--bce-loss", action="store_true",
                   help="binary cross-entropy (the sigmoid loss of DeiT-III) instead of softmax cross-entropy, against the "
                        "same mixed / smoothed label rows; --label-smoothing is its smoothing")
    p.add_argument("--bce-target-threshold", type=float, default=None, metavar="T",
                   help="with --bce-loss: binarise the label rows, target = row > T (T in [0, 1); the recipes use 0.2)")
    p.add_argument("--bce-sum-classes", action="store_true",
                   help="with --bce-loss: sum the loss over the classes, then average over the batch (default: mean over both)")
    p.add_argument("--head-bias-init", type=float, default=None, metavar="V",
                   help="ViT: fill the classifier's bias with V before training. -log(C) for C classes is the usual choice "
                        "for a sigmoid loss: each class then starts at probability 1 / (1 + C) instead of 1 / 2, so the "
                        "first steps do not go into pushing C - 1 of C outputs down (default: the seeded initialisation)")
    p.add_argument("--random-erasing", type=float, default=0.0, metavar="P",
                   help="random erasing: erase one random box of each training image with this probability (0: off; "
                        "the DeiT recipe uses 0.25)")
    p.add_argument("--random-erasing-mode", choices=["pixel", "const"], default="pixel",
                   help="with --random-erasing: fill the box with per-pixel standard normal noise, or with the mean colour")
    p.add_argument("--model-ema", type=float, nargs="?", const=0.9999, default=None, metavar="DECAY",
                   help="keep an exponential moving average of the weights (bare flag: 0.9999): it is what the test "
                        "pass evaluates, checkpoints carry it and <name>_ema.pth is written beside the model")
    p.add_argument("--model-ema-warmup", action="store_true",
                   help="with --model-ema: ramp the decay, update n uses min(DECAY, (1 + n) / (10 + n))")
    return p


def build_batch_mix(args, rank: int = 0):
    """The :class:`~..data.batch_mix.BatchMix` of ``--mixup`` / ``--cutmix`` (None when both are off: label
    smoothing alone goes into the loss function), its generator seeded from ``--seed`` per rank."""
    if args.mixup <= 0 and args.cutmix <= 0:
        return None
    from ..data.batch_mix import BatchMix

    gen = torch.Generator().manual_seed(args.seed * 1_000_003 + 7919 + rank)
    return BatchMix(mixup_alpha=args.mixup, cutmix_alpha=args.cutmix, prob=args.mix_prob, switch_prob=args.mix_switch_prob,
                    label_smoothing=args.label_smoothing, generator=gen)


def build_loss(args):
    """The ``loss_fn`` of the run: ``nn.CrossEntropyLoss`` with ``--label-smoothing``, or with ``--bce-loss`` the
    :class:`~..losses.BinaryCrossEntropy` of ``--label-smoothing`` / ``--bce-target-threshold`` / ``--bce-sum-classes``."""
    if not args.bce_loss:
        return torch.nn.CrossEntropyLoss(label_smoothing=args.label_smoothing)
    from ..losses import BinaryCrossEntropy

    return BinaryCrossEntropy(smoothing=args.label_smoothing, target_threshold=args.bce_target_threshold,
                              sum_classes=args.bce_sum_classes)


def build_random_erasing(args, rank: int = 0):
    """The :class:`~..data.random_erasing.RandomErasing` of ``--random-erasing`` (None when it is 0), its generator
    seeded from ``--seed`` per rank."""
    if args.random_erasing <= 0:
        return None
    from ..data.random_erasing import RandomErasing

    gen = torch.Generator().manual_seed(args.seed * 1_000_003 + 15485863 + rank)
    return RandomErasing(prob=args.random_erasing, mode=args.random_erasing_mode, generator=gen)


def build_color_augment(args, rank: int = 0):
    """The :class:`~..data.color_augment.ColorAugment` of ``--three-augment`` / ``--color-jitter`` (None when both are
    off), its generator seeded from ``--seed`` per rank."""
    if not args.three_augment and args.color_jitter <= 0:
        return None
    from ..data.color_augment import ColorAugment

    gen = torch.Generator().manual_seed(args.seed * 1_000_003 + 32452843 + rank)
    return ColorAugment(three_augment=args.three_augment, jitter=(args.color_jitter,) * 3 if args.color_jitter > 0 else None,
                        generator=gen)


def build_model(args, ncls: int, rank: int = 0):
    """The model of ``--model`` with ``ncls`` outputs and the options of the command line (on the CPU, before a
    ``--resume`` loads into it)."""
    from ..data import DeviceInput, RandomResizedCropFlip
    from ..models import TinyVGG, vit

    if args.model == "tinyvgg":
        return TinyVGG(input_shape=3, hidden_units=args.hidden_units, output_shape=ncls)
    drop = {} if args.dropout is None else dict(mlp_dropout=args.dropout, embedding_dropout=args.dropout)
    model = vit(args.model, image_size=args.image_size, num_classes=ncls, drop_path=args.drop_path,
                drop_path_schedule=args.drop_path_schedule, patch_dropout=args.patch_dropout, layer_scale=args.layer_scale, **drop)
    if args.head_bias_init is not None:  # a --resume then loads the checkpoint's bias over it
        model.init_head_bias(args.head_bias_init)
    if args.dtype == "fp8":  # before a resume: the checkpoint's fp8 scaling state needs it
        model.enable_fp8(wgrad=not args.fp8_bf16_wgrad, grad_fmt=args.fp8_grad)
    if args.device_preprocess:
        # per-rank crop draws: every rank augments its own shard differently (not saved by --resume)
        gen = torch.Generator().manual_seed(args.seed * 1_000_003 + rank)
        aug = RandomResizedCropFlip(generator=gen) if args.augment == "rrc-flip" else None
        model.set_device_input(DeviceInput(augment=aug, color=build_color_augment(args, rank)))
    return model


def build_optimizer(args, model):
    """The optimizer of ``--optimizer`` / ``--torch-optimizer`` over the two weight-decay groups of the recipe."""
    from ..optim import FusedAdam, FusedLamb, FusedSGD, param_groups_weight_decay

    groups = param_groups_weight_decay(model, args.weight_decay)
    if args.optimizer == "lamb":
        return FusedLamb(groups, lr=args.lr, betas=(0.9, 0.999))
    if args.optimizer == "sgd":
        cls = torch.optim.SGD if args.torch_optimizer else FusedSGD
        return cls(groups, lr=args.lr, momentum=args.momentum, nesterov=args.nesterov)
    if args.torch_optimizer:
        return (torch.optim.AdamW if args.optimizer == "adamw" else torch.optim.Adam)(groups, lr=args.lr, betas=(0.9, 0.999))
    if args.optimizer == "adamw":
        return FusedAdam(groups, lr=args.lr, betas=(0.9, 0.999), decoupled_weight_decay=True)
    return FusedAdam(groups, lr=args.lr, betas=(0.9, 0.999))


def init_model_from(model, path: str) -> None:
    """``--init-from``: the model weights of ``path`` (a saved model's state dict, or the ``"model"`` entry of a
    checkpoint) into ``model`` through :func:`~..models.transfer.load_state_dict_resized`. A classifier of another
    shape than the model's is left out, so the model keeps its fresh head; every other key must match."""
    from ..models.transfer import load_state_dict_resized

    sd = torch.load(path, map_location="cpu", weights_only=True)
    if isinstance(sd.get("model"), dict):
        sd = sd["model"]
    own = model.state_dict()
    fresh = [k for k in sd if k.startswith("classifier.") and k in own and sd[k].shape != own[k].shape]
    sd = {k: v for k, v in sd.items() if k not in fresh}
    missing, unexpected = load_state_dict_resized(model, sd, strict=False)
    if set(missing) - set(fresh) or unexpected:
        raise SystemExit(f"--init-from {path}: missing keys {sorted(set(missing) - set(fresh))}, unexpected keys {list(unexpected)}")
    if _is_rank0():
        print(f"[INFO] Initialised the model from {path}" + (f" (fresh classifier: {', '.join(fresh)})" if fresh else ""))


def main(argv=None) -> int:
    from .. import engine
    from ..data import create_dataloaders, create_synthetic_dataloaders
    from ..data.transforms import default_vit_transform, uint8_transform
    from ..optim import ModelEma, warmup_cosine_decay, warmup_linear_decay
    from ..parallel import DistributedDataParallel, init_distributed, is_dist
    from .. import _ext
    from ..utils import load_checkpoint, save_model, set_seeds
    from ..utils.checkpoint import save_ema

    args = build_parser().parse_args(argv)
    if args.dtype == "fp8" and args.model == "tinyvgg":
        raise SystemExit("--dtype fp8 applies to the ViT models")
    if args.device_preprocess and args.model == "tinyvgg":
        raise SystemExit("--device-preprocess applies to the ViT models")
    if args.drop_path and args.model == "tinyvgg":
        raise SystemExit("--drop-path applies to the ViT models")
    if args.drop_path and args.dtype == "fp8":
        raise SystemExit("--drop-path does not combine with --dtype fp8")
    if args.patch_dropout and args.model == "tinyvgg":
        raise SystemExit("--patch-dropout applies to the ViT models")
    if args.patch_dropout and args.dtype == "fp8":
        raise SystemExit("--patch-dropout does not combine with --dtype fp8")
    if args.layer_scale is not None and args.model == "tinyvgg":
        raise SystemExit("--layer-scale applies to the ViT models")
    if args.layer_scale is not None and args.dtype == "fp8":
        raise SystemExit("--layer-scale does not combine with --dtype fp8")
    if not 0.0 <= args.patch_dropout < 1.0:
        raise SystemExit("--patch-dropout must be in [0, 1)")
    if not 0.0 <= args.random_erasing <= 1.0:
        raise SystemExit("--random-erasing must be in [0, 1]")
    if args.optimizer == "lamb" and args.torch_optimizer:
        raise SystemExit("--optimizer lamb has no torch.optim counterpart: drop --torch-optimizer")
    if args.nesterov and args.optimizer != "sgd":
        raise SystemExit("--nesterov needs --optimizer sgd")
    if args.init_from and args.model == "tinyvgg":
        raise SystemExit("--init-from applies to the ViT models")
    if args.model_ema_warmup and args.model_ema is None:
        raise SystemExit("--model-ema-warmup needs --model-ema")
    if not args.device_preprocess and (args.augment != "none" or args.source_size is not None):
        raise SystemExit("--augment and --source-size need --device-preprocess")
    if not args.device_preprocess and (args.three_augment or args.color_jitter != 0):
        raise SystemExit("--three-augment and --color-jitter need --device-preprocess")
    if not (args.color_jitter >= 0.0 and math.isfinite(args.color_jitter)):
        raise SystemExit("--color-jitter must be a finite value >= 0")
    if not args.bce_loss and (args.bce_target_threshold is not None or args.bce_sum_classes):
        raise SystemExit("--bce-target-threshold and --bce-sum-classes need --bce-loss")
    if args.bce_target_threshold is not None and not 0.0 <= args.bce_target_threshold < 1.0:
        raise SystemExit("--bce-target-threshold must be in [0, 1)")
    if args.head_bias_init is not None and args.model == "tinyvgg":
        raise SystemExit("--head-bias-init applies to the ViT models")
    if args.head_bias_init is not None and not math.isfinite(args.head_bias_init):
        raise SystemExit("--head-bias-init must be finite")
    src_size = args.source_size or args.image_size
    rank, world, device = init_distributed()
    set_seeds(args.seed)
    if args.synthetic or not args.train_dir:
        ncls = args.num_classes or 1000
        train_dl, test_dl, class_names = create_synthetic_dataloaders(
            args.batch_size, args.synthetic_train_len, args.synthetic_test_len,
            src_size if args.device_preprocess else args.image_size, ncls, num_workers=0, uint8=args.device_preprocess)
    else:
        tf = uint8_transform(src_size) if args.device_preprocess else default_vit_transform(args.image_size)
        train_dl, test_dl, class_names = create_dataloaders(args.train_dir, args.test_dir, tf, args.batch_size,
                                                            num_workers=args.num_workers)
    ncls = args.num_classes or len(class_names)
    model = build_model(args, ncls, rank)
    if args.init_from:
        init_model_from(model, args.init_from)
    model.to(device)
    opt = build_optimizer(args, model)
    sched = (warmup_cosine_decay if args.lr_schedule == "cosine" else warmup_linear_decay)(
        opt, args.epochs * len(train_dl), args.warmup_frac)
    ema = ModelEma(model, decay=args.model_ema, warmup=args.model_ema_warmup) if args.model_ema is not None else None
    start_epoch, results = 0, None
    if args.resume:
        # --epochs is the TOTAL epoch count: a resumed run trains only the epochs not yet done, on the
        # same (restored) LR schedule, so it ends where the uninterrupted run would have
        info = load_checkpoint(args.resume, model, opt, sched, model_ema=ema)
        start_epoch, results = int(info["epoch"]), info["results"]
        if _is_rank0():
            print(f"[INFO] Resumed {args.resume} at epoch {start_epoch} of {args.epochs}")
            saved = info.get("config") or {}
            was = (saved.get("drop_path", 0.0), saved.get("drop_path_schedule", "linear"))
            cfg = getattr(model, "config", None) or {}
            now = (cfg.get("drop_path", 0.0), cfg.get("drop_path_schedule", "linear"))
            if was != now and (was[0] or now[0]):
                print(f"[INFO] The run continues with --drop-path {now[0]} ({now[1]}); the checkpoint was written with {was[0]} ({was[1]})")
            was, now = saved.get("patch_dropout", 0.0), cfg.get("patch_dropout", 0.0)
            if was != now:
                print(f"[INFO] The run continues with --patch-dropout {now}; the checkpoint was written with {was}")
            if ("layer_scale" in saved) != ("layer_scale" in cfg):  # (load_state_dict has then already named the keys)
                print(f"[INFO] --layer-scale is {'on' if 'layer_scale' in cfg else 'off'}; the checkpoint was written with it "
                      f"{'on' if 'layer_scale' in saved else 'off'}")
    net = (DistributedDataParallel(model, bucket_cap_mb=args.bucket_mb,
                                   comm_dtype=torch.bfloat16 if args.comm_dtype == "bf16" else None)
           if is_dist() else model)
    with _ext.deterministic_mode() if args.deterministic else contextlib.nullcontext():
        engine.train(model=net, train_dataloader=train_dl, test_dataloader=test_dl, optimizer=opt,
                     loss_fn=build_loss(args), lr_scheduler=sched,
                     epochs=args.epochs, device=device, max_grad_norm=args.max_grad_norm, checkpoint_dir=args.checkpoint_dir,
                     metrics_path=args.metrics, start_epoch=start_epoch, results=results,
                     batch_mix=build_batch_mix(args, rank), model_ema=ema, random_erasing=build_random_erasing(args, rank))
    name = args.save_name or f"{args.model}_{args.epochs}_epochs.pth"
    save_model(model, args.save_dir, name)
    if ema is not None:
        stem, dot, suffix = name.rpartition(".")
        save_ema(ema, args.save_dir, f"{stem}_ema{dot}{suffix}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
