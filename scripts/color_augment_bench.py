"""Colour augmentation (3-Augment and colour jitter): what the device stage replaces, and its kernels' times.

Training-step A/B (ViT-B/16, batch 256, device-resident uint8 batches, one process, arms alternating):

  plain    ``engine.train_step`` on the uint8 batch with a plain ``DeviceInput``: the plain step;
  (a)      the same augmentation written as torch ops on the device batch before the model
           (``data.color_augment.color_reference``);
  (b)      ``DeviceInput(color=ColorAugment(...))``: the kernels of ``csrc/color.hip`` in front of the patchify kernel.

Arms (a) and (b) draw their plans from identically seeded samplers (3-Augment and jitter 0.3). Arm (a) is a hand
loop with the engine's step (zero_grad, backward, clipped FusedAdam step, scheduler step) but without its metric
accumulation. Each value is wall time of ``--steps`` steps closed by a synchronise.

    python scripts/color_augment_bench.py --out profiles/color_augment/step_ab.json

Kernel times: ``--kernels-only`` runs the stage on a 256 x 3 x 224 x 224 batch ``--reps`` times with one sampled plan;
``--parse DIR`` reads the ``*kernel_trace.csv`` a profiler run of it left in DIR and prints each kernel's mean time
and achieved bytes per second (the bytes follow from the plan: blur reads and writes its samples, the sum reads
the samples whose contrast factor is not 1, apply reads and writes everything).

    rocprofv3 --kernel-trace --stats -d DIR --output-format csv -- python scripts/color_augment_bench.py --kernels-only
    python scripts/color_augment_bench.py --parse DIR

Host cost: ``--host-cost`` times the PIL chain the recipes run in their CPU workers (one 3-Augment op, then
brightness, contrast and saturation) per image on one thread; no GPU.
"""
from __future__ import annotations

import argparse
import csv
import glob
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

KERNELS = ["color_blur_kernel", "color_sum_kernel", "color_apply_kernel"]


class Repeat:
    """``steps`` times the same device-resident batch."""

    def __init__(self, batch, steps):
        self.batch, self.steps = batch, steps

    def __len__(self):
        return self.steps

    def __iter__(self):
        for _ in range(self.steps):
            yield self.batch


def kernel_plan(B):
    from pytorch_vit_paper_replication_amd.data import ColorAugment

    return ColorAugment(generator=torch.Generator().manual_seed(0)).sample(B)


def plan_bytes(plan, S):
    px = 3 * S * S
    n_blur, n_sum = int((plan.op == 3).sum()), int((plan.factors[:, 1] != 1).sum())
    return {"color_blur_kernel": 2 * n_blur * px, "color_sum_kernel": n_sum * px, "color_apply_kernel": 2 * plan.batch * px}


def kernels_only(B, S, reps):
    from pytorch_vit_paper_replication_amd.ops.fused_vit import color_u8

    xu = torch.randint(0, 256, (B, 3, S, S), generator=torch.Generator().manual_seed(0), dtype=torch.uint8).cuda()
    plan = kernel_plan(B)
    for _ in range(reps):
        color_u8(xu, plan)
    torch.cuda.synchronize()
    print(json.dumps({"kernels_only": True, "reps": reps, "batch": B, "image_size": S, "blur_samples": int((plan.op == 3).sum()),
                      "sum_samples": int((plan.factors[:, 1] != 1).sum()), "bytes": plan_bytes(plan, S)}))


def parse_trace(directory, reps, B, S):
    rows = {k: [] for k in KERNELS}
    for path in glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True):
        with open(path, newline="") as f:
            for r in csv.DictReader(f):
                for k in KERNELS:
                    if k in r["Kernel_Name"]:
                        rows[k].append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"])))
    nbytes = plan_bytes(kernel_plan(B), S)
    res = {}
    for k in KERNELS:
        if len(rows[k]) != reps:
            raise SystemExit(f"expected {reps} dispatches of {k}, found {len(rows[k])}")
        t = sorted(d for _, d in sorted(rows[k])[2:])  # the first two launches are warm-up
        mean = sum(t) / len(t)
        res[k] = {"mean_us": round(mean / 1e3, 2), "min_us": round(t[0] / 1e3, 2), "max_us": round(t[-1] / 1e3, 2), "launches": len(t),
                  "bytes": nbytes[k], "TB_per_s": round(nbytes[k] / mean / 1e3, 3)}
    res["total_mean_us"] = round(sum(res[k]["mean_us"] for k in KERNELS), 2)
    print(json.dumps(res, indent=1))


def host_cost(S, images):
    """The PIL chain per image on this thread: mean microseconds per 3-Augment op, for the jitter, and in total."""
    import numpy as np
    from PIL import Image, ImageEnhance, ImageFilter, ImageOps

    torch.set_num_threads(1)
    g = torch.Generator().manual_seed(0)
    ims = [Image.fromarray(torch.randint(0, 256, (S, S, 3), generator=g, dtype=torch.uint8).numpy(), "RGB") for _ in range(16)]
    u = torch.rand(images, 5, generator=g, dtype=torch.float64)
    ops = {"grayscale": lambda im, s: ImageOps.grayscale(im).convert("RGB"), "solarize": lambda im, s: ImageOps.solarize(im),
           "blur": lambda im, s: im.filter(ImageFilter.GaussianBlur(radius=s))}

    def jitter(im, f):
        im = ImageEnhance.Brightness(im).enhance(f[0])
        im = ImageEnhance.Contrast(im).enhance(f[1])
        return ImageEnhance.Color(im).enhance(f[2])

    res = {}
    for name, op in ops.items():
        t0 = time.perf_counter()
        for i in range(images):
            np.asarray(op(ims[i % 16], 0.1 + 1.9 * float(u[i, 0])))
        res[name + "_us"] = round((time.perf_counter() - t0) / images * 1e6, 1)
    t0 = time.perf_counter()
    for i in range(images):
        np.asarray(jitter(ims[i % 16], (0.7 + 0.6 * u[i, 1:4]).tolist()))
    res["jitter_us"] = round((time.perf_counter() - t0) / images * 1e6, 1)
    res["three_augment_mean_us"] = round(sum(res[k + "_us"] for k in ops) / 3, 1)
    res["chain_us"] = round(res["three_augment_mean_us"] + res["jitter_us"], 1)
    res.update(image_size=S, images=images, threads=1)
    return res


def main(argv=None) -> int:
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    p.add_argument("--model", default="vit_b16")
    p.add_argument("--image-size", type=int, default=224)
    p.add_argument("--batch", type=int, default=256)
    p.add_argument("--classes", type=int, default=1000)
    p.add_argument("--steps", type=int, default=100)
    p.add_argument("--warmup", type=int, default=10)
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--kernels-only", action="store_true")
    p.add_argument("--reps", type=int, default=12, help="launches with --kernels-only / --parse")
    p.add_argument("--parse", default=None, metavar="DIR")
    p.add_argument("--host-cost", action="store_true")
    p.add_argument("--host-images", type=int, default=400)
    p.add_argument("--out", default=None)
    args = p.parse_args(argv)
    S, B, C = args.image_size, args.batch, args.classes

    def emit(result):
        print(json.dumps(result), flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write(json.dumps(result, indent=1) + "\n")

    if args.parse:
        parse_trace(args.parse, args.reps, B, S)
        return 0
    if args.host_cost:
        emit(host_cost(S, args.host_images))
        return 0
    if args.kernels_only:
        kernels_only(B, S, args.reps)
        return 0

    from pytorch_vit_paper_replication_amd import engine
    from pytorch_vit_paper_replication_amd.data import ColorAugment, DeviceInput, color_reference
    from pytorch_vit_paper_replication_amd.models import vit
    from pytorch_vit_paper_replication_amd.ops import fused_vit
    from pytorch_vit_paper_replication_amd.optim import FusedAdam, param_groups_weight_decay, warmup_linear_decay

    device = torch.device("cuda:0")
    torch.manual_seed(0)
    norm = ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
    model = vit(args.model, image_size=S, num_classes=C).to(device)
    opt = FusedAdam(param_groups_weight_decay(model, 0.03), lr=1e-4)
    sched = warmup_linear_decay(opt, 10 ** 6, 0.05)
    g = torch.Generator().manual_seed(0)
    batch = (torch.randint(0, 256, (B, 3, S, S), generator=g, dtype=torch.uint8).to(device), torch.randint(0, C, (B,), generator=g).to(device))
    samplers = {k: ColorAugment(generator=torch.Generator().manual_seed(1)) for k in "ab"}
    specs = {"plain": DeviceInput(*norm), "b": DeviceInput(*norm, color=samplers["b"])}
    loss_fn = torch.nn.CrossEntropyLoss()

    def plain(steps):
        model.set_device_input(specs["plain"])
        engine.train_step(model, Repeat(batch, steps), loss_fn, opt, sched, device)

    def arm_b(steps):
        model.set_device_input(specs["b"])
        engine.train_step(model, Repeat(batch, steps), loss_fn, opt, sched, device)

    def arm_a(steps):
        model.set_device_input(specs["plain"])
        model.train()
        X, y = batch
        for _ in range(steps):
            plan = samplers["a"].sample(B)
            loss = fused_vit.cross_entropy(model(color_reference(X, plan)), y)
            opt.zero_grad()
            fused_vit.backward(loss)
            opt.step(clip_norm=1.0)
            sched.step()
        torch.cuda.synchronize(device)

    arms = (("plain", plain), ("a_torch_ops", arm_a), ("b_color_kernels", arm_b))
    for _, fn in arms:
        fn(args.warmup)
    vals = {k: [] for k, _ in arms}
    for _ in range(args.rounds):
        for name, fn in arms:
            torch.cuda.synchronize(device)
            t0 = time.perf_counter()
            fn(args.steps)
            torch.cuda.synchronize(device)
            vals[name].append(round(B * args.steps / (time.perf_counter() - t0), 1))
    u = vals["plain"]
    med = {k: sorted(v)[len(v) // 2] for k, v in vals.items()}
    spread = round(max(u) - min(u), 1)
    emit({"model": args.model, "image_size": S, "batch": B, "steps": args.steps, "rounds": args.rounds, "three_augment": True,
          "jitter": 0.3, "img_per_s": vals, "median": med, "plain_spread": spread,
          "b_within_plain_spread": med["b_color_kernels"] >= med["plain"] - spread})
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
