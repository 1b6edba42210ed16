"""Random erasing: what the fused path replaces, and the patchify kernels' times.

Training-step A/B (ViT-B/16, batch 256, device-resident float batches, one process, arms alternating):

  plain    ``engine.train_step`` with ``nn.CrossEntropyLoss()``: the plain step;
  (a)      the same augmentation written as torch ops on the device batch before the model: a ``randn`` of the
           batch's shape and one ``where`` under the boxes' mask (``data.random_erasing.erase_reference``);
  (b)      ``engine.train_step(..., random_erasing=RandomErasing(...))``: the erase inside the patchify kernel.

Arms (a) and (b) draw their plans from identically seeded samplers (probability 0.25, "pixel" mode). Arm (a) is
a hand loop with the engine's step (zero_grad, backward, clipped FusedAdam step, scheduler step) but without
its metric accumulation. Each value is wall time of ``--steps`` steps closed by a synchronise.

    python scripts/random_erasing_bench.py --out profiles/random_erasing/step_ab.json

Kernel times: ``--kernels-only`` launches the float and the uint8 patchify kernel at 256 x 3 x 224 x 224 without
a plan and with an erase-only plan drawn at probability 0.25 in "pixel" mode, ``--reps`` times each in that
fixed order; ``--parse DIR`` reads the ``*kernel_trace.csv`` a profiler run of it left in DIR and prints the mean
time per variant.

    rocprofv3 --kernel-trace --stats -d DIR --output-format csv -- python scripts/random_erasing_bench.py --kernels-only
    python scripts/random_erasing_bench.py --parse DIR
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

VARIANTS = ["float none", "float erase", "u8 none", "u8 erase"]


class Repeat:
    """``steps`` times the same device-resident batch."""

    def __init__(self, batch, steps):
        self.batch, self.steps = batch, steps

    def __len__(self):
        return self.steps

    def __iter__(self):
        for _ in range(self.steps):
            yield self.batch


def kernel_plan(B, S):
    from pytorch_vit_paper_replication_amd.data import RandomErasing

    return RandomErasing(prob=0.25, generator=torch.Generator().manual_seed(0)).sample(B, S, S)


def erased_share(plan):
    x0, y0, x1, y1 = plan.box.long().unbind(1)
    return float(((x1 - x0) * (y1 - y0)).sum()) / (plan.batch * plan.size[0] * plan.size[1])


def kernels_only(B, S, P, reps):
    from pytorch_vit_paper_replication_amd import _ext
    from pytorch_vit_paper_replication_amd.ops.fused_vit import ERASE_SITE, SITE_SHIFT

    ext = _ext.ext()
    g = torch.Generator().manual_seed(0)
    xu = torch.randint(0, 256, (B, 3, S, S), generator=g, dtype=torch.uint8).cuda()
    xf = xu.float() / 255
    kp = (3 * P * P + 63) // 64 * 64
    out = torch.empty(B * (S // P) ** 2, kp, dtype=torch.bfloat16, device="cuda")
    mean, std = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
    plan = kernel_plan(B, S)
    seed = torch.tensor([12345], dtype=torch.int64, device="cuda")
    erase = dict(erase=plan.on("cuda"), erase_host=plan.rows, erase_mode="pixel", erase_seed=seed, erase_offset=ERASE_SITE << SITE_SHIFT)
    for kind in ("float", "u8"):
        for kw in ({}, erase):
            for _ in range(reps):
                if kind == "float":
                    ext.im2col(xf, out, P, kp, **kw)
                else:
                    ext.im2col_u8(xu, out, mean, std, None, S, S, P, kp, **kw)
            torch.cuda.synchronize()
    print(json.dumps({"kernels_only": True, "order": VARIANTS, "reps": reps, "batch": B, "image_size": S,
                      "erased_samples": int(plan.erased.sum()), "erased_pixel_share": round(erased_share(plan), 4)}))


def parse_trace(directory, reps):
    rows = []
    for path in glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True):
        with open(path, newline="") as f:
            for r in csv.DictReader(f):
                if "im2col" in r["Kernel_Name"]:
                    rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"]), r["Kernel_Name"]))
    rows.sort()
    if len(rows) != reps * len(VARIANTS):
        raise SystemExit(f"expected {reps * len(VARIANTS)} im2col dispatches, found {len(rows)}")
    res = {}
    for i, v in enumerate(VARIANTS):
        chunk = rows[i * reps:(i + 1) * reps][2:]  # the first two launches of a variant are warm-up
        t = sorted(c[1] for c in chunk)
        res[v] = {"mean_us": round(sum(t) / len(t) / 1e3, 2), "min_us": round(t[0] / 1e3, 2), "max_us": round(t[-1] / 1e3, 2),
                  "launches": len(t), "kernel": chunk[0][2][chunk[0][2].find("im2col"):].split("(")[0]}
    for kind in ("float", "u8"):
        res[f"{kind} erase / none"] = round(res[f"{kind} erase"]["mean_us"] / res[f"{kind} none"]["mean_us"], 3)
    print(json.dumps(res, indent=1))


def main(argv=None) -> int:
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    p.add_argument("--model", default="vit_b16")
    p.add_argument("--image-size", type=int, default=224)
    p.add_argument("--batch", type=int, default=256)
    p.add_argument("--classes", type=int, default=1000)
    p.add_argument("--steps", type=int, default=100)
    p.add_argument("--warmup", type=int, default=10)
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--prob", type=float, default=0.25)
    p.add_argument("--kernels-only", action="store_true")
    p.add_argument("--reps", type=int, default=12, help="launches per variant with --kernels-only / --parse")
    p.add_argument("--parse", default=None, metavar="DIR")
    p.add_argument("--out", default=None)
    args = p.parse_args(argv)
    if args.parse:
        parse_trace(args.parse, args.reps)
        return 0
    S, B, C = args.image_size, args.batch, args.classes
    if args.kernels_only:
        kernels_only(B, S, 16, args.reps)
        return 0

    from pytorch_vit_paper_replication_amd import engine
    from pytorch_vit_paper_replication_amd.data import RandomErasing, erase_reference
    from pytorch_vit_paper_replication_amd.models import vit
    from pytorch_vit_paper_replication_amd.ops import fused_vit
    from pytorch_vit_paper_replication_amd.optim import FusedAdam, param_groups_weight_decay, warmup_linear_decay

    device = torch.device("cuda:0")
    torch.manual_seed(0)
    model = vit(args.model, image_size=S, num_classes=C).to(device)
    opt = FusedAdam(param_groups_weight_decay(model, 0.03), lr=1e-4)
    sched = warmup_linear_decay(opt, 10 ** 6, 0.05)
    g = torch.Generator().manual_seed(0)
    batch = (torch.randn(B, 3, S, S, generator=g).to(device), torch.randint(0, C, (B,), generator=g).to(device))
    erasers = {k: RandomErasing(prob=args.prob, generator=torch.Generator().manual_seed(1)) for k in "ab"}
    loss_fn = torch.nn.CrossEntropyLoss()

    def plain(steps):
        engine.train_step(model, Repeat(batch, steps), loss_fn, opt, sched, device)

    def arm_b(steps):
        engine.train_step(model, Repeat(batch, steps), loss_fn, opt, sched, device, random_erasing=erasers["b"])

    def arm_a(steps):
        model.train()
        X, y = batch
        for _ in range(steps):
            plan = erasers["a"].sample(B, S, S)
            loss = fused_vit.cross_entropy(model(erase_reference(X, plan)), y)
            opt.zero_grad()
            fused_vit.backward(loss)
            opt.step(clip_norm=1.0)
            sched.step()
        torch.cuda.synchronize(device)

    arms = (("plain", plain), ("a_torch_ops", arm_a), ("b_random_erasing", arm_b))
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
    result = {"model": args.model, "image_size": S, "batch": B, "steps": args.steps, "rounds": args.rounds, "prob": args.prob,
              "mode": "pixel", "img_per_s": vals, "median": med, "plain_spread": spread,
              "b_within_plain_spread": med["b_random_erasing"] >= med["plain"] - spread}
    print(json.dumps(result), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
