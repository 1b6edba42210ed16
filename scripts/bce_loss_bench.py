"""Binary cross-entropy loss: the fused kernel beside the softmax one, and what it costs in a training step.

Training-step A/B (ViT-B/16, batch 256, ``BatchMix`` on, device-resident float batches, one process, arms
alternating), every arm through ``engine.train_step(..., batch_mix=BatchMix(...))``:

  (s)  ``nn.CrossEntropyLoss()``: soft cross-entropy, the fused softmax kernel;
  (a)  binary cross-entropy as torch ops: ``F.binary_cross_entropy_with_logits`` on the ``soft_targets`` matrix,
       without the kernel's flags (the engine then counts with argmax / eq / sum);
  (b)  ``losses.BinaryCrossEntropy()``: the fused kernel of ``csrc/bce.hip``.

The arms draw their plans from identically seeded samplers. Each value is the wall time of ``--steps`` steps closed
by a synchronise.

    python scripts/bce_loss_bench.py --out profiles/bce_loss/step_ab.json

Kernel times: ``--kernels-only`` launches ``xent_soft_kernel`` and ``bce_kernel`` (mean and sum_classes) at
``--batch`` x ``--classes`` logits, ``--reps`` times each in that fixed order; ``--parse DIR`` reads the
``*kernel_trace.csv`` a profiler run of it left in DIR and prints the time per kernel.

    rocprofv3 --kernel-trace --stats -d DIR --output-format csv -- python scripts/bce_loss_bench.py --kernels-only
    python scripts/bce_loss_bench.py --parse DIR
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
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

VARIANTS = ["xent_soft", "bce mean", "bce sum_classes"]
WARM = 2  # launches per variant left out of the mean


class Repeat:
    """``steps`` times the same device-resident batch."""

    def __init__(self, batch, steps):
        self.batch, self.steps = batch, steps

    def __len__(self):
        return self.steps

    def __iter__(self):
        for _ in range(self.steps):
            yield self.batch


def kernels_only(B, C, reps, eps):
    from pytorch_vit_paper_replication_amd import _ext

    ext = _ext.ext()
    g = torch.Generator().manual_seed(0)
    logits = (torch.randn(B, C, generator=g) * 3).cuda()
    ya, yb = (torch.randint(0, C, (B,), generator=g).cuda() for _ in range(2))
    lam = torch.rand(B, generator=g).cuda()
    dl = torch.empty_like(logits)
    corr = torch.empty(B, dtype=torch.int32, device="cuda")
    mean = torch.empty(1, device="cuda")
    for name in VARIANTS:
        for _ in range(reps + WARM):
            if name == "xent_soft":
                ext.xent_soft(logits, ya, yb, lam, eps, dl, corr, 1.0 / B, mean)
            else:
                sc = name == "bce sum_classes"
                ext.bce(logits, ya, yb, lam, eps, -1.0, sc, dl, corr, 1.0 / B if sc else 1.0 / (B * C), mean)
        torch.cuda.synchronize()
    print(json.dumps({"kernels_only": True, "order": VARIANTS, "reps": reps, "warm": WARM, "batch": B, "classes": C}))


def parse_trace(directory, reps):
    rows = []
    for path in glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True):
        with open(path, newline="") as f:
            for r in csv.DictReader(f):
                if "xent_soft_kernel" in r["Kernel_Name"] or "bce_kernel" in r["Kernel_Name"]:
                    rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"]), r["Kernel_Name"]))
    rows.sort()
    n = reps + WARM
    if len(rows) != n * len(VARIANTS):
        raise SystemExit(f"expected {n * len(VARIANTS)} loss-kernel dispatches, found {len(rows)}")
    res = {}
    for i, v in enumerate(VARIANTS):
        chunk = rows[i * n:(i + 1) * n][WARM:]
        t = sorted(c[1] for c in chunk)
        want = "xent_soft_kernel" if v == "xent_soft" else "bce_kernel"
        assert all(want in c[2] for c in chunk), f"{v}: other kernels in its slot"
        res[v] = {"mean_us": round(sum(t) / len(t) / 1e3, 2), "min_us": round(t[0] / 1e3, 2), "max_us": round(t[-1] / 1e3, 2),
                  "launches": len(t)}
    for v in VARIANTS[1:]:
        res[f"{v} / xent_soft"] = round(res[v]["mean_us"] / res["xent_soft"]["mean_us"], 3)
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
    p.add_argument("--label-smoothing", type=float, default=0.1)
    p.add_argument("--kernels-only", action="store_true")
    p.add_argument("--reps", type=int, default=10, help="timed launches per kernel with --kernels-only / --parse")
    p.add_argument("--parse", default=None, metavar="DIR")
    p.add_argument("--out", default=None)
    args = p.parse_args(argv)
    if args.parse:
        parse_trace(args.parse, args.reps)
        return 0
    S, B, C, eps = args.image_size, args.batch, args.classes, args.label_smoothing
    if args.kernels_only:
        kernels_only(B, C, args.reps, eps)
        return 0

    from pytorch_vit_paper_replication_amd import engine
    from pytorch_vit_paper_replication_amd.data import BatchMix
    from pytorch_vit_paper_replication_amd.losses import BinaryCrossEntropy
    from pytorch_vit_paper_replication_amd.models import vit
    from pytorch_vit_paper_replication_amd.ops import fused_vit
    from pytorch_vit_paper_replication_amd.optim import FusedAdam, param_groups_weight_decay, warmup_linear_decay

    class TorchOpsBce(BinaryCrossEntropy):
        """Arm (a): the engine hands it the plan as it does for the fused module; the loss is torch's op chain."""

        def forward(self, logits, y, plan=None):
            fused_vit.last_correct = None  # no kernel, no flags
            return F.binary_cross_entropy_with_logits(logits, fused_vit.soft_targets(y, logits.shape[1], plan, self.smoothing))

    device = torch.device("cuda:0")
    torch.manual_seed(0)
    model = vit(args.model, image_size=S, num_classes=C).to(device)
    opt = FusedAdam(param_groups_weight_decay(model, 0.03), lr=1e-4)
    sched = warmup_linear_decay(opt, 10 ** 6, 0.05)
    g = torch.Generator().manual_seed(0)
    batch = (torch.randn(B, 3, S, S, generator=g).to(device), torch.randint(0, C, (B,), generator=g).to(device))
    losses = {"s_soft_xent": torch.nn.CrossEntropyLoss(), "a_bce_torch_ops": TorchOpsBce(), "b_bce_fused": BinaryCrossEntropy()}
    mixers = {k: BatchMix(label_smoothing=eps, generator=torch.Generator().manual_seed(1)) for k in losses}

    def run(name, steps):
        engine.train_step(model, Repeat(batch, steps), losses[name], opt, sched, device, batch_mix=mixers[name])

    for name in losses:
        run(name, args.warmup)
    vals = {k: [] for k in losses}
    for _ in range(args.rounds):
        for name in losses:
            torch.cuda.synchronize(device)
            t0 = time.perf_counter()
            run(name, args.steps)
            torch.cuda.synchronize(device)
            vals[name].append(round(B * args.steps / (time.perf_counter() - t0), 1))
    s = vals["s_soft_xent"]
    med = {k: sorted(v)[len(v) // 2] for k, v in vals.items()}
    spread = round(max(s) - min(s), 1)
    result = {"model": args.model, "image_size": S, "batch": B, "classes": C, "steps": args.steps, "rounds": args.rounds,
              "label_smoothing": eps, "img_per_s": vals, "median": med, "s_spread": spread,
              "b_within_s_spread": med["b_bce_fused"] >= med["s_soft_xent"] - spread,
              "b_over_a": round(med["b_bce_fused"] / med["a_bce_torch_ops"], 4)}
    print(json.dumps(result), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
