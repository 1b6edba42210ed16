"""FusedSGD against torch.optim.SGD and FusedAdam: the training step, peak memory, and the update kernels' times.

Training-step A/B (ViT-B/16, 224 px, batch 256, one device-resident float batch, one process, arms alternating)
on one fused model: (a) ``torch.optim.SGD(momentum=0.9)`` with ``clip_grad_norm_`` (about a thousand small
launches, and the store rebuilds its bf16 shadows before the next forward), (b) ``FusedSGD(momentum=0.9)``,
(c) ``FusedAdam``. All run the same hand loop (forward, fused cross-entropy, zero_grad, backward, clipped step,
scheduler step); each optimizer keeps its own state. Each value is wall time of ``--steps`` steps closed by a
synchronise.

    python scripts/sgd_bench.py --out profiles/sgd/step_ab.json

Peak memory: ``--peak-memory sgd|adam`` runs one arm alone in the process and prints
``torch.cuda.max_memory_allocated`` after ``--steps`` steps.

Kernel times: ``--kernels-only`` steps a ViT-B/16 store (encoder weights registered, so the tile forms run)
``--reps`` times with FusedAdam and ``--reps`` times with FusedSGD on fixed synthetic gradients; ``--parse DIR``
reads the ``*kernel_trace.csv`` a profiler run of it left in DIR (no counters collected in that run) and prints
the mean time of both update kernels, the first two launches of each dropped.

    rocprofv3 --kernel-trace --stats -d DIR --output-format csv -- python scripts/sgd_bench.py --kernels-only
    python scripts/sgd_bench.py --parse DIR
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

KERNELS = ("adam_t_kernel", "sgd_t_kernel")


def _fused_optimizers(model):
    from pytorch_vit_paper_replication_amd.optim import FusedAdam, FusedSGD, param_groups_weight_decay

    return {"adam": FusedAdam(param_groups_weight_decay(model, 0.03), lr=1e-4),
            "sgd": FusedSGD(param_groups_weight_decay(model, 0.0), lr=1e-3, momentum=0.9)}


def kernels_only(model_name, S, C, reps):
    from pytorch_vit_paper_replication_amd.models import vit
    from pytorch_vit_paper_replication_amd.runtime.param_store import get_store

    device = torch.device("cuda:0")
    torch.manual_seed(0)
    model = vit(model_name, image_size=S, num_classes=C).to(device)
    store = get_store(model, device)
    store.register_transposed([w for blk in model.transformer_encoder for w in blk.fused_params()[2:12:2] if w.dim() == 2])
    store.ensure_transposed()
    gen = torch.Generator(device=device).manual_seed(1)
    for q in model.parameters():  # per parameter: the store's padding keeps its zero gradient
        q.grad.normal_(generator=gen)
    for opt in _fused_optimizers(model).values():
        torch.cuda.synchronize(device)
        for _ in range(reps):
            opt.step(clip_norm=1.0)
        torch.cuda.synchronize(device)
        assert opt._tmeta_key is not None, "the tile form did not run"
    print(json.dumps({"kernels_only": True, "order": ["FusedAdam", "FusedSGD"], "reps": reps, "model": model_name,
                      "store_elements": store.numel}))


def parse_trace(directory, reps):
    rows = {k: [] for k in KERNELS}
    for path in glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True):
        with open(path, newline="") as f:
            for r in csv.DictReader(f):
                for k in KERNELS:
                    if k in r["Kernel_Name"]:
                        rows[k].append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"])))
    res = {}
    for key, rs in rows.items():
        rs.sort()
        if len(rs) != reps:
            raise SystemExit(f"expected {reps} {key} dispatches, found {len(rs)}")
        t = sorted(c[1] for c in rs[2:])  # the first two launches are warm-up
        res[key] = {"launches": len(t), "mean_us": round(sum(t) / len(t) / 1e3, 2), "min_us": round(t[0] / 1e3, 2),
                    "max_us": round(t[-1] / 1e3, 2)}
    res["sgd_t / adam_t"] = round(res["sgd_t_kernel"]["mean_us"] / res["adam_t_kernel"]["mean_us"], 3)
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
    p.add_argument("--kernels-only", action="store_true")
    p.add_argument("--reps", type=int, default=52, help="steps per optimizer with --kernels-only / --parse")
    p.add_argument("--parse", default=None, metavar="DIR")
    p.add_argument("--peak-memory", choices=["sgd", "adam"], default=None, help="run this arm alone and print the peak allocation")
    p.add_argument("--out", default=None)
    args = p.parse_args(argv)
    if args.parse:
        parse_trace(args.parse, args.reps)
        return 0
    S, B, C = args.image_size, args.batch, args.classes
    if args.kernels_only:
        kernels_only(args.model, S, C, args.reps)
        return 0

    from pytorch_vit_paper_replication_amd.models import vit
    from pytorch_vit_paper_replication_amd.ops import fused_vit
    from pytorch_vit_paper_replication_amd.optim import param_groups_weight_decay, warmup_cosine_decay

    device = torch.device("cuda:0")
    torch.manual_seed(0)
    model = vit(args.model, image_size=S, num_classes=C).to(device)
    opts = _fused_optimizers(model)
    if args.peak_memory:
        opts = {args.peak_memory: opts[args.peak_memory]}
    else:
        opts = {"torch_sgd": torch.optim.SGD(param_groups_weight_decay(model, 0.0), lr=1e-3, momentum=0.9), **opts}
    scheds = {k: warmup_cosine_decay(o, 10 ** 6, 0.05) for k, o in opts.items()}
    params = [q for q in model.parameters() if q.requires_grad]
    g = torch.Generator().manual_seed(0)
    X, y = torch.randn(B, 3, S, S, generator=g).to(device), torch.randint(0, C, (B,), generator=g).to(device)

    def run(name, steps):
        opt, sched = opts[name], scheds[name]
        model.train()
        for _ in range(steps):
            loss = fused_vit.cross_entropy(model(X), y)
            opt.zero_grad()
            fused_vit.backward(loss)
            if name == "torch_sgd":
                torch.nn.utils.clip_grad_norm_(params, 1.0)
                opt.step()
            else:
                opt.step(clip_norm=1.0)
            sched.step()
        torch.cuda.synchronize(device)

    if args.peak_memory:
        run(args.peak_memory, args.warmup + args.steps)
        result = {"arm": args.peak_memory, "model": args.model, "batch": B, "steps": args.warmup + args.steps,
                  "peak_allocated_bytes": torch.cuda.max_memory_allocated(device),
                  "peak_allocated_gb": round(torch.cuda.max_memory_allocated(device) / 1e9, 3)}
    else:
        for name in opts:
            run(name, args.warmup)
        vals = {k: [] for k in opts}
        for _ in range(args.rounds):
            for name in opts:
                torch.cuda.synchronize(device)
                t0 = time.perf_counter()
                run(name, args.steps)
                vals[name].append(round(B * args.steps / (time.perf_counter() - t0), 1))
        med = {k: sorted(v)[len(v) // 2] for k, v in vals.items()}
        result = {"model": args.model, "image_size": S, "batch": B, "steps": args.steps, "rounds": args.rounds, "img_per_s": vals,
                  "median": med, "adam_spread": round(max(vals["adam"]) - min(vals["adam"]), 1),
                  "sgd_vs_adam_percent": round(100.0 * (med["sgd"] / med["adam"] - 1.0), 3),
                  "torch_sgd_vs_sgd_percent": round(100.0 * (med["torch_sgd"] / med["sgd"] - 1.0), 3),
                  "fused": {k: getattr(o, "_fused", None) is not None and o._tmeta_key is not None for k, o in opts.items()
                            if k != "torch_sgd"}}
    print(json.dumps(result), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
