"""Patch dropout: what training on a subset of the patch tokens saves, and what its kernels cost.

Training-step A/B (ViT-B/16, 224 px, batch 256, one device-resident float batch, one process, arms
alternating; the hand loop of scripts/drop_path_bench.py: forward, fused cross-entropy, zero_grad,
backward, clipped FusedAdam step, scheduler step):

  (u)  the plain step;
  (q)  ``set_patch_dropout(0.25)``;
  (h)  ``set_patch_dropout(0.5)``.

Each value is wall time of ``--steps`` steps closed by a synchronise.

    python scripts/patch_dropout_bench.py --out profiles/patch_dropout/step_ab.json

Kernel times: ``--kernels-only`` launches the kernels the option adds or changes at the ViT-B/16 b256
shapes, ``--reps`` times each: the keep-table kernel, the position-addend gather, the float and the uint8
patchify kernels and the patch-embedding backward, each without and with the table (rate ``--rate``). It
prints device-event means itself; ``--parse DIR`` reads the ``*kernel_trace.csv`` a profiler run of it left in
DIR (no counters collected in that run) and prints the mean time per kernel instantiation, the first two
launches of each dropped.

    rocprofv3 --kernel-trace --stats -d DIR --output-format csv -- python scripts/patch_dropout_bench.py --kernels-only
    python scripts/patch_dropout_bench.py --parse DIR
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

sys.path.insert(0, os.environ.get("PVR_PKG_ROOT") or os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

KERNELS = ("patch_keep_kernel", "pos_gather_kernel", "im2col_kernel", "im2col_u8_kernel", "patch_bwd_kernel")


def _write(res, out):
    print(json.dumps(res), flush=True)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


def kernels_only(B, S, P, D, rate, reps, out):
    from pytorch_vit_paper_replication_amd import _ext
    from pytorch_vit_paper_replication_amd.models.vit import patch_keep_count
    from pytorch_vit_paper_replication_amd.ops.fused_vit import PATCH_DROP_SITE

    ext = _ext.ext()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    n_p = (S // P) ** 2
    n_keep = patch_keep_count(n_p, rate)
    kp = (3 * P * P + 63) // 64 * 64
    seed = torch.tensor([20240611], dtype=torch.int64, device=dev)
    keep, inv = ext.patch_keep_table(seed, PATCH_DROP_SITE << 32, B, n_p, n_keep)
    img = torch.randn(B, 3, S, S, device=dev)
    img8 = torch.randint(0, 256, (B, 3, S, S), dtype=torch.uint8, device=dev)
    mean, std = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
    pos = torch.randn(n_p + 1, D, device=dev)
    rows_full = torch.empty(B * n_p, kp, dtype=torch.bfloat16, device=dev)
    rows_keep = torch.empty(B * n_keep, kp, dtype=torch.bfloat16, device=dev)
    dE_full = torch.randn(B * (n_p + 1), D, device=dev).to(torch.bfloat16)
    dE_keep = torch.randn(B * (n_keep + 1), D, device=dev).to(torch.bfloat16)
    dconv_full = torch.empty(B * n_p, D, dtype=torch.bfloat16, device=dev)
    dconv_keep = torch.empty(B * n_keep, D, dtype=torch.bfloat16, device=dev)
    gpos, gcls, gb = torch.zeros((n_p + 1) * D, device=dev), torch.zeros(D, device=dev), torch.zeros(D, device=dev)

    cases = (
        ("patch_keep_table", lambda: ext.patch_keep_table(seed, PATCH_DROP_SITE << 32, B, n_p, n_keep)),
        ("pos_gather", lambda: ext.pos_gather(pos, keep)),
        ("im2col/plain", lambda: ext.im2col(img, rows_full, P, kp)),
        ("im2col/keep", lambda: ext.im2col(img, rows_keep, P, kp, keep=keep)),
        ("im2col_u8/plain", lambda: ext.im2col_u8(img8, rows_full, mean, std, None, S, S, P, kp)),
        ("im2col_u8/keep", lambda: ext.im2col_u8(img8, rows_keep, mean, std, None, S, S, P, kp, keep=keep)),
        ("patch_bwd/plain", lambda: ext.patch_bwd(dE_full, B, n_p + 1, D, gpos, gcls, dconv_full, gb, seed, 0, 0.1)),
        ("patch_bwd/keep", lambda: ext.patch_bwd(dE_keep, B, n_p + 1, D, gpos, gcls, dconv_keep, gb, seed, 0, 0.1, inv=inv,
                                                  n_keep=n_keep)),
    )
    res = {"shape": {"B": B, "n_p": n_p, "n_keep": n_keep, "D": D, "kp": kp}, "rate": rate, "reps": reps, "mean_us": {}}
    for name, fn in cases:
        for _ in range(2):
            fn()
        torch.cuda.synchronize(dev)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(reps + 1)]
        ev[0].record()
        for i in range(reps):
            fn()
            ev[i + 1].record()
        torch.cuda.synchronize(dev)
        t = sorted(ev[i].elapsed_time(ev[i + 1]) * 1e3 for i in range(reps))
        res["mean_us"][name] = {"mean": round(sum(t) / len(t), 2), "min": round(t[0], 2), "max": round(t[-1], 2)}
    # bytes the addend gather writes (the embedding GEMM's epilogue reads them back once)
    res["pos_gather_bytes"] = B * (n_keep + 1) * D * 4
    _write(res, out)


def parse_trace(directory, reps):
    rows = {}
    for path in glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True):
        with open(path, newline="") as f:
            for r in csv.DictReader(f):
                name = r["Kernel_Name"]
                hit = next((k for k in KERNELS if k in name), None)
                if hit:
                    key = name[name.find(hit):].split("(")[0]
                    rows.setdefault(key, []).append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"])))
    res = {}
    for key, rs in sorted(rows.items()):
        rs.sort()
        t = sorted(c[1] for c in rs[2:]) or [c[1] for c in rs]  # the first two launches of an instantiation are warm-up
        res[key] = {"launches": len(t), "mean_us": round(sum(t) / len(t) / 1e3, 2), "min_us": round(t[0] / 1e3, 2),
                    "max_us": round(t[-1] / 1e3, 2)}
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
    p.add_argument("--rates", type=float, nargs="+", default=[0.25, 0.5], help="the patch-dropout arms beside the plain one")
    p.add_argument("--rate", type=float, default=0.5, help="--kernels-only: the rate of the keep variants")
    p.add_argument("--kernels-only", action="store_true")
    p.add_argument("--reps", type=int, default=22, help="launches per case with --kernels-only / --parse")
    p.add_argument("--parse", default=None, metavar="DIR")
    p.add_argument("--out", default=None)
    args = p.parse_args(argv)
    if args.parse:
        parse_trace(args.parse, args.reps)
        return 0
    S, B, C = args.image_size, args.batch, args.classes
    if args.kernels_only:
        kernels_only(B, S, 16, 768, args.rate, args.reps, args.out)
        return 0

    from pytorch_vit_paper_replication_amd.models import vit
    from pytorch_vit_paper_replication_amd.ops import fused_vit
    from pytorch_vit_paper_replication_amd.optim import FusedAdam, param_groups_weight_decay, warmup_linear_decay

    device = torch.device("cuda:0")
    torch.manual_seed(0)
    model = vit(args.model, image_size=S, num_classes=C).to(device)
    opt = FusedAdam(param_groups_weight_decay(model, 0.03), lr=1e-4)
    sched = warmup_linear_decay(opt, 10 ** 6, 0.05)
    g = torch.Generator().manual_seed(0)
    X, y = torch.randn(B, 3, S, S, generator=g).to(device), torch.randint(0, C, (B,), generator=g).to(device)

    def run(steps, rate):
        model.set_patch_dropout(rate)
        model.train()
        for _ in range(steps):
            loss = fused_vit.cross_entropy(model(X), y)
            opt.zero_grad()
            fused_vit.backward(loss)
            opt.step(clip_norm=1.0)
            sched.step()
        torch.cuda.synchronize(device)

    arms = [("plain", 0.0)] + [(f"rate_{r:g}", r) for r in args.rates]
    for _, rate in arms:
        run(args.warmup, rate)
    vals = {k: [] for k, _ in arms}
    for _ in range(args.rounds):
        for name, rate in arms:
            torch.cuda.synchronize(device)
            t0 = time.perf_counter()
            run(args.steps, rate)
            vals[name].append(round(B * args.steps / (time.perf_counter() - t0), 1))
    med = {k: sorted(v)[len(v) // 2] for k, v in vals.items()}
    n_p = model.patch_embedding_block.number_of_patches
    from pytorch_vit_paper_replication_amd.models.vit import patch_keep_count

    result = {"model": args.model, "image_size": S, "batch": B, "steps": args.steps, "rounds": args.rounds, "img_per_s": vals,
              "median": med, "plain_spread": round(max(vals["plain"]) - min(vals["plain"]), 1),
              "tokens": {k: patch_keep_count(n_p, r) + 1 for k, r in arms},
              "speedup_over_plain": {k: round(med[k] / med["plain"], 4) for k, _ in arms[1:]},
              "token_ratio": {k: round((patch_keep_count(n_p, r) + 1) / (n_p + 1), 4) for k, r in arms[1:]}}
    _write(result, args.out)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
