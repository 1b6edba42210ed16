"""Stochastic depth (drop path): what the fused row-scale term costs.

Training-step A/B (ViT-B/16, batch 256, one device-resident float batch, one process, arms alternating;
the hand loop of scripts/model_ema_bench.py: forward, fused cross-entropy, zero_grad, backward, clipped
FusedAdam step, scheduler step):

  (u)  the plain step;
  (d)  ``set_drop_path(--rate)``.

Each value is wall time of ``--steps`` steps closed by a synchronise.

    python scripts/drop_path_bench.py --out profiles/drop_path/step_ab.json

Kernel times: ``--kernels-only`` launches the three kernels that carry the term at the ViT-B/16 b256
shapes (T = 50,432 token rows), ``--reps`` times without and ``--reps`` times with it: the
out-projection forward (K = 768), the fc2 forward (K = 3072, with its element dropout) and the LayerNorm
backward (without / with the extra ``dz`` output). It prints device-event means itself; ``--parse DIR``
reads the ``*kernel_trace.csv`` a profiler run of it left in DIR (no counters collected in that run) and
prints the mean time per kernel instantiation, the first two launches of each dropped.

    rocprofv3 --kernel-trace --stats -d DIR --output-format csv -- python scripts/drop_path_bench.py --kernels-only
    python scripts/drop_path_bench.py --parse DIR
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


def kernels_only(B, N, D, M, rate, reps, out):
    from pytorch_vit_paper_replication_amd import _ext
    from pytorch_vit_paper_replication_amd.ops import gemm as G
    from pytorch_vit_paper_replication_amd.ops.fused_vit import DROP_PATH_SITE

    ext = _ext.ext()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    T = B * N
    seed = torch.tensor([20240611], dtype=torch.int64, device=dev)
    o = torch.randn(T, D, device=dev).to(torch.bfloat16)
    h = torch.randn(T, M, device=dev).to(torch.bfloat16)
    wo = (0.02 * torch.randn(D, D, device=dev)).to(torch.bfloat16)
    w2 = (0.02 * torch.randn(D, M, device=dev)).to(torch.bfloat16)
    bias = torch.zeros(D, device=dev)
    x = torch.randn(T, D, device=dev).to(torch.bfloat16)
    y = torch.empty(T, D, dtype=torch.bfloat16, device=dev)
    gamma = torch.ones(D, device=dev)
    _, mean, rstd = ext.layernorm_fwd(x, gamma, bias, 1e-5, T, D)
    dx, dz = torch.empty_like(x), torch.empty_like(x)
    dw, db, ds = (torch.zeros(D, device=dev) for _ in range(3))
    dpa = (seed, DROP_PATH_SITE << 32, rate, N)
    dpm = (seed, (DROP_PATH_SITE + 1) << 32, rate, N)
    drop2 = (seed, 2 << 32, 0.1)

    def out_proj(dp):
        G.linear_fwd(o, wo, bias, resid=x, out=y, drop_path=dp)

    def fc2(dp):
        G.linear_fwd(h, w2, bias, resid=x, drop=drop2, out=y, drop_path=dp)

    def ln_bwd(dp):
        kw = dict(dz=dz, **G._drop_path_kw(dp)) if dp is not None else {}
        ext.layernorm_bwd(o, D, x, D, mean, rstd, gamma, h[:, :D], M, dx, D, dw, db, T, dsum=ds, **kw)

    res = {"shape": {"T": T, "D": D, "M": M}, "rate": rate, "reps": reps, "mean_us": {}}
    for name, fn, site in (("out_proj_fwd", out_proj, dpa), ("fc2_fwd", fc2, dpm), ("ln2_bwd", ln_bwd, dpa)):
        for label, dp in (("plain", None), ("drop_path", site)):
            for _ in range(2):
                fn(dp)
            torch.cuda.synchronize(dev)
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(reps + 1)]
            ev[0].record()
            for i in range(reps):
                fn(dp)
                ev[i + 1].record()
            torch.cuda.synchronize(dev)
            t = sorted(ev[i].elapsed_time(ev[i + 1]) * 1e3 for i in range(reps))
            res["mean_us"][f"{name}/{label}"] = {"mean": round(sum(t) / len(t), 2), "min": round(t[0], 2), "max": round(t[-1], 2)}
        a, b = res["mean_us"][f"{name}/plain"]["mean"], res["mean_us"][f"{name}/drop_path"]["mean"]
        res["mean_us"][f"{name}/ratio"] = round(b / a, 4)
    # bytes the LayerNorm backward moves: reads dy, x, dres; writes dx (+ dz with drop path)
    res["ln2_bwd_byte_ratio"] = round(5 / 4, 3)
    print(json.dumps(res), flush=True)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


def parse_trace(directory, reps):
    rows = {}
    for path in glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True):
        with open(path, newline="") as f:
            for r in csv.DictReader(f):
                name = r["Kernel_Name"]
                if "gemm_" in name or "ln_bwd_kernel" in name:
                    key = name[name.find("gemm_") if "gemm_" in name else name.find("ln_bwd_kernel"):].split("(")[0]
                    rows.setdefault(key, []).append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"])))
    res = {}
    per = reps + 2  # launches per (kernel, variant): two warm-up launches, then `reps`
    for key, rs in sorted(rows.items()):
        rs.sort()
        # one GEMM instantiation serves the out-projection and then the fc2 shape: consecutive runs of `per`
        phases = ["out_proj_fwd", "fc2_fwd"] if "gemm_" in key and len(rs) == 2 * per else [""]
        for i, ph in enumerate(phases):
            chunk = rs[i * per:(i + 1) * per] if ph else rs
            t = sorted(c[1] for c in chunk[2:]) or [c[1] for c in chunk]  # the first two launches of a variant are warm-up
            res[(ph + " " if ph else "") + key] = {"launches": len(t), "mean_us": round(sum(t) / len(t) / 1e3, 2),
                                                   "min_us": round(t[0] / 1e3, 2), "max_us": round(t[-1] / 1e3, 2)}
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
    p.add_argument("--rate", type=float, default=0.1)
    p.add_argument("--schedule", default="linear", choices=["linear", "constant"])
    p.add_argument("--kernels-only", action="store_true")
    p.add_argument("--reps", type=int, default=22, help="launches per variant with --kernels-only / --parse")
    p.add_argument("--parse", default=None, metavar="DIR")
    p.add_argument("--out", default=None)
    args = p.parse_args(argv)
    if args.parse:
        parse_trace(args.parse, args.reps)
        return 0
    S, B, C = args.image_size, args.batch, args.classes
    if args.kernels_only:
        kernels_only(B, (S // 16) ** 2 + 1, 768, 3072, args.rate, args.reps, args.out)
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
        model.set_drop_path(rate, args.schedule)
        model.train()
        for _ in range(steps):
            loss = fused_vit.cross_entropy(model(X), y)
            opt.zero_grad()
            fused_vit.backward(loss)
            opt.step(clip_norm=1.0)
            sched.step()
        torch.cuda.synchronize(device)

    arms = (("u_plain", 0.0), ("d_drop_path", args.rate))
    for _, rate in arms:
        run(args.warmup, rate)
    vals = {k: [] for k, _ in arms}
    for _ in range(args.rounds):
        for name, rate in arms:
            torch.cuda.synchronize(device)
            t0 = time.perf_counter()
            run(args.steps, rate)
            vals[name].append(round(B * args.steps / (time.perf_counter() - t0), 1))
    u = vals["u_plain"]
    med = {k: sorted(v)[len(v) // 2] for k, v in vals.items()}
    spread = round(max(u) - min(u), 1)
    result = {"model": args.model, "image_size": S, "batch": B, "steps": args.steps, "rounds": args.rounds, "rate": args.rate,
              "schedule": args.schedule, "img_per_s": vals, "median": med, "plain_spread": spread,
              "drop_path_over_plain": round(med["d_drop_path"] / med["u_plain"], 4),
              "d_within_plain_spread": med["d_drop_path"] >= med["u_plain"] - spread}
    print(json.dumps(result), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
