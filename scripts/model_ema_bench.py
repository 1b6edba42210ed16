"""Model EMA: the step with the average inside the Adam pass against the usual post-step foreach update,
and the Adam kernel's time with and without it.

Training-step A/B (ViT-B/16, batch 256, one device-resident float batch, one process, arms alternating).
All three arms run the same hand loop (forward, fused cross-entropy, zero_grad, backward, clipped
FusedAdam step, scheduler step):

  (u)  no EMA;
  (a)  the EMA as users write it without this feature: a separate fp32 copy of every parameter, updated
       after ``optimizer.step()`` with ``torch._foreach_mul_`` + ``torch._foreach_add_``;
  (b)  ``ModelEma(model, decay).attach(optimizer)``: the average inside ``adam_t_kernel``.

Each value is wall time of ``--steps`` steps closed by a synchronise.

    python scripts/model_ema_bench.py --out profiles/model_ema/step_ab.json

Kernel times: ``--kernels-only`` steps a ViT-B/16 store (encoder weights registered, so ``adam_t_kernel``
runs) ``--reps`` times without and ``--reps`` times with an attached EMA on fixed synthetic gradients;
``--parse DIR`` reads the ``*kernel_trace.csv`` a profiler run of it left in DIR (no counters collected
in that run) and prints the mean time of either instantiation, the first two launches of each dropped.

    rocprofv3 --kernel-trace --stats -d DIR --output-format csv -- python scripts/model_ema_bench.py --kernels-only
    python scripts/model_ema_bench.py --parse DIR
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


def kernels_only(model_name, S, C, reps):
    from pytorch_vit_paper_replication_amd.models import vit
    from pytorch_vit_paper_replication_amd.optim import FusedAdam, ModelEma, param_groups_weight_decay
    from pytorch_vit_paper_replication_amd.runtime.param_store import get_store

    device = torch.device("cuda:0")
    torch.manual_seed(0)
    model = vit(model_name, image_size=S, num_classes=C).to(device)
    store = get_store(model, device)
    store.register_transposed([w for blk in model.transformer_encoder for w in blk.fused_params()[2:12:2] if w.dim() == 2])
    store.ensure_transposed()
    opt = FusedAdam(param_groups_weight_decay(model, 0.03), lr=1e-4)
    gen = torch.Generator(device=device).manual_seed(1)
    for q in model.parameters():  # per parameter: the store's padding keeps its zero gradient
        q.grad.normal_(generator=gen)
    ema = ModelEma(model, decay=0.9999)
    for attached in (False, True):
        if attached:
            ema.attach(opt)
            ema.fused_buffer()
        torch.cuda.synchronize(device)
        for _ in range(reps):
            opt.step(clip_norm=1.0)
        torch.cuda.synchronize(device)
    assert opt._tmeta_key is not None, "adam_t_kernel did not run"
    print(json.dumps({"kernels_only": True, "order": ["no ema", "ema"], "reps": reps, "model": model_name,
                      "store_elements": store.numel}))


def parse_trace(directory, reps):
    rows = {"no ema": [], "ema": []}
    for path in glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True):
        with open(path, newline="") as f:
            for r in csv.DictReader(f):
                name = r["Kernel_Name"]
                if "adam_t_kernel" in name:
                    key = "ema" if "adam_t_kernel<true>" in name.replace(" ", "") else "no ema"
                    rows[key].append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"]), name))
    res = {}
    for key, rs in rows.items():
        rs.sort()
        if len(rs) != reps:
            raise SystemExit(f"expected {reps} adam_t_kernel dispatches for '{key}', found {len(rs)}")
        t = sorted(c[1] for c in rs[2:])  # the first two launches of a variant are warm-up
        res[key] = {"launches": len(t), "mean_us": round(sum(t) / len(t) / 1e3, 2), "min_us": round(t[0] / 1e3, 2),
                    "max_us": round(t[-1] / 1e3, 2), "kernel": rs[0][2][rs[0][2].find("adam_t_kernel"):].split("(")[0]}
    res["ema / no ema"] = round(res["ema"]["mean_us"] / res["no ema"]["mean_us"], 3)
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
    p.add_argument("--decay", type=float, default=0.9999)
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
        kernels_only(args.model, S, C, args.reps)
        return 0

    from pytorch_vit_paper_replication_amd.models import vit
    from pytorch_vit_paper_replication_amd.ops import fused_vit
    from pytorch_vit_paper_replication_amd.optim import FusedAdam, ModelEma, param_groups_weight_decay, warmup_linear_decay

    device = torch.device("cuda:0")
    torch.manual_seed(0)
    model = vit(args.model, image_size=S, num_classes=C).to(device)
    opt = FusedAdam(param_groups_weight_decay(model, 0.03), lr=1e-4)
    sched = warmup_linear_decay(opt, 10 ** 6, 0.05)
    g = torch.Generator().manual_seed(0)
    X, y = torch.randn(B, 3, S, S, generator=g).to(device), torch.randint(0, C, (B,), generator=g).to(device)
    ema = ModelEma(model, decay=args.decay)
    params = [q for q in model.parameters() if q.requires_grad]
    copies = [q.detach().clone() for q in params]  # arm (a)'s average: its own tensors, outside the store
    d, w = args.decay, 1.0 - args.decay

    def foreach_update():
        torch._foreach_mul_(copies, d)
        torch._foreach_add_(copies, [q.detach() for q in params], alpha=w)

    def run(steps, after_step=None):
        model.train()
        for _ in range(steps):
            loss = fused_vit.cross_entropy(model(X), y)
            opt.zero_grad()
            fused_vit.backward(loss)
            opt.step(clip_norm=1.0)
            sched.step()
            if after_step is not None:
                after_step()
        torch.cuda.synchronize(device)

    def arm_u(steps):
        run(steps)

    def arm_a(steps):
        run(steps, foreach_update)

    def arm_b(steps):
        ema.attach(opt)
        try:
            run(steps)
        finally:
            ema.detach()

    arms = (("u_no_ema", arm_u), ("a_foreach", arm_a), ("b_model_ema", arm_b))
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
    u = vals["u_no_ema"]
    med = {k: sorted(v)[len(v) // 2] for k, v in vals.items()}
    spread = round(max(u) - min(u), 1)
    result = {"model": args.model, "image_size": S, "batch": B, "steps": args.steps, "rounds": args.rounds, "decay": args.decay,
              "img_per_s": vals, "median": med, "no_ema_spread": spread,
              "b_within_no_ema_spread": med["b_model_ema"] >= med["u_no_ema"] - spread,
              "ema_updates": ema.num_updates}
    print(json.dumps(result), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
