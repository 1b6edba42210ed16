"""LayerScale: what the fold and the unfold cost.

Training-step A/B (ViT-B/16, batch 256, one device-resident float batch, one process, arms alternating; the hand
loop of scripts/drop_path_bench.py: forward, fused cross-entropy, zero_grad, backward, clipped FusedAdam step,
scheduler step), each arm a model of its own with its own optimizer:

  (u)  the plain model;
  (s)  ``set_layer_scale(--init)``: one fold per step, two unfolds per block per backward.

Each value is wall time of ``--steps`` steps closed by a synchronise.

    python scripts/layer_scale_bench.py --out profiles/layer_scale/step_ab.json

Kernel times: ``--kernels-only`` launches the fold over the 2 L scaled weights of the model (one launch) and the
two unfolds of one block (out-projection [D, D], fc2 [D, M]) ``--reps`` times each and prints device-event times;
under ``rocprofv3 --kernel-trace --stats`` the same run gives the profiler's figures (``layerscale_*`` rows).

    rocprofv3 --kernel-trace --stats -d DIR --output-format csv -- python scripts/layer_scale_bench.py --kernels-only
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.environ.get("PVR_PKG_ROOT") or os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _timed(fn, reps, dev):
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
    return {"mean": round(sum(t) / len(t), 2), "min": round(t[0], 2), "max": round(t[-1], 2)}


def kernels_only(model_name, S, init, reps, out):
    from pytorch_vit_paper_replication_amd import _ext
    from pytorch_vit_paper_replication_amd.models import vit
    from pytorch_vit_paper_replication_amd.runtime.param_store import get_store

    ext = _ext.ext()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = vit(model_name, image_size=S, num_classes=1000, layer_scale=init).to(dev)
    store = get_store(model, dev)
    triples = [t for blk in model.transformer_encoder for t in blk.folded_triples()]
    store.register_folded(triples)
    elems = sum(w.numel() for w, _, _ in triples)

    def fold():
        store._f_generation = -1
        store.fold()

    res = {"model": model_name, "reps": reps, "scaled_elements": elems, "us": {}}
    res["us"]["fold"] = _timed(fold, reps, dev)
    res["fold_bytes"] = 8 * elems  # 4 read, 2 + 2 written per element
    res["fold_TB_per_s"] = round(res["fold_bytes"] / res["us"]["fold"]["mean"] / 1e6, 3)
    total = 0.0
    for name, (w, b, g) in (("unfold_out_proj", triples[0]), ("unfold_fc2", triples[1])):
        dwh, dbh = torch.randn_like(w), torch.randn_like(b)
        gw, gb, gg = store.grad_dest(w), store.grad_dest(b), store.grad_dest(g)
        res["us"][name] = _timed(lambda: ext.layerscale_unfold(dwh, dbh, w, b, g, gW=gw, gb=gb, gg=gg), reps, dev)
        res["us"][name + "_scratch_clear"] = _timed(lambda: torch.zeros_like(dwh), reps, dev)
        total += res["us"][name]["mean"] + res["us"][name + "_scratch_clear"]["mean"]
    L = len(model.transformer_encoder)
    res["unfold_per_step_us"] = round(total * L, 1)  # both branches of every block, scratch clears included
    res["unfold_bytes"] = 20 * elems  # clear 4, GEMM's out += is not counted; dW-hat 4, W 4, gW 4 + 4
    print(json.dumps(res), flush=True)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


def main(argv=None) -> int:
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    p.add_argument("--model", default="vit_b16")
    p.add_argument("--image-size", type=int, default=224)
    p.add_argument("--batch", type=int, default=256)
    p.add_argument("--classes", type=int, default=1000)
    p.add_argument("--steps", type=int, default=100)
    p.add_argument("--warmup", type=int, default=10)
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--init", type=float, default=1e-4)
    p.add_argument("--kernels-only", action="store_true")
    p.add_argument("--reps", type=int, default=22, help="launches per kernel with --kernels-only")
    p.add_argument("--out", default=None)
    args = p.parse_args(argv)
    S, B, C = args.image_size, args.batch, args.classes
    if args.kernels_only:
        kernels_only(args.model, S, args.init, args.reps, args.out)
        return 0

    from pytorch_vit_paper_replication_amd.models import vit
    from pytorch_vit_paper_replication_amd.ops import fused_vit
    from pytorch_vit_paper_replication_amd.optim import FusedAdam, param_groups_weight_decay, warmup_linear_decay

    device = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    X, y = torch.randn(B, 3, S, S, generator=g).to(device), torch.randint(0, C, (B,), generator=g).to(device)

    def arm(layer_scale):
        torch.manual_seed(0)
        model = vit(args.model, image_size=S, num_classes=C, layer_scale=layer_scale).to(device)
        opt = FusedAdam(param_groups_weight_decay(model, 0.03), lr=1e-4)
        sched = warmup_linear_decay(opt, 10 ** 6, 0.05)

        def run(steps):
            model.train()
            for _ in range(steps):
                loss = fused_vit.cross_entropy(model(X), y)
                opt.zero_grad()
                fused_vit.backward(loss)
                opt.step(clip_norm=1.0)
                sched.step()
            torch.cuda.synchronize(device)

        return run

    arms = (("u_plain", arm(None)), ("s_layer_scale", arm(args.init)))
    for _, run in arms:
        run(args.warmup)
    vals = {k: [] for k, _ in arms}
    for _ in range(args.rounds):
        for name, run in arms:
            torch.cuda.synchronize(device)
            t0 = time.perf_counter()
            run(args.steps)
            vals[name].append(round(B * args.steps / (time.perf_counter() - t0), 1))
    u = vals["u_plain"]
    med = {k: sorted(v)[len(v) // 2] for k, v in vals.items()}
    spread = round(max(u) - min(u), 1)
    result = {"model": args.model, "image_size": S, "batch": B, "steps": args.steps, "rounds": args.rounds, "init": args.init,
              "img_per_s": vals, "median": med, "plain_spread": spread,
              "layer_scale_over_plain": round(med["s_layer_scale"] / med["u_plain"], 4),
              "s_within_plain_spread": med["s_layer_scale"] >= med["u_plain"] - spread}
    print(json.dumps(result), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
