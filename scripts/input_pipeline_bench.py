"""Input-pipeline A/B: fp32 batches normalised on the host against uint8 batches preprocessed on the device.

Both arms feed the same model from pinned host memory through ``DevicePrefetcher`` in one process:

  (a) fp32 ``[B, 3, S, S]`` batches, already scaled and normalised: today's pipeline at its best (its
      per-image CPU transform is not charged to it);
  (b) uint8 ``[B, 3, S, S]`` batches with ``ViT.set_device_input``: the ``im2col_u8`` kernel scales and
      normalises while it gathers the patch rows.

Two workloads: the ``inference_mode`` forward, and the frozen-backbone ``feature_extractor`` training
step (forward, head backward, FusedAdam on the head). Per workload the arms alternate a/b/a/b/...
for ``--rounds`` rounds of ``--steps`` steps after a warm-up of both; each value is device time between two
events around the whole loop (copies included: the prefetcher's copy stream gates every step), closed by
a synchronise. The script also times the host transform that arm (b) removes (``ToDtype(scale=True)`` +
``Normalize`` on one CPU thread) and writes everything as JSON.

    python scripts/input_pipeline_bench.py --out profiles/input_u8/results.json
    rocprofv3 --kernel-trace --stats -d DIR -- python scripts/input_pipeline_bench.py --kernels-only

``--kernels-only`` runs a few forward steps of each arm and nothing else, for the kernel-time comparison
of ``im2col_kernel`` against ``im2col_u8_kernel`` under the profiler.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pytorch_vit_paper_replication_amd.data import DeviceInput, DevicePrefetcher  # noqa: E402
from pytorch_vit_paper_replication_amd.data.transforms import IMAGENET_MEAN, IMAGENET_STD, Normalize, ToDtype  # noqa: E402
from pytorch_vit_paper_replication_amd.models import feature_extractor, vit  # noqa: E402
from pytorch_vit_paper_replication_amd.ops.fused_vit import cross_entropy  # noqa: E402
from pytorch_vit_paper_replication_amd.optim import FusedAdam  # noqa: E402


class PoolLoader:
    """``steps`` batches cycling through a small pool of pinned host batches (no per-step host work)."""

    def __init__(self, pool, steps):
        self.pool, self.steps = pool, steps

    def __len__(self):
        return self.steps

    def __iter__(self):
        for k in range(self.steps):
            yield self.pool[k % len(self.pool)]


def make_pools(batch, size, classes, n_pool, seed=0):
    g = torch.Generator().manual_seed(seed)
    norm = Normalize(IMAGENET_MEAN, IMAGENET_STD)
    to_float = ToDtype(torch.float32, scale=True)
    u8, f32 = [], []
    for _ in range(n_pool):
        x = torch.randint(0, 256, (batch, 3, size, size), generator=g, dtype=torch.uint8)
        y = torch.randint(0, classes, (batch,), generator=g)
        u8.append((x.pin_memory(), y.pin_memory()))
        f32.append((norm(to_float(x)).pin_memory(), y.pin_memory()))
    return u8, f32


def host_transform_cost(size, images, seed=1):
    """Single-thread CPU seconds per image of ToDtype(scale=True) + Normalize on a uint8 CHW image."""
    g = torch.Generator().manual_seed(seed)
    norm = Normalize(IMAGENET_MEAN, IMAGENET_STD)
    to_float = ToDtype(torch.float32, scale=True)
    imgs = [torch.randint(0, 256, (3, size, size), generator=g, dtype=torch.uint8) for _ in range(16)]
    old = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        for im in imgs:
            norm(to_float(im))
        t0 = time.process_time()
        for k in range(images):
            norm(to_float(imgs[k % len(imgs)]))
        return (time.process_time() - t0) / images
    finally:
        torch.set_num_threads(old)


def timed_loop(step, pool, steps, device):
    """Device milliseconds for ``steps`` steps fed through a fresh DevicePrefetcher."""
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(device)
    start.record()
    for x, y in DevicePrefetcher(PoolLoader(pool, steps), device):
        step(x, y)
    end.record()
    end.synchronize()
    return start.elapsed_time(end)


def main(argv=None) -> int:
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    p.add_argument("--model", default="vit_b16")
    p.add_argument("--image-size", type=int, default=224)
    p.add_argument("--batch", type=int, default=256)
    p.add_argument("--classes", type=int, default=10, help="classes of the fine-tune head")
    p.add_argument("--steps", type=int, default=100)
    p.add_argument("--warmup", type=int, default=10)
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--pool", type=int, default=4, help="distinct pinned host batches per arm")
    p.add_argument("--host-images", type=int, default=256, help="images of the host transform timing")
    p.add_argument("--kernels-only", action="store_true", help="a few forward steps per arm, no timing (profiler runs)")
    p.add_argument("--out", default=None, help="write the JSON result here too")
    args = p.parse_args(argv)

    device = torch.device("cuda:0")
    torch.manual_seed(0)
    S, B = args.image_size, args.batch
    u8_pool, f32_pool = make_pools(B, S, args.classes, args.pool)
    spec = DeviceInput(IMAGENET_MEAN, IMAGENET_STD)

    infer_model = vit(args.model, image_size=S).to(device).eval().set_device_input(spec)

    def infer_step(x, y):
        with torch.inference_mode():
            infer_model(x)

    if args.kernels_only:
        for pool in (f32_pool, u8_pool, f32_pool, u8_pool):
            timed_loop(infer_step, pool, 5, device)
        torch.cuda.synchronize(device)
        print(json.dumps({"kernels_only": True, "steps_per_arm": 10, "batch": B, "image_size": S}))
        return 0

    tune_model = feature_extractor(vit(args.model, image_size=S), num_classes=args.classes, seed=0).to(device).train()
    tune_model.set_device_input(spec)
    opt = FusedAdam([q for q in tune_model.parameters() if q.requires_grad], lr=1e-3)

    def tune_step(x, y):
        loss = cross_entropy(tune_model(x), y)
        opt.zero_grad()
        loss.backward()
        opt.step(clip_norm=1.0)

    result = {
        "model": args.model, "image_size": S, "batch": B, "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds,
        "h2d_bytes_per_image": {"a_fp32": 3 * S * S * 4, "b_uint8": 3 * S * S},
        "host_transform_us_per_image": round(host_transform_cost(S, args.host_images) * 1e6, 1),
        "workloads": {},
    }
    for name, step in (("inference", infer_step), ("finetune_frozen_backbone", tune_step)):
        for pool in (f32_pool, u8_pool):
            timed_loop(step, pool, args.warmup, device)
        vals = {"a_fp32": [], "b_uint8": []}
        for _ in range(args.rounds):
            for arm, pool in (("a_fp32", f32_pool), ("b_uint8", u8_pool)):
                ms = timed_loop(step, pool, args.steps, device)
                vals[arm].append(round(B * args.steps / ms * 1e3, 1))
        a, b = vals["a_fp32"], vals["b_uint8"]
        spread_a = max(a) - min(a)
        result["workloads"][name] = {
            "img_per_s": vals, "median": {k: sorted(v)[len(v) // 2] for k, v in vals.items()},
            "a_spread": round(spread_a, 1),
            # acceptance: (b) is not slower than (a) by more than the spread of (a)'s own values
            "b_within_a_spread": sorted(b)[len(b) // 2] >= sorted(a)[len(a) // 2] - spread_a,
        }
        print(f"[{name}] a fp32 {a} img/s | b uint8 {b} img/s | spread(a) {spread_a:.1f}", flush=True)
    line = json.dumps(result)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
