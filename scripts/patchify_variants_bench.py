"""Kernel times of the patchify instantiations that batch_mix_bench.py / random_erasing_bench.py do not launch:
the MIX and ERASE kernels under patch dropout (``--set keep``: float and uint8, half of the patches kept) and
under a crop box (``--set geom``: uint8 256 x 256 sources, boxes of 192 - 224 px, every other one flipped, with
and without patch dropout). 256 x 3 x 224 x 224, patch 16, the plans of those two scripts, ``--reps`` launches
per variant in a fixed order; ``--parse DIR`` reads the ``*kernel_trace.csv`` a profiler run left in DIR and
prints the mean time per variant (the first two launches of a variant are warm-up).

    rocprofv3 --kernel-trace --stats -d DIR --output-format csv -- python scripts/patchify_variants_bench.py --set keep
    python scripts/patchify_variants_bench.py --set keep --parse DIR

PVR_PKG_ROOT selects another build of the package (scripts/mk_abtree.sh), as in bench.py.
"""
from __future__ import annotations

import argparse
import csv
import glob
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.environ.get("PVR_PKG_ROOT") or os.path.dirname(HERE))

PLANS = ("cutmix", "mixup", "erase")
VARIANTS = {"keep": [f"{k} keep+{p}" for k in ("float", "u8") for p in PLANS],
            "geom": [f"geom {k}{p}" for k in ("", "keep+") for p in PLANS]}


def launch(which, reps):
    import torch

    from pytorch_vit_paper_replication_amd import _ext  # before the two scripts below, which put this tree first
    from pytorch_vit_paper_replication_amd.models.vit import patch_keep_count

    import batch_mix_bench
    import random_erasing_bench
    from pytorch_vit_paper_replication_amd.ops.fused_vit import ERASE_SITE, PATCH_DROP_SITE, SITE_SHIFT

    ext = _ext.ext()
    B, S, P = 256, 224, 16
    g = torch.Generator().manual_seed(0)
    xu = torch.randint(0, 256, (B, 3, S, S), generator=g, dtype=torch.uint8).cuda()
    xf = xu.float() / 255
    kp = (3 * P * P + 63) // 64 * 64
    n_p = (S // P) ** 2
    n_keep = patch_keep_count(n_p, 0.5)
    seed = torch.tensor([12345], dtype=torch.int64, device="cuda")
    keep, _ = ext.patch_keep_table(seed, PATCH_DROP_SITE << 32, B, n_p, n_keep)
    kept = torch.empty(B * n_keep, kp, dtype=torch.bfloat16, device="cuda")
    full = torch.empty(B * n_p, kp, dtype=torch.bfloat16, device="cuda")
    mean, std = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
    plans = batch_mix_bench.kernel_plans(B, S)
    ep = random_erasing_bench.kernel_plan(B, S)
    kws = [dict(mix=plans[n].on("cuda")[0], mix_host=plans[n].rows) for n in ("cutmix", "mixup")]
    kws.append(dict(erase=ep.on("cuda"), erase_host=ep.rows, erase_mode="pixel", erase_seed=seed, erase_offset=ERASE_SITE << SITE_SHIFT))
    if which == "keep":
        calls = [lambda kw: ext.im2col(xf, kept, P, kp, keep=keep, **kw),
                 lambda kw: ext.im2col_u8(xu, kept, mean, std, None, S, S, P, kp, keep=keep, **kw)]
    else:
        xs = torch.randint(0, 256, (B, 3, 256, 256), generator=g, dtype=torch.uint8).cuda()
        r = torch.rand(B, 3, generator=g)
        x0, y0, w = r[:, 0] * 32, r[:, 1] * 32, 192 + r[:, 2] * 32
        box = torch.stack([x0, y0, x0 + w, y0 + w], 1)
        box[::2] = box[::2][:, [2, 1, 0, 3]]
        geom = box.float().contiguous().cuda()
        calls = [lambda kw: ext.im2col_u8(xs, full, mean, std, geom, S, S, P, kp, **kw),
                 lambda kw: ext.im2col_u8(xs, kept, mean, std, geom, S, S, P, kp, keep=keep, **kw)]
    for call in calls:
        for kw in kws:
            for _ in range(reps):
                call(kw)
            torch.cuda.synchronize()
    print(json.dumps({"set": which, "order": VARIANTS[which], "reps": reps, "batch": B, "image_size": S, "n_keep": n_keep}))


def parse_trace(which, directory, reps):
    rows = []
    for path in glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True):
        with open(path, newline="") as f:
            for r in csv.DictReader(f):
                if "im2col" in r["Kernel_Name"]:
                    rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"]), r["Kernel_Name"]))
    rows.sort()
    if len(rows) != reps * len(VARIANTS[which]):
        raise SystemExit(f"expected {reps * len(VARIANTS[which])} im2col dispatches, found {len(rows)}")
    res = {}
    for i, v in enumerate(VARIANTS[which]):
        chunk = rows[i * reps:(i + 1) * reps][2:]
        t = sorted(c[1] for c in chunk)
        res[v] = {"mean_us": round(sum(t) / len(t) / 1e3, 2), "min_us": round(t[0] / 1e3, 2), "max_us": round(t[-1] / 1e3, 2),
                  "kernel": chunk[0][2][chunk[0][2].find("im2col"):].split("(")[0]}
    print(json.dumps(res, indent=1))


def main(argv=None) -> int:
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    p.add_argument("--set", choices=sorted(VARIANTS), required=True)
    p.add_argument("--reps", type=int, default=12)
    p.add_argument("--parse", default=None, metavar="DIR")
    args = p.parse_args(argv)
    if args.parse:
        parse_trace(args.set, args.parse, args.reps)
    else:
        launch(args.set, args.reps)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
