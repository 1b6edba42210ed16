#!/usr/bin/env python3
"""Record what the reference implementation computes, as the fixtures of tests/test_model_parity.py.

The parity tests compare this project's ``models.vit`` with the reference's pure-PyTorch model. They
read recorded data only (tests/golden/), so that the suite runs where the reference is absent; this
script writes that data from a checkout of the reference:

  python scripts/make_reference_fixtures.py --reference /path/to/reference [--out tests/golden]

Everything is CPU fp32 and seeded. The files hold tensors, names and shapes only:

  ref_vit_small_seed7.pth   the reference's own checkpoint (state_dict) of ViT(**SMALL) built under seed 7
  ref_vit_small_io.pt       a batch, the reference's eval logits for it and its parameter gradients
  ref_vit_blocks_seed3.pt   one encoder block and one patch embedding: weights, inputs, outputs
  ref_vit_no_classifier_keys.json   the state_dict keys of the reference's headless ViT
"""
import argparse
import importlib.util
import json
import os

import torch

SMALL = dict(image_size=32, patch_size=8, num_transformer_layer=2, num_heads=2, embedding_dim=64, mlp_size=128,
             num_classes=5)


def _load(root, rel, name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(root, rel))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference implementation")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  "tests", "golden"))
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    ref = _load(args.reference, "models/vit.py", "ref_vit")
    ref_nc = _load(args.reference, "models/vit_no_classifier.py", "ref_vit_nc")

    torch.manual_seed(7)
    m = ref.ViT(**SMALL)
    torch.save(m.state_dict(), os.path.join(args.out, "ref_vit_small_seed7.pth"))

    # same weights with dropout off: eval logits and train-mode gradients of sum(logsumexp(logits))
    r = ref.ViT(**dict(SMALL, mlp_dropout=0.0, embedding_dropout=0.0))
    r.load_state_dict(m.state_dict())
    torch.manual_seed(0)
    x = torch.randn(3, 3, 32, 32)
    r.eval()
    with torch.no_grad():
        logits = r(x)
    r.train()
    r(x).logsumexp(1).sum().backward()
    torch.save({"x": x, "eval_logits": logits, "grads": {n: p.grad.clone() for n, p in r.named_parameters()}},
               os.path.join(args.out, "ref_vit_small_io.pt"))

    torch.manual_seed(3)
    blk = ref.TransformerEncoderBlock(embedding_dim=64, num_heads=4, mlp_size=128, mlp_dropout=0.0)
    bx = torch.randn(2, 10, 64)
    pe = ref.PatchEmbedding(image_size=32, patch_size=8, embedding_dim=64, embedding_dropout=0.0)
    img = torch.randn(2, 3, 32, 32)
    with torch.no_grad():
        torch.save({"block_state": blk.state_dict(), "block_x": bx, "block_out": blk(bx),
                    "patch_state": pe.state_dict(), "patch_x": img, "patch_out": pe(img)},
                   os.path.join(args.out, "ref_vit_blocks_seed3.pt"))

    cfg = {k: v for k, v in SMALL.items() if k != "num_classes"}
    with open(os.path.join(args.out, "ref_vit_no_classifier_keys.json"), "w") as f:
        json.dump(list(ref_nc.ViT(**cfg).state_dict()), f, indent=1)
        f.write("\n")
    for n in sorted(os.listdir(args.out)):
        print(f"{os.path.getsize(os.path.join(args.out, n)):8d}  {n}")


if __name__ == "__main__":
    main()
