"""Patch-embedding GEMM (the production user of the shared row-remapped epilogue), ViT-B/16 b256."""
import os, statistics, sys
import torch
sys.path.insert(0, os.environ.get("PVR_PKG_ROOT") or os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from pytorch_vit_paper_replication_amd.ops import gemm as G
B, n_p, D, K = 256, 196, 768, 768
torch.manual_seed(0)
x = torch.randn(B * n_p, K, device="cuda", dtype=torch.bfloat16)
w = (torch.randn(D, K, device="cuda") * 0.02).to(torch.bfloat16)
b = torch.randn(D, device="cuda")
pos = torch.randn(n_p + 1, D, device="cuda")
out = torch.empty(B * (n_p + 1), D, device="cuda", dtype=torch.bfloat16)
seed = torch.tensor([1234], dtype=torch.int64, device="cuda")
fn = lambda: G.linear_fwd(x, w, b, addend=pos, addend_period=n_p + 1, row_remap=(n_p, n_p + 1, 1), drop=(seed, 0, 0.1), out=out)
ts = []
for r in range(7):
    for _ in range(5): fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(50): fn()
    e.record(); torch.cuda.synchronize()
    ts.append(s.elapsed_time(e) / 50)
print(f"patch-embed GEMM M{B*n_p} N{D} K{K} row-remap+addend+dropout: median {statistics.median(ts):.4f} ms, min {min(ts):.4f}, max {max(ts):.4f}")
