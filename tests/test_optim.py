"""Optimizer recipe parity: FusedAdam (reference-math fallback) vs torch.optim.Adam, param groups,
warmup/decay schedule (MAIN.ipynb:2792-2960)."""
import math

import numpy as np
import pytest
import torch

from tests import optim_reference as R
from pytorch_vit_paper_replication_amd.models import ViT
from pytorch_vit_paper_replication_amd.optim import FusedAdam, param_groups_weight_decay, warmup_linear_decay

SMALL = dict(image_size=32, patch_size=8, num_transformer_layer=2, num_heads=2, embedding_dim=32, mlp_size=64,
             num_classes=4)


def test_param_groups_counts_vit_b16():
    g = param_groups_weight_decay(ViT(num_classes=3), 0.03)
    assert len(g[0]["params"]) == 52 and sum(p.numel() for p in g[0]["params"]) == 85_678_848
    assert len(g[1]["params"]) == 100 and sum(p.numel() for p in g[1]["params"]) == 122_115
    assert g[0]["weight_decay"] == 0.03 and g[1]["weight_decay"] == 0.0


def test_fused_adam_matches_torch_adam_cpu():
    torch.manual_seed(0)
    a, b = ViT(**SMALL), ViT(**SMALL)
    b.load_state_dict(a.state_dict())
    oa = FusedAdam(param_groups_weight_decay(a, 0.03), lr=1e-2)
    ob = torch.optim.Adam(param_groups_weight_decay(b, 0.03), lr=1e-2, betas=(0.9, 0.999))
    for it in range(4):
        for pa, pb in zip(a.parameters(), b.parameters()):
            gr = torch.randn_like(pa) * (it + 1)
            pa.grad = gr.clone()
            pb.grad = gr.clone()
        oa.step(clip_norm=1.0)
        torch.nn.utils.clip_grad_norm_(b.parameters(), 1.0)
        ob.step()
    for pa, pb in zip(a.parameters(), b.parameters()):
        assert torch.allclose(pa, pb, atol=1e-6, rtol=1e-5)


def test_adamw_decoupled():
    torch.manual_seed(0)
    a, b = ViT(**SMALL), ViT(**SMALL)
    b.load_state_dict(a.state_dict())
    oa = FusedAdam(a.parameters(), lr=1e-2, weight_decay=0.1, decoupled_weight_decay=True)
    ob = torch.optim.AdamW(b.parameters(), lr=1e-2, weight_decay=0.1)
    for _ in range(3):
        for pa, pb in zip(a.parameters(), b.parameters()):
            gr = torch.randn_like(pa)
            pa.grad, pb.grad = gr.clone(), gr.clone()
        oa.step()
        ob.step()
    for pa, pb in zip(a.parameters(), b.parameters()):
        assert torch.allclose(pa, pb, atol=1e-6, rtol=1e-5)


@pytest.mark.parametrize("betas", R.BETAS, ids=lambda b: f"betas{b[0]}-{b[1]}")
@pytest.mark.parametrize("kind", ["coupled", "decoupled", "wd0"])
def test_adam_step64_matches_torch_float64(kind, betas):
    """The float64 reference of the GPU optimizer checks against torch.optim.Adam / AdamW run in float64
    (single-tensor), 4 steps on the checks' input recipe: 1e-12 relative, elementwise."""
    n, lr, eps = 1500, 1e-2, 1e-8
    wd = {"coupled": 0.03, "decoupled": 0.1, "wd0": 0.0}[kind]
    gen = torch.Generator().manual_seed(11)
    p0 = R.adam_inputs(n, gen)
    tp = torch.nn.Parameter(p0.double().clone())
    cls = torch.optim.AdamW if kind == "decoupled" else torch.optim.Adam
    opt = cls([tp], lr=lr, betas=betas, eps=eps, weight_decay=wd, foreach=False)
    p, m, v = p0.double(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    for step in range(1, 5):
        g = R.adam_grad(n, gen)
        assert int((g == 0).sum()) == len(range(0, n, 97)) and 1e-6 <= float(g[g != 0].abs().min()) and float(g.abs().max()) <= 1e2
        tp.grad = g.double()
        opt.step()
        p, m, v = R.adam_step64(p, g, m, v, R.group_row(lr, betas, eps, wd, step, kind == "decoupled"))
        st = opt.state[tp]
        for got, want in ((p, tp.detach()), (m, st["exp_avg"]), (v, st["exp_avg_sq"])):
            assert got.dtype == torch.float64
            torch.testing.assert_close(got, want, rtol=1e-12, atol=0.0)
    assert not torch.equal(p, p0.double())


def test_adam_step64_reads_a_float32_table_row_and_scales_the_gradient():
    gen = torch.Generator().manual_seed(3)
    p, g = R.adam_inputs(64, gen), R.adam_grad(64, gen)
    z = torch.zeros(64)
    tab = R.table_f32([R.group_row(1e-3, (0.8, 0.95), 1e-6, 0.1, 2, True), R.group_row(1e-3, (0.8, 0.95), 1e-6, 0.1, 2, False)])
    assert R.row_values(tab[0])[7] is True and R.row_values(tab[1])[7] is False
    assert R.row_values(tab[0])[0] == float(np.float32(1e-3))
    a = R.adam_step64(p, g, z, z, tab[1], 0.25)
    b = R.adam_step64(p, g * 0.25, z, z, tab[1])  # a power of two: the scaled gradient is exact
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    assert not torch.equal(a[0], R.adam_step64(p, g, z, z, tab[0], 0.25)[0])


def test_group_array_bias_corrections_and_flag_bits():
    """FusedAdam._group_array(step): bc1 = 1 - b1^t and bc2_sqrt = sqrt(1 - b2^t) from float64, rounded
    to fp32 once; the decoupled flag as integer bits; step 0 is treated as step 1."""
    ps = [torch.nn.Parameter(torch.zeros(4)) for _ in range(3)]
    groups = [dict(params=[ps[0]], lr=1e-2, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.03),
              dict(params=[ps[1]], lr=1e-3, betas=(0.8, 0.95), eps=1e-6, weight_decay=0.1, decoupled_weight_decay=True),
              dict(params=[ps[2]], lr=0.0, betas=(0.0, 0.5), eps=1e-5, weight_decay=0.0)]
    opt = FusedAdam(groups)
    for step in (1, 2, 10, 1000, 100000):
        arr = opt._group_array(step)
        assert arr.dtype == np.float32 and arr.shape == (3, 10)
        for i, g in enumerate(groups):
            b1, b2 = g["betas"]
            want = [g["lr"], b1, b2, g["eps"], g["weight_decay"], 1.0 - b1 ** step, math.sqrt(1.0 - b2 ** step)]
            assert arr[i, :7].tolist() == [float(np.float32(x)) for x in want], (step, i)
            # 1 - beta rounded once from the double, not formed from the fp32 beta
            assert arr[i, 8:].tolist() == [float(np.float32(1.0 - b1)), float(np.float32(1.0 - b2))], (step, i)
        assert np.array_equal(arr, R.table_f32([R.group_row(g["lr"], g["betas"], g["eps"], g["weight_decay"], step,
                                                            g.get("decoupled_weight_decay", False)) for g in groups]))
        assert arr.view(np.int32)[:, 7].tolist() == [0, 1, 0]
    assert abs(float(arr[0, 9]) / 1e-3 - 1.0) < 2.0 ** -24 < abs((1.0 - float(arr[0, 2])) / 1e-3 - 1.0)
    assert opt._group_array(100000)[0, 5] == 1.0 and opt._group_array(100000)[0, 6] == 1.0
    # step 0 (a table asked for before the first step): the rows of step 1, no division by bc1 = 0
    t0 = opt._group_table(0, torch.device("cpu"))
    assert t0.dtype == torch.float32 and torch.equal(t0, torch.from_numpy(opt._group_array(1)))
    assert float(t0[0, 5]) == float(np.float32(1.0 - 0.9))


def test_integer_bf16_rounding_equals_the_cpu_conversion():
    torch.manual_seed(5)
    x = torch.cat([torch.randn(4099), R.cast_planted_values()])
    bits = x.view(torch.int32)
    planted = R.cast_planted_values().view(torch.int32) & 0xFFFF
    assert int((planted == 0x8000).sum()) >= 8 and int((planted == 0x7FFF).sum()) >= 8 and int((planted == 0x8001).sum()) >= 8
    sub = ((bits & 0x7F800000) == 0) & ((bits & 0x007FFFFF) != 0)
    assert not bool(sub.any()), "no fp32 subnormals in the value set"
    got = R.bf16_rne_bits(x)
    want = R.bf16_bits(x.to(torch.bfloat16))
    nan = torch.isnan(x)
    assert int(nan.sum()) == 3
    assert torch.equal(got[~nan], want[~nan])
    assert bool(R.bf16_is_nan(got[nan]).all()) and bool(R.bf16_is_nan(want[nan]).all())
    # ties go to the even upper half; the largest finite fp32 rounds to Inf
    f = lambda b: torch.tensor([b], dtype=torch.int64).to(torch.int32).view(torch.float32)  # noqa: E731
    assert int(R.bf16_rne_bits(f(0x3F808000))) == 0x3F80 and int(R.bf16_rne_bits(f(0x3F818000))) == 0x3F82
    assert int(R.bf16_rne_bits(f(0x7F7FFFFF))) == 0x7F80 and int(R.bf16_rne_bits(f(0x3F807FFF))) == 0x3F80
    assert int(R.bf16_rne_bits(f(0x3F808001))) == 0x3F81


def test_reference_helpers_norm_and_segments():
    x = torch.tensor([3.0, 4.0, 0.0, 12.0])
    assert R.norm64(x) == 13.0
    big = torch.full((1 << 20,), 1e-4)
    assert abs(R.norm64(big) / (float(np.float32(1e-4)) * 1024.0) - 1.0) < 1e-14
    eg = R.expand_segments([0, 4, 12, 16], [0, -1, 2, -1], 24)
    assert eg.tolist() == [0] * 4 + [-1] * 8 + [2] * 4 + [-1] * 8
    assert R.expand_segments([0], [1], 8).tolist() == [1] * 8


def test_warmup_linear_decay_matches_reference_schedule():
    """EPOCHS=10, 8 batches/epoch -> 80 steps, warmup 4, decay 76 (MAIN.ipynb cell 87 output)."""
    m = torch.nn.Linear(2, 2)
    o1 = torch.optim.Adam(m.parameters(), lr=1e-3)
    s1 = warmup_linear_decay(o1, 80, 0.05)
    o2 = torch.optim.Adam(m.parameters(), lr=1e-3)
    w = torch.optim.lr_scheduler.LinearLR(o2, start_factor=1e-6, end_factor=1, total_iters=4)
    d = torch.optim.lr_scheduler.LinearLR(o2, start_factor=1, end_factor=0, total_iters=76)
    s2 = torch.optim.lr_scheduler.SequentialLR(o2, schedulers=[w, d], milestones=[4])
    for _ in range(80):
        assert abs(o1.param_groups[0]["lr"] - o2.param_groups[0]["lr"]) < 1e-12
        o1.step(), o2.step()
        s1.step(), s2.step()
