"""FusedAdam through a real ParamStore against fp32 torch.optim.Adam / AdamW on a twin model, one step at
a time: the twin is loaded with the fused model's parameters and moments before every step, so two
valid fp32 runs cannot drift apart. Each step is also computed in float64 (tests/optim_reference.py)
from the same state; the fused kernels' error against it may be 4x torch's own on every metric (the
yardstick of tests/kernel_checks.py: same fp32 operations, another association). The reference takes
the user's double-precision hyperparameters, so the fp32 group table is under test too: these tests
found 1 - beta2 formed from the fp32 beta2 (v 1.29e-5, first updates 6.6e-6 from torch's at betas
(0.9, 0.999)), which the table now carries rounded from the double. The 128-wide 2-layer
model of tests/test_gpu_model_ema.py, through adam_kernel and adam_t_kernel, with and without padding
between segments."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import optim_reference as R  # noqa: E402
from tests.test_gpu_model_ema import BUCKET_LAYOUT, DEV, NODROP, _encoder_weights, _masks  # noqa: E402

KERNELS = pytest.mark.parametrize("transposed", [False, True], ids=["adam_kernel", "adam_t_kernel"])
KERNELS_LAYOUTS = pytest.mark.parametrize(
    "transposed,layout", [(False, None), (True, None), (True, BUCKET_LAYOUT), (False, BUCKET_LAYOUT)],
    ids=["adam_kernel", "adam_t_kernel", "adam_t_kernel-buckets", "adam_kernel-buckets"])


def _freeze(m):
    m.transformer_encoder[1].mlp_block.mlp[0].weight.requires_grad_(False)  # a registered (tile) weight
    m.transformer_encoder[0].msa_block.layer_norm.bias.requires_grad_(False)  # a flat segment


def _model(transposed, layout=None, freeze=False, seed=0):
    from pytorch_vit_paper_replication_amd.models import ViT
    from pytorch_vit_paper_replication_amd.runtime.param_store import get_store

    torch.manual_seed(seed)
    m = ViT(**NODROP).to(DEV)
    if freeze:
        _freeze(m)
    st = get_store(m, torch.device(DEV), layout=layout)
    if transposed:
        st.register_transposed(_encoder_weights(m))
        st.ensure_transposed()
    return m, st


def _twin(m, freeze=False):
    from pytorch_vit_paper_replication_amd.models import ViT

    t = ViT(**NODROP).to(DEV)
    t.load_state_dict(m.state_dict())
    if freeze:
        _freeze(t)
    assert getattr(t, "_pvr_store", None) is None
    return t


def _trainable(m):
    return [p for p in m.parameters() if p.requires_grad]


def _write_grads(models, it, scale=None):
    """The gradient recipe of the kernel checks (or randn * scale) into every model's p.grad."""
    gen = torch.Generator(device=DEV).manual_seed(4000 + it)
    for ps in zip(*[_trainable(m) for m in models]):
        n = ps[0].numel()
        g = (R.adam_grad(n, gen, DEV) if scale is None else torch.randn(n, generator=gen, device=DEV) * scale).view(ps[0].shape)
        for p in ps:
            if p.grad is None:
                p.grad = g.clone()
            else:
                p.grad.copy_(g)


def _fused(st, opt):
    return st.flat, opt._fused[1], opt._fused[2], st.shadow


def _run_against_torch(m, st, opt, twin, topt, steps, transposed, sched=None, tsched=None, what=""):
    """``steps`` bare steps (no clip: the flag-only norm call, coef exactly 1) of both optimizers from the
    same state; returns the lr of the first group at every step."""
    fp, tp = _trainable(m), _trainable(twin)
    decoupled = isinstance(topt, torch.optim.AdamW)
    lrs = []
    for it in range(steps):
        with torch.no_grad():
            for a, b in zip(m.parameters(), twin.parameters()):
                b.copy_(a)
        if it > 0:
            for a, b in zip(fp, tp):
                topt.state[b] = {"step": torch.tensor(float(it)), "exp_avg": opt.state[a]["exp_avg"].clone(),
                                 "exp_avg_sq": opt.state[a]["exp_avg_sq"].clone()}
        _write_grads((m, twin), it)
        before = {id(b): (b.detach().clone(), b.grad.clone(),
                          topt.state[b]["exp_avg"].clone() if it > 0 else torch.zeros_like(b),
                          topt.state[b]["exp_avg_sq"].clone() if it > 0 else torch.zeros_like(b)) for b in tp}
        for fg, tg in zip(opt.param_groups, topt.param_groups):
            assert fg["lr"] == tg["lr"] and fg["weight_decay"] == tg["weight_decay"] and tuple(fg["betas"]) == tuple(tg["betas"])
        lrs.append(topt.param_groups[0]["lr"])
        opt.step()
        topt.step()
        torch.cuda.synchronize()
        assert (opt._tmeta_key is not None) == transposed, "the other kernel ran"
        got, yard, ref = [[], [], []], [[], [], []], [[], [], []]
        index = {id(b): a for a, b in zip(fp, tp)}
        for tg in topt.param_groups:
            dec = decoupled or bool(tg.get("decoupled_weight_decay", False))
            row = R.group_row(tg["lr"], tg["betas"], tg["eps"], tg["weight_decay"], it + 1, dec)  # the user's doubles
            for b in tg["params"]:
                a = index[id(b)]
                p0, g0, m0, v0 = before[id(b)]
                r = R.adam_step64(p0, g0, m0, v0, row)
                for k, (x, y, z) in enumerate(((a.detach(), b.detach(), r[0]), (opt.state[a]["exp_avg"], topt.state[b]["exp_avg"], r[1]),
                                               (opt.state[a]["exp_avg_sq"], topt.state[b]["exp_avg_sq"], r[2]))):
                    base = p0.double() if k == 0 else 0.0
                    got[k].append((x.double() - base).reshape(-1))
                    yard[k].append((y.double() - base).reshape(-1))
                    ref[k].append((z - base).reshape(-1))
        from tests.kernel_checks import errs64

        for k, name in enumerate(("p_after - p_before", "m", "v")):
            rr = torch.cat(ref[k])
            ek, ey = errs64(torch.cat(got[k]), rr), errs64(torch.cat(yard[k]), rr)
            print(f"{what} step {it + 1} {name}: fused l2 {ek[0]:.2e} max {ek[1]:.2e}; fp32 torch l2 {ey[0]:.2e} max {ey[1]:.2e} (limit 4x)")
            assert ek[0] <= 4.0 * ey[0] and ek[1] <= 4.0 * ey[1], f"{what} step {it + 1} {name}: {ek} vs 4 x {ey}"
        if sched is not None:
            sched.step()
            tsched.step()
    return lrs


def _check_shadow(st, train):
    assert torch.equal(R.bf16_bits(st.shadow)[train], R.bf16_rne_bits(st.flat)[train])


@KERNELS_LAYOUTS
def test_adamw_decoupled_decay_matches_torch_adamw(transposed, layout):
    from pytorch_vit_paper_replication_amd.optim import FusedAdam

    m, st = _model(transposed, layout)
    twin = _twin(m)
    opt = FusedAdam(m.parameters(), lr=1e-2, weight_decay=0.1, decoupled_weight_decay=True)
    topt = torch.optim.AdamW(twin.parameters(), lr=1e-2, weight_decay=0.1, foreach=False)
    _run_against_torch(m, st, opt, twin, topt, 3, transposed, what="AdamW")
    _check_shadow(st, _masks(st)[0])
    assert bool((st.flat[_masks(st)[2]] == 0).all())


@KERNELS_LAYOUTS
def test_twelve_param_groups_use_the_device_table(transposed, layout):
    """More groups than the kernel arguments hold: FusedAdam uploads the table through its pinned ring."""
    from pytorch_vit_paper_replication_amd.optim import FusedAdam

    m, st = _model(transposed, layout)
    twin = _twin(m)

    def groups(model):
        ps = _trainable(model)
        return [dict(params=ps[i::12], lr=1e-3 * (i + 1), weight_decay=0.01 * i) for i in range(12)]

    opt = FusedAdam(groups(m), lr=1.0)
    topt = torch.optim.Adam(groups(twin), lr=1.0, foreach=False)
    _run_against_torch(m, st, opt, twin, topt, 3, transposed, what="12 groups")
    assert opt._table_dev is not None and tuple(opt._table_dev.shape) == (12, 10) and opt._table_dev.is_cuda
    want = torch.from_numpy(opt._group_array(3)).to(DEV)
    assert torch.equal(opt._table_dev, want), "the device table is not the last step's"
    _check_shadow(st, _masks(st)[0])


@KERNELS
def test_lambda_lr_warmup_reaches_the_kernel_step_by_step(transposed):
    from pytorch_vit_paper_replication_amd.optim import FusedAdam, param_groups_weight_decay

    m, st = _model(transposed)
    twin = _twin(m)
    opt = FusedAdam(param_groups_weight_decay(m, 0.03), lr=1e-2)
    topt = torch.optim.Adam(param_groups_weight_decay(twin, 0.03), lr=1e-2, foreach=False)
    lam = lambda s: min(1.0, (s + 1) / 5.0)  # noqa: E731
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lam)
    tsched = torch.optim.lr_scheduler.LambdaLR(topt, lam)
    lrs = _run_against_torch(m, st, opt, twin, topt, 5, transposed, sched, tsched, what="LambdaLR")
    assert lrs == [1e-2 * min(1.0, (s + 1) / 5.0) for s in range(5)] and len(set(lrs)) == 5


@KERNELS_LAYOUTS
def test_moments_state_and_step_counter_match_torch(transposed, layout):
    """The reference recipe (coupled decay 0.03, two groups): opt.state[p]'s exp_avg / exp_avg_sq are the
    kernel's moments and follow torch's step by step; the state dict carries the step count."""
    from pytorch_vit_paper_replication_amd.optim import FusedAdam, param_groups_weight_decay

    m, st = _model(transposed, layout, freeze=True)
    twin = _twin(m, freeze=True)
    opt = FusedAdam(param_groups_weight_decay(m, 0.03), lr=1e-2, betas=(0.8, 0.95), eps=1e-6)
    topt = torch.optim.Adam(param_groups_weight_decay(twin, 0.03), lr=1e-2, betas=(0.8, 0.95), eps=1e-6, foreach=False)
    _run_against_torch(m, st, opt, twin, topt, 3, transposed, what="moments")
    sd = opt.state_dict()["state"]
    assert len(sd) == len(_trainable(m)) and all(float(s["step"]) == 3.0 for s in sd.values())
    for p in _trainable(m):
        off = st.offset(p)
        assert torch.equal(opt.state[p]["exp_avg"].reshape(-1), opt._fused[1][off:off + p.numel()])
        assert torch.equal(opt.state[p]["exp_avg_sq"].reshape(-1), opt._fused[2][off:off + p.numel()])


@KERNELS_LAYOUTS
def test_padding_stays_zero_and_frozen_parameters_unchanged(transposed, layout):
    from pytorch_vit_paper_replication_amd.optim import FusedAdam, param_groups_weight_decay

    m, st = _model(transposed, layout, freeze=True)
    opt = FusedAdam(param_groups_weight_decay(m, 0.03), lr=1e-2)
    train, frozen, pad = _masks(st)
    assert int(frozen.sum()) == 256 * 128 + 128 and int(pad.sum()) > 0
    flat0, shadow0 = st.flat.clone(), st.shadow.clone()
    wt0 = st.shadow_t.clone() if transposed else None
    assert bool((flat0[pad] == 0).all())
    for it in range(3):
        _write_grads((m,), it)
        opt.step(clip_norm=1.0)
    torch.cuda.synchronize()
    assert (opt._tmeta_key is not None) == transposed
    flat, mm, vv, shadow = _fused(st, opt)
    for name, t in (("flat", flat), ("m", mm), ("v", vv), ("shadow", shadow.float())):
        assert bool((t[pad] == 0).all()), f"{name}: padding moved"
    assert torch.equal(flat[frozen], flat0[frozen]) and torch.equal(shadow[frozen], shadow0[frozen])
    assert bool((mm[frozen] == 0).all()) and bool((vv[frozen] == 0).all())
    assert not torch.equal(flat[train], flat0[train])
    _check_shadow(st, train)
    if transposed:
        w = m.transformer_encoder[1].mlp_block.mlp[0].weight
        assert torch.equal(st.bf16_t(w), st.bf16(w).t())
        for x in _encoder_weights(m):
            assert torch.equal(st.bf16_t(x), st.bf16(x).t())
        assert not torch.equal(st.shadow_t, wt0)


def _pair(transposed, layout=None, **kw):
    from pytorch_vit_paper_replication_amd.optim import FusedAdam, param_groups_weight_decay

    out = []
    for _ in range(2):
        m, st = _model(transposed, layout)
        out.append((m, st, FusedAdam(param_groups_weight_decay(m, 0.03), lr=1e-2, **kw)))
    assert torch.equal(out[0][1].flat, out[1][1].flat)
    return out


def _assert_same(a, b, transposed):
    for x, y in zip(_fused(a[1], a[2]), _fused(b[1], b[2])):
        assert torch.equal(x, y)
    if transposed:
        assert torch.equal(a[1].shadow_t, b[1].shadow_t)


@KERNELS
def test_clip_grad_norm_then_bare_step_equals_step_with_clip_norm(transposed):
    a, b = _pair(transposed)
    for it in range(3):
        _write_grads((a[0], b[0]), it)
        na = a[2].clip_grad_norm_(1.0)
        assert a[2]._pending_clip
        a[2].step()
        assert not a[2]._pending_clip
        b[2].step(clip_norm=1.0)
        torch.cuda.synchronize()
        assert float(na) > 1.0, "the clip must bite"
        assert torch.equal(a[2].last_grad_norm, b[2].last_grad_norm) and torch.equal(a[2]._fused[6], b[2]._fused[6])
        _assert_same(a, b, transposed)
    assert not torch.equal(a[1].flat, _model(transposed)[1].flat)


@KERNELS
@pytest.mark.parametrize("skip_nonfinite", [True, False], ids=["flag_only_norm", "no_clip_argument"])
def test_a_clip_that_does_not_bite_is_no_clip(transposed, skip_nonfinite):
    """max_norm 1e3 on small gradients: coef is exactly 1, the step is the unclipped one bit for bit
    (whose kernel reads the flag-only norm's coef, or no clip tensor at all). The norm itself: 1e-6 of
    the float64 norm of the parameters' .grad tensors (the derived bound of check_grad_norm: under one
    float4 per thread here), and 2e-6 of torch.nn.utils.clip_grad_norm_'s return on the twin's gradients:
    the kernel's 1e-6 plus as much for torch's own fp32 reductions (a few hundred thousand terms summed
    as a tree: well under 1e-6)."""
    a, b = _pair(transposed, skip_nonfinite=skip_nonfinite)
    for it in range(2):
        _write_grads((a[0], b[0]), it, scale=1e-3)
        a[2].step(clip_norm=1e3)
        b[2].step()
        torch.cuda.synchronize()
        clip = a[2]._fused[6].cpu()
        assert float(clip[1]) == 1.0 and float(clip[2]) == 0.0
        _assert_same(a, b, transposed)
        # float64 norm from the parameters' own .grad tensors, not from the flat buffer the kernel reads
        want = math.sqrt(sum(float(p.grad.double().square().sum()) for p in _trainable(a[0])))
        theirs = float(torch.nn.utils.clip_grad_norm_(_trainable(b[0]), 1e3, foreach=False))
        ours = float(a[2].last_grad_norm)
        print(f"step {it + 1}: norm {ours!r} torch {theirs!r} float64 {want!r} rel {abs(ours - want) / want:.2e} "
              f"vs torch {abs(ours - theirs) / theirs:.2e}")
        assert 0.0 < want < 1e3 and abs(ours - want) <= 1e-6 * want
        assert abs(ours - theirs) <= 2e-6 * theirs
    assert not torch.equal(a[1].flat, _model(transposed)[1].flat)
