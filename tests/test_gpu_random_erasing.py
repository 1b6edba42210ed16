"""Random erasing inside the patchify kernels on the GPU.

The erased (and mixed) patch rows must carry the bits of the CPU reference (preprocess, then the per-sample
erase loop, then the per-sample mix loop) pushed through the existing plain float ``im2col``. In "pixel" mode
the reference takes the fill from ``ext.erase_noise``, the diagnostic kernel that calls the device function
the patchify kernels call; that function is checked against its float64 numpy replica.

Shapes are those of test_gpu_batch_mix.py: (B, P, S) = (3, 16, 32) takes the vector path, (2, 14, 28) and
(2, 4, 16) the element path with padded Kp. The fill's element index stays far below 2^31 here: an index
whose doubled value passes 2^32 needs a batch of 2^31 elements, which no test of a few seconds can hold."""
import math

import numpy as np
import pytest
import torch

from tests import erase_oracle as O
from tests.test_gpu_batch_mix import (CFG, IMAGENET, SHAPES, _bits, _geom_2x, _images, _kp, _model_plan, _plans, _same,
                                      loop_mix)

pytestmark = pytest.mark.gpu

DEV = "cuda"
SITE_OFF = O.ERASE_SITE << 32
VALUE = (0.25, -1.5, 2.0)
SEED = 40503


def _ext():
    from pytorch_vit_paper_replication_amd import _ext as E

    return E.ext()


def _seed_tensor(v):
    v = int(v)
    return torch.tensor([v - (1 << 64) if v >= 1 << 63 else v], dtype=torch.int64, device=DEV)


def _noise(v, B, C, H, W):
    """The "pixel" fill of a [B, C, H, W] batch at counter value v, on the host."""
    return _ext().erase_noise(_seed_tensor(v), SITE_OFF, B, C, H, W).cpu()


def _erase_plans(B, S, mode):
    """name -> ErasePlan for B samples of S x S."""
    from pytorch_vit_paper_replication_amd.data import ErasePlan

    cross, P = {32: ([5, 3, 27, 21], 16), 28: ([5, 3, 23, 17], 14), 16: ([3, 2, 11, 9], 4)}[S]
    # no side on a patch border, and the box spans one in x and in y
    assert all(v % P for v in cross) and cross[0] // P != (cross[2] - 1) // P and cross[1] // P != (cross[3] - 1) // P
    # contains the whole aligned 8-pixel run [8, 16) and cuts through the runs beside it (S = 16 has one such neighbour)
    run8 = [5, 1, min(19, S), S - 2]
    assert run8[0] % 8 and run8[0] < 8 and run8[2] >= 16 and (run8[2] % 8 or S == 16)
    rows = ([cross, [S - 5, 1, S, S], [0, 0, 0, 0]] if B == 3 else [[S - 5, 1, S, S], [0, 0, 0, 0]])  # one sample unerased
    mk = lambda boxes: ErasePlan(boxes, (S, S), mode, VALUE)  # noqa: E731
    return {
        "cross": mk([cross] * B),
        "run8": mk([run8] * B),
        "whole_image": mk([[0, 0, S, S]] * B),
        "empty": mk([[S // 2, 3, S // 2, 9]] * B),
        "per_sample": mk(rows[:B]),
    }


def _erase_kw(eplan, seed_v=SEED):
    kw = dict(erase=eplan.on(DEV), erase_host=eplan.rows, erase_mode=eplan.mode)
    if eplan.mode == "pixel":
        kw.update(erase_seed=_seed_tensor(seed_v), erase_offset=SITE_OFF)
    else:
        kw.update(erase_value=list(eplan.value))
    return kw


def _mix_kw(mplan):
    return {} if mplan is None else dict(mix=mplan.on(DEV)[0], mix_host=mplan.rows)


def _float_patches(xf_cpu, P, mplan=None, eplan=None, keep=None):
    img = xf_cpu.float().to(DEV).contiguous()
    B, C, H, W = img.shape
    n = keep.shape[1] if keep is not None else (H // P) * (W // P)
    out = torch.full((B * n, _kp(P, C)), float("nan"), dtype=torch.bfloat16, device=DEV)
    _ext().im2col(img, out, P, _kp(P, C), **_mix_kw(mplan), **({} if eplan is None else _erase_kw(eplan)),
                  **({} if keep is None else dict(keep=keep)))
    return out


def _u8_patches(x_gpu, P, size, norm, geom, mplan, eplan, keep=None):
    B, C = x_gpu.shape[:2]
    H, W = size
    n = keep.shape[1] if keep is not None else (H // P) * (W // P)
    out = torch.full((B * n, _kp(P, C)), float("nan"), dtype=torch.bfloat16, device=DEV)
    mean, std = norm if norm is not None else ((0.0,) * C, (1.0,) * C)
    vec = _ext().im2col_u8(x_gpu, out, list(mean), list(std), None if geom is None else geom.to(DEV), H, W, P, _kp(P, C),
                           **_mix_kw(mplan), **({} if eplan is None else _erase_kw(eplan)), **({} if keep is None else dict(keep=keep)))
    return out, vec


def _host_batch(xf, eplan, mplan, fill):
    x = O.loop_erase(xf, eplan, fill if eplan.mode == "pixel" else None)
    return x if mplan is None else loop_mix(x, mplan)


def _cases(B, S):
    """(mode, erase name, ErasePlan, mix name, MixPlan or None) of every combination"""
    mixes = dict(_plans(B, S), none=None)
    for mode in ("const", "pixel"):
        for en, ep in _erase_plans(B, S, mode).items():
            for mn, mp in mixes.items():
                yield mode, en, ep, mn, mp


# ----------------------------------------------------------------------------- the fill
@pytest.mark.parametrize("shape", [(2, 3, 32, 32), (1, 1, 512, 512)], ids=["6144", "2^18"])
def test_erase_noise_against_the_float64_replica(shape):
    """Kernel checked against float64: its max abs error may be 4x that of the same formula in float32 numpy
    on the same u1, u2 (the yardstick)."""
    n = math.prod(shape)
    for v in (0, 1, 12345, 40503, 2 ** 62 + 17):
        got = _ext().erase_noise(_seed_tensor(v), SITE_OFF, *shape)
        assert got.dtype == torch.float32 and tuple(got.shape) == shape
        u1, u2 = O.uniforms(v, n)
        z64 = O.normal64(u1, u2)
        yard = float(np.abs(O.normal32(u1, u2).astype(np.float64) - z64).max())
        err = float(np.abs(got.cpu().numpy().reshape(-1).astype(np.float64) - z64).max())
        print(f"erase_noise {shape} counter {v}: kernel max abs err {err:.3e}, float32 numpy yardstick {yard:.3e}")
        assert err <= 4 * yard, (v, err, yard)
        assert float(got.abs().max()) <= 5.77
    a, a2, b = (_ext().erase_noise(_seed_tensor(v), SITE_OFF, *shape) for v in (5, 5, 6))
    assert torch.equal(a, a2) and not torch.equal(a, b)
    assert not torch.equal(a, _ext().erase_noise(_seed_tensor(5), SITE_OFF + (1 << 32), *shape))  # another site
    with pytest.raises(RuntimeError, match="seed"):
        _ext().erase_noise(_seed_tensor(5).cpu(), SITE_OFF, *shape)


# ----------------------------------------------------------------------------- patchify kernels
@pytest.mark.parametrize("B,P,S", SHAPES)
def test_float_kernel_erased_rows_bit_identical(B, P, S):
    x = torch.randn(B, 3, S, S, generator=torch.Generator().manual_seed(P))
    fill = _noise(SEED, B, 3, S, S)
    kc = 3 * P * P
    base = {mn: _float_patches(x, P, mp) for mn, mp in dict(_plans(B, S), none=None).items()}
    for mode, en, ep, mn, mp in _cases(B, S):
        tag = (mode, en, mn)
        want = _float_patches(_host_batch(x, ep, mp, fill), P)
        got = _float_patches(x, P, mp, ep)
        assert not torch.isnan(got.float()).any(), tag
        assert torch.equal(_bits(got), _bits(want)), tag
        assert not got[:, kc:].any(), tag  # the padding columns are written, and zero
        assert torch.equal(_bits(got), _bits(base[mn])) == (en == "empty"), tag


@pytest.mark.parametrize("norm", [None, IMAGENET], ids=["scale_only", "imagenet"])
@pytest.mark.parametrize("B,P,S", SHAPES)
def test_u8_kernel_erased_rows_bit_identical(B, P, S, norm):
    from pytorch_vit_paper_replication_amd.data.device_input import preprocess_reference

    x = _images(B, S, S, seed=P)
    xf = preprocess_reference(x, *(norm or (None, None)))
    fill = _noise(SEED, B, 3, S, S)
    kc = 3 * P * P
    layouts = {"contiguous": x.to(DEV), "channels_last": x.to(DEV).contiguous(memory_format=torch.channels_last)}
    base = {mn: _float_patches(xf, P, mp) for mn, mp in dict(_plans(B, S), none=None).items()}
    for mode, en, ep, mn, mp in _cases(B, S):
        want = _float_patches(_host_batch(xf, ep, mp, fill), P)
        assert torch.equal(_bits(want), _bits(base[mn])) == (en == "empty"), (mode, en, mn)
        for lay, xg in layouts.items():
            tag = (mode, en, mn, lay)
            got, vec = _u8_patches(xg, P, (S, S), norm, None, mp, ep)
            assert vec == (1 if P == 16 and lay == "contiguous" else 0), tag
            assert torch.equal(_bits(got), _bits(want)), tag
            assert not got[:, kc:].any(), tag


@pytest.mark.parametrize("norm", [None, IMAGENET], ids=["scale_only", "imagenet"])
@pytest.mark.parametrize("B,P,S", SHAPES)
def test_u8_kernel_geom_erased_rows_bit_identical(B, P, S, norm):
    from pytorch_vit_paper_replication_amd.data.device_input import preprocess_reference

    x = _images(B, 64, 64, seed=P + 1)
    geom = _geom_2x(B, S)
    m, s = norm or (None, None)
    xf = preprocess_reference(x, m, s, geom, (S, S))
    fill = _noise(SEED, B, 3, S, S)
    kc = 3 * P * P
    layouts = {"contiguous": x.to(DEV), "channels_last": x.to(DEV).contiguous(memory_format=torch.channels_last)}
    base = {mn: _float_patches(xf, P, mp) for mn, mp in dict(_plans(B, S), none=None).items()}
    for mode, en, ep, mn, mp in _cases(B, S):
        want = _float_patches(_host_batch(xf, ep, mp, fill), P)
        assert torch.equal(_bits(want), _bits(base[mn])) == (en == "empty"), (mode, en, mn)
        for lay, xg in layouts.items():
            got, vec = _u8_patches(xg, P, (S, S), norm, geom, mp, ep)
            assert vec == 0
            assert torch.equal(_bits(got), _bits(want)), (mode, en, mn, lay)
            assert not got[:, kc:].any(), (mode, en, mn, lay)


@pytest.mark.parametrize("B,P,S", SHAPES)
def test_erased_rows_with_a_patch_dropout_keep_table(B, P, S):
    """With a keep table the rows are those of the kept patches of the same erased (and mixed) image."""
    from pytorch_vit_paper_replication_amd.data.device_input import preprocess_reference
    from pytorch_vit_paper_replication_amd.ops.fused_vit import PATCH_DROP_SITE, SITE_SHIFT

    n_p = (S // P) ** 2
    n_keep = max(1, n_p - n_p // 2)
    keep, _ = _ext().patch_keep_table(_seed_tensor(7), PATCH_DROP_SITE << SITE_SHIFT, B, n_p, n_keep)
    assert n_keep < n_p and tuple(keep.shape) == (B, n_keep)
    idx = keep.long()
    gather = lambda full: torch.stack([full.view(B, n_p, -1)[b, idx[b]] for b in range(B)]).view(B * n_keep, -1)  # noqa: E731
    xf = torch.randn(B, 3, S, S, generator=torch.Generator().manual_seed(S))
    xu = _images(B, S, S, seed=S)
    xg = _images(B, 64, 64, seed=S + 1)
    geom = _geom_2x(B, S)
    mixes = _plans(B, S)
    for mode in ("const", "pixel"):
        for en, ep in _erase_plans(B, S, mode).items():
            for mp in (None, mixes["per_sample"], mixes["cutmix"]):
                tag = (mode, en, mp is not None)
                assert torch.equal(_bits(_float_patches(xf, P, mp, ep, keep)), _bits(gather(_float_patches(xf, P, mp, ep)))), tag
                got, _ = _u8_patches(xu.to(DEV), P, (S, S), IMAGENET, None, mp, ep, keep)
                assert torch.equal(_bits(got), _bits(gather(_u8_patches(xu.to(DEV), P, (S, S), IMAGENET, None, mp, ep)[0]))), tag
                got, _ = _u8_patches(xg.to(DEV), P, (S, S), IMAGENET, geom, mp, ep, keep)
                assert torch.equal(_bits(got), _bits(gather(_u8_patches(xg.to(DEV), P, (S, S), IMAGENET, geom, mp, ep)[0]))), tag
    # and the rows are the erased image's: against the host-built batch through the plain kernel
    ep = _erase_plans(B, S, "pixel")["cross"]
    want = gather(_float_patches(_host_batch(preprocess_reference(xu, *IMAGENET), ep, mixes["cutmix"], _noise(SEED, B, 3, S, S)), P))
    got, _ = _u8_patches(xu.to(DEV), P, (S, S), IMAGENET, None, mixes["cutmix"], ep, keep)
    assert torch.equal(_bits(got), _bits(want))


def test_binding_refuses_bad_tables_before_any_launch():
    from pytorch_vit_paper_replication_amd.data import ErasePlan

    ext = _ext()
    B, S, P = 2, 32, 16
    xu = _images(B, S, S).to(DEV)
    xf = xu.float()
    m, s = [0.0] * 3, [1.0] * 3
    good = ErasePlan([[3, 4, 20, 32], [0, 0, 0, 0]], (S, S)).rows.clone()
    seed = _seed_tensor(1)
    px = dict(erase_mode="pixel", erase_seed=seed, erase_offset=SITE_OFF)

    def run(**kw):
        out = torch.full((B * 4, 768), float("nan"), dtype=torch.bfloat16, device=DEV)
        ext.im2col(xf, out, P, 768, **kw)
        out8 = torch.full((B * 4, 768), float("nan"), dtype=torch.bfloat16, device=DEV)
        ext.im2col_u8(xu, out8, m, s, None, S, S, P, 768, **kw)
        return out, out8

    def refused(**kw):
        for call in (lambda o: ext.im2col(xf, o, P, 768, **kw), lambda o: ext.im2col_u8(xu, o, m, s, None, S, S, P, 768, **kw)):
            out = torch.full((B * 4, 768), float("nan"), dtype=torch.bfloat16, device=DEV)
            with pytest.raises(RuntimeError):
                call(out)
            assert torch.isnan(out.float()).all()  # nothing was launched

    # the valid calls: host copy given or read back, both modes
    for kw in (dict(erase=good.to(DEV), erase_host=good, **px), dict(erase=good.to(DEV), **px),
               dict(erase=good.to(DEV), erase_host=good, erase_mode="const", erase_value=[0.5]),
               dict(erase=good.to(DEV), erase_mode="const", erase_value=[0.1, 0.2, 0.3])):
        for o in run(**kw):
            assert not torch.isnan(o.float()).any()

    def bad_rows(col, value):
        r = good.clone()
        r[0, col] = value
        return r

    for r in (bad_rows(0, -1), bad_rows(1, -1), bad_rows(2, S + 1), bad_rows(3, S + 1), bad_rows(0, 21), bad_rows(1, 33), bad_rows(2, 2)):
        refused(erase=r.to(DEV), erase_host=r, **px)
        refused(erase=r.to(DEV), **px)
    # device, rows, dtype, columns, host rows, alignment, host copy alone
    for kw in (dict(erase=good), dict(erase=good.to(DEV)[:1]), dict(erase=good.to(DEV).float()), dict(erase=good.to(DEV).long()),
               dict(erase=torch.zeros(B, 8, dtype=torch.int32, device=DEV)), dict(erase=good.to(DEV), erase_host=good[:1]),
               dict(erase=good.to(DEV), erase_host=good.to(DEV)),
               dict(erase=torch.zeros(B + 1, 4, dtype=torch.int32, device=DEV).view(-1)[1:1 + 4 * B].view(B, 4)),
               dict(erase_host=good)):
        refused(**kw, **px)
    # pixel mode without a seed, or with a bad one; an unknown mode; a value count that is neither 1 nor C
    refused(erase=good.to(DEV), erase_host=good, erase_mode="pixel")
    refused(erase=good.to(DEV), erase_host=good, erase_mode="pixel", erase_seed=seed.cpu())
    refused(erase=good.to(DEV), erase_host=good, erase_mode="pixel", erase_seed=seed.int())
    refused(erase=good.to(DEV), erase_host=good, erase_mode="colour")
    refused(erase=good.to(DEV), erase_host=good, erase_mode="const", erase_value=[0.0, 1.0])
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------- model and engine
def _model_erase(mode, B=4, S=64):
    from pytorch_vit_paper_replication_amd.data import ErasePlan

    return ErasePlan([[5, 3, 43, 37], [40, 0, 64, 64], [0, 0, 0, 0], [9, 20, 30, 41]], (S, S), mode, VALUE)


def _counter(m, v):
    """Set the model's device counter: its next forward draws at the value v."""
    m._dropout_seed(torch.device("cuda", torch.cuda.current_device()))
    m._pvr_rng.fill_(v)
    return m


def _step(make_logits, y, plan, cls=None, cfg=CFG):
    """Fresh seeded model -> (output, loss, parameter gradients, names)."""
    from pytorch_vit_paper_replication_amd.models import ViT
    from pytorch_vit_paper_replication_amd.ops.fused_vit import soft_cross_entropy

    torch.manual_seed(0)
    m = (cls or ViT)(**cfg).to(DEV).train()
    out = make_logits(m)
    loss = soft_cross_entropy(out, y, plan, 0.1) if cls is None else out.square().mean()
    loss.backward()
    torch.cuda.synchronize()
    assert getattr(m, "_pvr_store", None) is not None, "fused path did not run"
    return out.detach().clone(), loss.detach().clone(), [p.grad.detach().clone() for p in m.parameters()], [n for n, _ in m.named_parameters()]


@pytest.mark.parametrize("mode", ["const", "pixel"])
def test_model_with_plans_bitwise_equal_to_the_host_erased_and_mixed_batch(mode):
    from pytorch_vit_paper_replication_amd import _ext as E
    from pytorch_vit_paper_replication_amd.data import DeviceInput
    from pytorch_vit_paper_replication_amd.data.device_input import preprocess_reference
    from pytorch_vit_paper_replication_amd.models.vit_no_classifier import ViT as Backbone

    V = 31337
    mplan, eplan = _model_plan(), _model_erase(mode)
    fill = _noise(V, 4, 3, 64, 64)  # the step's counter value, replayed
    y = torch.randint(0, 10, (4,), generator=torch.Generator().manual_seed(0)).to(DEV)
    x = torch.randn(4, 3, 64, 64, generator=torch.Generator().manual_seed(1))
    xg = x.to(DEV)
    host = _host_batch(x, eplan, mplan, fill).to(DEV)
    host_e = _host_batch(x, eplan, None, fill).to(DEV)
    # uint8 entry: integer 64 x 64 windows of an 80 x 96 source, one per sample, the second right to left
    xu = _images(4, 80, 96, seed=7)
    geom = torch.tensor([[16.0, 8.0, 80.0, 72.0], [80.0, 8.0, 16.0, 72.0], [0.0, 0.0, 64.0, 64.0], [32.0, 16.0, 96.0, 80.0]])
    xuf = preprocess_reference(xu, *IMAGENET, geom, (64, 64))
    host_u = _host_batch(xuf, eplan, mplan, fill).to(DEV)
    xug, gg = xu.to(DEV), geom.to(DEV)
    bcfg = {k: v for k, v in CFG.items() if k != "num_classes"}
    with E.deterministic_mode():
        a = _step(lambda m: _counter(m, V)(xg, mix=mplan, erase=eplan), y, mplan)
        b = _step(lambda m: m(host), y, mplan)
        mixed_only = _step(lambda m: m(xg, mix=mplan), y, mplan)
        e = _step(lambda m: _counter(m, V)(xg, erase=eplan), y, None)
        eh = _step(lambda m: m(host_e), y, None)
        u = _step(lambda m: _counter(m.set_device_input(DeviceInput(*IMAGENET)), V)(xug, geom=gg, mix=mplan, erase=eplan), y, mplan)
        f = _step(lambda m: m(host_u), y, mplan)
        k = _step(lambda m: _counter(m, V)(xg, mix=mplan, erase=eplan), y, mplan, Backbone, bcfg)
        kh = _step(lambda m: m(host), y, mplan, Backbone, bcfg)
    _same(a, b)
    _same(e, eh)
    _same(u, f)
    _same(k, kh)
    assert not torch.equal(a[0], mixed_only[0])
    if mode == "pixel":  # another counter value, other noise
        with E.deterministic_mode():
            a2 = _step(lambda m: _counter(m, V + 1)(xg, mix=mplan, erase=eplan), y, mplan)
        assert not torch.equal(a[0], a2[0])


def test_model_eval_takes_a_pixel_plan_and_draws_a_counter_value():
    from pytorch_vit_paper_replication_amd.models import ViT

    V = 777
    eplan = _model_erase("pixel")
    x = torch.randn(4, 3, 64, 64, generator=torch.Generator().manual_seed(2))
    torch.manual_seed(0)
    m = _counter(ViT(**CFG).to(DEV).eval(), V)
    with torch.no_grad():
        got = m(x.to(DEV), erase=eplan)
        assert int(m._pvr_rng.item()) == V + 1  # the plan took the step's value although nothing else draws
        assert torch.equal(got, m(_host_batch(x, eplan, None, _noise(V, 4, 3, 64, 64)).to(DEV)))
        assert int(m._pvr_rng.item()) == V + 1
        assert not torch.equal(got, m(x.to(DEV), erase=eplan))  # the next value: other noise
    with pytest.raises(ValueError):
        m(x[:2].to(DEV), erase=eplan)


@pytest.mark.parametrize("with_mix", [False, True])
def test_train_step_with_random_erasing_under_fused_adam(with_mix):
    from pytorch_vit_paper_replication_amd import engine
    from pytorch_vit_paper_replication_amd.data import BatchMix, RandomErasing
    from pytorch_vit_paper_replication_amd.models import ViT
    from pytorch_vit_paper_replication_amd.optim import FusedAdam, param_groups_weight_decay, warmup_linear_decay

    torch.manual_seed(0)
    B = 4
    m = ViT(**CFG).to(DEV)
    opt = FusedAdam(param_groups_weight_decay(m, 0.03), lr=1e-3)
    g = torch.Generator().manual_seed(3)
    data = [(torch.randn(B, 3, 64, 64, generator=g), torch.randint(0, 10, (B,), generator=g)) for _ in range(2)]
    before = [p.detach().clone() for p in m.parameters()]
    eraser = RandomErasing(prob=1.0, generator=torch.Generator().manual_seed(5))
    mixer = BatchMix(generator=torch.Generator().manual_seed(4)) if with_mix else None
    loss, acc = engine.train_step(m, data, torch.nn.CrossEntropyLoss(), opt, warmup_linear_decay(opt, 10, 0.1), DEV,
                                  batch_mix=mixer, random_erasing=eraser)
    assert math.isfinite(loss) and 0.0 <= acc <= 1.0
    assert loss < math.log(10) + 1.0
    assert getattr(m, "_pvr_store", None) is not None and getattr(m, "_pvr_rng", None) is not None
    assert all(not torch.equal(a, b) for a, b in zip(before, m.parameters()))


class _WithPlan(torch.nn.Module):
    def __init__(self, inner, eplan):
        super().__init__()
        self.inner, self.eplan = inner, eplan

    def forward(self, x):
        return self.inner(x, erase=self.eplan)


def test_explicit_plan_under_a_graphed_train_step_sees_fresh_noise(monkeypatch):
    """The table is frozen in the graph; the noise is that of the counter value each replay draws. The
    learning rate is 0, so the weights stay and the loss of a replay is the eager loss on the batch erased
    with that value's noise. The two run the same kernels on the same values; the limit of 1e-3 allows for
    a bf16 rounding (2^-8) in one activation of one of them, averaged down by the loss, and the test checks
    that the two replays' noise moves the loss by at least ten times as much."""
    from pytorch_vit_paper_replication_amd.data import ErasePlan, RandomErasing
    from pytorch_vit_paper_replication_amd.models import ViT
    from pytorch_vit_paper_replication_amd.ops.fused_vit import cross_entropy
    from pytorch_vit_paper_replication_amd.optim import FusedAdam
    from pytorch_vit_paper_replication_amd.runtime.graph import GraphedTrainStep

    V, WARM, B = 4242, 3, 4
    torch.manual_seed(0)
    m = _counter(ViT(**CFG).to(DEV), V)
    opt = FusedAdam(m.parameters(), lr=0.0)
    eplan = ErasePlan([[0, 0, 64, 64], [3, 5, 50, 60], [0, 0, 0, 0], [20, 0, 64, 33]], (64, 64))
    x = torch.randn(B, 3, 64, 64, generator=torch.Generator().manual_seed(8))
    y = torch.randint(0, 10, (B,), generator=torch.Generator().manual_seed(9)).to(DEV)
    g = GraphedTrainStep(_WithPlan(m, eplan), opt, cross_entropy, x.to(DEV), y, clip_norm=1.0, warmup=WARM)
    losses = [g().clone() for _ in range(2)]
    torch.cuda.synchronize()
    assert int(m._pvr_rng.item()) == V + WARM + 2  # one value per step, replays included
    # CFG has no dropout: a training forward of the same weights draws nothing, so the counter stays
    want = [cross_entropy(m(_host_batch(x, eplan, None, _noise(V + WARM + j, B, 3, 64, 64)).to(DEV)), y).detach() for j in range(2)]
    assert int(m._pvr_rng.item()) == V + WARM + 2
    print(f"replay losses {[float(l) for l in losses]}, eager losses on the replayed noise {[float(w) for w in want]}")
    tol = 1e-3
    for l, w in zip(losses, want):
        assert math.isfinite(float(l)) and abs(float(l) - float(w)) <= tol, (losses, want)
    assert abs(float(want[0]) - float(want[1])) >= 10 * tol and float(losses[0]) != float(losses[1])
    # a sampler cannot run inside a capture (a replay would reuse one draw)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(RuntimeError, match="graph capture"):
        RandomErasing().sample(B, 64, 64)
