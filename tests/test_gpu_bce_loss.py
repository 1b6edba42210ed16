"""The binary cross-entropy kernel (csrc/bce.hip) on the GPU: the binding against float64, its exact identities and
host checks, then the autograd function, the loss module in the engine and under a captured training step.

Accuracy: the reference is float64 ``F.binary_cross_entropy_with_logits`` on explicit float64 target rows (built from
the fp32 values of ``lam`` and ``eps`` the kernel receives), the yardstick the same call in fp32 on the GPU. The
metrics are ``errs`` of tests/kernel_checks.py (relative L2, max error over max |ref|) for the loss rows, the mean
and ``dlogits``; each must stay within ``max(4 x the yardstick's, 5e-7)``: the factor 4 is the project's rule for
fp32 kernels against float64, the floor the bound tests/test_gpu_batch_mix.py applies to the softmax kernel (the
yardstick is exact at C = 1)."""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"
CFG = dict(image_size=64, patch_size=16, num_transformer_layer=2, num_heads=2, embedding_dim=128, mlp_size=256,
           num_classes=10, mlp_dropout=0.0, embedding_dropout=0.0)
SHAPES = [(1, 1), (1, 3), (5, 10), (5, 257), (8, 1000), (3, 1025)]
FLOOR, FACTOR = 5e-7, 4.0


def _ext():
    from pytorch_vit_paper_replication_amd import _ext as E

    return E.ext()


def _inputs(B, C):
    g = torch.Generator().manual_seed(B * 1000 + C)
    logits = (torch.randn(B, C, generator=g) * 3).to(DEV)
    ya = torch.randint(0, C, (B,), generator=g).to(DEV)
    yb = torch.randint(0, C, (B,), generator=g).to(DEV)
    yb[0] = ya[0]  # one row mixes a class with itself
    return logits, ya, yb


def _bce(logits, ya, yb, lam, eps, thr=-1.0, sum_classes=False, grad_scale=None):
    B, C = logits.shape
    dl = torch.full((B, C), float("nan"), device=DEV)
    corr = torch.full((B,), -1, dtype=torch.int32, device=DEV)
    mean = torch.full((1,), float("nan"), device=DEV)
    gs = grad_scale if grad_scale is not None else (1.0 / B if sum_classes else 1.0 / (B * C))
    rows = _ext().bce(logits, ya, yb, lam, eps, thr, sum_classes, dl, corr, gs, mean)
    return rows, dl, corr, mean


def _targets32(ya, yb, lam, eps, C, thr=-1.0):
    """The kernel's fp32 target, operation by operation."""
    one = torch.ones((), device=DEV)
    e = torch.tensor(eps, dtype=torch.float32, device=DEV)
    cols = torch.arange(C, device=DEV)[None]
    zero = torch.zeros((), device=DEV)
    w = torch.where(cols == ya[:, None], lam[:, None], zero) + torch.where(cols == yb[:, None], (one - lam)[:, None], zero)
    q = (one - e) * w + e / torch.tensor(float(C), device=DEV)
    return (q > thr).float() if thr >= 0 else q


def _targets64(ya, yb, lam, eps, C, thr=-1.0):
    e = float(torch.tensor(eps, dtype=torch.float32))
    l = lam.double()[:, None]
    q = (1.0 - e) * (l * F.one_hot(ya, C).double() + (1.0 - l) * F.one_hot(yb, C).double()) + e / C
    return (q > thr).double() if thr >= 0 else q


def _torch_bce(logits, t, sum_classes, grad_scale=None):
    """(rows, mean, d mean / d logits [times grad_scale's ratio to the mean's own]) by autograd, in t's dtype."""
    x = logits.to(t.dtype).clone().requires_grad_(True)
    el = F.binary_cross_entropy_with_logits(x, t, reduction="none")
    rows = el.sum(-1) if sum_classes else el.mean(-1)
    mean = rows.mean()
    mean.backward()
    B, C = logits.shape
    own = 1.0 / B if sum_classes else 1.0 / (B * C)
    g = x.grad if grad_scale is None else x.grad * (grad_scale / own)
    return rows.detach(), mean.detach(), g


def _check64(tag, got, logits, t32, t64, sum_classes, grad_scale=None):
    """got = (rows, dl, mean) of the kernel; prints the kernel's and the yardstick's metrics, then asserts."""
    from tests.kernel_checks import errs

    rows, dl, mean = got
    ref = _torch_bce(logits, t64, sum_classes, grad_scale)
    yard = _torch_bce(logits, t32, sum_classes, grad_scale)
    bad = []
    for name, k, y, r in (("rows", rows, yard[0], ref[0]), ("mean", mean.reshape(()), yard[1], ref[1]), ("dlogits", dl, yard[2], ref[2])):
        ek, ey = errs(k, r), errs(y, r)
        print(f"bce {tag} {name}: kernel l2 {ek[0]:.2e} max {ek[1]:.2e}; torch fp32 l2 {ey[0]:.2e} max {ey[1]:.2e}")
        for a, b, m in zip(ek, ey, ("l2", "max")):
            if not a <= max(FACTOR * b, FLOOR):
                bad.append(f"{tag} {name} {m}: {a:.3e} over max({FACTOR:g} x {b:.3e}, {FLOOR:g})")
    assert not bad, bad


# ----------------------------------------------------------------------------- binding: accuracy and flags
@pytest.mark.parametrize("sum_classes", [False, True], ids=["mean", "sum_classes"])
@pytest.mark.parametrize("B,C", SHAPES)
def test_against_float64(B, C, sum_classes):
    logits, ya, yb = _inputs(B, C)
    for lam in (0.0, 0.3, 1.0):
        for eps in (0.0, 0.1):
            lam_t = torch.full((B,), lam, device=DEV)
            rows, dl, corr, mean = _bce(logits, ya, yb, lam_t, eps, sum_classes=sum_classes)
            assert torch.equal(corr.bool(), logits.argmax(1) == ya)
            _check64(f"B{B} C{C} lam{lam} eps{eps} sum{int(sum_classes)}", (rows, dl, mean), logits,
                     _targets32(ya, yb, lam_t, eps, C), _targets64(ya, yb, lam_t, eps, C), sum_classes)


@pytest.mark.parametrize("B,C,cols", [(1, 3, (0, 2)), (5, 257, (3, 256)), (8, 1000, (70, 700)), (8, 1000, (5, 261)), (3, 1025, (1023, 1024))])
def test_flags_are_the_first_argmax(B, C, cols):
    """Rows 0 and 1 tie two columns (other waves, the same thread's two trips, the ragged last trip): the lower wins."""
    logits, ya, yb = _inputs(B, C)
    lo, hi = cols
    rows_tied = [0] if B == 1 else [0, 1]
    for r in rows_tied:
        logits[r, lo] = logits[r, hi] = 50.0
    ya[0] = lo
    if B > 1:
        ya[1] = hi
    want = logits.argmax(1)
    for r in rows_tied:
        want[r] = lo
    _, _, corr, _ = _bce(logits, ya, yb, torch.full((B,), 0.3, device=DEV), 0.1)
    assert torch.equal(corr.bool(), want == ya)
    assert corr[0].item() == 1 and (B == 1 or corr[1].item() == 0)


SAT = [-1e4, -104.0, -88.0, -30.0, -17.0, 0.0, 17.0, 30.0, 88.0, 104.0, 1e4]


def test_saturated_logits():
    B, C = 5, 257
    logits, ya, yb = _inputs(B, C)
    ya[2], yb[2], ya[3], yb[3] = 7, 200, 100, 100
    v = torch.tensor(SAT, device=DEV)
    logits[0, :11] = v                # the first trip of wave 0
    logits[1, C - 11:] = v            # across the end of the first trip and the ragged second
    logits[2, 7], logits[2, 200] = 1e4, -1e4     # both labels of a mixed row: confidently right and wrong
    logits[3, 100], logits[3, 101] = -104.0, 104.0  # the label of an unmixed row, and its neighbour
    logits[4, int(ya[4])] = 1e4
    lam_t = torch.full((B,), 0.3, device=DEV)
    for eps, thr in ((0.1, -1.0), (0.0, -1.0), (0.1, 0.2)):
        rows, dl, corr, mean = _bce(logits, ya, yb, lam_t, eps, thr, grad_scale=1.0)
        assert torch.isfinite(rows).all() and torch.isfinite(dl).all() and torch.isfinite(mean).all()
        t = _targets32(ya, yb, lam_t, eps, C, thr)
        big = logits.abs() >= 104
        assert int(big.sum()) == 2 * 4 + 2 + 2 + 1
        want = torch.where(logits > 0, torch.ones((), device=DEV) - t, -t)
        assert torch.equal(dl[big], want[big]), (dl[big], want[big])
        _check64(f"saturated eps{eps} thr{thr}", (rows, dl, mean), logits, t, _targets64(ya, yb, lam_t, eps, C, thr), False, 1.0)


# ----------------------------------------------------------------------------- binding: exact identities
@pytest.mark.parametrize("B,C", SHAPES)
def test_exact_identities(B, C):
    logits, ya, yb = _inputs(B, C)
    ones = torch.ones(B, device=DEV)
    ext = _ext()
    # lam = 1: the partner does not matter
    a, b = _bce(logits, ya, yb, ones, 0.1), _bce(logits, ya, ya, ones, 0.1)
    assert all(torch.equal(u, v) for u, v in zip(a, b))
    # hard labels are their own binarisation
    a, b = _bce(logits, ya, ya, ones, 0.0, 0.5), _bce(logits, ya, ya, ones, 0.0)
    assert all(torch.equal(u, v) for u, v in zip(a, b))
    # the two labels of a pair are interchangeable (the flags are not: they follow ya)
    a = _bce(logits, ya, yb, torch.full((B,), 0.25, device=DEV), 0.1)
    b = _bce(logits, yb, ya, torch.full((B,), 0.75, device=DEV), 0.1)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[3], b[3])
    # no gradient, no flags, no mean: the loss rows alone
    for sc in (False, True):
        lam_t = torch.full((B,), 0.3, device=DEV)
        assert torch.equal(ext.bce(logits, ya, yb, lam_t, 0.1, -1.0, sc, None, None, 1.0), _bce(logits, ya, yb, lam_t, 0.1, sum_classes=sc)[0])
    # a view of a wider matrix (ld > C) against its contiguous copy
    wide = torch.randn(B, C + 3, generator=torch.Generator().manual_seed(C)).to(DEV) * 3
    view = wide[:, :C]
    assert view.stride(0) == C + 3
    a, b = _bce(view, ya, yb, torch.full((B,), 0.3, device=DEV), 0.1), _bce(view.contiguous(), ya, yb, torch.full((B,), 0.3, device=DEV), 0.1)
    assert all(torch.equal(u, v) for u, v in zip(a, b))


def test_the_two_reductions_differ_by_the_class_count():
    B, C = 5, 257
    logits, ya, yb = _inputs(B, C)
    lam_t = torch.full((B,), 0.3, device=DEV)
    m = _bce(logits, ya, yb, lam_t, 0.1)
    s = _bce(logits, ya, yb, lam_t, 0.1, sum_classes=True)
    assert torch.allclose(s[0], m[0] * C, rtol=3e-7, atol=0) and torch.allclose(s[1], m[1] * C, rtol=3e-7, atol=0)


@pytest.mark.parametrize("thr", [0.2, 0.5])
def test_target_threshold(thr):
    """lam 0.3, eps 0.1, C 10: the rows hold 0.01, 0.28 (own class) and 0.64 (partner's), 0.91 where both agree."""
    B, C = 5, 10
    logits, ya, yb = _inputs(B, C)
    yb[1:] = (ya[1:] + 1 + torch.arange(B - 1, device=DEV) % (C - 1)) % C  # every other row mixes two different classes
    lam_t = torch.full((B,), 0.3, device=DEV)
    t64 = _targets64(ya, yb, lam_t, 0.1, C, thr)
    hot = F.one_hot(yb, C).bool() if thr == 0.5 else (F.one_hot(ya, C).bool() | F.one_hot(yb, C).bool())
    assert torch.equal(t64.bool(), hot) and torch.equal(_targets32(ya, yb, lam_t, 0.1, C, thr).bool(), hot)
    for sc in (False, True):
        rows, dl, corr, mean = _bce(logits, ya, yb, lam_t, 0.1, thr, sum_classes=sc)
        assert torch.equal(corr.bool(), logits.argmax(1) == ya)
        assert torch.equal((dl < 0), hot)  # sigmoid - 1 below zero exactly where the target is 1
        _check64(f"thr{thr} sum{int(sc)}", (rows, dl, mean), logits, hot.float(), t64, sc)


def test_out_of_range_rows_are_exactly_zero():
    B, C = 5, 257
    logits, ya, yb = _inputs(B, C)
    ya[1], yb[3] = C, -100
    for thr in (-1.0, 0.2):
        rows, dl, corr, mean = _bce(logits, ya, yb, torch.full((B,), 0.3, device=DEV), 0.1, thr)
        for r in (1, 3):
            assert rows[r].item() == 0.0 and not dl[r].any()
        assert torch.isfinite(rows).all() and torch.isfinite(dl).all() and torch.isfinite(mean).all()
        assert all(rows[r].item() > 0 and dl[r].abs().sum().item() > 0 for r in (0, 2, 4))
        assert corr[1].item() == 0 and corr[3].item() == int(logits[3].argmax() == ya[3])


def test_host_checks_refuse_before_any_launch():
    B, C = 4, 10
    logits, ya, yb = _inputs(B, C)
    lam = torch.full((B,), 0.3, device=DEV)
    dl = torch.full((B, C), float("nan"), device=DEV)
    corr = torch.full((B,), -1, dtype=torch.int32, device=DEV)
    mean = torch.full((1,), float("nan"), device=DEV)
    ext = _ext()

    def call(logits=logits, ya=ya, yb=yb, lam=lam, eps=0.1, thr=-1.0, dl=dl, corr=corr, mean=mean):
        return ext.bce(logits, ya, yb, lam, eps, thr, False, dl, corr, 1.0, mean)

    wide = torch.randn(B, 2 * C, device=DEV)
    cases = dict(half_logits=dict(logits=logits.half()), double_logits=dict(logits=logits.double()), bf16_logits=dict(logits=logits.bfloat16()),
                 strided_columns=dict(logits=wide[:, ::2]), transposed=dict(logits=torch.randn(C, B, device=DEV).t()),
                 int32_ya=dict(ya=ya.int()), int32_yb=dict(yb=yb.int()), short_lam=dict(lam=lam[:B - 1]), long_lam=dict(lam=torch.ones(B + 1, device=DEV)),
                 eps_high=dict(eps=1.5), eps_negative=dict(eps=-0.1), thr_one=dict(thr=1.0),
                 small_dlogits=dict(dl=torch.empty(B, C - 1, device=DEV)), large_dlogits=dict(dl=torch.empty(B + 1, C, device=DEV)),
                 half_dlogits=dict(dl=torch.empty(B, C, device=DEV, dtype=torch.float16)), short_correct=dict(corr=corr[:B - 1]),
                 int64_correct=dict(corr=corr.long()), empty_mean=dict(mean=mean[:0]), cpu_labels=dict(ya=ya.cpu()), short_labels=dict(yb=yb[:B - 1]))
    for name, kw in cases.items():
        with pytest.raises(RuntimeError):
            call(**kw)
        torch.cuda.synchronize()
        assert torch.isnan(dl).all() and (corr == -1).all() and torch.isnan(mean).all(), f"{name}: something was written"
    rows = call()  # and the call they were derived from is valid
    torch.cuda.synchronize()
    assert torch.isfinite(rows).all() and torch.isfinite(dl).all() and (corr >= 0).all() and torch.isfinite(mean).all()


# ----------------------------------------------------------------------------- model and engine
def _model_plan(B=4, S=64):
    from pytorch_vit_paper_replication_amd.data import MixPlan

    return MixPlan([3, 2, 1, 0], [0.3, 1.0, 1.0, 0.75], [[0, 0, 0, 0], [5, 9, 43, 30], [0, 20, 64, 64], [0, 0, 0, 0]], (S, S))


def test_function_wiring_is_the_kernels_gradient_bit_for_bit():
    """One training step through binary_cross_entropy against the same seeded model driven by
    ``logits.backward(gradient=dl)`` with dl straight from the binding: same logits, same parameter gradients."""
    from pytorch_vit_paper_replication_amd import _ext as E
    from pytorch_vit_paper_replication_amd.models import ViT
    from pytorch_vit_paper_replication_amd.ops import fused_vit

    B, C = 4, 10
    plan = _model_plan()
    y = torch.randint(0, C, (B,), generator=torch.Generator().manual_seed(0)).to(DEV)
    x = torch.randn(B, 3, 64, 64, generator=torch.Generator().manual_seed(1)).to(DEV)

    def step(by_hand):
        torch.manual_seed(0)
        m = ViT(**CFG).to(DEV).train()
        logits = m(x, mix=plan)
        if by_hand:
            _, partner, lam = plan.on(DEV)
            dl = torch.empty(B, C, device=DEV)
            mean = torch.empty(1, device=DEV)
            E.ext().bce(logits.detach(), y, y.index_select(0, partner), lam, 0.1, -1.0, False, dl, None, 1.0 / (B * C), mean)
            logits.backward(gradient=dl)
            loss = mean[0]
        else:
            fused_vit.last_correct = None
            loss = fused_vit.binary_cross_entropy(logits, y, plan, 0.1)
            assert fused_vit.last_correct is not None and torch.equal(fused_vit.last_correct.bool(), logits.argmax(1) == y)
            loss.backward()
        torch.cuda.synchronize()
        assert getattr(m, "_pvr_store", None) is not None, "fused path did not run"
        return logits.detach().clone(), loss.detach().clone(), [(n, p.grad.detach().clone()) for n, p in m.named_parameters()]

    with E.deterministic_mode():
        a, b = step(False), step(True)
    assert torch.isfinite(a[1]).item() and torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    for (n, ga), (_, gb) in zip(a[2], b[2]):
        assert torch.equal(ga, gb), f"grad {n}"
        assert ga.abs().sum().item() > 0, f"grad {n} is zero"


def test_train_step_with_batch_mix_keeps_the_module():
    from pytorch_vit_paper_replication_amd import _ext as E
    from pytorch_vit_paper_replication_amd import engine
    from pytorch_vit_paper_replication_amd.data import BatchMix
    from pytorch_vit_paper_replication_amd.losses import BinaryCrossEntropy
    from pytorch_vit_paper_replication_amd.models import ViT
    from pytorch_vit_paper_replication_amd.ops import fused_vit
    from pytorch_vit_paper_replication_amd.optim import FusedAdam, param_groups_weight_decay, warmup_linear_decay

    B = 4
    g = torch.Generator().manual_seed(3)
    data = [(torch.randn(B, 3, 64, 64, generator=g), torch.randint(0, 10, (B,), generator=g)) for _ in range(2)]

    def run(record):
        torch.manual_seed(0)
        m = ViT(**CFG).to(DEV)
        opt = FusedAdam(param_groups_weight_decay(m, 0.03), lr=1e-3)
        before = [p.detach().clone() for p in m.parameters()]
        seen = []
        if record:
            m.register_forward_hook(lambda mod, args, out: seen.append(out.detach().clone()))
        fused_vit.last_correct = None
        mixer = BatchMix(label_smoothing=0.1, generator=torch.Generator().manual_seed(4))
        loss, acc = engine.train_step(m, data, BinaryCrossEntropy(), opt, warmup_linear_decay(opt, 10, 0.1), DEV, batch_mix=mixer)
        moved = all(not torch.equal(a, b) for a, b in zip(before, m.parameters()))
        return loss, acc, moved, seen

    with E.deterministic_mode():
        loss, acc, moved, _ = run(False)
        assert fused_vit.last_correct is not None and fused_vit.last_correct.numel() == B and fused_vit.last_correct.dtype == torch.int32
        loss2, acc2, _, seen = run(True)
    assert math.isfinite(loss) and moved and loss == loss2 and acc == acc2
    assert len(seen) == 2
    want = sum(float((o.argmax(1) == y.to(DEV)).float().mean()) for o, (_, y) in zip(seen, data)) / 2
    assert acc == want
    # a mean over [B, C] of per-class losses near log 2 at initialisation
    assert 0.0 < loss < math.log(2) + 1.0


def test_test_step_uses_the_module_unmixed():
    from pytorch_vit_paper_replication_amd import engine
    from pytorch_vit_paper_replication_amd.losses import BinaryCrossEntropy
    from pytorch_vit_paper_replication_amd.models import ViT
    from pytorch_vit_paper_replication_amd.ops.fused_vit import soft_targets

    B = 4
    g = torch.Generator().manual_seed(5)
    data = [(torch.randn(B, 3, 64, 64, generator=g), torch.randint(0, 10, (B,), generator=g)) for _ in range(2)]
    torch.manual_seed(0)
    m = ViT(**CFG).to(DEV)
    for lf in (BinaryCrossEntropy(smoothing=0.1), BinaryCrossEntropy(smoothing=0.1, target_threshold=0.2, sum_classes=True)):
        loss, acc = engine.test_step(m, data, lf, DEV)
        want, hits = [], []
        with torch.inference_mode():
            for X, y in data:
                logits, y = m(X.to(DEV)), y.to(DEV)
                t = soft_targets(y, 10, None, 0.1)
                if lf.target_threshold is not None:
                    t = t.gt(lf.target_threshold).float()
                el = F.binary_cross_entropy_with_logits(logits, t, reduction="none")
                want.append(float(el.sum(-1).mean() if lf.sum_classes else el.mean()))
                hits.append(float((logits.argmax(1) == y).float().mean()))
        assert loss == pytest.approx(sum(want) / 2, rel=1e-6) and acc == sum(hits) / 2


def test_graphed_train_step_with_the_module_as_loss_fn():
    """Capture with the module as loss_fn, replay twice: the parameters after each replay are those of an eager run
    of the same steps, bit for bit (deterministic mode: fixed-order reductions on both sides)."""
    from pytorch_vit_paper_replication_amd import _ext as E
    from pytorch_vit_paper_replication_amd.losses import BinaryCrossEntropy
    from pytorch_vit_paper_replication_amd.models import ViT
    from pytorch_vit_paper_replication_amd.ops import fused_vit
    from pytorch_vit_paper_replication_amd.optim import FusedAdam, param_groups_weight_decay
    from pytorch_vit_paper_replication_amd.runtime.graph import GraphedTrainStep

    WARM, B = 2, 4
    lf = BinaryCrossEntropy(smoothing=0.1)
    x = torch.rand(B, 3, 64, 64, generator=torch.Generator().manual_seed(6)).to(DEV)
    y = torch.randint(0, 10, (B,), generator=torch.Generator().manual_seed(7)).to(DEV)
    with E.deterministic_mode():
        torch.manual_seed(0)
        ma, mb = ViT(**CFG).to(DEV), ViT(**CFG).to(DEV)
        mb.load_state_dict(ma.state_dict())
        oa = FusedAdam(param_groups_weight_decay(ma, 0.03), lr=1e-3)
        ob = FusedAdam(param_groups_weight_decay(mb, 0.03), lr=1e-3)
        eager = []
        for _ in range(WARM + 2):
            ma.train()
            loss = lf(ma(x), y)
            oa.zero_grad()
            fused_vit.backward(loss)
            oa.step(clip_norm=1.0)
            torch.cuda.synchronize()
            eager.append((float(loss.detach()), [p.detach().clone() for p in ma.parameters()]))
        g = GraphedTrainStep(mb, ob, lf, x, y, clip_norm=1.0, warmup=WARM)
        for j in range(2):
            loss = float(g())
            torch.cuda.synchronize()
            want_loss, want = eager[WARM + j]
            worst = max(float((p.detach() - w).abs().max()) for p, w in zip(mb.parameters(), want))
            print(f"replay {j}: loss {loss} (eager {want_loss}), largest parameter difference {worst:.3e}")
            assert math.isfinite(loss)
            for (n, p), w in zip(mb.named_parameters(), want):
                assert torch.equal(p.detach(), w), f"replay {j}: {n}"
    assert ob.step_count == oa.step_count == WARM + 2
