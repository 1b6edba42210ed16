"""The binary cross-entropy loss without a GPU: ``binary_cross_entropy`` against torch's function on the explicit
target rows, the engine's handling of a ``BinaryCrossEntropy`` loss_fn (with and without ``batch_mix``), that every
other loss_fn keeps its path, and the command-line flags."""
import math

import pytest
import torch
import torch.nn.functional as F

from pytorch_vit_paper_replication_amd import engine
from pytorch_vit_paper_replication_amd.data import BatchMix, MixPlan, mix_reference
from pytorch_vit_paper_replication_amd.losses import BinaryCrossEntropy
from pytorch_vit_paper_replication_amd.models import vit
from pytorch_vit_paper_replication_amd.ops import fused_vit
from pytorch_vit_paper_replication_amd.ops.fused_vit import binary_cross_entropy, soft_targets


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _case(B=6, C=7, seed=1):
    g = _gen(seed)
    x = torch.randn(B, C, generator=g) * 3
    y = torch.randint(0, C, (B,), generator=g)
    plan = MixPlan([(b + 1) % B for b in range(B)], [0.3, 1.0, 0.0, 0.625, 0.5, 0.9][:B], [[0, 0, 0, 0]] * B, (8, 8))
    return x, y, plan


# ----------------------------------------------------------------------------- function
@pytest.mark.parametrize("sum_classes", [False, True])
@pytest.mark.parametrize("thr", [None, 0.2])
@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("mixed", [False, True])
def test_function_is_torchs_bce_on_the_explicit_rows(mixed, eps, thr, sum_classes):
    x, y, plan = _case()
    plan = plan if mixed else None
    t = soft_targets(y, x.shape[1], plan, eps, x.dtype)
    if thr is not None:
        t = t.gt(thr).to(x.dtype)
    want = F.binary_cross_entropy_with_logits(x, t, reduction="none").sum(-1).mean() if sum_classes \
        else F.binary_cross_entropy_with_logits(x, t)
    fused_vit.last_correct = "stale"
    got = binary_cross_entropy(x, y, plan, eps, thr, sum_classes)
    assert torch.equal(got, want) and fused_vit.last_correct is None
    mod = BinaryCrossEntropy(smoothing=eps, target_threshold=thr, sum_classes=sum_classes)
    assert torch.equal(mod(x, y, plan), want)
    # and it differentiates: torch's own gradient of the same expression
    xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    binary_cross_entropy(xa, y, plan, eps, thr, sum_classes).backward()
    (F.binary_cross_entropy_with_logits(xb, t, reduction="none").sum(-1).mean() if sum_classes
     else F.binary_cross_entropy_with_logits(xb, t)).backward()
    assert torch.equal(xa.grad, xb.grad)


def test_threshold_picks_the_mixed_classes():
    """lam 0.3, eps 0.1, C 10: rows hold 0.01, 0.28 and 0.64; 0.2 keeps both mixed classes, 0.5 the 0.7 side."""
    y = torch.tensor([2, 5])
    plan = MixPlan([1, 0], [0.3, 0.3], [[0, 0, 0, 0]] * 2, (8, 8))
    x = torch.zeros(2, 10, requires_grad=True)
    binary_cross_entropy(x, y, plan, 0.1, 0.2, True).backward()
    assert torch.equal(x.grad < 0, F.one_hot(y, 10).bool() | F.one_hot(y.flip(0), 10).bool())
    x.grad = None
    binary_cross_entropy(x, y, plan, 0.1, 0.5, True).backward()
    assert torch.equal(x.grad < 0, F.one_hot(y.flip(0), 10).bool())  # lam 0.3: the partner's class carries 0.7


def test_plan_batch_mismatch_and_bad_arguments_raise():
    x, y, plan = _case()
    with pytest.raises(ValueError):
        binary_cross_entropy(x[:3], y[:3], plan, 0.1)
    for thr in (1.0, -0.1):
        with pytest.raises(ValueError):
            binary_cross_entropy(x, y, None, 0.0, thr)
        with pytest.raises(ValueError):
            BinaryCrossEntropy(target_threshold=thr)
    with pytest.raises(ValueError):
        BinaryCrossEntropy(smoothing=1.5)


# ----------------------------------------------------------------------------- engine
class _NoSched:
    def step(self):
        pass


class _Recording(BinaryCrossEntropy):
    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.calls = []

    def forward(self, logits, y, plan=None):
        self.calls.append((plan, self.smoothing))
        return super().forward(logits, y, plan)


def _batches(n, B, S, C, seed):
    g = _gen(seed)
    return [(torch.randn(B, 3, S, S, generator=g), torch.randint(0, C, (B,), generator=g)) for _ in range(n)]


def _tiny():
    torch.manual_seed(0)
    return vit("vit_tiny_test", image_size=32, num_classes=5, mlp_dropout=0.0, embedding_dropout=0.0)


def test_train_step_hands_the_plan_to_the_module(monkeypatch):
    model = _tiny()
    data = _batches(2, 4, 32, 5, seed=9)
    mixer = BatchMix(per_sample=True, label_smoothing=0.1, generator=_gen(10))
    lf = _Recording(sum_classes=True)
    soft_calls = []
    monkeypatch.setattr(engine, "soft_cross_entropy", lambda *a, **kw: soft_calls.append(a) or fused_vit.soft_cross_entropy(*a, **kw))
    lr0 = torch.optim.SGD(model.parameters(), lr=0.0)  # parameters stay put: the losses can be recomputed
    loss, acc = engine.train_step(model, data, lf, lr0, _NoSched(), "cpu", batch_mix=mixer)
    assert not soft_calls
    assert len(lf.calls) == 2 and all(isinstance(p, MixPlan) and p.batch == 4 for p, _ in lf.calls)
    assert lf.calls[0][0] is not lf.calls[1][0]
    assert [s for _, s in lf.calls] == [0.1, 0.1] and lf.smoothing == 0.0  # batch_mix's smoothing, for the call only
    want, hits = [], []
    with torch.no_grad():  # train mode without dropout is deterministic
        for (X, y), (p, _) in zip(data, lf.calls):
            logits = model(mix_reference(X, p))
            t = soft_targets(y, 5, p, 0.1)
            want.append(float(F.binary_cross_entropy_with_logits(logits, t, reduction="none").sum(-1).mean()))
            hits.append(float((logits.argmax(1) == y).float().mean()))
    assert loss == pytest.approx(sum(want) / 2, rel=1e-6) and acc == pytest.approx(sum(hits) / 2)
    # the same smoothing on both sides is no conflict, and the parameters move under a real optimizer
    before = [p.detach().clone() for p in model.parameters()]
    engine.train_step(model, data, BinaryCrossEntropy(smoothing=0.1), torch.optim.SGD(model.parameters(), lr=0.1), _NoSched(),
                      "cpu", batch_mix=mixer)
    assert any(not torch.equal(a, b) for a, b in zip(before, model.parameters()))


def test_without_batch_mix_and_in_test_step_the_module_gets_no_plan():
    model = _tiny()
    data = _batches(2, 4, 32, 5, seed=11)
    lf = _Recording(smoothing=0.1, target_threshold=0.2)
    loss, _ = engine.train_step(model, data, lf, torch.optim.SGD(model.parameters(), lr=0.0), _NoSched(), "cpu")
    assert [c for c in lf.calls] == [(None, 0.1)] * 2
    with torch.no_grad():
        want = [float(F.binary_cross_entropy_with_logits(model(X), soft_targets(y, 5, None, 0.1).gt(0.2).float())) for X, y in data]
    assert loss == pytest.approx(sum(want) / 2, rel=1e-6)
    lf.calls.clear()
    tl, ta = engine.test_step(model, data, lf, "cpu")
    assert [c for c in lf.calls] == [(None, 0.1)] * 2
    with torch.no_grad():
        model.eval()
        outs = [model(X) for X, _ in data]
    want = [float(F.binary_cross_entropy_with_logits(o, soft_targets(y, 5, None, 0.1).gt(0.2).float())) for o, (_, y) in zip(outs, data)]
    assert tl == pytest.approx(sum(want) / 2, rel=1e-6)
    assert ta == pytest.approx(sum(float((o.argmax(1) == y).float().mean()) for o, (_, y) in zip(outs, data)) / 2)


def test_smoothing_conflict_raises_before_any_batch():
    model = _tiny()
    lf = _Recording(smoothing=0.2)

    def no_data():
        raise AssertionError("the loader was read")
        yield

    with pytest.raises(ValueError, match="smoothing"):
        engine.train_step(model, no_data(), lf, torch.optim.SGD(model.parameters(), lr=0.0), _NoSched(), "cpu",
                          batch_mix=BatchMix(label_smoothing=0.1, generator=_gen(1)))
    assert not lf.calls


def _old_rule(loss_fn, batch_mix):
    """engine.train_step's choice of the loss before BinaryCrossEntropy existed, literally."""
    return engine._fused_loss(loss_fn) if batch_mix is None else engine._SoftLoss(batch_mix.label_smoothing)


@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("mixed", [False, True])
def test_cross_entropy_takes_the_path_it_took(mixed, eps):
    data = _batches(2, 4, 32, 5, seed=14)

    def mixer():
        return BatchMix(per_sample=True, label_smoothing=eps, generator=_gen(15)) if mixed else None

    # the old rule, driven by hand over the same batches and plans
    model = _tiny()
    bm, lf = mixer(), None
    lf = _old_rule(torch.nn.CrossEntropyLoss(label_smoothing=eps), bm)
    assert type(lf) is engine._SoftLoss if (mixed or eps) else lf is engine.cross_entropy
    opt = torch.optim.SGD(model.parameters(), lr=0.1)
    model.train()
    losses = []
    for X, y in data:
        if bm is not None:
            lf.plan = bm.sample(4, 32, 32)
            out = model(X, mix=lf.plan)
        else:
            out = model(X)
        loss = lf(out, y)
        opt.zero_grad()
        loss.backward()
        torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm=1.0)
        opt.step()
        losses.append(loss.detach().float())
    want_loss = float(torch.stack(losses).double().mean())
    want = [p.detach().clone() for p in model.parameters()]
    # the engine
    model = _tiny()
    loss, _ = engine.train_step(model, data, torch.nn.CrossEntropyLoss(label_smoothing=eps), torch.optim.SGD(model.parameters(), lr=0.1),
                                _NoSched(), "cpu", batch_mix=mixer())
    assert loss == pytest.approx(want_loss, rel=1e-6)
    for a, b in zip(want, model.parameters()):
        assert torch.equal(a, b)


# ----------------------------------------------------------------------------- command line
def _main_spy(monkeypatch, tmp_path, *flags):
    from pytorch_vit_paper_replication_amd.cli import train as T

    seen = {}
    monkeypatch.setattr(engine, "train", lambda **kw: seen.update(kw))
    rc = T.main(["--model", "vit_tiny_test", "--synthetic", "--epochs", "1", "--batch-size", "4", "--image-size", "32",
                 "--num-classes", "3", "--synthetic-train-len", "8", "--synthetic-test-len", "4", "--save-dir", str(tmp_path),
                 "--torch-optimizer", *flags])
    assert rc == 0
    return seen


def test_cli_flags_build_the_loss(tmp_path, monkeypatch):
    from pytorch_vit_paper_replication_amd.cli import train as T

    a = T.build_parser().parse_args([])
    assert a.bce_loss is False and a.bce_target_threshold is None and a.bce_sum_classes is False and a.head_bias_init is None
    lf = T.build_loss(T.build_parser().parse_args(["--label-smoothing", "0.1"]))
    assert type(lf) is torch.nn.CrossEntropyLoss and lf.label_smoothing == 0.1
    lf = T.build_loss(T.build_parser().parse_args(["--bce-loss", "--bce-target-threshold", "0.2", "--label-smoothing", "0.1"]))
    assert type(lf) is BinaryCrossEntropy and (lf.smoothing, lf.target_threshold, lf.sum_classes) == (0.1, 0.2, False)
    assert T.build_loss(T.build_parser().parse_args(["--bce-loss", "--bce-sum-classes"])).sum_classes is True
    seen = _main_spy(monkeypatch, tmp_path, "--bce-loss", "--bce-target-threshold", "0.2", "--label-smoothing", "0.1", "--cutmix", "1.0")
    lf = seen["loss_fn"]
    assert type(lf) is BinaryCrossEntropy and (lf.smoothing, lf.target_threshold, lf.sum_classes) == (0.1, 0.2, False)
    assert isinstance(seen["batch_mix"], BatchMix) and seen["batch_mix"].label_smoothing == 0.1
    seen = _main_spy(monkeypatch, tmp_path, "--label-smoothing", "0.1")
    assert type(seen["loss_fn"]) is torch.nn.CrossEntropyLoss and seen["loss_fn"].label_smoothing == 0.1
    for bad in (["--bce-target-threshold", "0.2"], ["--bce-sum-classes"], ["--bce-loss", "--bce-target-threshold", "1.0"],
                ["--model", "tinyvgg", "--head-bias-init", "-1"]):
        with pytest.raises(SystemExit):
            T.main(["--synthetic", *bad])


def test_cli_head_bias_init_fills_the_bias_and_nothing_else(tmp_path, monkeypatch):
    plain = _main_spy(monkeypatch, tmp_path)["model"].state_dict()
    got = _main_spy(monkeypatch, tmp_path, "--head-bias-init", "-6.9")["model"].state_dict()
    assert list(got) == list(plain)
    for k in plain:
        if k == "classifier.0.bias":
            assert torch.equal(got[k], torch.full_like(plain[k], -6.9)) and not torch.equal(got[k], plain[k])
        else:
            assert torch.equal(got[k], plain[k]), k


def test_init_head_bias_makes_the_stores_shadow_stale():
    """An outside write to a parameter is seen through its version counter; the method's write is one."""
    m, plain = _tiny(), _tiny()
    b = m.classifier[0].bias
    v0 = b._version
    assert m.init_head_bias(-math.log(5)) is m
    assert b._version > v0 and torch.equal(b, torch.full_like(b, -math.log(5)))
    assert list(m.state_dict()) == list(plain.state_dict())
    x = torch.randn(2, 3, 32, 32, generator=_gen(3))
    with torch.no_grad():  # the logits move by the change of the bias, class by class
        moved = m.eval()(x) - plain.eval()(x)
    assert torch.allclose(moved, (b - plain.classifier[0].bias).expand(2, 5), rtol=0, atol=1e-5)
