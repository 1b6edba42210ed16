"""Mixup / CutMix / label smoothing without a GPU: the plan sampler, ``mix_reference`` against a
per-sample slicing loop, ``soft_cross_entropy`` against torch's soft-target cross-entropy, the engine
path and the command-line flags."""
import math

import pytest
import torch
import torch.nn.functional as F

from pytorch_vit_paper_replication_amd import engine
from pytorch_vit_paper_replication_amd.data import BatchMix, MixPlan, mix_reference
from pytorch_vit_paper_replication_amd.models import TinyVGG, vit
from pytorch_vit_paper_replication_amd.ops.fused_vit import soft_cross_entropy, soft_targets


def loop_mix(x, partner, lam, boxes):
    """The mix formula one sample at a time, with slices (fp32 throughout)."""
    out = torch.empty_like(x)
    for b in range(x.shape[0]):
        own, par = x[b], x[int(partner[b])]
        l = torch.tensor(float(lam[b]), dtype=torch.float32)
        if float(l) == 1.0:
            out[b] = own
        else:
            out[b] = l * own + (torch.tensor(1.0, dtype=torch.float32) - l) * par
        x0, y0, x1, y1 = (int(v) for v in boxes[b])
        out[b, :, y0:y1, x0:x1] = par[:, y0:y1, x0:x1]
    return out


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ----------------------------------------------------------------------------- sampler
@pytest.mark.parametrize("per_sample", [False, True])
def test_sampler_is_seeded_and_in_range(per_sample):
    H, W, B = 24, 40, 7
    a, b = (BatchMix(per_sample=per_sample, generator=_gen(5)) for _ in range(2))
    seen_cut = seen_mix = 0
    for _ in range(40):
        p, q = a.sample(B, H, W), b.sample(B, H, W)
        assert torch.equal(p.rows, q.rows) and torch.equal(p.lam_eff, q.lam_eff) and torch.equal(p.partner, q.partner)
        assert p.size == (H, W) and p.batch == B
        assert bool(((p.lam >= 0) & (p.lam <= 1)).all()) and bool(((p.lam_eff >= 0) & (p.lam_eff <= 1)).all())
        x0, y0, x1, y1 = p.box.unbind(1)
        assert bool(((0 <= x0) & (x0 <= x1) & (x1 <= W) & (0 <= y0) & (y0 <= y1) & (y1 <= H)).all())
        assert bool(((p.partner >= 0) & (p.partner < B)).all())
        if not per_sample:
            untouched = p.lam_eff == 1
            assert torch.equal(p.partner[~untouched], (B - 1 - torch.arange(B))[~untouched])
        cut = (x1 > x0) & (y1 > y0)
        assert bool((p.lam[cut] == 1).all())  # CutMix rows select, mixup rows have no box
        seen_cut += int(cut.any())
        seen_mix += int((p.lam < 1).any())
        # the kernels' table
        assert p.rows.dtype == torch.int32 and tuple(p.rows.shape) == (B, 8)
        assert torch.equal(p.rows[:, 0].long(), p.partner) and torch.equal(p.rows[:, 1].view(torch.float32), p.lam)
        assert torch.equal(p.rows[:, 2:6], p.box)
    assert seen_cut > 5 and seen_mix > 5  # switch_prob = 0.5: both kinds are drawn
    assert not torch.equal(a.sample(B, H, W).rows, BatchMix(per_sample=per_sample, generator=_gen(6)).sample(B, H, W).rows)


def test_lam_eff_is_the_kept_pixel_fraction():
    H, W, B = 20, 28, 6
    mixer = BatchMix(mixup_alpha=0.0, cutmix_alpha=1.0, per_sample=True, generator=_gen(1))
    x = (torch.arange(B, dtype=torch.float32) + 1).view(B, 1, 1, 1).expand(B, 3, H, W).contiguous()
    clipped = 0
    for _ in range(20):
        p = mixer.sample(B, H, W)
        out = mix_reference(x, p)
        for b in range(B):
            if int(p.partner[b]) == b:  # a fixed point of the permutation: replaced by itself, nothing to count
                continue
            replaced = (out[b, 0] != x[b, 0]).sum().item()
            x0, y0, x1, y1 = p.box[b].tolist()
            assert replaced == (x1 - x0) * (y1 - y0) and bool((out[b] == out[b, :1]).all())
            assert float(p.lam_eff[b]) == pytest.approx(1.0 - replaced / (H * W), abs=1e-6)
            clipped += int((x1 > x0) and (x0 == 0 or y0 == 0 or x1 == W or y1 == H))
    assert clipped > 0  # boxes clipped by the image border are counted by what is left of them


def test_prob_zero_and_no_alpha_give_the_identity_plan():
    x = torch.randn(4, 3, 8, 8, generator=_gen(0))
    for mixer in (BatchMix(prob=0.0, generator=_gen(2)), BatchMix(mixup_alpha=0.0, cutmix_alpha=0.0, generator=_gen(2))):
        p = mixer.sample(4, 8, 8)
        ident = MixPlan.identity(4, (8, 8))
        assert torch.equal(p.rows, ident.rows) and bool((p.lam_eff == 1).all())
        assert torch.equal(p.partner, torch.arange(4)) and not p.box.any()
        assert torch.equal(mix_reference(x, p), x)


def test_plan_validates():
    with pytest.raises(ValueError):
        MixPlan([0, 2], [1.0, 1.0], [[0, 0, 0, 0]] * 2, (8, 8))   # partner == B
    with pytest.raises(ValueError):
        MixPlan([0, 1], [1.0, 1.0], [[0, 0, 9, 4]] * 2, (8, 8))   # box outside
    with pytest.raises(ValueError):
        MixPlan([0, 1], [1.5, 1.0], [[0, 0, 0, 0]] * 2, (8, 8))   # lam
    with pytest.raises(ValueError):
        mix_reference(torch.zeros(3, 3, 8, 8), MixPlan.identity(2, (8, 8)))  # batch mismatch
    with pytest.raises(ValueError):
        BatchMix(label_smoothing=1.0)


# ----------------------------------------------------------------------------- mix_reference
PLANS = {
    "mixup": ([2, 1, 0], [0.3, 0.3, 0.3], [[0, 0, 0, 0]] * 3),
    "cutmix": ([2, 1, 0], [1.0] * 3, [[3, 5, 13, 9]] * 3),
    "two_edges": ([1, 2, 0], [1.0] * 3, [[7, 0, 16, 6], [0, 4, 5, 12], [0, 0, 16, 12]]),
    "empty_box": ([2, 1, 0], [1.0] * 3, [[4, 4, 4, 9], [0, 0, 0, 0], [16, 12, 16, 12]]),
    "self_partner": ([0, 1, 2], [0.3, 1.0, 0.7], [[0, 0, 0, 0], [2, 2, 9, 9], [0, 0, 0, 0]]),
    "both": ([1, 0, 1], [0.25, 0.6, 1.0], [[2, 3, 11, 8], [0, 0, 16, 1], [15, 11, 16, 12]]),
}


@pytest.mark.parametrize("name", sorted(PLANS))
def test_mix_reference_equals_the_slicing_loop(name):
    partner, lam, boxes = PLANS[name]
    x = torch.randn(3, 3, 12, 16, generator=_gen(3))
    plan = MixPlan(partner, lam, boxes, (12, 16))
    got = mix_reference(x, plan)
    assert got.dtype == torch.float32 and torch.equal(got, loop_mix(x, partner, lam, boxes))
    if name == "empty_box":
        assert torch.equal(got, x)
    else:
        assert not torch.equal(got, x)
    # integer batches are cast first
    xi = torch.randint(0, 256, (3, 3, 12, 16), generator=_gen(4), dtype=torch.uint8)
    assert torch.equal(mix_reference(xi, plan), loop_mix(xi.float(), partner, lam, boxes))


# ----------------------------------------------------------------------------- loss
@pytest.mark.parametrize("eps", [0.0, 0.1])
def test_soft_cross_entropy_cpu(eps):
    B, C = 5, 11
    x = torch.randn(B, C, generator=_gen(7)) * 3
    y = torch.randint(0, C, (B,), generator=_gen(8))
    plan = MixPlan([4, 3, 2, 1, 0], [1.0, 0.3, 1.0, 0.6, 1.0], [[0, 0, 4, 2], [0, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0], [1, 1, 3, 4]], (4, 8))
    lam = plan.lam_eff.double().view(B, 1)
    assert plan.lam_eff.tolist() == pytest.approx([0.75, 0.3, 1.0, 0.6, 1.0 - 6 / 32])
    q = lam * F.one_hot(y, C).double() + (1 - lam) * F.one_hot(y[plan.partner], C).double()
    want = F.cross_entropy(x.double(), q, label_smoothing=eps)
    got = soft_cross_entropy(x, y, plan, eps)
    assert got.dtype == torch.float32 and float(got) == pytest.approx(float(want), rel=2e-6)
    assert torch.allclose(soft_targets(y, C, plan, eps, torch.float64), (1 - eps) * q + eps / C, atol=1e-7)
    # no plan: torch's own label smoothing, to the bit
    assert torch.equal(soft_cross_entropy(x, y, None, eps), F.cross_entropy(x, y, label_smoothing=eps))
    with pytest.raises(ValueError):
        soft_cross_entropy(x[:3], y[:3], plan, eps)


# ----------------------------------------------------------------------------- engine
class _RecordingMix(BatchMix):
    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.plans = []

    def sample(self, *a):
        self.plans.append(super().sample(*a))
        return self.plans[-1]


class _NoSched:
    def step(self):
        pass


def _batches(n, B, S, C, seed):
    g = _gen(seed)
    return [(torch.randn(B, 3, S, S, generator=g), torch.randint(0, C, (B,), generator=g)) for _ in range(n)]


def test_train_step_with_batch_mix_on_the_tiny_vit():
    torch.manual_seed(0)
    model = vit("vit_tiny_test", image_size=32, num_classes=5, mlp_dropout=0.0, embedding_dropout=0.0)
    data = _batches(2, 4, 32, 5, seed=9)
    mixer = _RecordingMix(per_sample=True, label_smoothing=0.1, generator=_gen(10))
    lr0 = torch.optim.SGD(model.parameters(), lr=0.0)  # parameters stay put: the losses can be recomputed
    loss, acc = engine.train_step(model, data, torch.nn.CrossEntropyLoss(), lr0, _NoSched(), "cpu", batch_mix=mixer)
    assert len(mixer.plans) == 2 and all(p.size == (32, 32) and p.batch == 4 for p in mixer.plans)
    assert any(bool((p.lam_eff < 1).any()) for p in mixer.plans)
    want, hits = [], []
    with torch.no_grad():  # train mode without dropout is deterministic
        for (X, y), p in zip(data, mixer.plans):
            logits = model(mix_reference(X, p))
            lam = p.lam_eff.view(-1, 1)
            q = lam * F.one_hot(y, 5).float() + (1 - lam) * F.one_hot(y[p.partner], 5).float()
            want.append(float(F.cross_entropy(logits, q, label_smoothing=0.1)))
            hits.append(float((logits.argmax(1) == y).float().mean()))
    assert loss == pytest.approx(sum(want) / 2, rel=1e-5) and acc == pytest.approx(sum(hits) / 2)
    # and the parameters move under a real optimizer
    before = [p.detach().clone() for p in model.parameters()]
    engine.train_step(model, data, torch.nn.CrossEntropyLoss(), torch.optim.SGD(model.parameters(), lr=0.1), _NoSched(), "cpu",
                      batch_mix=mixer)
    assert any(not torch.equal(a, b) for a, b in zip(before, model.parameters()))


def test_model_forward_takes_a_plan_in_eval_mode():
    torch.manual_seed(0)
    model = vit("vit_tiny_test", image_size=32, num_classes=5).eval()
    (X, _), = _batches(1, 3, 32, 5, seed=11)
    plan = MixPlan([2, 1, 0], [0.4, 1.0, 1.0], [[0, 0, 0, 0], [0, 0, 0, 0], [5, 6, 30, 17]], (32, 32))
    with torch.no_grad():
        assert torch.equal(model(X, mix=plan), model(mix_reference(X, plan)))
        assert torch.equal(model(X, mix=None), model(X)) and not torch.equal(model(X, mix=plan), model(X))
        with pytest.raises(ValueError):
            model(X[:2], mix=plan)


def test_engine_mixes_the_batch_itself_for_a_model_without_mix():
    torch.manual_seed(0)
    model = TinyVGG(input_shape=3, hidden_units=4, output_shape=3)
    data = _batches(1, 4, 64, 3, seed=12)
    mixer = _RecordingMix(label_smoothing=0.0, generator=_gen(13))
    seen = []
    model.register_forward_pre_hook(lambda mod, args: seen.append(args[0].detach().clone()))
    loss, _ = engine.train_step(model, data, torch.nn.CrossEntropyLoss(), torch.optim.SGD(model.parameters(), lr=0.0), _NoSched(),
                                "cpu", batch_mix=mixer)
    assert mixer.plans[0].size == (64, 64) and torch.equal(seen[0], mix_reference(data[0][0], mixer.plans[0]))
    assert math.isfinite(loss)


def test_label_smoothing_loss_keeps_torchs_value_on_cpu():
    torch.manual_seed(0)
    model = vit("vit_tiny_test", image_size=32, num_classes=5, mlp_dropout=0.0, embedding_dropout=0.0)
    data = _batches(2, 4, 32, 5, seed=14)
    lf = torch.nn.CrossEntropyLoss(label_smoothing=0.1)
    assert isinstance(engine._fused_loss(lf), engine._SoftLoss)
    assert engine._fused_loss(torch.nn.CrossEntropyLoss()) is engine.cross_entropy
    for other in (torch.nn.CrossEntropyLoss(label_smoothing=0.1, reduction="sum"),
                  torch.nn.CrossEntropyLoss(label_smoothing=0.1, weight=torch.ones(5)),
                  torch.nn.CrossEntropyLoss(label_smoothing=0.1, ignore_index=0)):
        assert engine._fused_loss(other) is other
    loss, _ = engine.train_step(model, data, lf, torch.optim.SGD(model.parameters(), lr=0.0), _NoSched(), "cpu")
    with torch.no_grad():
        want = [float(lf(model(X), y)) for X, y in data]
    assert loss == pytest.approx(sum(want) / 2, rel=1e-6)
    tl, _ = engine.test_step(model, data, lf, "cpu")
    with torch.no_grad():
        model.eval()
        assert tl == pytest.approx(sum(float(lf(model(X), y)) for X, y in data) / 2, rel=1e-6)


# ----------------------------------------------------------------------------- command line
def test_cli_flags_build_the_batch_mix(tmp_path, monkeypatch):
    from pytorch_vit_paper_replication_amd.cli import train as T

    a = T.build_parser().parse_args([])
    assert a.mixup == 0 and a.cutmix == 0 and a.mix_prob == 1.0 and a.mix_switch_prob == 0.5 and a.label_smoothing == 0
    assert T.build_batch_mix(a) is None
    a = T.build_parser().parse_args(["--mixup", "0.8", "--cutmix", "1.0", "--mix-prob", "0.9", "--mix-switch-prob", "0.25",
                                     "--label-smoothing", "0.1", "--seed", "3"])
    m, m2 = T.build_batch_mix(a), T.build_batch_mix(a)
    assert isinstance(m, BatchMix) and (m.mixup_alpha, m.cutmix_alpha, m.prob, m.switch_prob, m.label_smoothing) == (0.8, 1.0, 0.9, 0.25, 0.1)
    assert torch.equal(m.sample(4, 32, 32).rows, m2.sample(4, 32, 32).rows)  # seeded from --seed
    assert not torch.equal(T.build_batch_mix(a, rank=1).sample(4, 32, 32).rows, T.build_batch_mix(a).sample(4, 32, 32).rows)
    assert T.build_batch_mix(T.build_parser().parse_args(["--label-smoothing", "0.1"])) is None

    seen = {}
    orig = engine.train

    def spy(**kw):
        seen.update(batch_mix=kw["batch_mix"], loss_fn=kw["loss_fn"])
        return orig(**kw)

    monkeypatch.setattr(engine, "train", spy)
    rc = T.main(["--model", "vit_tiny_test", "--synthetic", "--epochs", "1", "--batch-size", "4", "--image-size", "32",
                 "--num-classes", "3", "--synthetic-train-len", "8", "--synthetic-test-len", "4", "--save-dir", str(tmp_path),
                 "--cutmix", "1.0", "--label-smoothing", "0.1"])
    assert rc == 0 and isinstance(seen["batch_mix"], BatchMix) and seen["batch_mix"].mixup_alpha == 0
    assert seen["loss_fn"].label_smoothing == 0.1
    assert math.isfinite(float(torch.load(tmp_path / "vit_tiny_test_1_epochs.pth", weights_only=True)["classifier.0.weight"].sum()))
