"""Random erasing without a GPU: the plan and its sampler, ``erase_reference`` against a per-sample slicing
loop (alone and followed by the batch mix), the float64 replica of the "pixel" fill, the model and engine
surface and the command-line flags."""
import math

import numpy as np
import pytest
import torch

from pytorch_vit_paper_replication_amd import engine
from pytorch_vit_paper_replication_amd.data import BatchMix, ErasePlan, MixPlan, RandomErasing, erase_reference, mix_reference
from pytorch_vit_paper_replication_amd.models import TinyVGG, ViT, vit
from tests import erase_oracle as O
from tests.test_batch_mix_cpu import loop_mix


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ----------------------------------------------------------------------------- plan
def test_plan_refuses_bad_boxes_and_wrong_batches():
    H, W = 24, 40
    good = ErasePlan([[3, 2, 17, 9], [0, 0, W, H], [5, 5, 5, 5]], (H, W))
    assert good.batch == 3 and good.size == (H, W) and good.mode == "pixel" and good.erased.tolist() == [True, True, False]
    assert good.rows.dtype == torch.int32 and tuple(good.rows.shape) == (3, 4) and torch.equal(good.rows, good.box)
    assert good.on("cpu") is good.rows
    good.check(3, (H, W))
    for bad in ([-1, 0, 4, 4], [0, -1, 4, 4], [0, 0, W + 1, 4], [0, 0, 4, H + 1], [9, 0, 4, 4], [0, 9, 4, 4]):
        with pytest.raises(ValueError, match="boxes"):
            ErasePlan([bad], (H, W))
    with pytest.raises(ValueError):
        good.check(2, (H, W))
    with pytest.raises(ValueError):
        good.check(3, (W, H))
    with pytest.raises(ValueError, match="mode"):
        ErasePlan([[0, 0, 1, 1]], (H, W), mode="colour")
    with pytest.raises(ValueError, match="value"):
        ErasePlan([[0, 0, 1, 1]], (H, W), mode="const", value=[0.0] * 5)
    none = ErasePlan.none(5, (H, W), mode="const", value=(0.1, 0.2, 0.3))
    assert none.batch == 5 and not none.box.any() and not none.erased.any() and none.channel_values(3) == (0.1, 0.2, 0.3)
    assert ErasePlan.none(2, (H, W), "const", 0.5).channel_values(3) == (0.5, 0.5, 0.5)
    with pytest.raises(ValueError):
        none.channel_values(4)
    x = torch.zeros(3, 3, H, W)
    with pytest.raises(ValueError):
        erase_reference(x, ErasePlan.none(2, (H, W)))
    with pytest.raises(ValueError):
        erase_reference(x, ErasePlan.none(3, (H, H)))


# ----------------------------------------------------------------------------- sampler
def test_sampler_prob_zero_and_seeding():
    a = RandomErasing(prob=0.0, generator=_gen(1))
    p = a.sample(64, 224, 224)
    assert p.batch == 64 and p.size == (224, 224) and not p.box.any() and not p.erased.any()
    b, c = (RandomErasing(prob=0.5, generator=_gen(7)) for _ in range(2))
    for _ in range(5):
        assert torch.equal(b.sample(16, 224, 224).rows, c.sample(16, 224, 224).rows)
    # the number of values drawn does not depend on the decisions
    g0, g1 = _gen(9), _gen(9)
    RandomErasing(prob=0.0, generator=g0).sample(8, 224, 224)
    RandomErasing(prob=1.0, generator=g1).sample(8, 224, 224)
    assert torch.equal(g0.get_state(), g1.get_state())
    for bad in (dict(prob=1.5), dict(scale=(0.0, 0.3)), dict(scale=(0.5, 0.3)), dict(ratio=(0.0, 3.3)), dict(mode="rand")):
        with pytest.raises(ValueError):
            RandomErasing(**bad)


def test_sampler_prob_one_boxes_and_the_rounding_bound():
    H = W = 224
    s = RandomErasing(prob=1.0, generator=_gen(3))
    n = 0
    for _ in range(8):
        p = s.sample(250, H, W)
        x0, y0, x1, y1 = (t.long() for t in p.box.unbind(1))
        w, h = x1 - x0, y1 - y0
        hit = p.erased
        assert torch.equal(hit, ~torch.isnan(s.last_area)) and torch.equal(hit, ~torch.isnan(s.last_ratio))
        assert bool(((w[hit] > 0) & (w[hit] < W) & (h[hit] > 0) & (h[hit] < H)).all())
        assert bool(((x0 >= 0) & (x1 <= W) & (y0 >= 0) & (y1 <= H))[hit].all())
        assert not p.box[~hit].any()
        area, r = s.last_area[hit], s.last_ratio[hit]
        assert bool(((area >= 0.02 * H * W) & (area <= H * W / 3) & (r >= 0.3) & (r <= 3.3)).all())
        # h = round(a), w = round(b) with a * b = area: |h * w - area| <= (a + b) / 2 + 1/4
        bound = (torch.sqrt(area * r) + torch.sqrt(area / r)) / 2 + 0.25
        assert bool((((h * w)[hit].double() - area).abs() <= bound).all())
        n += int(hit.sum())
    assert n > 1900  # at 224 x 224 nearly every sample finds a box within 10 attempts
    # top-left corners reach both ends of their range
    assert int(p.box[:, 0].min()) <= 3 and int(p.box[:, 1].min()) <= 3
    assert int(p.box[:, 2].max()) >= W - 3 and int(p.box[:, 3].max()) >= H - 3


def test_sampler_erased_fraction_follows_prob():
    N, H, W = 4000, 224, 224
    acc = float(RandomErasing(prob=1.0, generator=_gen(11)).sample(N, H, W).erased.double().mean())
    frac = float(RandomErasing(prob=0.25, generator=_gen(11)).sample(N, H, W).erased.double().mean())
    q = 0.25 * acc
    sigma = math.sqrt(q * (1 - q) / N)
    print(f"acceptance {acc:.4f}, erased fraction {frac:.4f}, expected {q:.4f} +- {sigma:.4f}")
    assert acc > 0.9 and abs(frac - q) <= 5 * sigma


def test_sampler_small_image_without_an_accepted_attempt_is_not_erased():
    # scale (0.9, 1) of a 4 x 4 image: every box is at least as large as the image along one side
    p = RandomErasing(prob=1.0, scale=(0.99, 1.0), ratio=(1.0, 1.0), generator=_gen(0)).sample(32, 4, 4)
    assert not p.erased.any() and not p.box.any()


# ----------------------------------------------------------------------------- reference formula
def _plan(B, H, W, mode, value=0.0):
    boxes = [[3, 2, 17, 9], [0, 0, W, H], [5, 5, 5, 9], [W - 4, H - 3, W, H]]
    return ErasePlan(boxes[:B], (H, W), mode, value)


@pytest.mark.parametrize("mode,value", [("const", 0.0), ("const", (0.25, -1.5, 2.0)), ("pixel", 0.0)])
def test_erase_reference_equals_the_slicing_loop(mode, value):
    B, C, H, W = 4, 3, 24, 40
    x = torch.randn(B, C, H, W, generator=_gen(1))
    fill = torch.randn(B, C, H, W, generator=_gen(2)) if mode == "pixel" else None
    plan = _plan(B, H, W, mode, value)
    got = erase_reference(x, plan, fill)
    want = O.loop_erase(x, plan, fill)
    assert torch.equal(got, want)
    assert torch.equal(got[2], x[2]) and not torch.equal(got[0], x[0])  # empty box: untouched
    assert torch.equal(erase_reference(x, ErasePlan.none(B, (H, W), mode, value), fill), x)
    # integer batches are cast first
    xi = torch.randint(0, 256, (B, C, H, W), generator=_gen(3), dtype=torch.uint8)
    assert torch.equal(erase_reference(xi, plan, fill), O.loop_erase(xi.float(), plan, fill))
    if mode == "pixel":  # fill=None draws from torch's RNG
        torch.manual_seed(5)
        z = torch.randn(B, C, H, W)
        torch.manual_seed(5)
        assert torch.equal(erase_reference(x, plan), O.loop_erase(x, plan, z))
        with pytest.raises(ValueError, match="fill"):
            erase_reference(x, plan, fill[:, :1])
    else:
        with pytest.raises(ValueError, match="fill"):
            erase_reference(x, plan, torch.zeros_like(x))


@pytest.mark.parametrize("mode", ["const", "pixel"])
def test_erase_then_mix_equals_the_loop_version(mode):
    B, C, H, W = 4, 3, 24, 40
    x = torch.randn(B, C, H, W, generator=_gen(4))
    fill = torch.randn(B, C, H, W, generator=_gen(5)) if mode == "pixel" else None
    eplan = _plan(B, H, W, mode, (0.5, 0.0, -0.5))
    mplan = MixPlan([1, 0, 3, 2], [0.3, 1.0, 1.0, 0.75], [[0, 0, 0, 0], [5, 1, 30, 20], [0, 0, W, H], [0, 0, 0, 0]], (H, W))
    got = mix_reference(erase_reference(x, eplan, fill), mplan)
    want = loop_mix(O.loop_erase(x, eplan, fill), mplan.partner, mplan.lam, mplan.box)
    assert torch.equal(got, want)
    # sample 2 is replaced by its partner 3, whose corner box is erased under the partner's plan
    e3 = O.loop_erase(x, eplan, fill)[3]
    assert torch.equal(got[2], e3) and not torch.equal(e3, x[3])


# ----------------------------------------------------------------------------- the fill
def test_fill_replica_moments():
    """Counter 0, 2^18 elements: mean, variance and lag-1 correlation of the float64 replica inside 5 sigma of a
    standard normal's (1 / sqrt(n), sqrt(2 / n), 1 / sqrt(n)); |z| <= 5.77; the float32 yardstick agrees."""
    n = 1 << 18
    u1, u2 = O.uniforms(0, n)
    assert u1.min() > 0 and u1.max() <= 1 and u2.min() >= 0 and u2.max() < 1
    assert np.array_equal(u1.astype(np.float32).astype(np.float64), u1) and np.array_equal(u2.astype(np.float32).astype(np.float64), u2)
    z = O.normal64(u1, u2)
    mean, var = z.mean(), z.var()
    lag1 = np.corrcoef(z[:-1], z[1:])[0, 1]
    kurt = ((z - mean) ** 4).mean() / var ** 2
    print(f"mean {mean:.5f} var {var:.5f} lag1 {lag1:.5f} kurtosis {kurt:.4f} max|z| {np.abs(z).max():.3f}")
    assert abs(mean) <= 5 / math.sqrt(n)
    assert abs(var - 1) <= 5 * math.sqrt(2 / n)
    assert abs(lag1) <= 5 / math.sqrt(n)
    assert np.abs(z).max() <= 5.77
    z32 = O.normal32(u1, u2)
    assert z32.dtype == np.float32 and np.abs(z32.astype(np.float64) - z).max() < 1e-5
    # another counter value, another tensor
    assert not np.array_equal(O.normal64(*O.uniforms(1, 4096)), z[:4096])


# ----------------------------------------------------------------------------- model, engine, CLI
TINY = dict(image_size=32, patch_size=8, num_transformer_layer=2, num_heads=2, embedding_dim=128, mlp_size=256, num_classes=5,
            mlp_dropout=0.0, embedding_dropout=0.0)


@pytest.mark.parametrize("mode", ["const", "pixel"])
def test_cpu_model_with_a_plan_equals_the_model_on_the_erased_batch(mode, monkeypatch):
    from pytorch_vit_paper_replication_amd.data import random_erasing as RE
    from pytorch_vit_paper_replication_amd.models.vit_no_classifier import ViT as Backbone

    B, S = 4, 32
    x = torch.randn(B, 3, S, S, generator=_gen(6))
    fill = torch.randn(B, 3, S, S, generator=_gen(7)) if mode == "pixel" else None
    eplan = _plan(B, S, S, mode, (0.5, 0.0, -0.5))
    mplan = MixPlan([1, 0, 3, 2], [0.3, 1.0, 1.0, 0.75], [[0, 0, 0, 0], [5, 1, 30, 20], [0, 0, S, S], [0, 0, 0, 0]], (S, S))
    if mode == "pixel":  # inject the fill where the model draws it
        orig = RE.erase_reference
        monkeypatch.setattr(RE, "erase_reference", lambda t, p, f=None: orig(t, p, fill if f is None else f))
    for cls, cfg in ((ViT, TINY), (Backbone, {k: v for k, v in TINY.items() if k != "num_classes"})):
        torch.manual_seed(0)
        m = cls(**cfg).eval()
        with torch.no_grad():
            erased = O.loop_erase(x, eplan, fill)
            assert torch.equal(m(x, erase=eplan), m(erased))
            assert not torch.equal(m(x, erase=eplan), m(x))
            assert torch.equal(m(x, mix=mplan, erase=eplan), m(mix_reference(erased, mplan)))
            assert torch.equal(m(x, erase=ErasePlan.none(B, (S, S), mode)), m(x))
        with pytest.raises(ValueError):
            m(x[:2], erase=eplan)


class _NoSched:
    def step(self):
        pass


class _Recording(RandomErasing):
    def __init__(self, **kw):
        super().__init__(**kw)
        self.plans = []

    def sample(self, *a):
        self.plans.append(super().sample(*a))
        return self.plans[-1]


@pytest.mark.parametrize("with_mix", [False, True])
def test_train_step_with_random_erasing_on_the_tiny_vit(with_mix):
    torch.manual_seed(0)
    model = vit("vit_tiny_test", image_size=32, num_classes=5, mlp_dropout=0.0, embedding_dropout=0.0)
    g = _gen(9)
    data = [(torch.randn(4, 3, 32, 32, generator=g), torch.randint(0, 5, (4,), generator=g)) for _ in range(2)]
    eraser = _Recording(prob=1.0, mode="const", value=0.5, generator=_gen(10))
    mixer = BatchMix(per_sample=True, generator=_gen(11)) if with_mix else None
    lr0 = torch.optim.SGD(model.parameters(), lr=0.0)  # parameters stay put: the loss can be recomputed
    loss, acc = engine.train_step(model, data, torch.nn.CrossEntropyLoss(), lr0, _NoSched(), "cpu", batch_mix=mixer,
                                  random_erasing=eraser)
    assert math.isfinite(loss) and 0.0 <= acc <= 1.0
    assert len(eraser.plans) == 2 and all(p.size == (32, 32) and p.batch == 4 and p.erased.any() for p in eraser.plans)
    if not with_mix:
        with torch.no_grad():  # train mode without dropout is deterministic
            want = [float(torch.nn.functional.cross_entropy(model(erase_reference(X, p)), y)) for (X, y), p in zip(data, eraser.plans)]
        assert loss == pytest.approx(sum(want) / 2, rel=1e-5)
    # pixel mode runs too (the noise comes from torch's RNG on the CPU)
    loss2, _ = engine.train_step(model, data, torch.nn.CrossEntropyLoss(), lr0, _NoSched(), "cpu", batch_mix=mixer,
                                 random_erasing=RandomErasing(prob=1.0, generator=_gen(12)))
    assert math.isfinite(loss2)


def test_train_step_erases_the_batch_for_a_model_without_the_keyword():
    torch.manual_seed(0)
    model = TinyVGG(input_shape=3, hidden_units=4, output_shape=5)
    seen = []
    model.register_forward_pre_hook(lambda mod, args: seen.append(args[0].detach().clone()))
    g = _gen(13)
    data = [(torch.randn(4, 3, 64, 64, generator=g), torch.randint(0, 5, (4,), generator=g))]
    eraser = _Recording(prob=1.0, mode="const", value=(1.0, 2.0, 3.0), generator=_gen(14))
    opt = torch.optim.SGD(model.parameters(), lr=0.0)
    loss, _ = engine.train_step(model, data, torch.nn.CrossEntropyLoss(), opt, _NoSched(), "cpu", random_erasing=eraser)
    assert math.isfinite(loss) and len(seen) == 1
    assert torch.equal(seen[0], O.loop_erase(data[0][0], eraser.plans[0])) and not torch.equal(seen[0], data[0][0])


def test_cli_flags_build_the_sampler(tmp_path, monkeypatch):
    from pytorch_vit_paper_replication_amd.cli import train as T

    a = T.build_parser().parse_args([])
    assert a.random_erasing == 0 and a.random_erasing_mode == "pixel" and T.build_random_erasing(a) is None
    a = T.build_parser().parse_args(["--random-erasing", "0.25", "--random-erasing-mode", "const", "--seed", "3"])
    s, s2 = T.build_random_erasing(a), T.build_random_erasing(a)
    assert isinstance(s, RandomErasing) and s.prob == 0.25 and s.mode == "const"
    assert torch.equal(s.sample(64, 32, 32).rows, s2.sample(64, 32, 32).rows)  # seeded from --seed
    assert not torch.equal(T.build_random_erasing(a, rank=1).sample(64, 32, 32).rows, T.build_random_erasing(a).sample(64, 32, 32).rows)
    with pytest.raises(SystemExit):
        T.build_parser().parse_args(["--random-erasing-mode", "rand"])

    seen = {}
    orig = engine.train

    def spy(**kw):
        seen.update(random_erasing=kw["random_erasing"])
        return orig(**kw)

    monkeypatch.setattr(engine, "train", spy)
    rc = T.main(["--model", "vit_tiny_test", "--synthetic", "--epochs", "1", "--batch-size", "4", "--image-size", "32",
                 "--num-classes", "3", "--synthetic-train-len", "8", "--synthetic-test-len", "4", "--save-dir", str(tmp_path),
                 "--random-erasing", "1.0"])
    assert rc == 0 and isinstance(seen["random_erasing"], RandomErasing) and seen["random_erasing"].mode == "pixel"
    with pytest.raises(SystemExit):
        T.main(["--model", "vit_tiny_test", "--synthetic", "--random-erasing", "1.5"])
