"""Colour augmentation (data/color_augment.py) without a GPU: ``color_reference`` against PIL byte for byte on
the pointwise ops and the jitter, its blur against an independent numpy implementation of the formula
(bytes) and against PIL's own Gaussian blur (a sanity bound), the sampler, and the CLI."""
import numpy as np
import pytest
import torch
from PIL import Image, ImageFilter

from pytorch_vit_paper_replication_amd.data import ColorAugment, ColorPlan, DeviceInput, color_reference
from pytorch_vit_paper_replication_amd.data.color_augment import blur_weights
from pytorch_vit_paper_replication_amd.models.vit import ViT

from . import color_oracle as O

TINY = dict(image_size=32, patch_size=16, num_transformer_layer=1, num_heads=2, embedding_dim=128, mlp_size=256, num_classes=3,
            mlp_dropout=0.0, embedding_dropout=0.0)  # no dropout: training forwards differ by the colour draw alone


@pytest.mark.parametrize("shape", [(37, 45), (32, 64)])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_reference_equals_pil_on_pointwise_ops_and_jitter(shape, seed):
    x, plan = O.pointwise_case(7, *shape, seed)
    keep = x.clone()
    got, want = color_reference(x, plan), O.pil_chain(x, plan)
    assert got.dtype == torch.uint8 and got.shape == x.shape
    assert int((got != want).sum()) == 0
    assert torch.equal(x, keep)
    # channels_last gives the same bytes
    assert torch.equal(color_reference(x.contiguous(memory_format=torch.channels_last), plan), got)


def test_every_fixed_factor_in_every_order_equals_pil():
    x = O.images(4, 16, 24, 5)
    for op in (0, 1, 2):
        for order in range(6):
            for i, f in enumerate(O.FIXED_FACTORS):
                fac = torch.tensor([[f, O.FIXED_FACTORS[(i + 1) % 5], O.FIXED_FACTORS[(i + 2) % 5]]]).repeat(4, 1)
                plan = ColorPlan([op] * 4, None, fac, [order] * 4)
                assert int((color_reference(x, plan) != O.pil_chain(x, plan)).sum()) == 0, (op, order, f)


def test_contrast_mean_rounding():
    # half the pixels at L = 10 and half at L = 11: the mean 10.5 rounds to m = 11, and factor 0 returns m everywhere
    x = torch.full((3, 3, 4, 6), 10, dtype=torch.uint8)
    x[0, :, :, 3:] = 11
    x[1], x[2] = 255, 0
    out = color_reference(x, ColorPlan([0, 0, 0], None, [[1.0, 0.0, 1.0]] * 3, [0, 0, 0]))
    assert out[0].unique().tolist() == [11] and out[1].unique().tolist() == [255] and out[2].unique().tolist() == [0]
    assert torch.equal(out, O.pil_chain(x, ColorPlan([0, 0, 0], None, [[1.0, 0.0, 1.0]] * 3, [0, 0, 0])))


def test_identity_plan_returns_the_input_bytes():
    x = O.images(5, 9, 11, 3)
    assert torch.equal(color_reference(x, ColorPlan.none(5)), x)


@pytest.mark.parametrize("shape", [(37, 45), (32, 64), (70, 150), (5, 7)])
def test_reference_blur_equals_the_numpy_formula(shape):
    for seed, sigma in enumerate((0.1, 0.5, 1.0, 2.0, 0.34, 1.67)):
        x = O.images(2, *shape, seed)
        got = color_reference(x, ColorPlan([3, 3], [sigma, sigma]))
        w = blur_weights(sigma).numpy()
        for b in range(2):
            assert np.array_equal(got[b].numpy(), O.numpy_blur(x[b].numpy(), w)), (sigma, b)


def test_blur_weights():
    for sigma in (0.1, 0.33, 0.5, 1.0, 1.5, 2.0):
        w = blur_weights(sigma).double()
        R = min(6, max(1, int(np.ceil(3 * sigma))))
        assert w.shape == (13,) and abs(float(w.sum()) - 1) < 1e-6 and torch.equal(w, w.flip(0))
        assert bool((w[:6 - R] == 0).all()) and bool((w[6 - R:7 + R] > 0).all() or sigma < 0.2)
        k = torch.arange(-R, R + 1, dtype=torch.float64)
        e = torch.exp(-k * k / (2 * sigma * sigma))
        assert torch.equal(w[6 - R:7 + R].float(), (e / e.sum()).float())
    for bad in (0.0, -1.0, 2.5, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            blur_weights(bad)


def test_blur_stays_near_pil_gaussian_blur():
    # PIL's filter is a three-pass box approximation: a sanity bound, not a yardstick
    H = W = 48
    g = torch.Generator().manual_seed(11)
    ys, xs = torch.arange(H).view(H, 1), torch.arange(W).view(1, W)
    ramp = torch.stack([(5 * xs + 0 * ys) % 256, (5 * ys + 0 * xs) % 256, (3 * (xs + ys)) % 256]).double()
    x = (ramp + 12.0 * torch.randn(3, H, W, generator=g, dtype=torch.float64)).round().clamp(0, 255).to(torch.uint8)[None]
    im = Image.fromarray(np.ascontiguousarray(x[0].permute(1, 2, 0).numpy()), "RGB")
    for sigma in (0.5, 1.0, 1.5, 2.0):
        got = color_reference(x, ColorPlan([3], [sigma]))[0].permute(1, 2, 0).numpy().astype(np.float64)
        pil = np.asarray(im.filter(ImageFilter.GaussianBlur(radius=sigma))).astype(np.float64)
        mad = float(np.abs(got - pil).mean())
        print(f"sigma {sigma}: mean abs difference from PIL {mad:.3f} LSB")
        assert mad < 1.0, (sigma, mad)


def test_plan_validation():
    ok = dict(op=[0, 3], sigma=[1.0, 1.0], factors=[[1.0, 1.0, 1.0]] * 2, order=[0, 5])
    p = ColorPlan(**ok)
    assert p.batch == 2 and p.rows.shape == (2, 20) and p.rows.dtype == torch.float32
    assert p.rows.view(torch.int32)[:, 0].tolist() == [0, 3] and p.rows.view(torch.int32)[:, 1].tolist() == [0, 5]
    assert torch.equal(p.rows[1, 6:19], blur_weights(1.0)) and p.rows[0, 6:19].tolist() == [0.0] * 6 + [1.0] + [0.0] * 6
    for bad in (dict(op=[0, 4]), dict(op=[-1, 0]), dict(order=[0, 6]), dict(order=[-1, 0]), dict(factors=[[1.0, -0.1, 1.0]] * 2),
                dict(factors=[[float("nan"), 1.0, 1.0]] * 2), dict(factors=[[1.0, 1.0, float("inf")]] * 2), dict(sigma=[1.0, 0.0]),
                dict(sigma=[1.0, 2.5]), dict(sigma=[1.0, float("nan")]), dict(order=[0])):
        with pytest.raises(ValueError):
            ColorPlan(**{**ok, **bad})
    x = O.images(2, 8, 8, 0)
    with pytest.raises(ValueError):
        color_reference(x, ColorPlan.none(3))  # a plan for another batch size
    with pytest.raises(ValueError):
        color_reference(x.float(), p)
    with pytest.raises(ValueError):
        color_reference(torch.zeros(2, 4, 8, 8, dtype=torch.uint8), p)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def test_sampler_is_deterministic_and_in_range():
    s = ColorAugment(generator=_gen(3))
    a, b = s.sample(512), ColorAugment(generator=_gen(3)).sample(512)
    assert torch.equal(a.rows, b.rows) and not torch.equal(a.rows, s.sample(512).rows)
    assert sorted(a.op.unique().tolist()) == [1, 2, 3] and sorted(a.order.unique().tolist()) == [0, 1, 2, 3, 4, 5]
    lo, hi = torch.tensor(0.7).float(), torch.tensor(1.3).float()
    assert bool(((a.factors >= lo) & (a.factors <= hi)).all()) and float(a.factors.std()) > 0.1
    assert bool(((a.sigma >= 0.1) & (a.sigma <= 2.0)).all()) and float(a.sigma.max()) > 1.5 and float(a.sigma.min()) < 0.5
    counts = torch.bincount(a.op.long(), minlength=4)[1:]
    assert int(counts.min()) > 512 // 3 - 60  # uniform over the three ops
    wide = ColorAugment(jitter=(1.5, 0.4, 0.0), generator=_gen(4)).sample(256).factors
    assert float(wide[:, 0].min()) >= 0.0 and float(wide[:, 0].max()) <= 2.5 and bool((wide[:, 2] == 1).all())
    assert float(wide[:, 1].min()) >= torch.tensor(0.6).float() and float(wide[:, 1].max()) <= torch.tensor(1.4).float()


def test_sampler_draw_count_does_not_depend_on_the_decisions():
    after = []
    for kw in (dict(), dict(prob=0.0), dict(prob=0.5), dict(three_augment=False), dict(jitter=None), dict(jitter=0.4, sigma=(0.5, 0.5))):
        g = _gen(9)
        ColorAugment(generator=g, **kw).sample(33)
        after.append(torch.rand(4, generator=g, dtype=torch.float64))
    assert all(torch.equal(after[0], t) for t in after[1:])


def test_sampler_switches():
    p = ColorAugment(prob=0.0, generator=_gen(1)).sample(64)
    assert bool((p.op == 0).all()) and not bool((p.factors == 1).all())
    p = ColorAugment(three_augment=False, generator=_gen(1)).sample(64)
    assert bool((p.op == 0).all())
    p = ColorAugment(jitter=None, generator=_gen(1)).sample(64)
    assert bool((p.factors == 1).all()) and bool((p.op > 0).all())
    half = ColorAugment(prob=0.5, generator=_gen(2)).sample(400)
    assert 140 < int((half.op == 0).sum()) < 260
    for bad in (dict(prob=1.5), dict(sigma=(0.0, 1.0)), dict(sigma=(0.1, 2.5)), dict(sigma=(1.0, 0.5)), dict(jitter=-0.1),
                dict(jitter=(0.1, 0.2))):
        with pytest.raises(ValueError):
            ColorAugment(**bad)


def test_cpu_model_applies_a_plan_and_draws_in_training_only():
    from pytorch_vit_paper_replication_amd.models.vit_no_classifier import ViT as Backbone

    x, plan = O.blur_case(4, 32, 32, 1)
    for cls, cfg in ((ViT, TINY), (Backbone, {k: v for k, v in TINY.items() if k != "num_classes"})):
        torch.manual_seed(0)
        m = cls(**cfg).eval().set_device_input(DeviceInput())
        with torch.no_grad():
            assert torch.equal(m(x, color=plan), m(color_reference(x, plan)))
            assert not torch.equal(m(x, color=plan), m(x))
            plain = m(x)
            m.set_device_input(DeviceInput(color=ColorAugment(generator=_gen(5))))
            assert torch.equal(m(x), plain)  # evaluation never draws
            m.train()
            a, b = m(x), m(x)
            assert not torch.equal(a, b)
            m.set_device_input(DeviceInput(color=ColorAugment(generator=_gen(5))))
            assert torch.equal(m(x), a)  # the same seed reproduces the draw
            m.set_device_input(DeviceInput())
        with pytest.raises(ValueError):
            m(x.float() / 255, color=plan)
        with pytest.raises(ValueError):
            m.set_device_input(None)(x, color=plan)
        with pytest.raises(ValueError):
            m.set_device_input(DeviceInput())(x, color=ColorPlan.none(3))


def test_cli_flags_reach_the_model(tmp_path, monkeypatch):
    from pytorch_vit_paper_replication_amd import engine
    from pytorch_vit_paper_replication_amd.cli import train as T

    a = T.build_parser().parse_args([])
    assert a.three_augment is False and a.color_jitter == 0 and T.build_color_augment(a) is None
    a = T.build_parser().parse_args(["--three-augment", "--color-jitter", "0.3", "--seed", "3"])
    s, s2 = T.build_color_augment(a, 0), T.build_color_augment(a, 0)
    assert isinstance(s, ColorAugment) and s.three_augment and s.jitter == (0.3, 0.3, 0.3)
    assert torch.equal(s.sample(8).rows, s2.sample(8).rows)
    assert not torch.equal(T.build_color_augment(a, 0).sample(8).rows, T.build_color_augment(a, 1).sample(8).rows)  # per rank
    j = T.build_color_augment(T.build_parser().parse_args(["--color-jitter", "0.4"]))
    assert j.three_augment is False and j.jitter == (0.4, 0.4, 0.4)
    assert T.build_color_augment(T.build_parser().parse_args(["--three-augment"])).jitter is None

    seen = {}
    orig = engine.train

    def spy(**kw):
        seen["spec"] = kw["model"]._device_input_spec
        return orig(**kw)

    monkeypatch.setattr(engine, "train", spy)
    common = ["--model", "vit_tiny_test", "--synthetic", "--epochs", "1", "--batch-size", "4", "--image-size", "32",
              "--num-classes", "3", "--synthetic-train-len", "8", "--synthetic-test-len", "4", "--save-dir", str(tmp_path)]
    # the CPU reference path trains one epoch on synthetic uint8 data
    rc = T.main(common + ["--device-preprocess", "--three-augment", "--color-jitter", "0.3"])
    assert rc == 0 and isinstance(seen["spec"].color, ColorAugment) and seen["spec"].color.three_augment
    seen.clear()
    assert T.main(common + ["--device-preprocess"]) == 0 and seen["spec"].color is None
    for flags in (["--three-augment"], ["--color-jitter", "0.3"]):
        with pytest.raises(SystemExit, match="--device-preprocess"):
            T.main(common + flags)
    with pytest.raises(SystemExit):
        T.main(common + ["--device-preprocess", "--color-jitter", "-0.5"])
