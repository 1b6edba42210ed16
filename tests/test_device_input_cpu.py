"""uint8 input with device-side preprocessing (ViT.set_device_input), the parts that run without a GPU:
the fp32 torch preprocessing the model uses off the fused path (it is also the reference of
tests/test_gpu_device_input.py), the crop-box sampler, input dispatch and the CLI flags."""
import math

import pytest
import torch

from pytorch_vit_paper_replication_amd.data import DeviceInput, RandomResizedCropFlip, center_box, full_box
from pytorch_vit_paper_replication_amd.data.device_input import preprocess_reference
from pytorch_vit_paper_replication_amd.data.transforms import (IMAGENET_MEAN, IMAGENET_STD, Normalize, ToDtype,
                                                               uint8_transform)
from pytorch_vit_paper_replication_amd.models import ViT
from pytorch_vit_paper_replication_amd.models.vit_no_classifier import ViT as ViTNoClassifier

CFG = dict(image_size=32, patch_size=8, num_transformer_layer=2, num_heads=2, embedding_dim=64, mlp_size=128,
           num_classes=5, mlp_dropout=0.0, embedding_dropout=0.0)


def _images(b, h, w, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(0, 256, (b, 3, h, w), generator=g, dtype=torch.uint8)
    x[0, 0, 0, 0], x[0, 1, 0, 1] = 0, 255  # both ends of the range are present
    return x


def _host_pipeline(x, mean, std):
    """What the float pipeline does to a uint8 image on the CPU today."""
    f = ToDtype(torch.float32, scale=True)(x)
    return f if mean is None else Normalize(mean, std)(f)


@pytest.fixture(scope="module")
def model():
    torch.manual_seed(0)
    return ViT(**CFG).eval()


@pytest.mark.parametrize("mean,std", [(None, None), (IMAGENET_MEAN, IMAGENET_STD)])
def test_identity_matches_host_transforms_exactly(model, mean, std):
    x = _images(3, 32, 32)
    ref = _host_pipeline(x, mean, std)
    assert torch.equal(preprocess_reference(x, mean, std), ref)
    model.set_device_input(DeviceInput(mean=mean, std=std))
    try:
        with torch.no_grad():
            assert torch.equal(model(x), model(ref))
    finally:
        model.set_device_input(None)


def test_integer_crop_and_flip_is_a_slice(model):
    x = _images(2, 40, 48, seed=1)
    geom = torch.tensor([[48.0, 4.0, 16.0, 36.0]]).repeat(2, 1)  # x 16..48 right to left, y 4..36
    want = _host_pipeline(x[:, :, 4:36, 16:48].flip(-1), IMAGENET_MEAN, IMAGENET_STD)
    got = preprocess_reference(x, IMAGENET_MEAN, IMAGENET_STD, geom, (32, 32))
    assert torch.equal(got, want)
    model.set_device_input(DeviceInput(IMAGENET_MEAN, IMAGENET_STD))
    try:
        with torch.no_grad():
            assert torch.equal(model(x, geom=geom), model(want))
    finally:
        model.set_device_input(None)


def test_resize_convention_and_float64_agreement():
    # whole 64x64 source -> 32x32: every output pixel is the mean of a 2x2 block's inner corners, i.e.
    # the sample point (2*o + 0.5) lies halfway between source pixels 2*o and 2*o + 1
    x = _images(1, 64, 64, seed=2)
    got = preprocess_reference(x, geom=full_box(1, 64, 64), size=(32, 32)) * 255.0
    f = x.float()
    want = (f[:, :, 0::2, 0::2] + f[:, :, 0::2, 1::2] + f[:, :, 1::2, 0::2] + f[:, :, 1::2, 1::2]) / 4.0
    assert torch.allclose(got, want, atol=1e-4)
    # random boxes: fp32 against the same formulas in fp64
    g = torch.Generator().manual_seed(3)
    boxes = RandomResizedCropFlip(generator=g).sample(16, 64, 64)
    xs = x.expand(16, -1, -1, -1)
    a = preprocess_reference(xs, IMAGENET_MEAN, IMAGENET_STD, boxes, (32, 32))
    b = preprocess_reference(xs, IMAGENET_MEAN, IMAGENET_STD, boxes, (32, 32), dtype=torch.float64)
    assert (a.double() - b).abs().max().item() < 5e-4


def test_boxes_helpers():
    assert full_box(2, 40, 48).tolist() == [[0.0, 0.0, 48.0, 40.0]] * 2
    assert center_box(1, 40, 48, 32).tolist() == [[8.0, 4.0, 40.0, 36.0]]
    assert center_box(1, 40, 48, 20, 30).tolist() == [[9.0, 10.0, 39.0, 30.0]]
    with pytest.raises(ValueError):
        center_box(1, 40, 48, 41)


@pytest.mark.parametrize("scale,ratio", [((0.08, 1.0), (3 / 4, 4 / 3)), ((0.3, 0.6), (0.5, 2.0))])
def test_sampler_boxes(scale, ratio):
    Hs, Ws, n = 40, 48, 4096
    aug = RandomResizedCropFlip(scale=scale, ratio=ratio, generator=torch.Generator().manual_seed(7))
    box = aug.sample(n, Hs, Ws)
    assert box.shape == (n, 4) and box.dtype == torch.float32
    x0, y0, x1, y1 = box.double().unbind(1)
    flipped = x0 > x1
    lo, hi = torch.minimum(x0, x1), torch.maximum(x0, x1)
    assert (lo >= 0).all() and (hi <= Ws).all() and (y0 >= 0).all() and (y1 <= Hs).all() and (y1 > y0).all()
    w, h = hi - lo, y1 - y0
    eps = 1e-4  # boxes are stored as float32
    area = w * h / (Hs * Ws)
    assert (area >= scale[0] * (1 - eps)).all() and (area <= scale[1] * (1 + eps)).all()
    assert (w / h >= ratio[0] * (1 - eps)).all() and (w / h <= ratio[1] * (1 + eps)).all()
    assert abs(flipped.double().mean().item() - 0.5) <= 0.03
    again = RandomResizedCropFlip(scale=scale, ratio=ratio, generator=torch.Generator().manual_seed(7)).sample(n, Hs, Ws)
    assert torch.equal(box, again)
    other = RandomResizedCropFlip(scale=scale, ratio=ratio, generator=torch.Generator().manual_seed(8)).sample(n, Hs, Ws)
    assert not torch.equal(box, other)


def test_sampler_fallback_is_centred_and_inside_ratio():
    # a 10x100 source cannot hold any box of aspect <= 4/3 with >= 90 % of its area: every draw falls back
    aug = RandomResizedCropFlip(scale=(0.9, 1.0), flip=0.0, generator=torch.Generator().manual_seed(0))
    box = aug.sample(8, 10, 100)
    w = 10 * 4 / 3
    want = torch.tensor([(100 - w) / 2, 0.0, (100 - w) / 2 + w, 10.0], dtype=torch.float64).to(torch.float32)
    assert torch.equal(box, want.repeat(8, 1))


def test_float_input_ignores_the_spec(model):
    x = torch.rand(2, 3, 32, 32, generator=torch.Generator().manual_seed(4))
    with torch.no_grad():
        base = model(x)
        model.set_device_input(DeviceInput(IMAGENET_MEAN, IMAGENET_STD, RandomResizedCropFlip()))
        try:
            assert torch.equal(model(x), base)
            with pytest.raises(ValueError):
                model(x, geom=full_box(2, 32, 32))
        finally:
            model.set_device_input(None)


def test_uint8_input_without_spec_is_not_preprocessed(model):
    """No spec: a uint8 batch is handed on as it is, as before (the fused GPU path converts it with
    ``.float()``, tests/test_gpu_device_input.py; the CPU convolution refuses the dtype, as before)."""
    x = _images(2, 32, 32)
    same, pre = model._device_input(x, None)
    assert same is x and pre is None
    with torch.no_grad(), pytest.raises(RuntimeError):
        model(x)
    with pytest.raises(ValueError):
        model(x, geom=full_box(2, 32, 32))


def test_channels_last_equals_contiguous(model):
    x = _images(2, 40, 48, seed=5)
    xl = x.contiguous(memory_format=torch.channels_last)
    assert not xl.is_contiguous() and torch.equal(x, xl)
    geom = torch.tensor([[2.25, 1.5, 42.25, 33.5], [48.0, 4.0, 16.0, 36.0]])
    model.set_device_input(DeviceInput(IMAGENET_MEAN, IMAGENET_STD))
    try:
        with torch.no_grad():
            assert torch.equal(model(x, geom=geom), model(xl, geom=geom))
            assert torch.equal(model(x[:, :, :32, :32]), model(xl[:, :, :32, :32]))
    finally:
        model.set_device_input(None)


def test_geom_defaults(model):
    """eval / no augment: whole source (none when the sizes match); training + augment: the sampler's draws."""
    x = _images(2, 40, 48, seed=6)
    aug = RandomResizedCropFlip(generator=torch.Generator().manual_seed(11))
    model.set_device_input(DeviceInput(augment=aug))
    try:
        assert model._device_input(x[:, :, :32, :32], None)[1][2] is None
        assert torch.equal(model._device_input(x, None)[1][2], full_box(2, 40, 48))
        with torch.no_grad():
            assert torch.equal(model(x), model(x, geom=full_box(2, 40, 48)))
            model.train()
            drawn = model(x)
            want = RandomResizedCropFlip(generator=torch.Generator().manual_seed(11)).sample(2, 40, 48)
            assert torch.equal(drawn, model(x, geom=want))
            assert not torch.equal(drawn, model(x, geom=full_box(2, 40, 48)))
        with pytest.raises(ValueError):
            model(x, geom=torch.zeros(3, 4))
    finally:
        model.eval()
        model.set_device_input(None)


def test_backbone_without_classifier_takes_uint8():
    torch.manual_seed(0)
    cfg = {k: v for k, v in CFG.items() if k != "num_classes"}
    m = ViTNoClassifier(**cfg).eval().set_device_input(DeviceInput(IMAGENET_MEAN, IMAGENET_STD))
    x = _images(2, 40, 48, seed=7)
    geom = torch.tensor([[48.0, 4.0, 16.0, 36.0]]).repeat(2, 1)
    with torch.no_grad():
        want = m(_host_pipeline(x[:, :, 4:36, 16:48].flip(-1), IMAGENET_MEAN, IMAGENET_STD))
        assert torch.equal(m(x, geom=geom), want)


def test_uint8_transform_returns_uint8_chw():
    from PIL import Image

    img = Image.fromarray(_images(1, 50, 70)[0].permute(1, 2, 0).numpy())
    out = uint8_transform(32)(img)
    assert out.dtype == torch.uint8 and out.shape == (3, 32, 32)
    batch = torch.utils.data.default_collate([out, out])
    assert batch.dtype == torch.uint8 and batch.shape == (2, 3, 32, 32)


def test_cli_device_preprocess(tmp_path, monkeypatch):
    from pytorch_vit_paper_replication_amd.cli import train as T
    from pytorch_vit_paper_replication_amd.models import presets

    made, seen = [], []
    orig = presets.vit

    def spy(*a, **kw):
        m = orig(*a, **kw)
        made.append(m)
        m.register_forward_pre_hook(lambda mod, args: seen.append((args[0].dtype, tuple(args[0].shape[1:]), mod.training)))
        return m

    monkeypatch.setattr("pytorch_vit_paper_replication_amd.models.vit", spy)
    rc = T.main(["--synthetic", "--device-preprocess", "--augment", "rrc-flip", "--model", "vit_tiny_test", "--epochs", "1",
                 "--batch-size", "4", "--image-size", "32", "--source-size", "40", "--num-classes", "3",
                 "--synthetic-train-len", "8", "--synthetic-test-len", "4", "--save-dir", str(tmp_path)])
    assert rc == 0 and made
    spec = made[0]._device_input_spec
    assert isinstance(spec, DeviceInput) and isinstance(spec.augment, RandomResizedCropFlip) and spec.mean is None
    assert seen and all(d == torch.uint8 and s == (3, 40, 40) for d, s, _ in seen)
    assert any(t for _, _, t in seen) and any(not t for _, _, t in seen)
    a = T.build_parser().parse_args([])
    assert not a.device_preprocess and a.augment == "none" and a.source_size is None
    with pytest.raises(SystemExit):
        T.main(["--synthetic", "--augment", "rrc-flip", "--model", "vit_tiny_test"])
    assert math.isfinite(float(torch.load(tmp_path / "vit_tiny_test_1_epochs.pth", weights_only=True)
                               ["classifier.0.weight"].sum()))
