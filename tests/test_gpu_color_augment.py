"""Colour augmentation on the GPU (csrc/color.hip through ``ops.fused_vit.color_u8``).

Every comparison is byte equality: the arithmetic is integer, or fp32 with every operation rounded once. The
yardsticks are PIL for the pointwise ops and the jitter, and ``color_reference`` (checked against PIL and an
independent numpy blur in test_color_augment_cpu.py) for everything, blur included.

Shapes: 3x37x45 has an odd width (per-element path), 3x32x64 takes the 8-byte path when contiguous and the
per-element path as channels_last, 3x70x150 has 3 x 3 blur tiles with partial ones on both edges, and 3x5x7 is
smaller than the blur's halo."""
import pytest
import torch

from tests import color_oracle as O
from tests.test_gpu_batch_mix import CFG, IMAGENET, _images, _model_plan, _same
from tests.test_gpu_random_erasing import _counter, _model_erase, _step

pytestmark = pytest.mark.gpu

DEV = "cuda"
POINT_SHAPES = [(37, 45), (32, 64)]
BLUR_SHAPES = POINT_SHAPES + [(70, 150), (5, 7)]


def _color_u8(x, plan):
    from pytorch_vit_paper_replication_amd.ops.fused_vit import color_u8

    return color_u8(x, plan)


def _layouts(x):
    """(name, the batch on the GPU) contiguous and channels_last."""
    xg = x.to(DEV)
    return [("nchw", xg), ("channels_last", xg.contiguous(memory_format=torch.channels_last))]


def _run(x, plan):
    """The kernels' output for both layouts, checked for layout and purity; returns the bytes on the host."""
    outs = []
    for name, xg in _layouts(x):
        keep = xg.clone()
        out = _color_u8(xg, plan)
        torch.cuda.synchronize()
        assert out.dtype == torch.uint8 and out.shape == xg.shape and out.stride() == xg.stride(), name
        assert out.data_ptr() != xg.data_ptr() and torch.equal(xg, keep), f"{name}: the input was modified"
        outs.append(out.cpu())
    assert torch.equal(outs[0], outs[1]), "contiguous and channels_last disagree"
    return outs[0]


@pytest.mark.parametrize("shape", POINT_SHAPES)
@pytest.mark.parametrize("seed", [0, 1])
def test_kernels_equal_pil_on_pointwise_ops_and_jitter(shape, seed):
    x, plan = O.pointwise_case(7, *shape, seed)
    got = _run(x, plan)
    assert int((got != O.pil_chain(x, plan)).sum()) == 0


@pytest.mark.parametrize("shape", BLUR_SHAPES)
@pytest.mark.parametrize("seed", [0, 1])
def test_kernels_equal_the_reference_blur_included(shape, seed):
    from pytorch_vit_paper_replication_amd.data import color_reference

    x, plan = O.blur_case(7, *shape, seed)
    assert sorted(set(plan.sigma[plan.op == 3].tolist())) == pytest.approx([0.1, 0.5, 1.0, 2.0])
    assert plan.op[4] == 3 and plan.factors[4, 1] != 1  # blur, then contrast: the sum reads the blurred bytes
    got = _run(x, plan)
    want = color_reference(x, plan)
    assert int((got != want).sum()) == 0
    # the reference as torch ops on the device gives the same bytes (the benchmark's arm, PVR_DISABLE_FUSED's path)
    assert torch.equal(color_reference(x.to(DEV), plan).cpu(), want)


@pytest.mark.parametrize("shape", POINT_SHAPES)
def test_products_are_rounded_before_they_are_added(shape):
    """Factors whose fp32 value lies above the decimal (1.1, 0.9, 1.7) on pixels a multiple of 10 below the mean: a
    product fused into the add lands just below the integer PIL reaches (m = 56, v = 6: 56 - 55.0000012 against 1)."""
    from pytorch_vit_paper_replication_amd.data import ColorPlan

    x = O.images(7, *shape, 6)
    fac = torch.tensor([[1.0, 1.1, 1.0], [1.1, 0.9, 1.1], [1.0, 1.7, 1.0], [0.9, 1.1, 1.7], [1.7, 1.1, 0.9], [1.0, 0.9, 1.0], [1.0, 1.9, 1.1]])
    for op in (0, 2):
        plan = ColorPlan([op] * 7, None, fac, [0, 1, 2, 3, 4, 5, 0])
        assert int((_run(x, plan) != O.pil_chain(x, plan)).sum()) == 0


def test_vector_path_on_an_offset_view_and_a_large_batch():
    """A view whose base is not 8-byte aligned takes the per-element path; 40 samples of 3x64x72 are more than one
    workgroup per sample and more blur workgroups than one wave of them."""
    from pytorch_vit_paper_replication_amd.data import ColorAugment, color_reference

    plan = ColorAugment(generator=torch.Generator().manual_seed(2)).sample(40)
    x = O.images(40, 64, 72, 4)
    assert torch.equal(_run(x, plan), color_reference(x, plan))
    wide = torch.zeros(40, 3, 64, 76, dtype=torch.uint8, device=DEV)
    view = wide[:, :, :, 4:]
    view.copy_(x)
    out = _color_u8(view, plan)
    assert out.is_contiguous() and torch.equal(out.cpu(), color_reference(x, plan)) and torch.equal(view.cpu(), x)
    assert int(wide[:, :, :, :4].sum()) == 0


def test_contrast_mean_rounding():
    from pytorch_vit_paper_replication_amd.data import ColorPlan

    # half the pixels at L = 10 and half at L = 11: m = 11; factor 0 returns m everywhere
    x = torch.full((3, 3, 40, 64), 10, dtype=torch.uint8)
    x[0, :, :, 32:] = 11
    x[1], x[2] = 255, 0
    plan = ColorPlan([0, 0, 0], None, [[1.0, 0.0, 1.0]] * 3, [0, 3, 5])
    out = _run(x, plan)
    assert out[0].unique().tolist() == [11] and out[1].unique().tolist() == [255] and out[2].unique().tolist() == [0]


@pytest.mark.parametrize("shape", POINT_SHAPES)
def test_identity_plan_returns_the_input_bytes(shape):
    from pytorch_vit_paper_replication_amd.data import ColorPlan

    x = O.images(7, *shape, 3)
    assert torch.equal(_run(x, ColorPlan.none(7)), x)
    # ... and per sample beside samples that are changed
    op, fac = torch.tensor([0, 1, 0, 2, 0, 3, 0]), torch.ones(7, 3)
    fac[1] = torch.tensor([0.5, 1.5, 0.2])
    out = _run(x, ColorPlan(op, None, fac, None))
    assert torch.equal(out[0::2], x[0::2]) and all(not torch.equal(out[b], x[b]) for b in (1, 3, 5))


def test_host_checks_refuse_before_any_launch():
    from pytorch_vit_paper_replication_amd import _ext as E
    from pytorch_vit_paper_replication_amd.data import ColorPlan

    ext = E.ext()
    x = O.images(2, 16, 16, 0).to(DEV)
    good = ColorPlan([1, 3], [1.0, 1.0], [[0.5, 1.5, 1.0]] * 2, [0, 5])
    assert torch.equal(ext.color_u8(x, good.on(DEV), good.rows), ext.color_u8(x, good.on(DEV)))  # host copy optional

    def refused(rows, img=x):
        rows = rows.contiguous()
        for kw in (dict(plan_host=rows), dict()):  # with the host copy and with the read-back
            with pytest.raises(RuntimeError, match="color_u8"):
                ext.color_u8(img, rows.to(DEV), **kw)

    def edit(col, val, row=1, as_int=False):
        rows = good.rows.clone()
        (rows.view(torch.int32) if as_int else rows)[row, col] = val
        return rows

    refused(edit(0, 4, as_int=True))  # op
    refused(edit(0, -1, as_int=True))
    refused(edit(1, 6, as_int=True))  # order
    refused(edit(1, -1, as_int=True))
    for col in (2, 3, 4):  # factors
        for bad in (-0.25, float("nan"), float("inf")):
            refused(edit(col, bad, row=0))
    refused(edit(5, 0.0))  # sigma of the blur row
    refused(edit(5, 2.5))
    refused(edit(5, float("nan")))
    refused(edit(6 + 6, 0.9))  # weights that do not sum to 1
    refused(edit(6 + 2, float("nan")))
    refused(good.rows, torch.zeros(2, 4, 16, 16, dtype=torch.uint8, device=DEV))  # C = 4
    refused(good.rows, torch.zeros(2, 1, 16, 16, dtype=torch.uint8, device=DEV))
    refused(good.rows, x.float())  # float input
    refused(good.rows, x[:1])  # a plan for another batch size
    refused(good.rows[:, :19])
    with pytest.raises(RuntimeError, match="color_u8"):
        ext.color_u8(x, good.rows)  # the table on the host
    with pytest.raises(RuntimeError, match="color_u8"):
        ext.color_u8(x.cpu(), good.on(DEV), good.rows)
    with pytest.raises(RuntimeError, match="color_u8"):
        ext.color_u8(x, good.on(DEV), good.rows.to(DEV))
    with pytest.raises(ValueError):
        _color_u8(x, ColorPlan.none(3))
    for bad in (dict(op=[0, 4]), dict(order=[0, 6]), dict(factors=[[1.0, -1.0, 1.0]] * 2), dict(op=[0, 3], sigma=[1.0, 2.5]),
                dict(op=[0, 3], sigma=[1.0, 0.0])):
        with pytest.raises(ValueError):
            ColorPlan(**{**dict(op=[0, 0], sigma=None, factors=None, order=None), **bad})
    torch.cuda.synchronize()


def _model_color(B=4):
    from pytorch_vit_paper_replication_amd.data import ColorPlan

    return ColorPlan([3, 1, 0, 2], [1.3, 1.0, 1.0, 1.0], [[0.8, 1.3, 0.7], [1.2, 0.75, 1.0], [1.0, 1.0, 1.0], [0.9, 1.1, 1.25]],
                     [2, 5, 0, 1])


def test_model_with_a_color_plan_bitwise_equal_to_the_model_on_the_reference_batch():
    """The tiny ViT of the other feature tests, patch dropout on, crop boxes, an erase plan and a mix plan:
    logits, loss and every gradient with color= are those of the same step on color_reference's batch."""
    from pytorch_vit_paper_replication_amd import _ext as E
    from pytorch_vit_paper_replication_amd.data import DeviceInput, color_reference
    from pytorch_vit_paper_replication_amd.models.vit_no_classifier import ViT as Backbone

    V = 2718
    mplan, eplan, cplan = _model_plan(), _model_erase("pixel"), _model_color()
    y = torch.randint(0, 10, (4,), generator=torch.Generator().manual_seed(0)).to(DEV)
    xu = _images(4, 80, 96, seed=7)
    geom = torch.tensor([[16.0, 8.0, 80.0, 72.0], [80.0, 8.0, 16.0, 72.0], [0.0, 0.0, 64.0, 64.0], [32.0, 16.0, 96.0, 80.0]]).to(DEV)
    ref = color_reference(xu, cplan).to(DEV)
    xg = xu.to(DEV)
    assert not torch.equal(ref, xg)

    def prep(m):
        return _counter(m.set_patch_dropout(0.5).set_device_input(DeviceInput(*IMAGENET)), V)

    kw = dict(geom=geom, erase=eplan, mix=mplan)
    bcfg = {k: v for k, v in CFG.items() if k != "num_classes"}
    with E.deterministic_mode():
        a = _step(lambda m: prep(m)(xg, color=cplan, **kw), y, mplan)
        b = _step(lambda m: prep(m)(ref, **kw), y, mplan)
        plain = _step(lambda m: prep(m)(xg, **kw), y, mplan)
        k = _step(lambda m: prep(m)(xg, color=cplan, **kw), y, mplan, Backbone, bcfg)
        kh = _step(lambda m: prep(m)(ref, **kw), y, mplan, Backbone, bcfg)
        # no crop, channels_last: the stage's output feeds the patchify kernel's own layout handling
        x64 = _images(4, 64, 64, seed=8)
        c = _step(lambda m: prep(m)(x64.to(DEV).contiguous(memory_format=torch.channels_last), color=cplan), y, None)
        d = _step(lambda m: prep(m)(color_reference(x64, cplan).to(DEV)), y, None)
    _same(a, b)
    _same(k, kh)
    _same(c, d)
    assert not torch.equal(a[0], plain[0])


def test_model_color_argument_needs_a_uint8_batch_and_a_spec():
    from pytorch_vit_paper_replication_amd.data import DeviceInput
    from pytorch_vit_paper_replication_amd.models import ViT

    torch.manual_seed(0)
    m = ViT(**CFG).to(DEV).eval()
    xu = _images(4, 64, 64, seed=1).to(DEV)
    with torch.no_grad():
        with pytest.raises(ValueError, match="set_device_input"):
            m(xu, color=_model_color())  # no spec
        m.set_device_input(DeviceInput())
        with pytest.raises(ValueError, match="uint8"):
            m(xu.float() / 255, color=_model_color())
        with pytest.raises(ValueError):
            m(xu[:2], color=_model_color())
        assert m(xu, color=_model_color()).shape == (4, 10)


def test_model_draws_from_the_sampler_in_training_only():
    from pytorch_vit_paper_replication_amd.data import ColorAugment, DeviceInput, color_reference
    from pytorch_vit_paper_replication_amd.models import ViT

    torch.manual_seed(0)
    m = ViT(**CFG).to(DEV)  # CFG has no dropout: training forwards differ by the draw alone
    xu = _images(4, 64, 64, seed=2).to(DEV)

    def sampler(seed=5):
        return DeviceInput(color=ColorAugment(generator=torch.Generator().manual_seed(seed)))

    with torch.no_grad():
        m.eval().set_device_input(DeviceInput())
        plain = m(xu)
        m.set_device_input(sampler())
        assert torch.equal(m(xu), plain)  # evaluation never draws
        m.train()
        a, b = m(xu), m(xu)
        assert not torch.equal(a, b) and not torch.equal(a, plain)
        m.set_device_input(sampler())
        assert torch.equal(m(xu), a)  # the same seed reproduces the draw
        first = ColorAugment(generator=torch.Generator().manual_seed(5)).sample(4)
        m.set_device_input(DeviceInput())
        assert torch.equal(m(xu, color=first), a) and torch.equal(m(color_reference(xu, first)), a)


def test_sampler_refuses_a_capture_and_an_explicit_plan_replays_to_the_eager_bytes():
    from pytorch_vit_paper_replication_amd.data import ColorAugment, DeviceInput
    from pytorch_vit_paper_replication_amd.models import ViT

    torch.manual_seed(0)
    m = ViT(**CFG).to(DEV).train().set_device_input(DeviceInput(color=ColorAugment(generator=torch.Generator().manual_seed(1))))
    cplan = _model_color()
    batches = [_images(4, 64, 64, seed=3).to(DEV), _images(4, 64, 64, seed=4).to(DEV)]
    eager = [_color_u8(b, cplan).clone() for b in batches]  # also uploads the table before the capture
    buf = batches[0].clone()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        with pytest.raises(RuntimeError, match="graph capture"):
            m(buf)  # the sampler would draw on the host: refused before any launch
        out = _color_u8(buf, cplan)
    torch.cuda.synchronize()
    for i in (0, 1, 0):
        buf.copy_(batches[i])
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager[i]) and torch.equal(buf, batches[i])


class _WithColor(torch.nn.Module):
    def __init__(self, inner, cplan):
        super().__init__()
        self.inner, self.cplan = inner, cplan

    def forward(self, x):
        return self.inner(x, color=self.cplan)


def test_explicit_plan_under_a_graphed_train_step():
    """The learning rate is 0, so the weights stay and the loss of a replay is the eager loss on color_reference's
    batch. The two run the same kernels on the same bytes; the limit of 1e-3 is the one the graphed random-erasing
    test allows between a replay and an eager step."""
    import math

    from pytorch_vit_paper_replication_amd.data import DeviceInput, color_reference
    from pytorch_vit_paper_replication_amd.models import ViT
    from pytorch_vit_paper_replication_amd.ops.fused_vit import cross_entropy
    from pytorch_vit_paper_replication_amd.optim import FusedAdam
    from pytorch_vit_paper_replication_amd.runtime.graph import GraphedTrainStep

    torch.manual_seed(0)
    m = ViT(**CFG).to(DEV).set_device_input(DeviceInput(*IMAGENET))
    opt = FusedAdam(m.parameters(), lr=0.0)
    cplan = _model_color()
    xs = [_images(4, 64, 64, seed=5), _images(4, 64, 64, seed=6)]
    y = torch.randint(0, 10, (4,), generator=torch.Generator().manual_seed(9)).to(DEV)
    g = GraphedTrainStep(_WithColor(m, cplan), opt, cross_entropy, xs[0].to(DEV), y, clip_norm=1.0, warmup=2)
    for x in xs:
        loss = float(g(x.to(DEV), y))
        torch.cuda.synchronize()
        want = float(cross_entropy(m(color_reference(x, cplan).to(DEV)), y).detach())
        plain = float(cross_entropy(m(x.to(DEV)), y).detach())
        print(f"replay loss {loss}, eager loss on the reference batch {want}, without the plan {plain}")
        assert math.isfinite(loss) and abs(loss - want) <= 1e-3 and want != plain
