"""uint8 input on the GPU: the ``im2col_u8`` kernel (scale, normalise, crop / resize / flip fused into
the patch gather) against the CPU fp32 preprocessing (data.device_input.preprocess_reference), and
the models' uint8 entry against the equivalent float input.

Bit-exact cases: no geom, and crop boxes whose sample points and weights are exactly representable
(every intermediate up to the interpolated pixel value is then exact in fp32, so the only roundings
are the two divisions, the subtraction and the bf16 cast, which the CPU performs identically)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

IMAGENET = ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
CFG = dict(image_size=64, patch_size=16, num_transformer_layer=2, num_heads=2, embedding_dim=128, mlp_size=256,
           num_classes=10, mlp_dropout=0.0, embedding_dropout=0.0)


def _images(b, h, w, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(0, 256, (b, 3, h, w), generator=g, dtype=torch.uint8)
    x[:, 0, 0, 0], x[:, 1, 0, 1], x[:, 2, -1, -1], x[:, 0, -1, 0] = 0, 255, 0, 255
    return x


def _kp(P, C=3):
    return (C * P * P + 63) // 64 * 64


def _bits(t):
    return t.view(torch.int16)


def _float_patches(xf_cpu, P):
    """The existing float kernel on an already preprocessed CPU image: bf16 patch rows on the GPU."""
    from pytorch_vit_paper_replication_amd import _ext

    img = xf_cpu.float().cuda().contiguous()
    B, C, H, W = img.shape
    out = torch.full((B * (H // P) * (W // P), _kp(P, C)), float("nan"), dtype=torch.bfloat16, device="cuda")
    _ext.ext().im2col(img, out, P, _kp(P, C))
    return out


def _u8_patches(x_gpu, P, size, norm=IMAGENET, geom=None):
    from pytorch_vit_paper_replication_amd import _ext

    B, C = x_gpu.shape[:2]
    H, W = size
    out = torch.full((B * (H // P) * (W // P), _kp(P, C)), float("nan"), dtype=torch.bfloat16, device="cuda")
    mean, std = norm if norm is not None else ((0.0,) * C, (1.0,) * C)
    vec = _ext.ext().im2col_u8(x_gpu, out, list(mean), list(std), None if geom is None else geom.cuda(), H, W, P, _kp(P, C))
    return out, vec


def _layouts(x_cpu):
    xc = x_cpu.cuda()
    return {"contiguous": xc, "channels_last": xc.contiguous(memory_format=torch.channels_last)}


@pytest.mark.parametrize("norm", [None, IMAGENET], ids=["scale_only", "imagenet"])
@pytest.mark.parametrize("B,P,S,vec_expected", [(3, 16, 32, 1), (2, 14, 28, 0), (2, 4, 16, 0)])
def test_kernel_no_geom_bit_identical(B, P, S, vec_expected, norm):
    from pytorch_vit_paper_replication_amd.data.device_input import preprocess_reference

    x = _images(B, S, S, seed=P)
    assert x.min() == 0 and x.max() == 255
    want = _float_patches(preprocess_reference(x, *(norm or (None, None))), P)
    kc = 3 * P * P
    assert not want[:, kc:].any() and not torch.isnan(want.float()).any()
    for name, xg in _layouts(x).items():
        got, vec = _u8_patches(xg, P, (S, S), norm)
        assert vec == (vec_expected if name == "contiguous" else 0), name
        assert torch.equal(_bits(got), _bits(want)), name
        assert not got[:, kc:].any(), name  # the padding columns are written, and zero


def test_kernel_misaligned_base_takes_the_element_path():
    from pytorch_vit_paper_replication_amd.data.device_input import preprocess_reference

    x = _images(3, 32, 32, seed=1)
    want = _float_patches(preprocess_reference(x, *IMAGENET), 16)
    buf = torch.zeros(x.numel() + 16, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 8 == 0
    view = buf[1:1 + x.numel()].view(x.shape)
    view.copy_(x)
    assert view.data_ptr() % 8 == 1 and view.is_contiguous()
    got, vec = _u8_patches(view, 16, (32, 32))
    assert vec == 0 and torch.equal(_bits(got), _bits(want))
    # a row stride that is no multiple of 8 (a 32-wide window of a 36-wide image) does too
    wide = torch.zeros(3, 3, 32, 36, dtype=torch.uint8, device="cuda")
    wide[..., :32] = x.cuda()
    got, vec = _u8_patches(wide[..., :32], 16, (32, 32))
    assert vec == 0 and torch.equal(_bits(got), _bits(want))


def test_kernel_grid_stride_at_benchmark_size():
    """256 x 224 x 224, P = 16: 4.8 M threads' worth of work on the capped grid (16384 blocks)."""
    from pytorch_vit_paper_replication_amd.data.device_input import preprocess_reference

    x = _images(256, 224, 224, seed=2)
    want = _float_patches(preprocess_reference(x, *IMAGENET), 16)
    got, vec = _u8_patches(x.cuda(), 16, (224, 224))
    assert vec == 1 and torch.equal(_bits(got), _bits(want))


EXACT_CASES = {
    # source 40 x 48 -> 32 x 32, P = 16: identity window, integer crop + flip, a 1.25x box at quarter-pixel
    # offsets, and a 0.5x / 1.25x (2.5x vertical squeeze relative to x) box that touches the top and bottom edges
    "p16": (40, 48, 32, 16, [(0, 0, 32, 32), (48, 4, 16, 36), (2.25, 1.5, 42.25, 33.5), (8, 0, 24, 40)]),
    # source 35 x 42 -> 28 x 28, P = 14: box widths 28 * {1, 1.25, 0.75, -1}
    "p14": (35, 42, 28, 14, [(3, 2, 31, 30), (1.5, 0, 36.5, 35), (10.25, 4.5, 31.25, 25.5), (40, 5, 12, 33)]),
}


@pytest.mark.parametrize("case", sorted(EXACT_CASES))
def test_kernel_geom_exact_boxes_bit_identical(case):
    from pytorch_vit_paper_replication_amd.data.device_input import preprocess_reference

    Hs, Ws, S, P, boxes = EXACT_CASES[case]
    geom = torch.tensor(boxes, dtype=torch.float32)
    x = _images(len(boxes), Hs, Ws, seed=3)
    ref = preprocess_reference(x, *IMAGENET, geom, (S, S))
    ref64 = preprocess_reference(x, *IMAGENET, geom, (S, S), dtype=torch.float64)
    # the premise: at these boxes the fp32 reference carries only the roundings of its last three operations
    # (two divisions and a subtraction, each <= 0.5 ulp, the first amplified by 1 / std <= 4.5)
    assert (ref.double() - ref64).abs().max().item() < 2e-6
    want = _float_patches(ref, P)
    for name, xg in _layouts(x).items():
        got, vec = _u8_patches(xg, P, (S, S), geom=geom)
        assert vec == 0
        assert torch.equal(_bits(got), _bits(want)), name


def _patchify(t, P):
    B, C, H, W = t.shape
    return t.reshape(B, C, H // P, P, W // P, P).permute(0, 2, 4, 1, 3, 5).reshape(B * (H // P) * (W // P), C * P * P)


def test_kernel_random_boxes_against_float64():
    """64 boxes anywhere inside a 40 x 48 source (x endpoints unordered: about half are flipped).
    |got - ref| <= 2^-8 |ref| + 5e-4: bf16 rounding, plus the fp32 coordinate error (<= ~3e-5 px at these
    sizes) times the largest slope of the normalised image per pixel, 2 * 255 / 255 / 0.2."""
    from pytorch_vit_paper_replication_amd.data.device_input import preprocess_reference

    Hs, Ws, S, P, n = 40, 48, 32, 16, 64
    g = torch.Generator().manual_seed(5)
    xs = torch.rand(n, 2, generator=g) * Ws
    ys = (torch.rand(n, 2, generator=g) * Hs).sort(dim=1).values
    geom = torch.stack([xs[:, 0], ys[:, 0], xs[:, 1], ys[:, 1]], dim=1)
    flips = int((geom[:, 0] > geom[:, 2]).sum())
    assert 16 <= flips <= 48
    x = _images(n, Hs, Ws, seed=6)
    ref = _patchify(preprocess_reference(x, *IMAGENET, geom, (S, S), dtype=torch.float64), P)
    got, _ = _u8_patches(x.cuda(), P, (S, S), geom=geom)
    got = got.cpu().double()
    err = (got - ref).abs()
    bound = ref.abs() * 2.0 ** -8 + 5e-4
    worst = (err - bound).max().item()
    print(f"random boxes: max |err| {err.max().item():.3e}, max (err - bound) {worst:.3e}, mean |err| {err.mean().item():.3e}")
    assert worst <= 0.0


def test_binding_validates_its_arguments():
    from pytorch_vit_paper_replication_amd import _ext

    ext = _ext.ext()
    x = _images(2, 32, 32).cuda()
    out = torch.empty(2 * 4, 768, dtype=torch.bfloat16, device="cuda")
    m, s = [0.0] * 3, [1.0] * 3
    g = torch.tensor([[0.0, 0.0, 32.0, 32.0]] * 2, device="cuda")
    ext.im2col_u8(x, out, m, s, g, 32, 32, 16, 768)  # the valid call
    bad = [
        lambda: ext.im2col_u8(x.float(), out, m, s, None, 32, 32, 16, 768),                         # dtype
        lambda: ext.im2col_u8(x[0], out, m, s, None, 32, 32, 16, 768),                              # dims
        lambda: ext.im2col_u8(torch.zeros(2, 5, 32, 32, dtype=torch.uint8, device="cuda"), out, [0.0] * 5, [1.0] * 5,
                              None, 32, 32, 16, 1280),                                              # C > 4
        lambda: ext.im2col_u8(x, out, m, s, None, 32, 32, 12, 768),                                 # H % P
        lambda: ext.im2col_u8(x, out, m, s, None, 16, 16, 16, 768),                                 # resize without geom
        lambda: ext.im2col_u8(x, out, m, s, g[:1], 32, 32, 16, 768),                                # geom shape
        lambda: ext.im2col_u8(x, out, m, s, g.double(), 32, 32, 16, 768),                           # geom dtype
        lambda: ext.im2col_u8(x, out, m, s, g.cpu(), 32, 32, 16, 768),                              # geom device
        lambda: ext.im2col_u8(x, out[:4], m, s, None, 32, 32, 16, 768),                             # out rows
        lambda: ext.im2col_u8(x, out, m[:2], s, None, 32, 32, 16, 768),                             # mean length
        lambda: ext.im2col_u8(x, out, m, [1.0, 0.0, 1.0], None, 32, 32, 16, 768),                   # zero std
    ]
    for call in bad:
        with pytest.raises(RuntimeError):
            call()


def _crop_flip_case(B=4):
    """uint8 80 x 96 source, the integer window x 16..80 (right to left), y 8..72, and its float twin."""
    from pytorch_vit_paper_replication_amd.data.device_input import preprocess_reference

    x = _images(B, 80, 96, seed=7)
    geom = torch.tensor([[80.0, 8.0, 16.0, 72.0]]).repeat(B, 1)
    xf = preprocess_reference(x[:, :, 8:72, 16:80].flip(-1).contiguous(), *IMAGENET)
    return x.cuda(), geom.cuda(), xf.cuda()


def test_model_training_step_bitwise_equal_to_float_input():
    from pytorch_vit_paper_replication_amd import _ext
    from pytorch_vit_paper_replication_amd.data import DeviceInput
    from pytorch_vit_paper_replication_amd.models import ViT
    from pytorch_vit_paper_replication_amd.ops.fused_vit import cross_entropy
    from pytorch_vit_paper_replication_amd.optim import FusedAdam, param_groups_weight_decay

    x, geom, xf = _crop_flip_case()
    y = torch.randint(0, 10, (x.shape[0],), generator=torch.Generator().manual_seed(0)).cuda()

    def step(u8):
        torch.manual_seed(0)
        m = ViT(**CFG).cuda().train()
        opt = FusedAdam(param_groups_weight_decay(m, 0.03), lr=1e-3)
        if u8:
            m.set_device_input(DeviceInput(*IMAGENET))
        loss = cross_entropy(m(x, geom=geom) if u8 else m(xf), y)
        opt.zero_grad()
        loss.backward()
        grads = [p.grad.detach().clone() for p in m.parameters()]
        opt.step(clip_norm=1.0)
        torch.cuda.synchronize()
        assert getattr(m, "_pvr_store", None) is not None, "fused path did not run"
        return loss.detach().clone(), grads, [p.detach().clone() for p in m.parameters()], [n for n, _ in m.named_parameters()]

    with _ext.deterministic_mode():
        lu, gu, pu, names = step(True)
        lf, gf, pf, _ = step(False)
    assert torch.isfinite(lu).item() and torch.equal(lu, lf)
    for n, a, b in zip(names, gu, gf):
        assert torch.equal(a, b), f"grad {n}"
        assert a.abs().sum().item() > 0, f"grad {n} is zero"
    for n, a, b in zip(names, pu, pf):
        assert torch.equal(a, b), f"param {n}"


@pytest.mark.parametrize("inference", [False, True], ids=["no_grad", "inference_mode"])
@pytest.mark.parametrize("backbone", [False, True], ids=["vit", "no_classifier"])
def test_model_forward_bitwise_equal_to_float_input(backbone, inference):
    from pytorch_vit_paper_replication_amd.data import DeviceInput
    from pytorch_vit_paper_replication_amd.models import ViT
    from pytorch_vit_paper_replication_amd.models.vit_no_classifier import ViT as Backbone

    x, geom, xf = _crop_flip_case()
    torch.manual_seed(0)
    m = (Backbone(**{k: v for k, v in CFG.items() if k != "num_classes"}) if backbone else ViT(**CFG)).cuda().eval()
    with (torch.inference_mode() if inference else torch.no_grad()):
        want = m(xf)
        m.set_device_input(DeviceInput(*IMAGENET))
        got = m(x, geom=geom)
        assert torch.equal(m(xf), want)  # a float input with a spec set: unchanged
    assert getattr(m, "_pvr_store", None) is not None, "fused path did not run"
    assert got.shape == want.shape and torch.isfinite(got).all() and torch.equal(got, want)


def test_model_uint8_without_spec_is_the_float_cast():
    from pytorch_vit_paper_replication_amd.models import ViT

    torch.manual_seed(0)
    m = ViT(**CFG).cuda().eval()
    x = _images(2, 64, 64, seed=8).cuda()
    with torch.no_grad():
        assert torch.equal(m(x), m(x.float()))


def test_model_augment_and_default_geom():
    from pytorch_vit_paper_replication_amd.data import DeviceInput, RandomResizedCropFlip, full_box
    from pytorch_vit_paper_replication_amd.models import ViT

    torch.manual_seed(0)
    m = ViT(**CFG).cuda()
    x = _images(8, 80, 96, seed=9).cuda()
    m.set_device_input(DeviceInput(*IMAGENET, augment=RandomResizedCropFlip(generator=torch.Generator().manual_seed(3))))
    draws = RandomResizedCropFlip(generator=torch.Generator().manual_seed(3)).sample(8, 80, 96)
    with torch.no_grad():
        m.train()
        drawn = m(x)
        assert torch.equal(drawn, m(x, geom=draws))
        assert not torch.equal(drawn, m(x))  # the generator has moved on
        m.eval()
        whole = m(x)  # eval: no draw, the whole 80 x 96 source resized
        assert torch.equal(whole, m(x, geom=full_box(8, 80, 96)))
        assert torch.equal(whole, m(x)) and not torch.equal(whole, drawn)
