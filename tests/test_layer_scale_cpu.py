"""LayerScale, the parts that need no GPU: the public surface (``ViT.set_layer_scale``, ``folded_state_dict``, presets,
CLI flag, checkpoint ``config``), the reference-path formula, the float64 equivalence of the LayerScale model and the
plain model that holds its folded weights, and the fp8 exclusion."""
import pytest
import torch

from pytorch_vit_paper_replication_amd.models import ViT

CFG = dict(image_size=32, patch_size=8, num_heads=2, embedding_dim=128, mlp_size=256, num_classes=10)


def randomise_scales(m, lo=-2.0, hi=2.0, zeros=3, seed=0):
    """Random scales in ``[lo, hi]`` with ``zeros`` exact zeros per vector, and non-zero biases in the two scaled
    Linear layers (the out-projection's start at zero, which would hide the bias terms)."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for blk in m.transformer_encoder:
            for p in (blk.layer_scale_1, blk.layer_scale_2):
                v = torch.rand(p.shape, generator=g, dtype=torch.float64) * (hi - lo) + lo
                v[torch.randperm(p.numel(), generator=g)[:zeros]] = 0.0
                p.copy_(v.to(device=p.device, dtype=p.dtype))
            for b in (blk.msa_block.multi_head_attention.out_proj.bias, blk.mlp_block.mlp[3].bias):
                b.copy_((torch.randn(b.shape, generator=g, dtype=torch.float64) * 0.1).to(device=b.device, dtype=b.dtype))
    return m


# ----------------------------------------------------------------------------- surface
@pytest.mark.parametrize("depth", [1, 3])
def test_key_counts_init_values_and_removal(depth):
    m = ViT(**CFG, num_transformer_layer=depth)
    plain_keys = list(m.state_dict().keys())
    assert m.set_layer_scale(1e-4) is m
    sd = m.state_dict()
    assert len(sd) == len(plain_keys) + 2 * depth
    new = [k for k in sd if k not in plain_keys]
    assert sorted(new) == sorted(f"transformer_encoder.{i}.layer_scale_{j}" for i in range(depth) for j in (1, 2))
    for k in new:
        assert sd[k].shape == (128,) and sd[k].dtype == torch.float32
        assert torch.equal(sd[k], torch.full((128,), 1e-4))
    for blk in m.transformer_encoder:
        assert isinstance(blk.layer_scale_1, torch.nn.Parameter) and blk.layer_scale_1.requires_grad
        assert blk.fused_params()[12:] == (blk.layer_scale_1, blk.layer_scale_2)
    assert m.config["layer_scale"] == 1e-4 and m.has_layer_scale()
    m.set_layer_scale(0.5)  # again: replaced, not added twice
    assert len(m.state_dict()) == len(plain_keys) + 2 * depth and m.config["layer_scale"] == 0.5
    assert torch.equal(m.transformer_encoder[0].layer_scale_2.detach(), torch.full((128,), 0.5))
    m.set_layer_scale(None)
    assert list(m.state_dict().keys()) == plain_keys and "layer_scale" not in m.config and not m.has_layer_scale()
    assert len(m.transformer_encoder[0].fused_params()) == 12


def test_full_size_key_counts():
    m = ViT(num_classes=1000)
    assert len(m.state_dict()) == 152
    assert len(m.set_layer_scale(1e-4).state_dict()) == 152 + 2 * 12
    assert len(m.folded_state_dict()) == 152
    assert len(m.set_layer_scale(None).state_dict()) == 152


def test_vectors_land_in_the_no_decay_group():
    from pytorch_vit_paper_replication_amd.optim import param_groups_weight_decay

    m = ViT(**CFG, num_transformer_layer=2).set_layer_scale(1e-4)
    groups = param_groups_weight_decay(m, 0.05)
    decay = [g for g in groups if g["weight_decay"] != 0.0]
    no_decay = [g for g in groups if g["weight_decay"] == 0.0]
    assert len(decay) == 1 and len(no_decay) == 1
    ids = {id(p) for p in no_decay[0]["params"]}
    for blk in m.transformer_encoder:
        assert id(blk.layer_scale_1) in ids and id(blk.layer_scale_2) in ids
    assert all(id(blk.layer_scale_1) not in {id(p) for p in decay[0]["params"]} for blk in m.transformer_encoder)


def test_a_covering_store_refuses_the_option():
    """After the flat store has laid the parameters out (the first fused forward, a fused optimizer, DDP) the option
    can no longer add parameters: ``RuntimeError`` naming the store."""
    from pytorch_vit_paper_replication_amd.runtime.param_store import get_store

    m = ViT(**CFG, num_transformer_layer=1)
    get_store(m, torch.device("cpu"))
    with pytest.raises(RuntimeError, match="ParamStore already covers"):
        m.set_layer_scale(1e-4)
    with pytest.raises(RuntimeError, match="ParamStore already covers"):
        m.set_layer_scale(None)


def test_store_fold_on_the_cpu_follows_the_generation():
    """The store's folded copies (torch fallback of the fold kernel): the bf16 of ``g[:, None] * W`` and its transpose,
    fp32 ``g * b``, rebuilt when and only when the generation moved."""
    from pytorch_vit_paper_replication_amd.runtime.param_store import get_store

    m = randomise_scales(ViT(**CFG, num_transformer_layer=2).set_layer_scale(1e-4))
    st = get_store(m, torch.device("cpu"))
    triples = [t for blk in m.transformer_encoder for t in blk.folded_triples()]
    assert len(triples) == 4
    st.register_folded(triples)
    st.refresh_shadow()
    st.fold()
    for w, b, g in triples:
        w16, wt16 = st.folded_w(w)
        want = (g.detach()[:, None] * w.detach()).to(torch.bfloat16)
        assert torch.equal(w16, want) and torch.equal(wt16, want.t()) and wt16.is_contiguous()
        assert torch.equal(st.folded_b(b), g.detach() * b.detach())
    w, b, g = triples[1]
    before = st.folded_w(w)[0].clone()
    st.fold()  # nothing moved
    assert torch.equal(st.folded_w(w)[0], before)
    with torch.no_grad():
        g.mul_(2.0)  # an outside write: the version counter moves, refresh_shadow bumps the generation
    st.refresh_shadow()
    st.fold()
    assert torch.equal(st.folded_w(w)[0], (g.detach()[:, None] * w.detach()).to(torch.bfloat16))
    assert not torch.equal(st.folded_w(w)[0], before)
    with pytest.raises(ValueError, match="multiples of 8"):
        st.register_folded([(torch.nn.Parameter(torch.zeros(12, 8)), torch.nn.Parameter(torch.zeros(12)), torch.nn.Parameter(torch.zeros(12)))])


# ----------------------------------------------------------------------------- reference-path semantics
def test_reference_path_formula_against_a_hand_written_block(monkeypatch):
    from pytorch_vit_paper_replication_amd.models.vit import TransformerEncoderBlock

    torch.manual_seed(2)
    blk = TransformerEncoderBlock(embedding_dim=64, num_heads=2, mlp_size=128, mlp_dropout=0.0).eval()
    x = torch.randn(4, 5, 64)
    plain = blk(x)
    g1, g2 = torch.randn(64), torch.randn(64)
    g1[3] = 0.0
    blk.register_parameter("layer_scale_1", torch.nn.Parameter(g1.clone()))
    blk.register_parameter("layer_scale_2", torch.nn.Parameter(g2.clone()))
    x1 = g1 * blk.msa_block(x) + x
    want = g2 * blk.mlp_block(x1) + x1
    assert torch.equal(blk(x), want) and not torch.equal(want, plain)  # the same fp32 operations: the same bits
    assert torch.equal(x1[..., 3], x[..., 3])  # a zero scale: the channel passes through the attention branch
    # with drop path: the scale before the per-sample factor and the residual add
    blk.train()
    blk.drop_path = 0.5
    keeps = {0: torch.tensor([True, False, True, False]), 1: torch.tensor([False, False, True, True])}
    monkeypatch.setattr(blk, "_draw_drop_path", lambda batch, p, branch, device: keeps[branch])
    s_a = keeps[0].float().view(4, 1, 1) * 2.0
    s_m = keeps[1].float().view(4, 1, 1) * 2.0
    x1 = s_a * (g1 * blk.msa_block(x)) + x
    assert torch.equal(blk(x), s_m * (g2 * blk.mlp_block(x1)) + x1)
    assert torch.equal(blk(x)[1], x[1])  # both branches dropped
    # scales of one are the plain block
    with torch.no_grad():
        blk.layer_scale_1.fill_(1.0)
        blk.layer_scale_2.fill_(1.0)
    blk.eval()
    assert torch.equal(blk(x), plain)


@pytest.mark.parametrize("train", [False, True])
def test_float64_equivalence_of_the_model_and_its_fold(train):
    """``M.double()`` against ``P.double()`` loaded with ``M.double().folded_state_dict()``: logits, loss and the
    gradient identities of the fold, to 1e-12 relative, in eval and in training mode (dropout 0: the reference path
    draws its masks from torch's RNG)."""
    torch.manual_seed(5)
    cfg = dict(CFG, num_transformer_layer=3, mlp_dropout=0.0, embedding_dropout=0.0)
    M = randomise_scales(ViT(**cfg).set_layer_scale(1e-4)).double()
    P = ViT(**cfg).double()
    P.load_state_dict(M.folded_state_dict())
    M.train(train)
    P.train(train)
    x = torch.rand(3, 3, 32, 32, dtype=torch.float64)
    y = torch.tensor([1, 7, 3])
    a, b = M(x), P(x)

    def rel(u, v):
        return ((u - v).abs().max() / v.abs().max().clamp_min(1e-300)).item()

    assert rel(a, b) <= 1e-12
    la, lb = torch.nn.functional.cross_entropy(a, y), torch.nn.functional.cross_entropy(b, y)
    assert rel(la, lb) <= 1e-12
    la.backward()
    lb.backward()
    gp = dict(P.named_parameters())
    scaled = {}
    for i, blk in enumerate(M.transformer_encoder):
        for (w, bias, g), name in zip(blk.folded_triples(), (f"transformer_encoder.{i}.msa_block.multi_head_attention.out_proj",
                                                                f"transformer_encoder.{i}.mlp_block.mlp.3")):
            scaled[name] = (w, bias, g)
    for n, p in M.named_parameters():
        if ".layer_scale_" in n or n.rsplit(".", 1)[0] in scaled:
            continue
        assert rel(p.grad, gp[n].grad) <= 1e-12, n
    for name, (w, bias, g) in scaled.items():
        dwh, dbh = gp[name + ".weight"].grad, gp[name + ".bias"].grad
        nz = g.detach() != 0
        assert nz.sum() < g.numel() and rel(w.grad, g.detach()[:, None] * dwh) <= 1e-12, name
        assert rel(bias.grad, g.detach() * dbh) <= 1e-12, name
        # dW-hat's rows are those of the plain model, whose weight rows are g * W: with g = 0 the row of W is free
        assert rel(g.grad, (dwh * w.detach()).sum(1) + dbh * bias.detach()) <= 1e-12, name


def test_folded_state_dict_loads_into_a_plain_model_and_matches_in_fp32():
    torch.manual_seed(6)
    cfg = dict(CFG, num_transformer_layer=2)
    M = randomise_scales(ViT(**cfg).set_layer_scale(1e-4)).eval()
    sd = M.folded_state_dict()
    P = ViT(**cfg).eval()
    assert list(sd.keys()) == list(P.state_dict().keys())
    P.load_state_dict(sd)  # strict
    blk = M.transformer_encoder[1]
    w, b, g = blk.folded_triples()[1]
    assert torch.equal(sd["transformer_encoder.1.mlp_block.mlp.3.weight"], g.detach()[:, None] * w.detach())
    assert torch.equal(sd["transformer_encoder.1.mlp_block.mlp.3.bias"], g.detach() * b.detach())
    assert sd["transformer_encoder.1.mlp_block.mlp.3.weight"].data_ptr() != w.data_ptr()
    x = torch.rand(2, 3, 32, 32)
    a, c = M(x), P(x)
    # fp32: g * (a W^T + b) against a (g W)^T + g b differ by the rounding of a 256-term dot product
    assert torch.allclose(a, c, rtol=1e-4, atol=1e-5)
    # a model without the option: a copy of its state dict
    sd2 = P.folded_state_dict()
    assert all(torch.equal(sd2[k], v) and sd2[k].data_ptr() != v.data_ptr() for k, v in P.state_dict().items())


def test_no_classifier_backbone_and_presets():
    from pytorch_vit_paper_replication_amd.models import vit
    from pytorch_vit_paper_replication_amd.models.vit_no_classifier import ViT as ViTNoClassifier

    m = vit("vit_tiny_test", image_size=32, num_classes=3, layer_scale=1e-4)
    assert m.has_layer_scale() and m.config["layer_scale"] == 1e-4 and len(m.state_dict()) == len(m.folded_state_dict()) + 4
    plain = vit("vit_tiny_test", image_size=32, num_classes=3)
    assert not plain.has_layer_scale() and "layer_scale" not in plain.config
    assert all(len(blk.fused_params()) == 12 for blk in plain.transformer_encoder)
    nc = ViTNoClassifier(**{k: v for k, v in CFG.items() if k != "num_classes"}, num_transformer_layer=3)
    n0 = len(nc.state_dict())
    assert len(nc.set_layer_scale(1e-4).state_dict()) == n0 + 6 and len(nc.folded_state_dict()) == n0
    randomise_scales(nc).eval()
    pn = ViTNoClassifier(**{k: v for k, v in CFG.items() if k != "num_classes"}, num_transformer_layer=3).eval()
    pn.load_state_dict(nc.folded_state_dict())
    x = torch.rand(2, 3, 32, 32)
    assert torch.allclose(nc(x), pn(x), rtol=1e-4, atol=1e-5)


def test_config_survives_the_checkpoint_helpers(tmp_path):
    from pytorch_vit_paper_replication_amd.utils import load_checkpoint
    from pytorch_vit_paper_replication_amd.utils.checkpoint import save_checkpoint

    m = randomise_scales(ViT(**CFG, num_transformer_layer=2).set_layer_scale(1e-4))
    path = save_checkpoint(str(tmp_path), m, epoch=2)
    m2 = ViT(**CFG, num_transformer_layer=2)
    with pytest.raises(RuntimeError, match="layer_scale"):  # the keys differ: the caller sets the option first
        load_checkpoint(str(path), m2)
    m2.set_layer_scale(0.0)
    info = load_checkpoint(str(path), m2)
    assert info["epoch"] == 2 and info["config"]["layer_scale"] == 1e-4 and info["config"] is not m.config
    assert m2.config["layer_scale"] == 0.0  # returned, not applied
    for (n, a), (_, b) in zip(m.state_dict().items(), m2.state_dict().items()):
        assert torch.equal(a, b), n
    path = save_checkpoint(str(tmp_path), ViT(**CFG, num_transformer_layer=2), name="plain.pt")
    assert "layer_scale" not in load_checkpoint(str(path), ViT(**CFG, num_transformer_layer=2))["config"]


def test_cli_flag_parses_and_reaches_the_model(tmp_path, monkeypatch):
    from pytorch_vit_paper_replication_amd.cli import train as T
    from pytorch_vit_paper_replication_amd.models import presets

    assert T.build_parser().parse_args([]).layer_scale is None
    assert T.build_parser().parse_args(["--layer-scale", "1e-4"]).layer_scale == 1e-4
    made = []
    orig = presets.vit

    def spy(*args, **kw):
        made.append(orig(*args, **kw))
        return made[-1]

    monkeypatch.setattr("pytorch_vit_paper_replication_amd.models.vit", spy)
    common = ["--model", "vit_tiny_test", "--synthetic", "--epochs", "1", "--batch-size", "4", "--image-size", "32",
              "--num-classes", "3", "--synthetic-train-len", "8", "--synthetic-test-len", "4", "--save-dir", str(tmp_path)]
    assert T.main(common + ["--layer-scale", "1e-4"]) == 0
    assert made[0].has_layer_scale() and made[0].config["layer_scale"] == 1e-4
    # one step of training moved the vectors off their init
    assert any(not torch.equal(blk.layer_scale_1.detach().cpu(), torch.full((128,), 1e-4)) for blk in made[0].transformer_encoder)
    assert T.main(common) == 0  # without the flag: what it constructed before
    assert not made[1].has_layer_scale() and "layer_scale" not in made[1].config
    assert len(made[1].state_dict()) == 8 + 12 * 2 and len(made[0].state_dict()) == 8 + 14 * 2  # 2 blocks
    with pytest.raises(SystemExit):
        T.main(["--model", "vit_tiny_test", "--synthetic", "--layer-scale", "1e-4", "--dtype", "fp8", "--save-dir", str(tmp_path)])
    with pytest.raises(SystemExit):
        T.main(["--model", "tinyvgg", "--synthetic", "--layer-scale", "1e-4", "--save-dir", str(tmp_path)])


def test_fp8_with_layer_scale_raises_on_the_fused_path(monkeypatch):
    """``enable_fp8()`` + LayerScale: the first fused forward raises, naming both options. The fused path is entered
    through a stubbed ``use_fused`` (nothing on it runs before the check)."""
    from pytorch_vit_paper_replication_amd import _ext

    m = ViT(**CFG, num_transformer_layer=2).set_layer_scale(1e-4).enable_fp8().train()
    monkeypatch.setattr(_ext, "use_fused", lambda t: True)
    x = torch.rand(2, 3, 32, 32)
    with pytest.raises(NotImplementedError, match="enable_fp8.*set_layer_scale"):
        m(x)
    monkeypatch.undo()
    assert m(x).shape == (2, 10)  # the plain CPU path: no error
    assert getattr(m, "_pvr_store", None) is None  # the check came before the store: the option can still be removed
    m.set_layer_scale(None)
