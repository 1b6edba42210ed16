"""Patch dropout, the parts that need no GPU: the kept-patch count, the public surface
(``ViT.set_patch_dropout``, ``PatchEmbedding.patch_keep``, presets, CLI flag, checkpoint config), the
reference-path forward and its gradients, the fp8 exclusion, and a numpy oracle of the keep table that
``csrc/elementwise.hip`` ``patch_keep_kernel`` builds on the device (tests/test_gpu_patch_dropout.py
compares the kernel against it). The oracle stands on the numpy replica of the counter hash in
tests/test_drop_path_cpu.py."""
import numpy as np
import pytest
import torch

from pytorch_vit_paper_replication_amd.models import ViT
from tests import test_drop_path_cpu as H

CFG = dict(image_size=32, patch_size=8, num_heads=2, embedding_dim=128, mlp_size=256, num_classes=10)  # n_p = 16
PATCH_DROP_SITE = 1 << 22


# ----------------------------------------------------------------------------- the keep table, in numpy
def patch_keys(seed: int, B: int, n_p: int) -> np.ndarray:
    """uint64 [B, n_p]: the 32-bit key of patch j of sample b at counter value ``seed``."""
    idx = np.arange(B * n_p, dtype=np.uint64)
    return H.rng_hash(H.site_seed(seed, PATCH_DROP_SITE), idx).reshape(B, n_p)


def select(keys_row, n_keep: int) -> np.ndarray:
    """The ``n_keep`` patches with the smallest (key, index) pairs of one sample, ascending by index."""
    keys_row = np.asarray(keys_row)
    j = np.arange(len(keys_row))
    return np.sort(np.lexsort((j, keys_row))[:n_keep])


def keep_table(seed: int, B: int, n_p: int, n_keep: int) -> np.ndarray:
    """int32 [B, n_keep]: the kept patch indices of every sample, each row strictly ascending."""
    keys = patch_keys(seed, B, n_p)
    return np.stack([select(keys[b], n_keep) for b in range(B)]).astype(np.int32)


def inv_table(keep: np.ndarray, n_p: int) -> np.ndarray:
    """int32 [B, n_p]: the slot of a patch in its sample's keep row, -1 if dropped."""
    inv = np.full((keep.shape[0], n_p), -1, dtype=np.int32)
    for b in range(keep.shape[0]):
        inv[b, keep[b]] = np.arange(keep.shape[1])
    return inv


def test_numpy_oracle_against_a_hand_computed_case():
    assert PATCH_DROP_SITE == __import__("pytorch_vit_paper_replication_amd.ops.fused_vit", fromlist=["x"]).PATCH_DROP_SITE
    # ties go to the smaller index: pairs (3,1) (3,3) (7,0) (7,2) (9,4)
    assert select([7, 3, 7, 3, 9], 3).tolist() == [0, 1, 3]
    assert select([7, 3, 7, 3, 9], 4).tolist() == [0, 1, 2, 3]
    assert select([5, 5, 5], 1).tolist() == [0]
    # counter value 5, two samples of four patches. The site's key is rng_key(5 + (PATCH_DROP_SITE << 32)) and the
    # key of patch j of sample b is rng_mix32((4 b + j) ^ that key):
    assert int(H.rng_key(H.site_seed(5, PATCH_DROP_SITE))) == 0xD5F25C0B
    keys = patch_keys(5, 2, 4)
    assert [[int(v) for v in r] for r in keys] == [[0x16C89492, 0x2F8B76E4, 0xDA56887B, 0xC2A18D91],
                                                   [0x9D7FEFCB, 0xA70734D1, 0x3507F84C, 0x9A21009E]]
    # sample 0 by key: patches 0, 1, 3, 2; sample 1: patches 2, 3, 0, 1
    assert keep_table(5, 2, 4, 1).tolist() == [[0], [2]]
    assert keep_table(5, 2, 4, 2).tolist() == [[0, 1], [2, 3]]
    assert keep_table(5, 2, 4, 3).tolist() == [[0, 1, 3], [0, 2, 3]]
    assert keep_table(5, 2, 4, 4).tolist() == [[0, 1, 2, 3]] * 2
    assert inv_table(keep_table(5, 2, 4, 3), 4).tolist() == [[0, 1, -1, 2], [0, -1, 1, 2]]
    # the sample index reaches the key: sample 1 of a batch is not sample 0 of another
    assert not np.array_equal(patch_keys(5, 2, 4)[1], patch_keys(5, 1, 4)[0])


# ----------------------------------------------------------------------------- the kept-patch count and the surface
def test_keep_counts_and_rate_checks():
    from pytorch_vit_paper_replication_amd.models.vit import patch_keep_count

    assert patch_keep_count(196, 0.5) == 98
    assert patch_keep_count(196, 0.25) == 147
    assert patch_keep_count(196, 0.1) == 177
    assert patch_keep_count(16, 0.99) == 1
    assert patch_keep_count(196, 0.0) == 196 and patch_keep_count(16, 0.01) == 16  # n_keep == n_p: off
    m = ViT(**CFG, num_transformer_layer=1)
    pe = m.patch_embedding_block
    assert pe.patch_keep == 0 and "patch_dropout" not in m.config
    assert m.set_patch_dropout(0.5) is m and pe.patch_keep == 8 and m.config["patch_dropout"] == 0.5
    assert m.set_patch_dropout(0.99).patch_embedding_block.patch_keep == 1
    assert m.set_patch_dropout(0.01).patch_embedding_block.patch_keep == 0  # keeps all 16: off
    assert m.set_patch_dropout(0.0).patch_embedding_block.patch_keep == 0 and m.config["patch_dropout"] == 0.0
    for bad in (1.0, -0.1, 1.5):
        with pytest.raises(ValueError, match="patch-dropout"):
            m.set_patch_dropout(bad)
    assert pe.patch_keep == 0  # a rejected rate changes nothing


def test_option_on_and_off_bit_identity_and_state_dict():
    torch.manual_seed(0)
    plain = ViT(**CFG, num_transformer_layer=2)
    pd = ViT(**CFG, num_transformer_layer=2)
    pd.load_state_dict(plain.state_dict())
    x = torch.rand(3, 3, 32, 32)
    pd.set_patch_dropout(0.5).eval()
    plain.eval()
    assert torch.equal(pd(x), plain(x))  # eval never drops
    pd.train()
    plain.train()
    for ctx in (torch.no_grad, torch.inference_mode):  # nor does a forward without grad mode
        torch.manual_seed(1)
        with ctx():
            a = pd(x)
        torch.manual_seed(1)
        with ctx():
            b = plain(x)
        assert torch.equal(a, b)
    torch.manual_seed(1)
    on = pd(x)
    torch.manual_seed(1)
    assert not torch.equal(on, plain(x))  # training with grad mode on does
    pd.set_patch_dropout(0.0)
    torch.manual_seed(1)
    a = pd(x)
    torch.manual_seed(1)
    b = plain(x)
    assert torch.equal(a, b)  # rate 0: the code path without the option, no draw taken from the RNG
    assert list(pd.state_dict().keys()) == list(plain.state_dict().keys())
    assert len(ViT(num_classes=1000).set_patch_dropout(0.5).state_dict()) == 152


def test_presets_cli_flag_and_no_classifier_backbone(tmp_path, monkeypatch):
    from pytorch_vit_paper_replication_amd.cli import train as T
    from pytorch_vit_paper_replication_amd.models import presets, vit
    from pytorch_vit_paper_replication_amd.models.vit_no_classifier import ViT as ViTNoClassifier

    assert vit("vit_tiny_test", image_size=32, num_classes=3, patch_dropout=0.5).patch_embedding_block.patch_keep == 8
    m = vit("vit_tiny_test", image_size=32, num_classes=3)
    assert m.patch_embedding_block.patch_keep == 0 and "patch_dropout" not in m.config
    nc = ViTNoClassifier(**{k: v for k, v in CFG.items() if k != "num_classes"}, num_transformer_layer=1)
    assert nc.set_patch_dropout(0.25) is nc and nc.patch_embedding_block.patch_keep == 12
    assert T.build_parser().parse_args([]).patch_dropout == 0.0
    assert T.build_parser().parse_args(["--patch-dropout", "0.25"]).patch_dropout == 0.25
    made = []
    orig = presets.vit

    def spy(*args, **kw):
        made.append(orig(*args, **kw))
        return made[-1]

    monkeypatch.setattr("pytorch_vit_paper_replication_amd.models.vit", spy)
    rc = T.main(["--model", "vit_tiny_test", "--synthetic", "--epochs", "1", "--batch-size", "4", "--image-size", "32",
                 "--num-classes", "3", "--synthetic-train-len", "8", "--synthetic-test-len", "4", "--save-dir", str(tmp_path),
                 "--patch-dropout", "0.5"])
    assert rc == 0 and made[0].patch_embedding_block.patch_keep == 8 and made[0].config["patch_dropout"] == 0.5
    with pytest.raises(SystemExit):
        T.main(["--model", "vit_tiny_test", "--synthetic", "--patch-dropout", "0.5", "--dtype", "fp8", "--save-dir", str(tmp_path)])
    with pytest.raises(SystemExit):
        T.main(["--model", "vit_tiny_test", "--synthetic", "--patch-dropout", "1.0", "--save-dir", str(tmp_path)])


def test_config_survives_the_checkpoint_helpers(tmp_path):
    from pytorch_vit_paper_replication_amd.utils import load_checkpoint
    from pytorch_vit_paper_replication_amd.utils.checkpoint import save_checkpoint

    m = ViT(**CFG, num_transformer_layer=2).set_patch_dropout(0.25)
    path = save_checkpoint(str(tmp_path), m, epoch=2)
    m2 = ViT(**CFG, num_transformer_layer=2)
    info = load_checkpoint(str(path), m2)
    assert info["config"] == m.config and info["config"]["patch_dropout"] == 0.25
    assert m2.patch_embedding_block.patch_keep == 0 and "patch_dropout" not in m2.config  # returned, not applied
    m2.set_patch_dropout(info["config"]["patch_dropout"])
    assert m2.config == m.config and m2.patch_embedding_block.patch_keep == 12
    path = save_checkpoint(str(tmp_path), ViT(**CFG, num_transformer_layer=2), name="plain.pt")
    assert "patch_dropout" not in load_checkpoint(str(path), m2)["config"]


# ----------------------------------------------------------------------------- reference-path semantics
def test_reference_path_draws_are_sorted_subsets():
    pe = ViT(**CFG, num_transformer_layer=1).patch_embedding_block
    torch.manual_seed(3)
    k = pe._draw_patch_keep(64, 16, 8, torch.device("cpu"))
    assert k.shape == (64, 8) and int(k.min()) >= 0 and int(k.max()) <= 15
    assert bool((k[:, 1:] > k[:, :-1]).all())  # strictly ascending: distinct patches in raster order
    assert len({tuple(r) for r in k.tolist()}) > 32  # and they differ between samples
    counts = torch.bincount(pe._draw_patch_keep(4096, 16, 8, torch.device("cpu")).reshape(-1), minlength=16)
    assert counts.min().item() > 1700 and counts.max().item() < 2400  # every patch kept about half the time


def test_reference_training_forward_equals_a_hand_written_gather(monkeypatch):
    from pytorch_vit_paper_replication_amd.models.vit_no_classifier import ViT as ViTNoClassifier

    torch.manual_seed(4)
    B, D, n_p, n_keep = 3, 128, 16, 8
    cfg = {k: v for k, v in CFG.items() if k != "num_classes"}
    m = ViTNoClassifier(**cfg, num_transformer_layer=2, mlp_dropout=0.0, embedding_dropout=0.0).set_patch_dropout(0.5).train()
    pe = m.patch_embedding_block
    # positions 5 and 9 (patches 4 and 8) are kept by no sample
    keep = torch.tensor([[0, 1, 2, 3, 5, 6, 7, 15], [1, 2, 3, 6, 7, 9, 10, 11], [0, 2, 5, 9, 12, 13, 14, 15]])
    calls = []

    def fixed(batch, np_, nk, device):
        calls.append((batch, np_, nk))
        return keep

    monkeypatch.setattr(pe, "_draw_patch_keep", fixed)
    x = torch.rand(B, 3, 32, 32)
    y = m(x)
    assert calls == [(B, n_p, n_keep)] and y.shape == (B, n_keep + 1, D)
    # by hand: the un-dropped embedding, rows [0] + (keep + 1) of every sample, the same blocks
    conv = pe.patch_and_flatten(x).permute(0, 2, 1)
    full = torch.cat((pe.class_token.expand(B, -1, -1), conv), dim=1) + pe.position_embedding
    sub = torch.stack([full[b, [0] + [int(j) + 1 for j in keep[b]]] for b in range(B)])
    want = m.layer_norm(m.transformer_encoder(sub))
    assert torch.equal(y, want)
    y.square().sum().backward()
    g = pe.position_embedding.grad[0]
    kept_pos = sorted({0} | {int(j) + 1 for j in keep.reshape(-1)})
    dropped = [n for n in range(n_p + 1) if n not in kept_pos]
    assert dropped == [5, 9]
    assert bool((g[dropped] == 0).all())  # exactly zero where no sample kept the patch
    assert all(float(g[n].abs().sum()) > 0 for n in kept_pos)
    # the classifier model: the head reads token 0 whatever the token count
    mc = ViT(**CFG, num_transformer_layer=1).set_patch_dropout(0.5).train()
    assert mc(x).shape == (B, 10)


def test_embedding_dropout_runs_after_the_gather(monkeypatch):
    """The dropout mask has the compact shape [B, n_keep + 1, D]."""
    m = ViT(**CFG, num_transformer_layer=1).set_patch_dropout(0.5).train()
    pe = m.patch_embedding_block
    seen = []
    monkeypatch.setattr(pe.dropout, "forward", lambda t: seen.append(tuple(t.shape)) or t)
    m(torch.rand(2, 3, 32, 32))
    assert seen == [(2, 9, 128)]


def test_fp8_with_patch_dropout_raises_on_the_fused_path(monkeypatch):
    """``enable_fp8()`` + a non-zero rate: the first fused training forward raises, naming both options.
    The fused path is entered through a stubbed ``use_fused`` (nothing on it runs before the check)."""
    from pytorch_vit_paper_replication_amd import _ext

    m = ViT(**CFG, num_transformer_layer=2).set_patch_dropout(0.5).enable_fp8().train()
    monkeypatch.setattr(_ext, "use_fused", lambda t: True)
    x = torch.rand(2, 3, 32, 32)
    with pytest.raises(NotImplementedError, match="enable_fp8.*set_patch_dropout"):
        m(x)
    m.set_patch_dropout(0.0)
    monkeypatch.undo()
    assert m(x).shape == (2, 10)  # rate 0 with fp8 configured: the plain CPU path, no error
