"""ModelEma off the GPU: the torch path, attach(), applied(), state dicts, checkpoints, the CLI."""
import re

import numpy as np
import pytest
import torch
from torch import nn
from torch.utils.data import DataLoader, TensorDataset

from pytorch_vit_paper_replication_amd import engine
from pytorch_vit_paper_replication_amd.models import ViT
from pytorch_vit_paper_replication_amd.optim import FusedAdam, ModelEma, param_groups_weight_decay
from pytorch_vit_paper_replication_amd.utils.checkpoint import load_checkpoint, save_checkpoint

SMALL = dict(image_size=32, patch_size=16, num_transformer_layer=2, num_heads=2, embedding_dim=32, mlp_size=64,
             num_classes=3)


class Tiny(nn.Module):
    def __init__(self, n=3):
        super().__init__()
        self.l = nn.Linear(4, n)
        self.frozen = nn.Linear(4, 4)
        self.frozen.requires_grad_(False)

    def forward(self, x):
        return self.l(self.frozen(x))


def _loader(n, bs):
    g = torch.Generator().manual_seed(0)
    x = torch.randn(n, 4, generator=g)
    y = torch.randint(0, 3, (n,), generator=g)
    return DataLoader(TensorDataset(x, y), batch_size=bs, shuffle=False)


def _perturb(model, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in model.parameters():
            if p.requires_grad:
                p.add_(torch.randn(p.shape, generator=g) * 0.1)


@pytest.mark.parametrize("warmup", [False, True])
def test_torch_path_matches_hand_loop(warmup):
    """update() is ema = d * ema + (1 - d) * p with the fp32 pair of that update; the hand loop runs the
    same two torch ops, so the values are bit-equal. Frozen parameters never move."""
    torch.manual_seed(0)
    m = Tiny()
    ema = ModelEma(m, decay=0.9, warmup=warmup)
    want = {n: p.detach().clone() for n, p in m.named_parameters()}
    frozen0 = {n: p.detach().clone() for n, p in m.named_parameters() if not p.requires_grad}
    assert frozen0
    for n_upd in range(4):
        _perturb(m, n_upd)
        d = min(0.9, (1 + n_upd) / (10 + n_upd)) if warmup else 0.9
        d32, w32 = np.float32(d), np.float32(1.0 - d)
        assert ema.pair_at(n_upd) == (d32, w32)
        ema.update()
        for n, p in m.named_parameters():
            if p.requires_grad:
                want[n] = want[n].mul(float(d32)).add(p.detach(), alpha=float(w32))
        got = ema.state_dict()
        for n in want:
            assert torch.equal(got[n], want[n]), (n_upd, n)
    assert ema.num_updates == 4
    for n, v in frozen0.items():
        assert torch.equal(ema.state_dict()[n], v)
    if warmup:
        assert [ema.decay_at(n) for n in range(3)] == [1 / 10, 2 / 11, 3 / 12] and ema.decay_at(10 ** 6) == 0.9


def test_exact_ends_on_the_torch_path():
    torch.manual_seed(0)
    m = Tiny()
    e0, e1 = ModelEma(m, decay=0.0), ModelEma(m, decay=1.0)
    init = {n: p.detach().clone() for n, p in m.named_parameters()}
    for i in range(2):
        _perturb(m, i)
        e0.update()
        e1.update()
    for n, p in m.named_parameters():
        assert torch.equal(e0.state_dict()[n], p.detach())
        assert torch.equal(e1.state_dict()[n], init[n])
    with pytest.raises(ValueError):
        ModelEma(m, decay=1.5)


def test_state_dict_has_the_models_keys_and_loads_strict():
    torch.manual_seed(0)
    m = ViT()
    ema = ModelEma(m)
    sd = ema.state_dict()
    assert list(sd) == list(m.state_dict()) and len(sd) == 152
    assert all(v.dtype == torch.float32 and v.device.type == "cpu" for v in sd.values())
    fresh = ViT()
    fresh.load_state_dict(sd, strict=True)
    for a, b in zip(m.parameters(), fresh.parameters()):
        assert torch.equal(a, b)
    # own storages: writing into the state dict does not reach the average
    sd["classifier.0.bias"].add_(1.0)
    assert not torch.equal(ema.state_dict()["classifier.0.bias"], sd["classifier.0.bias"])
    # round trip through load_state_dict
    other = ModelEma(ViT())
    other.load_state_dict(ema.state_dict())
    for k, v in ema.state_dict().items():
        assert torch.equal(other.state_dict()[k], v), k
    with pytest.raises(KeyError):
        other.load_state_dict({})


def test_attached_cpu_fused_adam_updates_once_per_step():
    """A FusedAdam that falls back to the reference math updates its attached EMA inside step()."""
    torch.manual_seed(0)
    m = ViT(**SMALL)
    opt = FusedAdam(param_groups_weight_decay(m, 0.03), lr=1e-2)
    ema = ModelEma(m, decay=0.5).attach(opt)
    assert ema.updated_by(opt)
    want = {n: p.detach().clone() for n, p in m.named_parameters()}
    for it in range(3):
        for p in m.parameters():
            p.grad = torch.randn_like(p)
        opt.step(clip_norm=1.0)
        assert ema.num_updates == it + 1
        for n, p in m.named_parameters():
            want[n] = want[n].mul(0.5).add(p.detach(), alpha=0.5)
    got = ema.state_dict()
    for n in want:
        assert torch.equal(got[n], want[n]), n
    ema.detach()
    assert not ema.updated_by(opt) and opt._ema is None


@pytest.mark.parametrize("fused", [False, True])
def test_train_step_updates_exactly_once_per_step(fused):
    """engine.train_step attaches the EMA: a FusedAdam updates it in step(), torch.optim.Adam gets the
    update after its step. Either way one update per batch."""
    torch.manual_seed(0)
    m = Tiny()
    params = [p for p in m.parameters() if p.requires_grad]
    opt = FusedAdam(params, lr=1e-2) if fused else torch.optim.Adam(params, lr=1e-2)
    sched = torch.optim.lr_scheduler.LinearLR(opt, start_factor=1.0, end_factor=0.5, total_iters=100)
    ema = ModelEma(m, decay=0.0)
    engine.train_step(m, _loader(10, 4), nn.CrossEntropyLoss(), opt, sched, "cpu", model_ema=ema)
    assert ema.num_updates == 3 and ema.updated_by(opt) == fused
    for n, p in m.named_parameters():  # decay 0: the average is the weights after the last step
        assert torch.equal(ema.state_dict()[n], p.detach()), n


def test_applied_swaps_and_restores_also_when_the_body_raises():
    torch.manual_seed(0)
    m = Tiny()
    ema = ModelEma(m, decay=0.5)
    _perturb(m, 0)
    ema.update()
    before = [(p.data, p.detach().clone()) for p in m.parameters()]
    x = torch.randn(5, 4)
    out_trained = m(x)
    fresh = Tiny()
    fresh.load_state_dict(ema.state_dict())
    with ema.applied():
        assert torch.equal(m(x), fresh(x))
        assert not torch.equal(m(x), out_trained)
    with pytest.raises(RuntimeError, match="boom"):
        with ema.applied():
            raise RuntimeError("boom")
    for p, (data, val) in zip(m.parameters(), before):
        assert p.data.data_ptr() == data.data_ptr() and torch.equal(p.detach(), val)
    assert torch.equal(m(x), out_trained)


def test_checkpoint_round_trip(tmp_path, capsys):
    torch.manual_seed(0)
    m = ViT(**SMALL)
    opt = FusedAdam(param_groups_weight_decay(m, 0.03), lr=1e-2)
    ema = ModelEma(m, decay=0.9, warmup=True).attach(opt)
    for _ in range(2):
        for p in m.parameters():
            p.grad = torch.randn_like(p)
        opt.step()
    path = save_checkpoint(str(tmp_path), m, opt, epoch=1, model_ema=ema)
    state = torch.load(path, map_location="cpu", weights_only=True)
    assert set(state["model_ema"]) == {"params", "num_updates", "decay", "warmup"}
    assert state["model_ema"]["num_updates"] == 2 and state["model_ema"]["decay"] == 0.9 and state["model_ema"]["warmup"] is True
    assert list(state["model_ema"]["params"]) == list(m.state_dict())

    torch.manual_seed(1)
    m2 = ViT(**SMALL)
    opt2 = FusedAdam(param_groups_weight_decay(m2, 0.03), lr=1e-2)
    ema2 = ModelEma(m2, decay=0.9, warmup=True).attach(opt2)
    load_checkpoint(str(path), m2, opt2, model_ema=ema2)
    assert ema2.num_updates == 2
    for k, v in ema.state_dict().items():
        assert torch.equal(ema2.state_dict()[k], v), k
    assert not any(torch.equal(ema2.state_dict()[k], m2.state_dict()[k]) for k in ("classifier.0.weight",))

    # a checkpoint without the entry: the average starts from the loaded weights, and rank 0 says so
    old = save_checkpoint(str(tmp_path), m, opt, epoch=1, name="no_ema.pt")
    assert "model_ema" not in torch.load(old, map_location="cpu", weights_only=True)
    capsys.readouterr()
    ema3 = ModelEma(m2, decay=0.9)
    ema3.num_updates = 5
    load_checkpoint(str(old), m2, opt2, model_ema=ema3)
    assert capsys.readouterr().out.count("holds no model EMA") == 1
    assert ema3.num_updates == 0
    for k, v in m.state_dict().items():
        assert torch.equal(ema3.state_dict()[k], v), k
    # without an EMA given, the entry is ignored
    load_checkpoint(str(path), m2, opt2)


def test_cli_flags_and_ema_file(tmp_path):
    from pytorch_vit_paper_replication_amd.cli import train as T

    a = T.build_parser().parse_args([])
    assert a.model_ema is None and a.model_ema_warmup is False
    assert T.build_parser().parse_args(["--model-ema"]).model_ema == 0.9999
    a = T.build_parser().parse_args(["--model-ema", "0.999", "--model-ema-warmup"])
    assert a.model_ema == 0.999 and a.model_ema_warmup is True
    help_text = T.build_parser().format_help()
    assert "--model-ema [DECAY]" in help_text and "--model-ema-warmup" in help_text
    with pytest.raises(SystemExit):
        T.main(["--model", "tinyvgg", "--synthetic", "--model-ema-warmup"])

    args = ["--model", "tinyvgg", "--synthetic", "--epochs", "1", "--batch-size", "4", "--image-size", "64", "--num-classes", "3",
            "--synthetic-train-len", "8", "--synthetic-test-len", "4", "--save-dir", str(tmp_path), "--save-name", "t.pth"]
    assert T.main(args + ["--model-ema", "0.9", "--checkpoint-dir", str(tmp_path / "ck")]) == 0
    sd = torch.load(tmp_path / "t.pth", weights_only=True)
    sd_ema = torch.load(tmp_path / "t_ema.pth", weights_only=True)
    assert list(sd) == list(sd_ema)
    assert any(not torch.equal(sd[k], sd_ema[k]) for k in sd)
    # --resume restores the average: one more epoch continues the update counter from the checkpoint
    ck = torch.load(tmp_path / "ck" / "checkpoint.pt", weights_only=True)
    assert ck["model_ema"]["num_updates"] == 2 and ck["model_ema"]["decay"] == 0.9
    assert T.main(args[:4] + ["2"] + args[5:] + ["--model-ema", "0.9", "--resume", str(tmp_path / "ck" / "checkpoint.pt"),
                                                  "--checkpoint-dir", str(tmp_path / "ck2")]) == 0
    assert torch.load(tmp_path / "ck2" / "checkpoint.pt", weights_only=True)["model_ema"]["num_updates"] == 4
    # without the flag nothing new is written
    assert T.main(args[:-1] + ["plain.pth"]) == 0
    assert (tmp_path / "plain.pth").exists() and not (tmp_path / "plain_ema.pth").exists()


def test_engine_train_with_model_ema_keeps_the_reference_surface(capsys):
    torch.manual_seed(0)
    m = Tiny()
    opt = torch.optim.Adam([p for p in m.parameters() if p.requires_grad], lr=1e-1)
    sched = torch.optim.lr_scheduler.LinearLR(opt, start_factor=1.0, end_factor=0.5, total_iters=100)
    ema = ModelEma(m, decay=0.9)
    res = engine.train(m, _loader(10, 4), _loader(6, 4), opt, nn.CrossEntropyLoss(), sched, epochs=2, device="cpu", model_ema=ema)
    assert set(res) == {"train_loss", "train_acc", "test_loss", "test_acc"}
    assert all(len(v) == 2 for v in res.values())
    out = capsys.readouterr().out
    lines = [l for l in out.splitlines() if l.startswith("Epoch:")]
    assert len(lines) == 2
    assert re.fullmatch(r"Epoch: 1 \| train_loss: \d+\.\d{4} \| train_acc: \d+\.\d{4} \| test_loss: \d+\.\d{4} \| "
                        r"test_acc: \d+\.\d{4}", lines[0])
    assert ema.num_updates == 6
    # the test metrics are those of the averaged weights
    with ema.applied():
        want = engine.test_step(m, _loader(6, 4), nn.CrossEntropyLoss(), "cpu")
    assert (res["test_loss"][-1], res["test_acc"][-1]) == want
    assert engine.test_step(m, _loader(6, 4), nn.CrossEntropyLoss(), "cpu")[0] != want[0]
