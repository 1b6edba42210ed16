"""FusedSGD off the fused path, the float64 reference of tests/sgd_reference.py, the cosine schedule and the
CLI's SGD / schedule / ``--init-from`` flags. No GPU."""
import copy
import itertools
import math

import numpy as np
import pytest
import torch

from tests import optim_reference as R
from tests import sgd_reference as S

SHAPES = ((7, 5), (33,), (4, 3, 2))
# momentum x nesterov x weight decay (Nesterov needs a momentum)
CASES = [(m, n, wd) for m, n, wd in itertools.product((0.0, 0.9), (False, True), (0.0, 0.03)) if not (n and m == 0.0)]


def _params(dtype, seed=0):
    gen = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(R.adam_inputs(int(np.prod(s)), gen).view(s).to(dtype)) for s in SHAPES]


def _set_grads(ps, it, dtype):
    gen = torch.Generator().manual_seed(100 + it)
    for p in ps:
        p.grad = R.adam_grad(p.numel(), gen).view(p.shape).to(dtype)


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max()) / float(np.abs(b).max())


@pytest.mark.parametrize("clip", [None, 1.0])
@pytest.mark.parametrize("momentum,nesterov,wd", CASES)
def test_reference_equals_float64_torch_sgd(momentum, nesterov, wd, clip):
    """tests/sgd_reference.py against torch.optim.SGD in float64 on the CPU, 5 steps, to float64 rounding; the clip
    coefficient is torch's clip_grad_norm_'s, min(1, max_norm / (norm + 1e-6))."""
    ps = _params(torch.float64)
    lr = 1e-2
    opt = torch.optim.SGD(ps, lr=lr, momentum=momentum, weight_decay=wd, nesterov=nesterov, foreach=False)
    state = [(p.detach().numpy().copy(), np.zeros(p.shape)) for p in ps]
    for it in range(5):
        _set_grads(ps, it, torch.float64)
        grads = [p.grad.numpy().copy() for p in ps]
        c = 1.0
        if clip is not None:
            norm = math.sqrt(sum(float((g * g).sum()) for g in grads))
            c = min(1.0, clip / (norm + 1e-6))
            assert c < 1.0
            torch.nn.utils.clip_grad_norm_(ps, clip, foreach=False)
        opt.step()
        for k, p in enumerate(ps):
            pr, br = S.sgd_step64(state[k][0], grads[k], state[k][1], lr, momentum, wd, nesterov, c)
            state[k] = (pr, br)
            assert _rel(p.detach().numpy(), pr) <= 1e-14, f"step {it + 1} p[{k}]"
            if momentum != 0:
                assert _rel(opt.state[p]["momentum_buffer"].numpy(), br) <= 1e-14, f"step {it + 1} buf[{k}]"
            else:
                assert "momentum_buffer" not in opt.state.get(p, {}) or opt.state[p]["momentum_buffer"] is None
                assert np.array_equal(br, np.zeros(p.shape))


def _two_groups(ps):
    return [{"params": ps[:2], "weight_decay": 0.03, "momentum": 0.9, "nesterov": True},
            {"params": ps[2:], "lr": 3e-3, "momentum": 0.0}]


def test_torch_ops_in_fp32_equal_torch_sgd_bit_for_bit():
    """FusedSGD off the fused path against torch.optim.SGD (single-tensor, foreach=False) in fp32: two param groups
    (Nesterov momentum with decay; no momentum, another lr), 5 steps, equal bits."""
    from pytorch_vit_paper_replication_amd.optim import FusedSGD

    a, b = _params(torch.float32), _params(torch.float32)
    oa = FusedSGD(_two_groups(a), lr=1e-2, momentum=0.5)
    ob = torch.optim.SGD(_two_groups(b), lr=1e-2, momentum=0.5, foreach=False)
    for it in range(5):
        _set_grads(a, it, torch.float32)
        _set_grads(b, it, torch.float32)
        oa.step()
        ob.step()
        for x, y in zip(a, b):
            assert torch.equal(x, y), f"step {it + 1}"
    for x, y in zip(a[:2], b[:2]):
        assert torch.equal(oa.state[x]["momentum_buffer"], ob.state[y]["momentum_buffer"])
    assert "momentum_buffer" not in oa.state.get(a[2], {})


def test_clip_norm_and_plain_defaults_follow_torch():
    from pytorch_vit_paper_replication_amd.optim import FusedSGD

    a, b = _params(torch.float32), _params(torch.float32)
    oa, ob = FusedSGD(a, lr=1e-2, momentum=0.9), torch.optim.SGD(b, lr=1e-2, momentum=0.9, foreach=False)
    for it in range(3):
        _set_grads(a, it, torch.float32)
        _set_grads(b, it, torch.float32)
        oa.step(clip_norm=1.0)
        n = torch.nn.utils.clip_grad_norm_(b, 1.0)
        ob.step()
        assert torch.equal(oa.last_grad_norm, n)
        assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_state_dict_interchanges_with_torch_sgd_both_ways():
    from pytorch_vit_paper_replication_amd.optim import FusedSGD

    a, b = _params(torch.float32), _params(torch.float32)
    oa = FusedSGD(_two_groups(a), lr=1e-2, momentum=0.5)
    ob = torch.optim.SGD(_two_groups(b), lr=1e-2, momentum=0.5, foreach=False)
    for it in range(2):
        _set_grads(a, it, torch.float32)
        oa.step()
    sd = oa.state_dict()
    assert set(sd["state"]) == {0, 1} and all(set(v) == {"momentum_buffer"} for v in sd["state"].values())
    with torch.no_grad():
        for x, y in zip(a, b):
            y.copy_(x)
    ob.load_state_dict(copy.deepcopy(sd))  # FusedSGD -> torch.optim.SGD (a copy: loading shares the tensors)
    c = _params(torch.float32)
    with torch.no_grad():
        for x, y in zip(a, c):
            y.copy_(x)
    oc = FusedSGD(_two_groups(c), lr=1.0, momentum=0.1)
    oc.load_state_dict(copy.deepcopy(ob.state_dict()))  # torch.optim.SGD -> FusedSGD
    assert [g["lr"] for g in oc.param_groups] == [1e-2, 3e-3] and [g["momentum"] for g in oc.param_groups] == [0.9, 0.0]
    for it in range(2, 5):
        for ps in (a, b, c):
            _set_grads(ps, it, torch.float32)
        oa.step()
        ob.step()
        oc.step()
        for x, y, z in zip(a, b, c):
            assert torch.equal(x, y) and torch.equal(x, z), f"step {it + 1}"


def test_rejected_arguments():
    from pytorch_vit_paper_replication_amd.optim import FusedSGD

    ps = _params(torch.float32)
    with pytest.raises(NotImplementedError):
        FusedSGD(ps, lr=1e-2, momentum=0.9, dampening=0.1)
    with pytest.raises(NotImplementedError):
        FusedSGD(ps, lr=1e-2, maximize=True)
    with pytest.raises(ValueError):
        FusedSGD(ps, lr=1e-2, nesterov=True)
    with pytest.raises(ValueError):
        FusedSGD([{"params": ps[:1]}, {"params": ps[1:], "momentum": 0.0}], lr=1e-2, momentum=0.9, nesterov=True)
    with pytest.raises(ValueError):
        FusedSGD(ps, lr=-1.0)
    opt = FusedSGD(ps, lr=1e-2, momentum=0.9)
    assert set(opt.param_groups[0]) >= {"lr", "momentum", "weight_decay", "nesterov", "dampening", "maximize"}
    assert "betas" not in opt.param_groups[0] and "betas" not in opt.defaults
    opt.param_groups[0]["dampening"] = 0.5  # changed behind the constructor's back
    _set_grads(ps, 0, torch.float32)
    with pytest.raises(NotImplementedError):
        opt.step()


@pytest.mark.parametrize("momentum,nesterov,wd", CASES)
def test_rounding_floors_hold_the_fp32_torch_ops_step(momentum, nesterov, wd):
    """The floors the GPU tests grant the kernels come from operation counts (tests/sgd_reference.py); the fp32
    torch-ops step, the other fp32 evaluation at hand, stays inside them elementwise."""
    from pytorch_vit_paper_replication_amd.optim import FusedSGD

    gen = torch.Generator().manual_seed(7)
    n, lr, c = 4096, 1e-2, 0.37
    lr32, mom32, wd32 = (float(np.float32(x)) for x in (lr, momentum, wd))
    p = torch.nn.Parameter(R.adam_inputs(n, gen))
    opt = FusedSGD([p], lr=lr32, momentum=mom32, weight_decay=wd32, nesterov=nesterov)
    for it in range(3):
        g = R.adam_grad(n, gen)
        p0 = p.detach().clone()
        b0 = opt.state[p]["momentum_buffer"].clone() if momentum and it else torch.zeros(n)
        p.grad = g * c  # the kernel's first operation, rounded once
        opt.step()
        pr, br = S.sgd_step64(p0, g, b0, lr32, mom32, wd32, nesterov, c)
        fl = S.sgd_rounding_floors(p0, g, b0, lr32, mom32, wd32, nesterov, c)
        dp_err = np.abs((p.detach().double() - p0.double()).numpy() - (pr - p0.double().numpy()))
        assert (dp_err <= fl["dp"]).all(), f"step {it + 1}: dp off its floor by {float((dp_err - fl['dp']).max())}"
        if momentum:
            b_err = np.abs(opt.state[p]["momentum_buffer"].double().numpy() - br)
            assert (b_err <= fl["buf"]).all(), f"step {it + 1}: buf off its floor"


def test_warmup_cosine_decay_follows_the_closed_form():
    from pytorch_vit_paper_replication_amd.optim import FusedSGD, warmup_cosine_decay
    from pytorch_vit_paper_replication_amd.optim.schedule import warmup_cosine_factor

    total, frac = 200, 0.05
    w = int(frac * total)
    for mn in (0.0, 0.1):
        p = torch.nn.Parameter(torch.zeros(4))
        opt = FusedSGD([p], lr=0.5, momentum=0.9)
        sched = warmup_cosine_decay(opt, total, frac, min_lr_frac=mn)
        lrs = []
        for _ in range(total + 1):
            lrs.append(opt.param_groups[0]["lr"])
            opt.step()
            sched.step()
        mid = w + (total - w) // 2
        want = {0: 1.0 / (w + 1), w - 1: w / (w + 1), w: 1.0, mid: mn + (1 - mn) * 0.5 * (1 + math.cos(math.pi * (mid - w) / (total - w))),
                total - 1: mn + (1 - mn) * 0.5 * (1 + math.cos(math.pi * (total - 1 - w) / (total - w))), total: mn}
        for s, f in want.items():
            assert lrs[s] == pytest.approx(0.5 * f, rel=1e-12, abs=1e-18), f"step {s} (min_lr_frac {mn})"
            assert warmup_cosine_factor(s, total, frac, mn) == pytest.approx(f, rel=1e-12, abs=1e-18)
        assert lrs[total] == pytest.approx(0.5 * mn, abs=1e-17)  # min_lr_frac is where it ends
        assert all(b <= a for a, b in zip(lrs[w:], lrs[w + 1:])) and all(b > a for a, b in zip(lrs[:w], lrs[1:w + 1]))
    p = torch.nn.Parameter(torch.zeros(4))
    sched = warmup_cosine_decay(FusedSGD([p], lr=1.0), 10, warmup_frac=0.0)  # no warmup: starts at 1
    assert sched.get_last_lr() == [1.0]
    with pytest.raises(ValueError):
        warmup_cosine_decay(FusedSGD([p], lr=1.0), 10, min_lr_frac=1.5)


# ----------------------------------------------------------------------------- CLI
CLI = ["--model", "vit_tiny_test", "--synthetic", "--epochs", "1", "--batch-size", "4", "--image-size", "32", "--num-classes", "3",
       "--synthetic-train-len", "8", "--synthetic-test-len", "4"]


def test_cli_parses_the_new_flags_and_keeps_its_defaults():
    from pytorch_vit_paper_replication_amd.cli.train import build_parser

    a = build_parser().parse_args([])
    assert (a.optimizer, a.momentum, a.nesterov, a.lr_schedule, a.init_from) == ("adam", 0.9, False, "linear", None)
    a = build_parser().parse_args(["--optimizer", "sgd", "--momentum", "0.8", "--nesterov", "--lr-schedule", "cosine", "--init-from", "x.pth"])
    assert (a.optimizer, a.momentum, a.nesterov, a.lr_schedule, a.init_from) == ("sgd", 0.8, True, "cosine", "x.pth")
    with pytest.raises(SystemExit):
        build_parser().parse_args(["--lr-schedule", "step"])


def test_cli_constructs_sgd_the_cosine_schedule_and_the_defaults(tmp_path, monkeypatch):
    from pytorch_vit_paper_replication_amd import engine
    from pytorch_vit_paper_replication_amd.cli.train import main
    from pytorch_vit_paper_replication_amd.optim import FusedAdam, FusedSGD

    seen = []
    monkeypatch.setattr(engine, "train", lambda **kw: seen.append((kw["optimizer"], kw["lr_scheduler"])))
    base = CLI + ["--save-dir", str(tmp_path)]
    assert main(base + ["--optimizer", "sgd", "--weight-decay", "0", "--nesterov", "--lr-schedule", "cosine", "--lr", "0.03"]) == 0
    assert main(base + ["--optimizer", "sgd", "--momentum", "0.5", "--torch-optimizer"]) == 0
    assert main(base) == 0
    (o1, s1), (o2, s2), (o3, s3) = seen
    assert type(o1) is FusedSGD and isinstance(s1, torch.optim.lr_scheduler.LambdaLR)
    assert [(g["momentum"], g["nesterov"], g["weight_decay"]) for g in o1.param_groups] == [(0.9, True, 0.0)] * 2
    assert o1.param_groups[0]["initial_lr"] == 0.03
    assert type(o2) is torch.optim.SGD and o2.param_groups[0]["momentum"] == 0.5 and not o2.param_groups[0]["nesterov"]
    assert [g["weight_decay"] for g in o2.param_groups] == [0.03, 0.0]
    assert isinstance(s2, torch.optim.lr_scheduler.LinearLR)  # warmup_linear_decay (two steps: no warmup phase)
    # a run without the new flags: what it constructed before
    assert type(o3) is FusedAdam and isinstance(s3, torch.optim.lr_scheduler.LinearLR)
    assert [g["weight_decay"] for g in o3.param_groups] == [0.03, 0.0] and o3.param_groups[0]["betas"] == (0.9, 0.999)
    assert not any(g["decoupled_weight_decay"] for g in o3.param_groups)
    with pytest.raises(SystemExit) as e:
        main(base + ["--nesterov"])
    assert "--nesterov" in str(e.value.code)


def test_cli_sgd_runs_one_synthetic_epoch_and_init_from_resizes(tmp_path, monkeypatch):
    """One real epoch with --optimizer sgd at 32 px writes a model; a second run at 48 px and another class count
    starts from it: every weight but the position grid and the classifier is the file's."""
    from pytorch_vit_paper_replication_amd import engine
    from pytorch_vit_paper_replication_amd.cli.train import main
    from pytorch_vit_paper_replication_amd.models.transfer import POS_KEY, resize_position_embedding

    assert main(CLI + ["--save-dir", str(tmp_path), "--save-name", "a.pth", "--optimizer", "sgd", "--lr", "0.01", "--lr-schedule", "cosine"]) == 0
    sd = torch.load(tmp_path / "a.pth", map_location="cpu", weights_only=True)
    seen = []
    monkeypatch.setattr(engine, "train", lambda **kw: seen.append(kw["model"]))
    args = [x for x in CLI]
    args[args.index("--image-size") + 1] = "48"
    args[args.index("--num-classes") + 1] = "5"
    assert main(args + ["--save-dir", str(tmp_path), "--init-from", str(tmp_path / "a.pth"), "--optimizer", "sgd"]) == 0
    new = seen[0].state_dict()
    P = seen[0].config["patch_size"]
    assert seen[0].config["image_size"] == 48 and new["classifier.0.weight"].shape[0] == 5
    for k, v in sd.items():
        if k == POS_KEY:
            assert torch.equal(new[k].cpu(), resize_position_embedding(v, 48 // P, "bicubic"))
        elif k.startswith("classifier."):
            assert new[k].shape != v.shape
        else:
            assert torch.equal(new[k].cpu(), v), k
    with pytest.raises(SystemExit):
        main(["--model", "tinyvgg", "--synthetic", "--init-from", str(tmp_path / "a.pth")])
