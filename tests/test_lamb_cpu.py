"""FusedLamb off the fused path (torch ops per tensor, the parameters' dtype) against the float64
reference of tests/lamb_reference.py, its special cases, its options and state dict, and the CLI's
``--optimizer``."""
import numpy as np
import pytest
import torch

from tests import lamb_reference as L
from tests import optim_reference as R

SHAPES = ((7, 5), (33,), (4, 3, 2))
# (weight decay, always_adapt): adapting with decay, plain Adam steps, adapting without decay
MODES = ((0.03, False), (0.0, False), (0.0, True))


def _params(dtype, seed=0):
    gen = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(R.adam_inputs(int(np.prod(s)), gen).view(s).to(dtype)) for s in SHAPES]


def _set_grads(ps, it, dtype):
    gen = torch.Generator().manual_seed(100 + it)
    for p in ps:
        p.grad = R.adam_grad(p.numel(), gen).view(p.shape).to(dtype)


def _close(a, b, what):
    a, b = torch.as_tensor(a, dtype=torch.float64), torch.as_tensor(b, dtype=torch.float64)
    scale = float(b.abs().max())
    err = float((a - b).abs().max())
    assert err <= 1e-12 * scale, f"{what}: {err} against {scale}"


@pytest.mark.parametrize("betas", R.BETAS)
@pytest.mark.parametrize("wd,always", MODES)
def test_torch_ops_in_float64_equal_the_reference(betas, wd, always):
    from pytorch_vit_paper_replication_amd.optim import FusedLamb

    ps = _params(torch.float64)
    lr, eps = 1e-2, 1e-6
    opt = FusedLamb(ps, lr=lr, betas=betas, eps=eps, weight_decay=wd, always_adapt=always)
    state = [(p.detach().clone(), torch.zeros_like(p), torch.zeros_like(p)) for p in ps]
    for it in range(3):
        _set_grads(ps, it, torch.float64)
        opt.step()
        row = R.group_row(lr, betas, eps, wd, it + 1, False)
        assert opt.last_trust.shape == (len(ps), 3) and opt.last_trust.dtype == torch.float64
        for k, p in enumerate(ps):
            pr, mr, vr, wn, un, r = L.lamb_step64(*state[k][:1], p.grad, *state[k][1:], row, wd != 0 or always)
            state[k] = (pr, mr, vr)
            _close(p.detach(), pr, f"step {it + 1} p[{k}]")
            assert pr.shape == p.shape
            _close(opt.state[p]["exp_avg"], mr, f"step {it + 1} m[{k}]")
            _close(opt.state[p]["exp_avg_sq"], vr, f"step {it + 1} v[{k}]")
            _close(opt.last_trust[k], [wn, un, r], f"step {it + 1} trust[{k}]")
            assert (r != 1.0) == (wd != 0 or always)


@pytest.mark.parametrize("betas", R.BETAS)
def test_a_group_that_does_not_adapt_takes_fused_adams_steps(betas):
    from pytorch_vit_paper_replication_amd.optim import FusedAdam, FusedLamb

    a, b = _params(torch.float32), _params(torch.float32)
    la = FusedLamb(a, lr=1e-2, betas=betas, eps=1e-6, weight_decay=0.0)
    ad = FusedAdam(b, lr=1e-2, betas=betas, eps=1e-6, weight_decay=0.0)
    for it in range(3):
        _set_grads(a, it, torch.float32)
        _set_grads(b, it, torch.float32)
        la.step()
        ad.step()
        for x, y in zip(a, b):
            assert torch.equal(x, y) and torch.equal(la.state[x]["exp_avg"], ad.state[y]["exp_avg"])
            assert torch.equal(la.state[x]["exp_avg_sq"], ad.state[y]["exp_avg_sq"])
        assert bool((la.last_trust[:, 2] == 1).all())
    assert not torch.equal(a[0], _params(torch.float32)[0])


def test_an_all_zero_tensor_with_decay_gets_ratio_one():
    from pytorch_vit_paper_replication_amd.optim import FusedLamb

    p = torch.nn.Parameter(torch.zeros(5, 3))
    q = torch.nn.Parameter(torch.zeros(5, 3))
    opt = FusedLamb([p], lr=1e-2, weight_decay=0.1)
    ref = FusedLamb([q], lr=1e-2, weight_decay=0.0)  # u is the same where w = 0; this one takes r = 1 by its group
    _set_grads([p], 0, torch.float32)
    _set_grads([q], 0, torch.float32)
    opt.step()
    ref.step()
    wn, un, r = opt.last_trust[0].tolist()
    assert wn == 0.0 and un > 0.0 and r == 1.0
    assert bool(torch.isfinite(p).all()) and bool((p != 0).any())
    torch.testing.assert_close(p, q, rtol=1e-6, atol=0.0)


def test_zero_gradient_and_moments_under_always_adapt_do_not_move():
    from pytorch_vit_paper_replication_amd.optim import FusedLamb

    p = _params(torch.float32)[0]
    before = p.detach().clone()
    opt = FusedLamb([p], lr=1e-2, weight_decay=0.0, always_adapt=True)
    p.grad = torch.zeros_like(p)
    opt.step()
    wn, un, r = opt.last_trust[0].tolist()
    assert wn > 0.0 and un == 0.0 and r == 1.0
    assert torch.equal(p.detach(), before)


def test_options_and_group_table():
    from pytorch_vit_paper_replication_amd.optim import FusedAdam, FusedLamb

    p0, p1, p2 = (torch.nn.Parameter(torch.zeros(4)) for _ in range(3))
    for val in (True, False):
        with pytest.raises(ValueError, match="decoupled_weight_decay"):
            FusedLamb([dict(params=[p0], decoupled_weight_decay=val)])
    with pytest.raises(TypeError):
        FusedLamb([p0], decoupled_weight_decay=True)
    opt = FusedLamb([dict(params=[p0], weight_decay=0.05), dict(params=[p1], always_adapt=True)], lr=3e-3)
    with pytest.raises(ValueError, match="decoupled_weight_decay"):
        opt.add_param_group(dict(params=[p2], decoupled_weight_decay=False))
    opt.add_param_group(dict(params=[p2]))
    assert isinstance(opt, FusedAdam) and opt.defaults["eps"] == 1e-6
    assert all("decoupled_weight_decay" not in g for g in opt.param_groups) and "decoupled_weight_decay" not in opt.defaults
    assert [g["always_adapt"] for g in opt.param_groups] == [False, True, False]
    tab = opt._group_array(2)
    assert tab.shape == (3, 10) and tab.view(np.int32)[:, 7].tolist() == [0, 2, 0]  # bit 1: always_adapt; bit 0 (decoupled) clear
    assert tab[0, 4] == np.float32(0.05) and tab[0, 8] == np.float32(1.0 - 0.9) and tab[0, 9] == np.float32(1.0 - 0.999)


def test_state_dict_round_trip_then_one_more_step():
    from pytorch_vit_paper_replication_amd.optim import FusedLamb

    def make():
        ps = _params(torch.float32)
        return ps, FusedLamb([dict(params=ps[:2], weight_decay=0.03), dict(params=ps[2:], always_adapt=True)], lr=1e-2)

    a, oa = make()
    for it in range(3):
        _set_grads(a, it, torch.float32)
        oa.step()
    b, ob = make()
    for it in range(2):
        _set_grads(b, it, torch.float32)
        ob.step()
    sd = ob.state_dict()
    assert sorted(sd["state"][0]) == ["exp_avg", "exp_avg_sq", "step"]
    c, oc = make()
    with torch.no_grad():
        for x, y in zip(c, b):
            x.copy_(y)
    oc.load_state_dict(sd)
    assert [g["always_adapt"] for g in oc.param_groups] == [False, True]
    _set_grads(c, 2, torch.float32)
    oc.step()
    for x, y in zip(a, c):
        assert torch.equal(x, y) and torch.equal(oa.state[x]["exp_avg_sq"], oc.state[y]["exp_avg_sq"])
    assert torch.equal(oa.last_trust, oc.last_trust)


CLI = ["--model", "vit_tiny_test", "--synthetic", "--epochs", "1", "--batch-size", "4", "--image-size", "32", "--num-classes", "3",
       "--synthetic-train-len", "8", "--synthetic-test-len", "4"]


@pytest.mark.parametrize("name", ["lamb", "adamw"])
def test_cli_optimizer_runs_one_synthetic_epoch(tmp_path, monkeypatch, name):
    from pytorch_vit_paper_replication_amd import engine
    from pytorch_vit_paper_replication_amd.cli.train import main
    from pytorch_vit_paper_replication_amd.optim import FusedAdam, FusedLamb

    seen = []
    orig = engine.train

    def spy(*a, **kw):
        seen.append(kw["optimizer"])
        return orig(*a, **kw)

    monkeypatch.setattr(engine, "train", spy)
    rc = main(CLI + ["--save-dir", str(tmp_path), "--save-name", "v.pth", "--optimizer", name, "--lr", "3e-3"])
    assert rc == 0 and (tmp_path / "v.pth").exists() and len(seen) == 1
    opt = seen[0]
    if name == "lamb":
        assert type(opt) is FusedLamb and opt.last_trust is not None and opt.step_count == 2
        assert [g["weight_decay"] for g in opt.param_groups] == [0.03, 0.0]
    else:
        assert type(opt) is FusedAdam and all(g["decoupled_weight_decay"] for g in opt.param_groups)


def test_cli_defaults_and_the_torch_optimizer_choices(tmp_path, monkeypatch):
    from pytorch_vit_paper_replication_amd import engine
    from pytorch_vit_paper_replication_amd.cli.train import build_parser, main

    a = build_parser().parse_args([])
    assert a.optimizer == "adam" and a.lr == 1e-3 and a.weight_decay == 0.03
    text = build_parser().format_help()
    assert "3e-3" in text and "0.02-0.05" in text
    with pytest.raises(SystemExit) as e:
        main(CLI + ["--save-dir", str(tmp_path), "--optimizer", "lamb", "--torch-optimizer"])
    assert e.value.code not in (0, None) and "lamb" in str(e.value.code)
    seen = []
    monkeypatch.setattr(engine, "train", lambda **kw: seen.append(kw["optimizer"]))
    assert main(CLI + ["--save-dir", str(tmp_path), "--optimizer", "adamw", "--torch-optimizer"]) == 0
    assert main(CLI + ["--save-dir", str(tmp_path), "--torch-optimizer"]) == 0
    assert [type(o) for o in seen] == [torch.optim.AdamW, torch.optim.Adam]


@pytest.mark.parametrize("betas", R.BETAS)
@pytest.mark.parametrize("wd,always", MODES)
def test_rounding_floors_hold_the_fp32_torch_ops_step(betas, wd, always):
    """The bounds the GPU tests grant the kernels (tests/lamb_reference.py lamb_rounding_floors) are worked out
    from operation counts; here the fp32 torch-ops step, the other fp32 evaluation at hand, stays inside
    them element by element over three steps, and the trust row inside its bounds."""
    from pytorch_vit_paper_replication_amd.optim import FusedLamb

    ps = _params(torch.float32)
    lr, eps = 1e-2, 1e-6
    opt = FusedLamb(ps, lr=lr, betas=betas, eps=eps, weight_decay=wd, always_adapt=always)
    for it in range(3):
        _set_grads(ps, it, torch.float32)
        st0 = [(p.detach().clone(), opt.state[p]["exp_avg"].clone() if it else torch.zeros_like(p),
                opt.state[p]["exp_avg_sq"].clone() if it else torch.zeros_like(p)) for p in ps]
        opt.step()
        row = R.group_row(lr, betas, eps, wd, it + 1, False)
        for k, p in enumerate(ps):
            p0, m0, v0 = st0[k]
            adapt = wd != 0 or always
            pr, mr, vr, wn, un, r = L.lamb_step64(p0, p.grad, m0, v0, row, adapt)
            fl, (wb, ub, rb) = L.lamb_rounding_floors(p0, p.grad, m0, v0, row, adapt)
            for name, got, ref in (("dp", p.detach().double() - p0.double(), pr - p0.double()), ("m", opt.state[p]["exp_avg"], mr),
                                   ("v", opt.state[p]["exp_avg_sq"], vr)):
                over = ((got.double() - ref).abs() - fl[name]).max()
                assert float(over) <= 0.0, f"step {it + 1} tensor {k} {name}: {float(over)} over its bound"
            tw, tu, tr = opt.last_trust[k].double().tolist()
            assert abs(tw - wn) <= wb * wn and abs(tu - un) <= ub * un and abs(tr - r) <= max(rb, 0.0) * r
