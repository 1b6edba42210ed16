"""Conditions on the inputs of tests/test_gpu_attn_regimes.py, proved on the CPU before any GPU figure
is trusted (tests/attn_reference.py):

* onehot really is one-hot, on every (batch, head) pair of every shape the GPU test runs, and the
  bf16-staged emulation then returns V[perm] and dO[perm^-1] bit for bit;
* ramp reaches both branches of the tiled forward's lazy rescale, under the documented rule;
* sharp and shift_* are what their names say;
* the emulation is a usable yardstick: finite, non-zero, well below 1 on every regime.
"""
import math

import pytest
import torch

from tests import attn_reference as AR

ALL_SHAPES = AR.SHAPES + AR.DBIAS_SHAPES + (AR.DET_SHAPE,) + AR.CLS_SHAPES
ONEHOT_SHAPES = sorted({s[1:] for s in ALL_SHAPES}) + [AR.HANDOFF_SHAPE[1:]]


@pytest.mark.parametrize("B,H,N,dh", ONEHOT_SHAPES)
def test_onehot_is_one_hot(B, H, N, dh):
    c = AR.make("onehot", B, N, H, dh)
    D = H * dh
    top, gap, peak = AR.row_stats(c.qkv, B, N, H)
    print(f"onehot B{B} H{H} N{N} dh{dh}: top >= {top.min().item():.17g}, gap >= {gap.min().item():.1f} nat, "
          f"score {peak.min().item():.1f}")
    assert top.min().item() >= 1 - 1e-12
    assert gap.min().item() >= 40.0
    # the matching key is perm[i]: K_perm[i] = Q_i, so its score is the row's largest
    s = AR.scores64(c.qkv, B, N, H)
    assert torch.equal(s.argmax(-1), c.perm)
    assert all(torch.equal(p.sort().values, torch.arange(N)) for p in c.perm)
    if B * H > 64:  # the pair hand-off case: the emulation at this size proves nothing new
        return
    e = AR.emulate(c.qkv, c.do, B, N, H)
    assert torch.equal(e.o, AR.gather_rows(c.qkv[:, 2 * D:], c.perm, B, N, H))
    assert torch.equal(e.dqkv[:, 2 * D:], AR.gather_rows(c.do, AR.inverse_perm(c.perm), B, N, H))


@pytest.mark.parametrize("N,dh,KT", [(577, 64, 64), (370, 64, 64), (257, 64, 64), (257, 80, 32), (272, 64, 64), (577, 80, 64)])
def test_ramp_reaches_both_branches_of_the_lazy_rescale(N, dh, KT):
    B, H = 2, 2
    c = AR.make("ramp", B, N, H, dh)
    grew, stale = AR.lazy_rescale_model(c.qkv, B, N, H, KT)
    f_grow = grew.float().mean().item()
    f_stale = ((~grew) & (stale >= 6.0)).float().mean().item()
    print(f"ramp N{N} dh{dh} KT{KT}: {f_grow:.2f} of (group, tile) pairs grow, {f_stale:.2f} take a stale max with "
          f"P >= 2^6, largest stale P 2^{stale.max().item():.2f}")
    assert f_grow >= 0.25
    assert f_stale >= 0.25
    assert stale.max().item() <= 8.0
    # the ramp itself: key N - 1 lies RAMP_LAST log2 units below key 0, the keys before it rise at RAMP_RATE
    s2 = AR.scores64(c.qkv, B, N, H).mean(1) * AR.LOG2E  # [BH, N]: mean over the queries
    # (each key's own noise term 0.3 u.n is 0.3 log2e = 0.43 log2 units at any dh: 4 sigma of a difference)
    assert ((s2[:, 0] - s2[:, N - 1]) - AR.RAMP_LAST).abs().max().item() < 2.5
    slope = (s2[:, N - 2] - s2[:, 0]) / (N - 2)
    assert (slope / AR.RAMP_RATE - 1).abs().max().item() < 0.1


@pytest.mark.parametrize("regime,peak_min", [("sharp", 30.0), ("shift_pos", 100.0), ("shift_neg", 100.0)])
@pytest.mark.parametrize("N,dh", [(197, 64), (257, 80)])
def test_regimes_are_what_their_names_say(regime, peak_min, N, dh):
    B, H = 2, 2
    c = AR.make(regime, B, N, H, dh)
    top, _, peak = AR.row_stats(c.qkv, B, N, H)
    s = AR.scores64(c.qkv, B, N, H)
    print(f"{regime} N{N} dh{dh}: median top probability {top.median().item():.3f}, peak |score| {peak.max().item():.1f} nat")
    assert 0.2 <= top.median().item() <= 0.95
    assert peak.max().item() >= peak_min
    if regime == "shift_pos":
        assert s.min().item() >= 100.0  # every score, not only the peak
    if regime == "shift_neg":
        assert s.max().item() <= -100.0


def test_uniform_and_gauss_baselines():
    B, H, N, dh = 2, 2, 197, 64
    u = AR.make("uniform", B, N, H, dh)
    r = AR.ref64(u.qkv, u.do, B, N, H)
    assert torch.equal(r.lse, torch.full_like(r.lse, math.log(N)))
    assert (r.dqkv[:, H * dh:2 * H * dh] == 0).all()
    top, _, peak = AR.row_stats(AR.make("gauss", B, N, H, dh).qkv, B, N, H)
    assert top.median().item() < 0.1 and peak.max().item() < 8.0


def test_ref64_matches_autograd_with_dropout():
    """The written-out float64 algebra against autograd of kernel_checks._attn_ref's formula."""
    B, H, N, dh, p = 2, 2, 33, 64, 0.25
    c = AR.make("sharp", B, N, H, dh)
    keep = torch.rand(B * H, N, N, generator=torch.Generator().manual_seed(3)) >= p
    r = AR.ref64(c.qkv, c.do, B, N, H, keep, p)
    x = c.qkv.double().requires_grad_(True)
    q, k, v = AR.split_heads(x, B, N, H)
    s = (q @ k.transpose(-1, -2)) / math.sqrt(dh)
    pr = torch.softmax(s, -1) * keep.view(B, H, N, N).double() * AR.drop_factor(p)
    o = AR.merge_heads(pr @ v)
    o.backward(c.do.double())
    torch.testing.assert_close(r.o, o.detach(), rtol=1e-12, atol=1e-13)
    torch.testing.assert_close(r.lse, torch.logsumexp(s, -1).reshape(B * H, N).detach(), rtol=1e-13, atol=0)
    torch.testing.assert_close(r.dqkv, x.grad, rtol=1e-11, atol=1e-12)


def test_figures():
    ref = torch.zeros(8, 128, dtype=torch.float64)
    ref[:, :] = 1.0
    out = ref.clone()
    out[3, 64:] = 0.0  # one head-slice row of 16 wrong in full
    l2, row = AR.figures(out, ref, 64)
    assert l2 == pytest.approx(0.25) and row == pytest.approx(1.0)
    ref[5, :64] = 1e-3  # a small row: its error counts against the mean row, not against itself
    out = ref.clone()
    out[5, :64] = 2e-3
    l2, row = AR.figures(out, ref, 64)
    assert row == pytest.approx(1e-3 * 8 / ref.reshape(-1, 64).norm(dim=1).mean().item(), rel=1e-6)
    z = torch.zeros(4, 64)
    e = z.clone()
    e[1, 0] = 3e-4
    assert AR.figures(e, z, 64) == (pytest.approx(3e-4), pytest.approx(3e-4))  # zero reference: absolute


@pytest.mark.parametrize("regime", AR.REGIMES)
@pytest.mark.parametrize("N,dh", [(197, 64), (257, 80)])
def test_emulation_is_a_usable_yardstick(regime, N, dh):
    B, H = 2, 2
    D = H * dh
    c = AR.make(regime, B, N, H, dh)
    r, e = AR.ref64(c.qkv, c.do, B, N, H), AR.emulate(c.qkv, c.do, B, N, H)
    figs = {"O": AR.figures(e.o, r.o, dh)}
    for i, name in enumerate(("dQ", "dK", "dV")):
        figs[name] = AR.figures(e.dqkv[:, i * D:(i + 1) * D], r.dqkv[:, i * D:(i + 1) * D], dh)
    print(f"{regime} N{N} dh{dh}: " + " ".join(f"{k} l2={a:.2e} row={b:.2e}" for k, (a, b) in figs.items()))
    exact = {"onehot": ("O", "dV"), "uniform": ("dK",)}.get(regime, ())  # bit-exact by construction
    for k, (a, b) in figs.items():
        assert math.isfinite(a) and math.isfinite(b)
        assert a < 0.2 and b < 0.2
        if k in exact:
            assert a == 0 and b == 0
        elif regime != "onehot":  # onehot dQ, dK: the reference is zero, the emulation's 1e-6 is absolute
            assert a > 0 and b > 0
    _, _, peak = AR.row_stats(c.qkv, B, N, H)
    assert ((e.lse.double() - r.lse).abs() <= 4e-7 * peak.clamp_min(1.0)).all()
