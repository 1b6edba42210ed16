"""LayerScale on the GPU: the fold / unfold kernels (csrc/layerscale.hip) on raw buffers, and the fused model against the
plain model that holds its folded weights.

Let ``M`` be a LayerScale model and ``P`` the plain model loaded with ``M.folded_state_dict()``. The fold makes most
checks exact (same dropout counter, same batch, deterministic mode):

* forward: ``M``'s folded bf16 weights are the bf16 shadows of ``P``'s, bit for bit, and so are the biases: logits and
  loss are bit-identical for any scale;
* backward: every gradient except those of the four scaled tensors per block is bit-identical; ``gW_M == g[:, None] *
  gW_P`` and ``gb_M == g * gb_P`` bit for bit from a zeroed buffer (one fp32 multiply, then ``0 + x``);
* the scale's gradient is ``sum_j gW_P[i][j] W[i][j] + gb_P[i] b[i]``: compared against float64 of that expression, each
  figure of ``errs64`` (relative L2, max error over max) within ``max(4 x fp32 torch's error on the same inputs, 5e-7)``,
  the project's rule for fp32 kernels against float64 (tests/test_gpu_bce_loss.py)."""
import os

import pytest
import torch

from tests.test_layer_scale_cpu import randomise_scales

pytestmark = pytest.mark.gpu

DEV = "cuda"
FLOOR, FACTOR = 5e-7, 4.0
SHAPES = [(8, 8), (64, 72), (136, 264), (256, 1032)]  # below one tile, across tile edges, > one trip of a 256-thread row loop


def _E():
    from pytorch_vit_paper_replication_amd import _ext

    return _ext


def _kc():
    from tests import kernel_checks as KC

    return KC


def _within(name, got, ref64, yard):
    """The 4x rule: ``errs64(got)`` against ``max(4 x errs64(yard), 5e-7)`` per figure; prints, then asserts."""
    KC = _kc()
    e, y = KC.errs64(got, ref64), KC.errs64(yard, ref64)
    lim = tuple(max(FACTOR * v, FLOOR) for v in y)
    print(f"{name}: rel-L2 {e[0]:.3e} (limit {lim[0]:.3e}), max/max {e[1]:.3e} (limit {lim[1]:.3e}); fp32 torch {y[0]:.3e} {y[1]:.3e}")
    assert e[0] <= lim[0] and e[1] <= lim[1], (name, e, lim)


def _scale_vector(R, gen):
    """Signs, exact zeros, 1e-4-scale values, +-1 and a large one."""
    g = torch.randn(R, generator=gen) * 1e-4
    g[::5] = 0.0
    g[1::7] = 1.0
    g[2::9] = -1.0
    g[3::11] = -3.7
    return g


# ----------------------------------------------------------------------------- fold
def _fold_table(shapes, gen):
    """A master buffer holding (W, g, b) of every shape at offsets that are multiples of 8 (with gaps), the table, the
    output sizes, and the per-matrix tensors."""
    parts, rows, off, ooff, boff, tiles = [], [], 0, 0, 0, 0
    mats = []
    for R, C in shapes:
        W, g, b = torch.randn(R, C, generator=gen), _scale_vector(R, gen), torch.randn(R, generator=gen)
        woff, goff, bo = off, off + R * C + 8, off + R * C + 8 + R + 3  # g at a multiple of 8, b at an odd offset
        end = bo + R
        buf = torch.full((end - off,), 7.0)
        buf[:R * C] = W.reshape(-1)
        buf[goff - off:goff - off + R] = g
        buf[bo - off:bo - off + R] = b
        parts.append(buf)
        rows.append([woff, goff, bo, R, C, ooff, boff, tiles])
        mats.append((W, g, b))
        tiles += ((R + 63) // 64) * ((C + 63) // 64)
        off = (end + 63) // 64 * 64
        parts.append(torch.full((off - end,), 7.0))
        ooff += (R * C + 63) // 64 * 64 + 64  # a gap after every output
        boff += R + 5
    return torch.cat(parts), torch.tensor(rows, dtype=torch.int64), ooff, boff, mats


def _run_fold(shapes, seed):
    gen = torch.Generator().manual_seed(seed)
    master, meta, n16, nb, mats = _fold_table(shapes, gen)
    master = master.to(DEV)
    w16 = torch.full((n16,), -5.0, dtype=torch.bfloat16, device=DEV)
    wt16 = torch.full((n16,), -5.0, dtype=torch.bfloat16, device=DEV)
    bhat = torch.full((nb,), -5.0, device=DEV)
    _E().ext().layerscale_fold(master, w16, wt16, bhat, meta.to(DEV), meta)
    torch.cuda.synchronize()
    seen16 = torch.zeros(n16, dtype=torch.bool)
    seenb = torch.zeros(nb, dtype=torch.bool)
    for (W, g, b), row in zip(mats, meta.tolist()):
        R, C, o, bo = row[3], row[4], row[5], row[6]
        W, g, b = W.to(DEV), g.to(DEV), b.to(DEV)
        want = (g[:, None].float() * W).to(torch.bfloat16)
        assert torch.equal(w16[o:o + R * C].view(R, C), want), (R, C)
        assert torch.equal(wt16[o:o + R * C].view(C, R), want.t()), (R, C)
        assert torch.equal(bhat[bo:bo + R], g * b), (R, C)
        seen16[o:o + R * C] = True
        seenb[bo:bo + R] = True
    # nothing outside the outputs was written (edge tiles are bounds-checked)
    assert (w16.cpu()[~seen16] == -5.0).all() and (wt16.cpu()[~seen16] == -5.0).all() and (bhat.cpu()[~seenb] == -5.0).all()
    assert (master.cpu()[0] == mats[0][0][0, 0]).item()  # the master is read only


@pytest.mark.parametrize("R,C", SHAPES)
def test_fold_is_bit_exact(R, C):
    _run_fold([(R, C)], seed=R + C)


def test_fold_batched_over_a_table():
    _run_fold(SHAPES + [(72, 64), (8, 136)], seed=3)


def test_fold_rounds_the_product_once_then_to_bf16():
    """Values chosen so that a product kept wider than fp32 (or a different rounding) would show: g and W with full
    24-bit mantissas."""
    gen = torch.Generator().manual_seed(11)
    R, C = 64, 64
    W = (torch.rand(R, C, generator=gen) + 1.0)
    g = (torch.rand(R, generator=gen) + 1.0)
    b = torch.rand(R, generator=gen) + 1.0
    master = torch.cat([W.reshape(-1), g, b]).to(DEV)
    meta = torch.tensor([[0, R * C, R * C + R, R, C, 0, 0, 0]], dtype=torch.int64)
    w16 = torch.empty(R * C, dtype=torch.bfloat16, device=DEV)
    wt16 = torch.empty_like(w16)
    bhat = torch.empty(R, device=DEV)
    _E().ext().layerscale_fold(master, w16, wt16, bhat, meta.to(DEV), meta)
    p64 = g.double()[:, None] * W.double()
    want = p64.float().to(torch.bfloat16)  # fl32 of the exact product (48 bits fit a double), then RNE to bf16
    assert torch.equal(w16.view(R, C).cpu(), want)
    assert torch.equal(bhat.cpu(), (g.double() * b.double()).float())


def test_fold_host_checks():
    ext = _E().ext()
    R, C = 16, 16
    master = torch.zeros(R * C + 2 * R, device=DEV)
    w16 = torch.zeros(R * C, dtype=torch.bfloat16, device=DEV)
    wt16 = torch.zeros_like(w16)
    bhat = torch.zeros(R, device=DEV)
    row = [0, R * C, R * C + R, R, C, 0, 0, 0]

    def call(r=row, **kw):
        a = dict(master=master, w16=w16, wt16=wt16, bhat=bhat)
        a.update(kw)
        meta = torch.tensor([r], dtype=torch.int64)
        ext.layerscale_fold(a["master"], a["w16"], a["wt16"], a["bhat"], a.get("meta", meta.to(DEV)), a.get("meta_host", meta))

    call()  # the valid call
    for bad in ([0, R * C, R * C + R, 12, C, 0, 0, 0], [0, R * C, R * C + R, R, 20, 0, 0, 0],  # R, C % 8
                [4, R * C, R * C + R, R, C, 0, 0, 0], [0, R * C, R * C + R, R, C, 4, 0, 0],  # offsets % 8
                [64, R * C, R * C + R, R, C, 0, 0, 0], [0, R * C + R + 8, R * C + R, R, C, 0, 0, 0],  # reads outside master
                [0, R * C, R * C + R, R, C, 8, 0, 0], [0, R * C, R * C + R, R, C, 0, 8, 0],  # writes outside the outputs
                [0, R * C, R * C + R, R, C, 0, 0, 1], [-8, R * C, R * C + R, R, C, 0, 0, 0]):  # tile prefix, negative
        with pytest.raises(RuntimeError, match="layerscale_fold"):
            call(bad)
    with pytest.raises(RuntimeError, match="bfloat16"):
        call(w16=torch.zeros(R * C, device=DEV))
    with pytest.raises(RuntimeError, match="float32"):
        call(master=torch.zeros(R * C + 2 * R, dtype=torch.float64, device=DEV))
    with pytest.raises(RuntimeError, match="GPU"):
        call(master=torch.zeros(R * C + 2 * R))
    with pytest.raises(RuntimeError, match="meta_host"):
        call(meta_host=torch.tensor([row, row], dtype=torch.int64))
    with pytest.raises(RuntimeError, match="two buffers"):
        call(wt16=w16)
    with pytest.raises(RuntimeError, match="contiguous"):
        call(w16=torch.zeros(2 * R * C, dtype=torch.bfloat16, device=DEV)[::2])


# ----------------------------------------------------------------------------- unfold
def _unfold_inputs(R, C, seed, offset=0):
    """(dw_hat, db_hat, W, b, g) on the GPU; ``offset`` elements into their storages (1: rows not 16-byte aligned)."""
    gen = torch.Generator().manual_seed(seed)

    def dev(t):
        buf = torch.empty(t.numel() + offset, device=DEV)
        v = buf[offset:].view(t.shape)
        v.copy_(t)
        return v

    return (dev(torch.randn(R, C, generator=gen) * 1e-3), dev(torch.randn(R, generator=gen) * 1e-2), dev(torch.randn(R, C, generator=gen)),
            dev(torch.randn(R, generator=gen)), dev(_scale_vector(R, gen)))


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("R,C", SHAPES)
def test_unfold_exact_products_and_the_scale_gradient(R, C, offset):
    ext = _E().ext()
    dwh, dbh, W, b, g = _unfold_inputs(R, C, R * 7 + C, offset)
    gen = torch.Generator().manual_seed(99)
    ref64 = (dwh.double() * W.double()).sum(1) + dbh.double() * b.double()
    yard = (dwh * W).sum(1) + dbh * b
    for zero in (True, False):  # from a zeroed buffer, and accumulated into a gradient that is already there
        def start(shape):
            t = torch.zeros(shape) if zero else torch.randn(shape, generator=gen) * 1e-3
            buf = torch.empty(t.numel() + offset, device=DEV)
            v = buf[offset:].view(shape)
            v.copy_(t)
            return v

        gW, gb, gg = start((R, C)), start((R,)), start((R,))
        gW0, gb0, gg0 = gW.clone(), gb.clone(), gg.clone()
        ext.layerscale_unfold(dwh, dbh, W, b, g, gW=gW, gb=gb, gg=gg)
        # one fp32 multiply rounded on its own, then one add: torch's two separate ops, bit for bit
        assert torch.equal(gW, gW0 + g[:, None] * dwh)
        assert torch.equal(gb, gb0 + g * dbh)
        _within(f"unfold {R}x{C} offset {offset} {'zeroed' if zero else 'accumulate'}: scale gradient", gg, gg0.double() + ref64, gg0 + yard)
        # null destinations: each alone gives the bits of the full call and leaves the inputs alone
        for which in range(3):
            d = [gW0.clone(), gb0.clone(), gg0.clone()]
            kw = {("gW", "gb", "gg")[which]: d[which]}
            ext.layerscale_unfold(dwh, dbh, W, b, g, **kw)
            assert torch.equal(d[which], (gW, gb, gg)[which]), which
    ext.layerscale_unfold(dwh, dbh, W, b, g)  # nothing to do: no launch, no error
    # g = 0 rows: nothing divides by g, the scale still gets its gradient
    z = (g == 0)
    assert z.any() and (gW[z] == gW0[z]).all() and torch.isfinite(gg).all() and (gg[z] != gg0[z]).any()


def test_unfold_is_deterministic():
    ext = _E().ext()
    dwh, dbh, W, b, g = _unfold_inputs(256, 1032, 5)
    outs = []
    for _ in range(2):
        gg = torch.zeros(256, device=DEV)
        ext.layerscale_unfold(dwh, dbh, W, b, g, gg=gg)
        outs.append(gg)
    assert torch.equal(outs[0], outs[1])


def test_unfold_host_checks():
    ext = _E().ext()
    dwh, dbh, W, b, g = _unfold_inputs(16, 24, 1)
    gW = torch.zeros(16, 24, device=DEV)
    ext.layerscale_unfold(dwh, dbh, W, b, g, gW=gW)
    with pytest.raises(RuntimeError, match="multiples of 8"):
        ext.layerscale_unfold(dwh[:, :20].contiguous(), dbh, W[:, :20].contiguous(), b, g)
    with pytest.raises(RuntimeError, match="multiples of 8"):
        ext.layerscale_unfold(dwh[:12].contiguous(), dbh[:12].contiguous(), W[:12].contiguous(), b[:12].contiguous(), g[:12].contiguous())
    with pytest.raises(RuntimeError, match="dw_hat"):
        ext.layerscale_unfold(dwh[:8].contiguous(), dbh, W, b, g, gW=gW)
    with pytest.raises(RuntimeError, match="db_hat"):
        ext.layerscale_unfold(dwh, dbh[:8].contiguous(), W, b, g, gW=gW)
    with pytest.raises(RuntimeError, match="contiguous"):
        ext.layerscale_unfold(dwh, dbh, W.t().contiguous().t(), b, g, gW=gW)
    with pytest.raises(RuntimeError, match="gW"):
        ext.layerscale_unfold(dwh, dbh, W, b, g, gW=torch.zeros(16, 32, device=DEV)[:, :24])
    with pytest.raises(RuntimeError, match="float32"):
        ext.layerscale_unfold(dwh, dbh, W, b, g.double(), gW=gW)
    with pytest.raises(RuntimeError, match="float32"):
        ext.layerscale_unfold(dwh, dbh, W, b, g, gg=torch.zeros(16, dtype=torch.float64, device=DEV))
    with pytest.raises(RuntimeError, match="GPU"):
        ext.layerscale_unfold(dwh, dbh, W, b.cpu(), g, gW=gW)
    with pytest.raises(RuntimeError, match="GPU"):
        ext.layerscale_unfold(dwh, dbh, W, b, g, gb=torch.zeros(16))
    assert (gW == g[:, None] * dwh).all()  # the refused calls launched nothing


# ----------------------------------------------------------------------------- whole model: M against P
# the configuration of tests/test_gpu_drop_path.py / tests/test_gpu_cls_last_block.py
CFG = dict(image_size=32, patch_size=8, num_heads=2, embedding_dim=128, mlp_size=256, num_classes=10,
           mlp_dropout=0.1, embedding_dropout=0.1)
# 16 x 257 = 4112 tokens, D 256: the out-projection and fc2 weight gradients take the split-K path (tile 12)
CFG_SPLITK = dict(image_size=64, patch_size=4, num_heads=4, embedding_dim=256, mlp_size=512, num_classes=10,
                  mlp_dropout=0.1, embedding_dropout=0.1)


def _make_pair(cfg, depth, scales, seed, drop_path=0.0, patch_dropout=0.0):
    """(M, P): a LayerScale model with random scales (``"small"``: in [-2e-4, 2e-4] with exact zeros; ``"ones"``) and the
    plain model that holds its folded weights; both with the same options."""
    from pytorch_vit_paper_replication_amd.models import ViT

    torch.manual_seed(seed)
    cfg = dict(cfg, num_transformer_layer=depth)
    M = ViT(**cfg).set_layer_scale(1e-4)
    randomise_scales(M, -2e-4, 2e-4, zeros=5, seed=seed)
    if scales == "ones":
        with torch.no_grad():
            for blk in M.transformer_encoder:
                blk.layer_scale_1.fill_(1.0)
                blk.layer_scale_2.fill_(1.0)
    M = M.to(DEV)
    P = ViT(**cfg).to(DEV)
    P.load_state_dict(M.folded_state_dict())
    for m in (M, P):
        if drop_path:
            m.set_drop_path(drop_path, "constant")
        if patch_dropout:
            m.set_patch_dropout(patch_dropout)
    return M, P


def _scaled_names(M):
    out = {}
    for i, blk in enumerate(M.transformer_encoder):
        for (w, b, g), name, k in zip(blk.folded_triples(), (f"transformer_encoder.{i}.msa_block.multi_head_attention.out_proj",
                                                               f"transformer_encoder.{i}.mlp_block.mlp.3"), (1, 2)):
            out[name] = (w, b, g, f"transformer_encoder.{i}.layer_scale_{k}")
    return out


def _steps(M, P, x, y, cls_on, counter=31337):
    from tests import test_gpu_cls_last_block as CL

    for m in (M, P):
        m._dropout_seed(x.device)
        m._pvr_rng.fill_(counter)
    rng0 = M._pvr_rng.clone()
    return CL._fused_step(M, x, y, rng0, cls_on), CL._fused_step(P, x, y, rng0, cls_on)


def _check_identities(M, rm, rp, tag):
    (loss_m, logits_m, gm, rows_m), (loss_p, logits_p, gp, rows_p) = rm, rp
    assert rows_m == rows_p  # the same GEMMs ran
    assert torch.equal(logits_m, logits_p) and torch.equal(loss_m, loss_p), tag
    scaled = _scaled_names(M)
    skip = {n + s for n in scaled for s in (".weight", ".bias")}
    assert len(gp) == len(gm) - len(scaled)
    for n, v in gp.items():
        if n not in skip:
            assert torch.equal(gm[n], v), (tag, n)
    for name, (w, b, g, gname) in scaled.items():
        gd = g.detach()
        dwh, dbh = gp[name + ".weight"], gp[name + ".bias"]
        assert dwh.abs().max() > 0 and dbh.abs().max() > 0
        assert torch.equal(gm[name + ".weight"], gd[:, None] * dwh), (tag, name)
        assert torch.equal(gm[name + ".bias"], gd * dbh), (tag, name)
        ref64 = (dwh.double() * w.detach().double()).sum(1) + dbh.double() * b.detach().double()
        yard = (dwh * w.detach()).sum(1) + dbh * b.detach()
        _within(f"{tag} {gname}", gm[gname], ref64, yard)


CASES = {
    # name: (cfg, depth, scales, batch, class-token last block, drop path, patch dropout)
    "depth2_small": (CFG, 2, "small", 8, True, 0.0, 0.0),
    "depth3_small_drop_path_patch_dropout": (CFG, 3, "small", 8, True, 0.3, 0.25),
    "depth2_ones": (CFG, 2, "ones", 8, True, 0.0, 0.0),
    "depth3_small_full_last_block": (CFG, 3, "small", 8, False, 0.0, 0.0),
    "depth2_ones_full_last_block_drop_path": (CFG, 2, "ones", 5, False, 0.3, 0.0),
    "depth2_small_split_k": (CFG_SPLITK, 2, "small", 16, False, 0.0, 0.0),
}


@pytest.mark.parametrize("case", list(CASES))
def test_training_step_identities_against_the_folded_plain_model(case):
    from pytorch_vit_paper_replication_amd.ops import gemm

    cfg, depth, scales, B, cls_on, dp, pd = CASES[case]
    M, P = _make_pair(cfg, depth, scales, seed=len(case), drop_path=dp, patch_dropout=pd)
    S = cfg["image_size"]
    x = torch.rand(B, 3, S, S, device=DEV)
    y = torch.randint(0, 10, (B,), device=DEV)
    assert M._fused_supported(x)
    D, Mlp = cfg["embedding_dim"], cfg["mlp_size"]
    T = B * ((S // cfg["patch_size"]) ** 2 + 1)
    tiles = (gemm._tile(D, D, T, "wgrad"), gemm._tile(D, Mlp, T, "wgrad"))
    assert tiles == ((12, 12) if cfg is CFG_SPLITK else (0, 0))  # the split-K path / the atomic path
    rm, rp = _steps(M, P, x, y, cls_on)
    if cls_on:  # the class-token block ran: its fc2 / fc1 / out dgrads have B rows
        assert [r[1] for r in rm[3][:3]] == [B, B, B]
    _check_identities(M, rm, rp, case)
    # the option does something: with scales other than one the logits are not those of the unscaled weights
    if scales == "small":
        from pytorch_vit_paper_replication_amd.models import ViT

        U = ViT(**dict(cfg, num_transformer_layer=depth)).to(DEV)
        U.load_state_dict({k: v for k, v in M.state_dict().items() if ".layer_scale_" not in k})
        U.eval()
        M.eval()
        with torch.inference_mode():
            assert not torch.equal(U(x), M(x))


def test_no_classifier_backbone_features_match_the_folded_plain_model():
    from pytorch_vit_paper_replication_amd.models.vit_no_classifier import ViT as ViTNoClassifier

    torch.manual_seed(3)
    cfg = {k: v for k, v in CFG.items() if k != "num_classes"}
    M = randomise_scales(ViTNoClassifier(**cfg, num_transformer_layer=2).set_layer_scale(1e-4), -2e-4, 2e-4, zeros=5).to(DEV)
    P = ViTNoClassifier(**cfg, num_transformer_layer=2).to(DEV)
    P.load_state_dict(M.folded_state_dict())
    x = torch.rand(4, 3, 32, 32, device=DEV)
    outs = []
    with _E().deterministic_mode():
        for m in (M, P):
            m._dropout_seed(x.device)
            m._pvr_rng.fill_(777)
            m.train()
            f = m(x)
            f.square().mean().backward()
            outs.append((f.detach().clone(), {n: p.grad.detach().clone() for n, p in m.named_parameters()}))
    torch.cuda.synchronize()
    assert torch.equal(outs[0][0], outs[1][0])
    skip = {n + s for n in _scaled_names(M) for s in (".weight", ".bias")}
    assert all(torch.equal(outs[0][1][n], v) for n, v in outs[1][1].items() if n not in skip)
    for name, (w, b, g, gname) in _scaled_names(M).items():
        assert torch.equal(outs[0][1][name + ".weight"], g.detach()[:, None] * outs[1][1][name + ".weight"])
        assert outs[0][1][gname].abs().max() > 0


def test_two_backwards_accumulate():
    """No ``zero_grad`` between two backwards of the same step (same counter value, deterministic mode): the unfold adds
    the same products a second time. Each tensor it writes takes one add per backward, ``d`` then ``d + d``, so the bound,
    2 ulp of the sum, has room to spare; the tensors checked are those the unfold writes."""
    from pytorch_vit_paper_replication_amd.ops import fused_vit

    M, _ = _make_pair(CFG, 2, "small", seed=21)
    x = torch.rand(8, 3, 32, 32, device=DEV)
    y = torch.randint(0, 10, (8,), device=DEV)
    M._dropout_seed(x.device)
    M.train()

    def backward_once():
        M._pvr_rng.fill_(4242)
        fused_vit.cross_entropy(M(x), y).backward()

    with _E().deterministic_mode():
        M.zero_grad(set_to_none=True)
        backward_once()
        torch.cuda.synchronize()
        one = {n: p.grad.detach().clone() for n, p in M.named_parameters()}
        M.zero_grad(set_to_none=True)
        backward_once()
        backward_once()
        torch.cuda.synchronize()
    names = [n + s for n in _scaled_names(M) for s in (".weight", ".bias")] + [v[3] for v in _scaled_names(M).values()]
    for n in names:
        two, want = dict(M.named_parameters())[n].grad, 2.0 * one[n]
        ulp = torch.nextafter(want.abs(), torch.full_like(want, float("inf"))) - want.abs()
        assert one[n].abs().max() > 0 and ((two - want).abs() <= 2.0 * ulp).all(), n


def _eval_logits(m, x):
    m.eval()
    with torch.inference_mode():
        out = m(x).clone()
    torch.cuda.synchronize()
    return out


def _fresh_plain(M, cfg, depth, sd=None):
    from pytorch_vit_paper_replication_amd.models import ViT

    P = ViT(**dict(cfg, num_transformer_layer=depth)).to(DEV)
    P.load_state_dict(M.folded_state_dict() if sd is None else sd)
    return P


@pytest.mark.parametrize("which", ["adam", "lamb"])
def test_optimizer_steps_move_the_scales_and_the_fold_follows(which):
    """Three FusedAdam steps (one FusedLamb step) change ``layer_scale_*``; the next forward equals a fresh plain model built
    from the updated weights, so the folded copies were rebuilt when the store's generation moved, and two evaluation
    forwards in a row launch no fold."""
    from pytorch_vit_paper_replication_amd.ops import fused_vit
    from pytorch_vit_paper_replication_amd.optim import FusedAdam, FusedLamb, param_groups_weight_decay

    M, _ = _make_pair(CFG, 2, "small", seed=33)
    before = {n: p.detach().clone() for n, p in M.named_parameters()}
    opt = (FusedAdam if which == "adam" else FusedLamb)(param_groups_weight_decay(M, 0.03), lr=1e-3)
    x = torch.rand(8, 3, 32, 32, device=DEV)
    y = torch.randint(0, 10, (8,), device=DEV)
    for _ in range(3 if which == "adam" else 1):
        M.train()
        loss = fused_vit.cross_entropy(M(x), y)
        opt.zero_grad()
        loss.backward()
        opt.step()
    torch.cuda.synchronize()
    for n, p in M.named_parameters():
        assert torch.isfinite(p).all(), n
        if ".layer_scale_" in n:
            assert not torch.equal(p, before[n]), n
    st = M._pvr_store
    assert st._f_generation != st.generation  # the optimizer moved the generation: the next forward folds
    a = _eval_logits(M, x)
    gen = st._f_generation
    assert gen == st.generation
    assert torch.equal(a, _eval_logits(_fresh_plain(M, CFG, 2), x))
    assert torch.equal(a, _eval_logits(M, x)) and st._f_generation == gen == st.generation  # no fold between evaluation forwards


def test_model_ema_applied_computes_with_the_folded_average():
    from pytorch_vit_paper_replication_amd.models import ViT
    from pytorch_vit_paper_replication_amd.ops import fused_vit
    from pytorch_vit_paper_replication_amd.optim import FusedAdam, ModelEma

    M, _ = _make_pair(CFG, 2, "small", seed=44)
    opt = FusedAdam(M.parameters(), lr=1e-3)
    ema = ModelEma(M, decay=0.5).attach(opt)
    x = torch.rand(8, 3, 32, 32, device=DEV)
    y = torch.randint(0, 10, (8,), device=DEV)
    for _ in range(2):
        M.train()
        loss = fused_vit.cross_entropy(M(x), y)
        opt.zero_grad()
        loss.backward()
        opt.step()
    trained = _eval_logits(M, x)
    E = ViT(**dict(CFG, num_transformer_layer=2)).set_layer_scale(0.0).to(DEV)
    E.load_state_dict(ema.state_dict())
    assert not torch.equal(E.transformer_encoder[0].layer_scale_1, M.transformer_encoder[0].layer_scale_1)
    want = _eval_logits(_fresh_plain(E, CFG, 2), x)
    with ema.applied():
        inside = _eval_logits(M, x)
    assert torch.equal(inside, want) and not torch.equal(inside, trained)
    assert torch.equal(_eval_logits(M, x), trained)  # the trained weights are back, and so is their fold


def test_frozen_parameters_skip_their_destinations():
    """``feature_extractor`` (frozen backbone): the step runs and leaves ``layer_scale_*.grad`` untouched. With only the
    out-projection weight of block 0 frozen its scale still gets the gradient it gets otherwise, bit for bit."""
    from pytorch_vit_paper_replication_amd.models.transfer import feature_extractor
    from pytorch_vit_paper_replication_amd.ops import fused_vit

    x = torch.rand(8, 3, 32, 32, device=DEV)
    y = torch.randint(0, 3, (8,), device=DEV)
    M, _ = _make_pair(CFG, 2, "small", seed=55)
    M = feature_extractor(M, 3, seed=0)
    M.train()
    fused_vit.cross_entropy(M(x), y).backward()
    torch.cuda.synchronize()
    st = M._pvr_store
    for blk in M.transformer_encoder:
        for p in (blk.layer_scale_1, blk.layer_scale_2):
            assert p.grad is None and not p.requires_grad
            assert (st._gviews[st._index[id(p)]] == 0).all()
    assert M.classifier[0].weight.grad.abs().max() > 0

    M, _ = _make_pair(CFG, 2, "small", seed=56)
    y = torch.randint(0, 10, (8,), device=DEV)
    M._dropout_seed(x.device)
    grads = []
    for freeze in (False, True):
        w = M.transformer_encoder[0].msa_block.multi_head_attention.out_proj.weight
        w.requires_grad = not freeze
        with _E().deterministic_mode():
            M._pvr_rng.fill_(99)
            M.train()
            M.zero_grad(set_to_none=True)
            fused_vit.cross_entropy(M(x), y).backward()
        torch.cuda.synchronize()
        grads.append({n: (None if p.grad is None else p.grad.detach().clone()) for n, p in M.named_parameters()})
    name = "transformer_encoder.0.msa_block.multi_head_attention.out_proj.weight"
    assert grads[0][name] is not None and grads[1][name] is None
    for n, v in grads[0].items():
        if n != name:
            assert torch.equal(v, grads[1][n]), n


TRAIN_CFG = dict(image_size=64, patch_size=16, num_transformer_layer=2, num_heads=2, embedding_dim=128, mlp_size=256,
                 num_classes=10, mlp_dropout=0.1, embedding_dropout=0.1)


def test_resume_is_bit_exact_with_layer_scale(tmp_path):
    from pytorch_vit_paper_replication_amd.models import ViT
    from pytorch_vit_paper_replication_amd.ops.fused_vit import cross_entropy
    from pytorch_vit_paper_replication_amd.optim import FusedAdam, param_groups_weight_decay, warmup_linear_decay
    from pytorch_vit_paper_replication_amd.utils.checkpoint import load_checkpoint, save_checkpoint
    from tests.test_gpu_train import _resume_check

    xs = [torch.rand(8, 3, 64, 64, device=DEV) for _ in range(4)]
    ys = [torch.randint(0, 10, (8,), device=DEV) for _ in range(4)]

    def make(seed):
        torch.manual_seed(seed)
        m = ViT(**TRAIN_CFG).set_layer_scale(1e-4).to(DEV)
        o = FusedAdam(param_groups_weight_decay(m, 0.03), lr=1e-3)
        return m, o, warmup_linear_decay(o, 10, 0.2)

    def run(m, o, s, steps):
        losses = []
        for i in steps:
            m.train()
            loss = cross_entropy(m(xs[i]), ys[i])
            o.zero_grad()
            loss.backward()
            o.step(clip_norm=1.0)
            s.step()
            losses.append(loss.detach().clone())
        torch.cuda.synchronize()
        return losses

    with _E().deterministic_mode():
        _resume_check(make, run, False, tmp_path, save_checkpoint, load_checkpoint)


def _ddp_cfg():
    return dict(TRAIN_CFG, mlp_dropout=0.0, embedding_dropout=0.0)


def _ddp_model(seed):
    from pytorch_vit_paper_replication_amd.models import ViT

    torch.manual_seed(seed)
    return randomise_scales(ViT(**_ddp_cfg()).set_layer_scale(1e-4), -2e-4, 2e-4, zeros=5, seed=seed)


def _gloo_layer_scale_worker(rank, world, port, out_dir):
    """One rank of a 2-process DDP run whose ranks share cuda:0 (gloo carries the gradients), the pattern of
    tests/test_gpu_train._gloo_gpu_worker, with LayerScale and two FusedAdam steps."""
    import torch.distributed as dist

    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    from pytorch_vit_paper_replication_amd.ops.fused_vit import cross_entropy
    from pytorch_vit_paper_replication_amd.optim import FusedAdam
    from pytorch_vit_paper_replication_amd.parallel import DistributedDataParallel

    m = _ddp_model(100 + rank).to(dev)  # different init per rank: the rank-0 broadcast must fix it
    ddp = DistributedDataParallel(m, bucket_cap_mb=0.1)
    # (rank 0's values: the wrapper broadcasts them to every rank at its first forward)
    init = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    opt = FusedAdam(m.parameters(), lr=1e-3)
    g = torch.Generator().manual_seed(7)
    x = torch.rand(4 * world, 3, 64, 64, generator=g)
    y = torch.randint(0, 10, (4 * world,), generator=g)
    xs, ys = x[4 * rank:4 * rank + 4].to(dev), y[4 * rank:4 * rank + 4].to(dev)
    main = torch.cuda.Stream(device=dev, priority=-1)
    main.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(main):
        for _ in range(2):  # the second step re-arms the buckets
            loss = cross_entropy(ddp(xs), ys)
            opt.zero_grad()
            loss.backward()
            opt.step()
    torch.cuda.synchronize()
    torch.save({"init": init, "state": {k: v.detach().cpu().clone() for k, v in m.state_dict().items()},
                "nbuckets": len(ddp._buckets), "x": x, "y": y}, os.path.join(out_dir, f"ls{rank}.pt"))
    dist.destroy_process_group()


def test_ddp_two_ranks_with_layer_scale(tmp_path):
    """Parameters are bitwise equal on both ranks after two steps (every bucket completed: the scales' gradients are
    announced), and equal to the single-process run on the whole batch to the bound of
    tests/test_gpu_train.test_ddp_two_ranks_fused_path_matches_single_process, 2e-2 relative L2, applied to what the
    two steps changed (the two runs sum the tokens' contributions in different orders)."""
    import torch.multiprocessing as mp

    from pytorch_vit_paper_replication_amd.models import ViT
    from pytorch_vit_paper_replication_amd.ops.fused_vit import cross_entropy
    from pytorch_vit_paper_replication_amd.optim import FusedAdam
    from tests.test_gpu_train import _free_port

    world = 2
    mp.spawn(_gloo_layer_scale_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    r = [torch.load(tmp_path / f"ls{i}.pt", weights_only=True) for i in range(world)]
    assert r[0]["nbuckets"] > 2
    for k in r[0]["state"]:
        assert torch.equal(r[0]["state"][k], r[1]["state"][k]), f"params differ across ranks after two steps: {k}"
    ref = ViT(**_ddp_cfg()).set_layer_scale(0.0).to(DEV)
    ref.load_state_dict(r[0]["init"])
    opt = FusedAdam(ref.parameters(), lr=1e-3)
    x, y = r[0]["x"].to(DEV), r[0]["y"].to(DEV)
    for _ in range(2):
        loss = cross_entropy(ref(x), y)
        opt.zero_grad()
        loss.backward()
        opt.step()
    torch.cuda.synchronize()
    for k, v in ref.state_dict().items():
        moved = (v.detach().cpu() - r[0]["init"][k]).norm()
        assert moved > 0, k
        err = ((r[0]["state"][k] - v.detach().cpu()).norm() / moved).item()
        assert err < 2e-2, f"{k}: DDP(2 ranks) vs single-process update rel err {err:.3e}"
        if ".layer_scale_" in k:
            assert not torch.equal(r[0]["state"][k], r[0]["init"][k])


def test_fp8_with_layer_scale_raises_on_the_gpu():
    from pytorch_vit_paper_replication_amd.models import ViT

    m = ViT(**dict(CFG, num_transformer_layer=2)).set_layer_scale(1e-4).to(DEV).enable_fp8().train()
    with pytest.raises(NotImplementedError, match="enable_fp8.*set_layer_scale"):
        m(torch.rand(2, 3, 32, 32, device=DEV))


def test_set_layer_scale_after_the_first_fused_forward_raises():
    from pytorch_vit_paper_replication_amd.models import ViT

    m = ViT(**dict(CFG, num_transformer_layer=1)).to(DEV)
    m(torch.rand(2, 3, 32, 32, device=DEV))
    with pytest.raises(RuntimeError, match="ParamStore already covers"):
        m.set_layer_scale(1e-4)
