"""The last encoder block on the class-token rows only (ops/fused_vit.py ``CLS_LAST_BLOCK``).

* the two class-token attention kernels against an fp32 PyTorch computation of query row 0, with the
  error measures and limits ``tests/kernel_checks.py`` applies to the full attention kernels;
* the dropout masks of B compact rows mapped to rows ``b * N`` against those of the full tensor, element
  for element, for every epilogue and the column-sum kernel the class-rows block uses;
* one training step of a small ViT with the switch on and with it off (same weights, same dropout
  counter, deterministic mode), each against an fp32 reference that replays the same masks, with
  the whole-model limits of ``kernel_checks.check_vit_fused_vs_reference``;
* the classifier-free backbone returns every token and ignores the switch.
"""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _kc():
    from tests import kernel_checks as KC

    return KC


def _report(name, metrics, limits):
    KC = _kc()
    print(f"{name}: {KC.fmt_metrics(metrics, limits)}")
    assert KC.passed(metrics, limits), f"{name}: {KC.fmt_metrics(metrics, limits)}"


# --------------------------------------------------------------------------- attention kernels
ATTN_SHAPES = [(2, 3, 197, 64), (3, 2, 17, 64), (1, 1, 1, 64), (2, 2, 257, 80), (2, 1, 65, 128), (1, 2, 33, 96)]


@pytest.mark.parametrize("B,H,N,dh", ATTN_SHAPES)
def test_attn_cls_kernels_vs_fp32_row0(B, H, N, dh):
    from pytorch_vit_paper_replication_amd import _ext

    KC = _kc()
    ext = _ext.ext()
    torch.manual_seed(N * 131 + dh)
    D = H * dh
    scale = 1.0 / math.sqrt(dh)
    qkv = KC.bf(KC.rnd(B * N, 3 * D))
    qr = qkv.float().requires_grad_(True)
    oref, lref = KC._attn_ref(qr, B, N, H)  # [B*N, D], [B*H, N]
    o0_ref = oref.view(B, N, D)[:, 0]
    lse0_ref = lref[:, 0]

    o0, lse0 = ext.attn_cls_fwd(qkv, B, N, H, scale)
    assert o0.shape == (B, D) and lse0.shape == (B * H,)
    m = KC.worst((o0, o0_ref))
    m["lse_l2"], m["lse_max"] = KC.errs(lse0, lse0_ref)
    # the limits of kernel_checks.check_attn_fwd
    _report(f"attn_cls_fwd B{B} N{N} H{H} dh{dh}", m, KC.lim(4.5e-3, 6e-3, lse_l2=1.5e-7 if N >= 8 else 3e-7, lse_max=3e-7))

    do0 = KC.bf(KC.rnd(B, D))
    o0_ref.backward(do0.float())
    gref = qr.grad  # [B*N, 3D]: only query row 0 of each image has an output gradient
    dqkv, dq0 = ext.attn_cls_bwd(do0, qkv, o0, lse0, B, N, H, scale)
    assert dqkv.shape == (B * N, 3 * D) and dq0.shape == (B, D)
    dbias = torch.zeros(3 * D, device=DEV)
    ext.attn_cls_dbias(dq0, do0, dbias)
    m = KC.worst((dqkv, gref), (dqkv[:, :D], gref[:, :D]), (dqkv[:, D:2 * D], gref[:, D:2 * D]), (dqkv[:, 2 * D:], gref[:, 2 * D:]),
                 (dq0, gref.view(B, N, 3 * D)[:, 0, :D]))
    m["dbias_l2"], m["dbias_max"] = KC.errs(dbias, gref.sum(0))
    other = dqkv.view(B, N, 3 * D)[:, 1:, :D]
    m["dq_other_rows_nonzero"] = float((other != 0).sum().item())
    m["dbias_k_nonzero"] = float((dbias[D:2 * D] != 0).sum().item())
    # the limits of kernel_checks.check_attn_bwd (with the fused bias gradient)
    _report(f"attn_cls_bwd B{B} N{N} H{H} dh{dh}", m,
            KC.lim(5e-3, 1e-2, dbias_l2=1.6e-3, dbias_max=1e-3, dq_other_rows_nonzero=0, dbias_k_nonzero=0))


# --------------------------------------------------------------------------- mask identity
def _mask_case():
    torch.manual_seed(5)
    B, N, K, C, p = 3, 5, 64, 128, 0.5
    seed = torch.tensor([0x1234567 * 2654435761 + 11], dtype=torch.int64, device=DEV)
    drop = (seed, 7 << 32, p)
    xf = (torch.randn(B * N, K, device=DEV) + 0.5).to(torch.bfloat16)
    w = (0.1 * torch.randn(C, K, device=DEV)).to(torch.bfloat16)
    bias = torch.randn(C, device=DEV) + 3.0  # keeps kept outputs away from an exact 0
    return B, N, K, C, drop, xf, w, bias


def test_mask_identity_plain_epilogue():
    from pytorch_vit_paper_replication_amd.ops import gemm as G

    B, N, K, C, drop, xf, w, bias = _mask_case()
    full = G.linear_fwd(xf, w, bias, drop=drop)
    comp = G.linear_fwd(xf[::N].contiguous(), w, bias, drop=drop, drop_row_mul=N)
    assert comp.shape == (B, C)
    zf, zc = full[::N] == 0, comp == 0
    assert torch.equal(zf, zc)
    assert 0.3 < zc.float().mean().item() < 0.7  # p = 0.5 over 384 elements
    assert torch.equal(full[::N], comp)  # the same tile, the same K loop: the same bits
    # and without the mapping the compact rows would draw the masks of rows 0 .. B-1 (another pattern)
    plain = G.linear_fwd(xf[::N].contiguous(), w, bias, drop=drop)
    assert not torch.equal(plain[1:] == 0, zc[1:])


def test_mask_identity_gelu_epilogue():
    from pytorch_vit_paper_replication_amd.ops import gemm as G

    B, N, K, C, drop, xf, w, bias = _mask_case()
    uf = torch.empty(B * N, C, dtype=torch.bfloat16, device=DEV)
    uc = torch.empty(B, C, dtype=torch.bfloat16, device=DEV)
    full = G.linear_fwd(xf, w, bias, gelu_aux=uf, gelu=True, drop=drop)
    comp = G.linear_fwd(xf[::N].contiguous(), w, bias, gelu_aux=uc, gelu=True, drop=drop, drop_row_mul=N)
    assert torch.equal(full[::N] == 0, comp == 0) and torch.equal(uf[::N] == 0, uc == 0)
    assert 0.3 < (uc == 0).float().mean().item() < 0.7
    assert torch.equal(full[::N], comp) and torch.equal(uf[::N], uc)


def test_mask_identity_residual_epilogue():
    from pytorch_vit_paper_replication_amd.ops import gemm as G

    B, N, K, C, drop, xf, w, bias = _mask_case()
    rf = torch.randn(B * N, C, device=DEV).to(torch.bfloat16)
    full = G.linear_fwd(xf, w, bias, resid=rf, drop=drop)
    # the compact GEMM reads its residual rows in place from the full tensor (row stride N * C)
    comp = G.linear_fwd(xf[::N].contiguous(), w, bias, resid=rf.view(B, N, C)[:, 0], drop=drop, drop_row_mul=N)
    # a dropped element is exactly its residual
    zf, zc = full[::N] == rf[::N], comp == rf[::N]
    assert torch.equal(zf, zc)
    assert 0.3 < zc.float().mean().item() < 0.7
    assert torch.equal(full[::N], comp)


def test_mask_identity_dropout_colsum_kernel():
    from pytorch_vit_paper_replication_amd.ops import gemm as G

    B, N, K, C, drop, _, _, _ = _mask_case()
    dyf = (torch.randn(B * N, C, device=DEV) + 3.0).to(torch.bfloat16)
    dzf, dzc = torch.empty_like(dyf), torch.empty(B, C, dtype=torch.bfloat16, device=DEV)
    dbf, dbc = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
    G.bias_grad(dyf, dbf, drop=drop, dz=dzf)
    G.bias_grad(dyf[::N].contiguous(), dbc, drop=drop, dz=dzc, row_mul=N)
    assert torch.equal(dzf[::N] == 0, dzc == 0)
    assert 0.3 < (dzc == 0).float().mean().item() < 0.7
    assert torch.equal(dzf[::N], dzc)
    torch.testing.assert_close(dbc, dzc.float().sum(0), rtol=1e-5, atol=1e-4)
    # the forward mask of the same site: the backward of the class-rows fc2 sees what its forward drew
    _, _, _, _, _, xf, w, bias = _mask_case()
    fwd = G.linear_fwd(xf[::N].contiguous(), w, bias, drop=drop, drop_row_mul=N)
    assert torch.equal(fwd == 0, dzc == 0)


# --------------------------------------------------------------------------- sparse-residual LayerNorm backward
@pytest.mark.parametrize("B,N,D,linked", [(3, 5, 128, False), (3, 5, 768, True), (2, 197, 768, True), (1, 1, 256, False)])
def test_layernorm_bwd_residual_on_class_rows_equals_zero_filled_carrier(B, N, D, linked):
    """dres_every = N with a compact [B, D] residual gradient against the dense kernel fed a [B*N, D]
    carrier that is zero off the class-token rows: the same sums in the same order, so the same bits
    (deterministic mode: ordered column sums). ``linked``: with the previous block's dropout backward."""
    from pytorch_vit_paper_replication_amd import _ext

    ext = _ext.ext()
    torch.manual_seed(B * 1000 + N + D)
    T = B * N
    x = torch.randn(T, D, device=DEV).to(torch.bfloat16)
    dy = torch.randn(T, D, device=DEV).to(torch.bfloat16)
    w, b = torch.randn(D, device=DEV), torch.randn(D, device=DEV)
    _, mean, rstd = ext.layernorm_fwd(x, w, b, 1e-5, T, D)
    dres = torch.randn(B, D, device=DEV).to(torch.bfloat16)
    carrier = torch.zeros(T, D, dtype=torch.bfloat16, device=DEV)
    carrier[::N] = dres
    seed = torch.tensor([987654321], dtype=torch.int64, device=DEV)
    outs = []
    with _ext.deterministic_mode():
        for res, every in ((carrier, 0), (dres, N)):
            dx = torch.empty(T, D, dtype=torch.bfloat16, device=DEV)
            dz = torch.empty_like(dx) if linked else None
            dw, db, ds = (torch.zeros(D, device=DEV) for _ in range(3))
            kw = dict(dsum=ds, dz=dz, seed=seed, seed_offset=4 << 32, drop_p=0.1) if linked else dict(dsum=ds)
            ext.layernorm_bwd(dy, D, x, D, mean, rstd, w, res, D, dx, D, dw, db, T, dres_every=every, **kw)
            outs.append((dx, dz, dw, db, ds))
    torch.cuda.synchronize()
    for a, c in zip(*outs):
        assert (a is None and c is None) or torch.equal(a, c)
    assert not torch.equal(outs[1][0][::N], outs[1][0][::N] - dres)  # the residual did reach the class rows


def test_host_checks_reject_unsupported_class_row_arguments():
    from pytorch_vit_paper_replication_amd import _ext

    ext = _ext.ext()
    x = torch.zeros(4, 64, dtype=torch.bfloat16, device=DEV)
    w = torch.zeros(128, 64, dtype=torch.bfloat16, device=DEV)
    out = torch.empty(4, 128, dtype=torch.bfloat16, device=DEV)
    seed = torch.tensor([1], dtype=torch.int64, device=DEV)
    with pytest.raises(RuntimeError, match="drop_row_mul"):  # the ping-pong epilogues hash the plain row
        ext.gemm(x, True, w, True, out, 4, 128, 64, 0, None, None, None, 0, None, 0, 0, 0, seed, 0, 0.5, 0, 12, drop_row_mul=5)
    assert not ext.attn_cls_ok(8193, 64) and not ext.attn_cls_ok(17, 72) and ext.attn_cls_ok(1, 128)
    with pytest.raises(RuntimeError, match="attn_cls_ok"):
        ext.attn_cls_fwd(torch.zeros(2 * 3, 3 * 72, dtype=torch.bfloat16, device=DEV), 2, 3, 1, 0.1)
    with pytest.raises(RuntimeError, match="dres_every"):  # a residual tensor too short for the rows
        d = torch.zeros(10, 128, dtype=torch.bfloat16, device=DEV)
        f = torch.zeros(128, device=DEV)
        ext.layernorm_bwd(d, 128, d, 128, f[:10], f[:10], f, d[:1], 128, torch.empty_like(d), 128, None, None, 10, dres_every=5)


# --------------------------------------------------------------------------- whole model
CFG = dict(image_size=32, patch_size=8, num_heads=2, embedding_dim=128, mlp_size=256, num_classes=10,
           mlp_dropout=0.1, embedding_dropout=0.1)
# kernel_checks.check_vit_fused_vs_reference: logits rel-L2 / max, worst per-parameter gradient rel-L2 / max
LIMITS = dict(logits_l2=2.1e-2, logits_max=2.8e-2, grad_l2=2.5e-2, grad_max=3.6e-2)


def _site_mask(ext, seed, site, p, rows, cols):
    """Keep mask * exact fp32 scale of dropout site ``site`` over a [rows, cols] tensor, drawn by the
    column-sum kernel from the same counter hash as every epilogue."""
    if p <= 0:
        return None
    m = torch.empty(rows, cols, dtype=torch.bfloat16, device=DEV)
    ext.colsum(torch.ones(rows, cols, dtype=torch.bfloat16, device=DEV), rows, cols, None, m, seed, site << 32, p)
    thr = min(int(round(p * 65536)), 65535)
    return (m != 0).float() * (65536.0 / (65536.0 - thr))


def _reference_step(mr, x, y, seed, B, train=True):
    """fp32 PyTorch forward + backward of ``mr`` with the fused path's dropout masks (``seed``: the device
    counter value the fused forward snapshots) replayed in every nn.Dropout."""
    from pytorch_vit_paper_replication_amd import _ext

    KC = _kc()
    ext = _ext.ext()
    c = mr.config
    N, D, M = mr.patch_embedding_block.number_of_patches + 1, c["embedding_dim"], c["mlp_size"]
    T = B * N
    patched = []

    def replay(mod, mask):
        if mask is not None:
            mod.forward = lambda t, k=mask: t * k.view_as(t)
            patched.append(mod)

    if train:
        replay(mr.patch_embedding_block.dropout, _site_mask(ext, seed, 0, c["embedding_dropout"], T, D))
        for i, blk in enumerate(mr.transformer_encoder):
            replay(blk.mlp_block.mlp[2], _site_mask(ext, seed, 1 + 2 * i, c["mlp_dropout"], T, M))
            replay(blk.mlp_block.mlp[4], _site_mask(ext, seed, 2 + 2 * i, c["mlp_dropout"], T, D))
    try:
        mr.train(train)
        logits = KC._reference_logits(mr, x)
        loss = F.cross_entropy(logits, y)
        if train:
            loss.backward()
    finally:
        for mod in patched:
            del mod.forward
    return loss.detach(), logits.detach()


def _fused_step(mf, x, y, rng0, cls_on, train=True):
    from pytorch_vit_paper_replication_amd import _ext
    from pytorch_vit_paper_replication_amd.ops import fused_vit

    rows = []
    old = fused_vit.CLS_LAST_BLOCK
    fused_vit.CLS_LAST_BLOCK = cls_on
    fused_vit.DGRAD_TAP = lambda which, t: rows.append((which, t.shape[0]))
    try:
        mf._pvr_rng.copy_(rng0)
        mf.train(train)
        mf.zero_grad(set_to_none=True)
        if train:
            with _ext.deterministic_mode():
                logits = mf(x)
                loss = fused_vit.cross_entropy(logits, y)
                loss.backward()
        else:
            with torch.inference_mode():
                logits = mf(x)
            loss = F.cross_entropy(logits.float(), y)
        torch.cuda.synchronize()
    finally:
        fused_vit.CLS_LAST_BLOCK = old
        fused_vit.DGRAD_TAP = None
    grads = {n: p.grad.detach().clone() for n, p in mf.named_parameters()} if train else {}
    return loss.detach(), logits.detach().clone(), grads, rows


@pytest.fixture(scope="module")
def parity():
    """Per (depth, batch): the fp32 reference with replayed masks (computed once) and both fused arms."""
    cache = {}

    def get(depth, B):
        if (depth, B) in cache:
            return cache[depth, B]
        from pytorch_vit_paper_replication_amd.models import ViT

        torch.manual_seed(depth * 10 + B)
        cfg = dict(CFG, num_transformer_layer=depth)
        mf = ViT(**cfg).to(DEV)
        mr = ViT(**cfg).to(DEV)
        mr.load_state_dict(mf.state_dict())
        x = torch.rand(B, 3, 32, 32, device=DEV)
        y = torch.randint(0, 10, (B,), device=DEV)
        assert mf._fused_supported(x)
        mf._dropout_seed(x.device)  # creates the device counter
        rng0 = mf._pvr_rng.clone()
        out = {"N": mr.patch_embedding_block.number_of_patches + 1, "B": B}
        out["ref"] = _reference_step(mr, x, y, rng0, B) + ({n: p.grad.detach().clone() for n, p in mr.named_parameters()},)
        out["ref_eval"] = _reference_step(mr, x, y, rng0, B, train=False)
        for name, on in (("cls", True), ("full", False)):
            out[name] = _fused_step(mf, x, y, rng0, on)
            out[name + "_eval"] = _fused_step(mf, x, y, rng0, on, train=False)
        cache[depth, B] = out
        return out

    return get


def _arm_metrics(arm, ref):
    KC = _kc()
    loss, logits, grads, _ = arm
    rloss, rlogits, rgrads = ref
    m = {}
    m["logits_l2"], m["logits_max"] = KC.errs(logits, rlogits)
    l2 = mx = 0.0
    for n, gr in rgrads.items():
        a, b = KC.errs(grads[n], gr)
        l2, mx = max(l2, a), max(mx, b)
    m["grad_l2"], m["grad_max"] = l2, mx
    # softmax cross-entropy moves by at most 2 max|dlogit|: the logits limit, in the loss's units
    m["loss_abs"] = abs(loss.item() - rloss.item())
    return m, dict(LIMITS, loss_abs=2 * LIMITS["logits_max"] * rlogits.abs().max().item())


@pytest.mark.parametrize("depth,B", [(2, 3), (1, 3), (2, 1)])
def test_training_step_parity_class_rows_vs_full_vs_fp32(parity, depth, B):
    r = parity(depth, B)
    N = r["N"]
    # the switch selects what runs: the last block's fc2 / fc1 / out dgrads have B rows, its qkv dgrad B*N
    assert r["cls"][3][:4] == [(0, B), (1, B), (2, B), (3, B * N)]
    assert all(rows == B * N for _, rows in r["full"][3]) and len(r["full"][3]) == 4 * depth == len(r["cls"][3])
    for name in ("full", "cls"):  # the class-rows arm meets the limits the full arm meets
        m, limits = _arm_metrics(r[name], r["ref"])
        _report(f"vit depth {depth} batch {B} {name} arm vs fp32 with the same masks", m, limits)
    # the arms against each other: the same maths on B rows or on all of them
    m, limits = _arm_metrics(r["cls"], (r["full"][0], r["full"][1], r["full"][2]))
    _report(f"vit depth {depth} batch {B} class-rows arm vs full arm", m, limits)


@pytest.mark.parametrize("depth,B", [(2, 3), (1, 3), (2, 1)])
def test_inference_logits_parity(parity, depth, B):
    KC = _kc()
    r = parity(depth, B)
    lim2 = {k: LIMITS[k] for k in ("logits_l2", "logits_max")}
    for name in ("full_eval", "cls_eval"):
        m = dict(zip(("logits_l2", "logits_max"), KC.errs(r[name][1], r["ref_eval"][1])))
        _report(f"vit depth {depth} batch {B} {name} logits vs fp32", m, lim2)
    assert r["cls_eval"][3] == [] and r["full_eval"][3] == []  # no backward ran


def test_no_classifier_backbone_returns_all_tokens_and_ignores_the_switch():
    from pytorch_vit_paper_replication_amd.models.vit_no_classifier import ViT as ViTNoClassifier
    from pytorch_vit_paper_replication_amd.ops import fused_vit

    torch.manual_seed(3)
    cfg = {k: v for k, v in CFG.items() if k != "num_classes"}
    m = ViTNoClassifier(**dict(cfg, num_transformer_layer=2)).to(DEV).train()
    x = torch.rand(3, 3, 32, 32, device=DEV)
    m._dropout_seed(x.device)
    rng0 = m._pvr_rng.clone()
    outs, grads = [], []
    old = fused_vit.CLS_LAST_BLOCK
    try:
        for on in (True, False):
            fused_vit.CLS_LAST_BLOCK = on
            m._pvr_rng.copy_(rng0)
            m.zero_grad(set_to_none=True)
            from pytorch_vit_paper_replication_amd import _ext

            with _ext.deterministic_mode():
                y = m(x)
                y.square().mean().backward()
            torch.cuda.synchronize()
            outs.append(y.detach().clone())
            grads.append([p.grad.detach().clone() for p in m.parameters()])
    finally:
        fused_vit.CLS_LAST_BLOCK = old
    assert outs[0].shape == (3, 17, 128)
    assert torch.equal(outs[0], outs[1])
    assert all(torch.equal(a, b) for a, b in zip(grads[0], grads[1]))
