"""Patch dropout on the fused path.

* ``patch_keep_table`` (csrc/elementwise.hip ``patch_keep_kernel``) against the numpy oracle of
  tests/test_patch_dropout_cpu.py, and its host checks;
* the keep variants of both patchify kernels against the plain kernels' rows gathered by the table, bit
  for bit, with and without a crop box and a mix plan;
* the embedding GEMM with the gathered position addend against an fp32 product;
* the patch-embedding backward with the inverse table against fp32 torch sums;
* one training step of a small ViT (class-token last block on and off, with and without drop path)
  against the fp32 reference model with the keep table and the dropout masks replayed at the compact
  token indices;
* the device counter: fresh tables every forward, reproducible from the counter, bit-exact resume,
  hipGraph replays; the fp8 exclusion.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import test_drop_path_cpu as H  # the numpy replica of the counter hash
from tests import test_patch_dropout_cpu as O  # the numpy oracle of the keep table

pytestmark = pytest.mark.gpu

DEV = "cuda"
SITE_OFF = O.PATCH_DROP_SITE << 32


def _kc():
    from tests import kernel_checks as KC

    return KC


def _E():
    from pytorch_vit_paper_replication_amd import _ext

    return _ext


def _seed_tensor(v):
    v = int(v)
    return torch.tensor([v - (1 << 64) if v >= 1 << 63 else v], dtype=torch.int64, device=DEV)


def _oracle(seed, B, n_p, n_keep):
    keep = O.keep_table(seed, B, n_p, n_keep)
    return torch.from_numpy(keep).to(DEV), torch.from_numpy(O.inv_table(keep, n_p)).to(DEV)


def _bits(t):
    return t.view(torch.int16)


# ----------------------------------------------------------------------------- the keep table
@pytest.mark.parametrize("B,n_p,n_keep", [(3, 16, 8), (4, 7, 1), (2, 16, 16), (5, 196, 98), (2, 576, 144)])
def test_keep_table_equals_the_numpy_oracle(B, n_p, n_keep):
    ext = _E().ext()
    for seed in (5, 123456789012345, 2 ** 62 + 17):
        keep, inv = ext.patch_keep_table(_seed_tensor(seed), SITE_OFF, B, n_p, n_keep)
        assert keep.dtype == torch.int32 and keep.shape == (B, n_keep) and inv.dtype == torch.int32 and inv.shape == (B, n_p)
        want = O.keep_table(seed, B, n_p, n_keep)
        k, i = keep.cpu().numpy(), inv.cpu().numpy()
        assert np.array_equal(k, want), seed
        assert (np.diff(k, axis=1) > 0).all()  # strictly ascending rows
        assert np.array_equal(i, O.inv_table(want, n_p))
        for b in range(B):  # inv is the inverse of keep, and -1 everywhere else
            assert np.array_equal(i[b, k[b]], np.arange(n_keep)) and int((i[b] >= 0).sum()) == n_keep
    if n_keep < n_p:  # another counter value, another table
        a = ext.patch_keep_table(_seed_tensor(5), SITE_OFF, B, n_p, n_keep)[0]
        b = ext.patch_keep_table(_seed_tensor(6), SITE_OFF, B, n_p, n_keep)[0]
        assert not torch.equal(a, b)


def test_keep_table_host_checks():
    ext = _E().ext()
    st = _seed_tensor(1)
    with pytest.raises(RuntimeError, match="n_keep"):
        ext.patch_keep_table(st, SITE_OFF, 2, 16, 17)
    with pytest.raises(RuntimeError, match="n_keep"):
        ext.patch_keep_table(st, SITE_OFF, 2, 16, 0)
    with pytest.raises(RuntimeError, match="n_p"):
        ext.patch_keep_table(st, SITE_OFF, 2, 4097, 8)
    with pytest.raises(RuntimeError, match="2\\^32"):
        ext.patch_keep_table(st, SITE_OFF, 2 ** 21, 4096, 8)
    with pytest.raises(RuntimeError, match="seed"):
        ext.patch_keep_table(st.cpu(), SITE_OFF, 2, 16, 8)
    keep, inv = ext.patch_keep_table(st, SITE_OFF, 2, 4096, 1)  # the largest n_p
    assert np.array_equal(keep.cpu().numpy(), O.keep_table(1, 2, 4096, 1))
    # the kernels that take the table check it against their shapes
    img = torch.zeros(2, 3, 32, 32, device=DEV)
    out = torch.empty(2 * 8, 192, dtype=torch.bfloat16, device=DEV)
    good = ext.patch_keep_table(st, SITE_OFF, 2, 16, 8)[0]
    ext.im2col(img, out, 8, 192, keep=good)
    for bad in (good[:1], good.long(), good.cpu(), ext.patch_keep_table(st, SITE_OFF, 2, 32, 17)[0]):
        with pytest.raises(RuntimeError, match="keep"):
            ext.im2col(img, out, 8, 192, keep=bad)
    with pytest.raises(RuntimeError, match="out"):
        ext.im2col(img, out[:8], 8, 192, keep=good)


# ----------------------------------------------------------------------------- patchify rows
def _kp(P, C=3):
    return (C * P * P + 63) // 64 * 64


def _gather_rows(plain, keep, n_p):
    B, n_keep = keep.shape
    rows = (torch.arange(B, device=DEV).view(B, 1) * n_p + keep.long()).reshape(-1)
    return plain[rows]


def _mix_plan(B, S):
    """One mixup row, one CutMix row whose box has no side on a patch border (the rest, if any: unmixed)."""
    from pytorch_vit_paper_replication_amd.data import MixPlan

    partner = [(b + 1) % B for b in range(B)]
    lam = [0.625, 1.0] + [1.0] * (B - 2)
    box = [[0, 0, 0, 0], [S // 4 + 1, 3, S - 5, S - S // 4 - 1]] + [[0, 0, 0, 0]] * (B - 2)
    return MixPlan(partner, lam, box, (S, S))


FLOAT_CASES = [(3, 3, 32, 8), (2, 3, 56, 14), (2, 3, 224, 16)]  # (2, 3, 56, 14): the per-element path


@pytest.mark.parametrize("mixed", [False, True], ids=["plain", "mix"])
@pytest.mark.parametrize("B,C,S,P", FLOAT_CASES)
def test_float_patchify_rows_equal_the_gathered_plain_rows(B, C, S, P, mixed):
    ext = _E().ext()
    g = torch.Generator().manual_seed(S + P)
    img = torch.randn(B, C, S, S, generator=g).to(DEV)
    n_p, kp = (S // P) ** 2, _kp(P, C)
    n_keep = max(1, n_p // 2)
    keep, _ = _oracle(77 + S, B, n_p, n_keep)
    plan = _mix_plan(B, S) if mixed else None
    kw = {} if plan is None else dict(mix=plan.on(DEV)[0], mix_host=plan.rows)
    plain = torch.full((B * n_p, kp), float("nan"), dtype=torch.bfloat16, device=DEV)
    ext.im2col(img, plain, P, kp, **kw)
    got = torch.full((B * n_keep, kp), float("nan"), dtype=torch.bfloat16, device=DEV)
    ext.im2col(img, got, P, kp, keep=keep, **kw)
    assert not torch.isnan(got.float()).any()  # every row and the zero padding are written
    assert torch.equal(_bits(got), _bits(_gather_rows(plain, keep, n_p)))
    if mixed:  # the plan did reach the kept rows
        nomix = torch.empty_like(got)
        ext.im2col(img, nomix, P, kp, keep=keep)
        assert not torch.equal(_bits(got), _bits(nomix))


@pytest.mark.parametrize("mixed", [False, True], ids=["plain", "mix"])
@pytest.mark.parametrize("geom", ["none", "center", "flipped"])
@pytest.mark.parametrize("layout", ["contiguous", "channels_last"])
def test_u8_patchify_rows_equal_the_gathered_plain_rows(layout, geom, mixed):
    """Source 40 x 48 (``geom``) or 32 x 32 (none) -> 32 x 32, P = 16 (the 8-byte path on contiguous input without a
    box) and P = 8."""
    from pytorch_vit_paper_replication_amd.data.device_input import center_box

    ext = _E().ext()
    B, S = 3, 32
    mean, std = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
    gen = torch.Generator().manual_seed(11)
    hs, ws = (S, S) if geom == "none" else (40, 48)
    x = torch.randint(0, 256, (B, 3, hs, ws), generator=gen, dtype=torch.uint8).to(DEV)
    if layout == "channels_last":
        x = x.contiguous(memory_format=torch.channels_last)
    box = None
    if geom == "center":
        box = center_box(B, hs, ws, 30.5).to(DEV)
    elif geom == "flipped":  # per-sample boxes, two of them right to left
        box = torch.tensor([[44.0, 2.0, 4.0, 38.0], [1.5, 0.0, 33.5, 32.0], [48.0, 8.0, 16.0, 40.0]], device=DEV)
    plan = _mix_plan(B, S) if mixed else None
    kw = {} if plan is None else dict(mix=plan.on(DEV)[0], mix_host=plan.rows)
    for P in (16, 8):
        n_p, kp = (S // P) ** 2, _kp(P)
        n_keep = max(1, n_p // 2)
        keep, _ = _oracle(31 + P, B, n_p, n_keep)
        plain = torch.full((B * n_p, kp), float("nan"), dtype=torch.bfloat16, device=DEV)
        vec_plain = ext.im2col_u8(x, plain, mean, std, box, S, S, P, kp, **kw)
        got = torch.full((B * n_keep, kp), float("nan"), dtype=torch.bfloat16, device=DEV)
        vec = ext.im2col_u8(x, got, mean, std, box, S, S, P, kp, keep=keep, **kw)
        assert vec == vec_plain == (1 if geom == "none" and layout == "contiguous" else 0)
        assert not torch.isnan(got.float()).any()
        assert torch.equal(_bits(got), _bits(_gather_rows(plain, keep, n_p))), P


# ----------------------------------------------------------------------------- embedding forward
# the limits kernel_checks.check_gemm_fwd applies
GEMM_LIM = dict(l2=3.5e-3, max=7e-3)


@pytest.mark.parametrize("B,n_p,n_keep,D,K", [(5, 196, 98, 768, 768), (3, 16, 8, 128, 192), (2, 7, 1, 64, 64)])
def test_embedding_gemm_with_the_gathered_position_addend(B, n_p, n_keep, D, K):
    from pytorch_vit_paper_replication_amd.ops import gemm as G

    KC = _kc()
    ext = _E().ext()
    torch.manual_seed(n_p + D)
    keep, _ = _oracle(99, B, n_p, n_keep)
    rows = n_keep + 1
    x, w, b = KC.bf(KC.rnd(B * n_keep, K)), KC.bf(KC.rnd(D, K, scale=0.05)), KC.rnd(D)
    pos = KC.rnd(n_p + 1, D)
    addend = ext.pos_gather(pos, keep)
    assert addend.shape == (B * rows, D) and addend.dtype == torch.float32
    want_add = torch.cat((pos[:1].expand(B, 1, D), pos[keep.long() + 1]), dim=1).reshape(B * rows, D)
    assert torch.equal(addend, want_add)  # a gather moves bits
    out = torch.full((B * rows, D), 7.0, dtype=torch.bfloat16, device=DEV)
    G.linear_fwd(x, w, b, addend=addend, addend_period=B * rows, row_remap=(n_keep, rows, 1), out=out)
    o3 = out.view(B, rows, D)
    assert bool((o3[:, 0] == 7.0).all())  # the class-token rows are not the GEMM's
    ref = (x.float() @ w.float().t() + b).view(B, n_keep, D) + pos[keep.long() + 1]
    m = KC.worst((o3[:, 1:], ref))
    print(f"patch-dropout embedding GEMM B{B} {n_p}->{n_keep} D{D} K{K}: {KC.fmt_metrics(m, GEMM_LIM)}")
    assert KC.passed(m, GEMM_LIM), KC.fmt_metrics(m, GEMM_LIM)


# ----------------------------------------------------------------------------- patch-embedding backward
# the limits of kernel_checks.check_patch_bwd
PB_LIM = {"sums_l2": 5e-6, "sums_max": 2e-5, "dconv_l2": 3.5e-3, "dconv_max": 7e-3}


def _site_mask(seed, site, p, rows, cols):
    """Keep mask (float 0 / 1) of dropout site ``site`` over a [rows, cols] tensor, from the column-sum kernel."""
    if p <= 0:
        return torch.ones(rows, cols, device=DEV)
    m = torch.empty(rows, cols, dtype=torch.bfloat16, device=DEV)
    _E().ext().colsum(torch.ones(rows, cols, dtype=torch.bfloat16, device=DEV), rows, cols, None, m, seed, site << 32, p)
    return (m != 0).float()


def _scale(p):
    return 65536.0 / (65536.0 - H.thr16(p)) if p > 0 else 1.0


@pytest.mark.parametrize("B,n_p,n_keep,D,p", [(37, 196, 98, 768, 0.1), (5, 16, 4, 1280, 0.0), (2, 16, 4, 128, 0.0)])
def test_patch_bwd_with_the_table(B, n_p, n_keep, D, p):
    KC = _kc()
    ext = _E().ext()
    torch.manual_seed(B + D)
    ntok, rows = n_p + 1, n_keep + 1
    # a counter value (chosen on the host with the oracle) at which some position is kept by no sample, where one exists
    want_hole = B * n_keep < n_p
    seed_v = next(v for v in range(4242, 5000)
                  if not want_hole or len(set(O.keep_table(v, B, n_p, n_keep).reshape(-1).tolist())) < n_p)
    keep, inv = _oracle(seed_v, B, n_p, n_keep)
    never = sorted(set(range(n_p)) - set(keep.reshape(-1).tolist()))
    if want_hole:
        assert never, "the case needs a position that no sample kept"
    seed = _seed_tensor(seed_v)
    dE = KC.bf(KC.rnd(B * rows, D))
    # the mask of the compact element index; a dropped element is +0 (a product with 0 would keep dE's sign)
    dpre = torch.where(_site_mask(seed, 3, p, B * rows, D) != 0, dE.float() * _scale(p), torch.zeros((), device=DEV))
    d3 = dpre.view(B, rows, D)
    ref_pos = torch.zeros(ntok, D, device=DEV)
    ref_pos[0] = d3[:, 0].sum(0)
    for b in range(B):
        ref_pos[keep[b].long() + 1] += d3[b, 1:]
    gpos, gcls, gb = torch.zeros(ntok, D, device=DEV), torch.zeros(D, device=DEV), torch.zeros(D, device=DEV)
    dconv = torch.full((B * n_keep, D), float("nan"), dtype=torch.bfloat16, device=DEV)
    ext.patch_bwd(dE, B, ntok, D, gpos.view(-1), gcls, dconv, gb, seed, 3 << 32, p, inv=inv, n_keep=n_keep)
    sums = KC.worst((gpos, ref_pos), (gcls, d3[:, 0].sum(0)), (gb, d3[:, 1:].sum((0, 1))))
    dc = KC.worst((dconv, d3[:, 1:].reshape(-1, D)))
    m = {"sums_l2": sums["l2"], "sums_max": sums["max"], "dconv_l2": dc["l2"], "dconv_max": dc["max"]}
    print(f"patch_bwd with the table B{B} {n_p}->{n_keep} D{D} p{p}: {KC.fmt_metrics(m, PB_LIM)}")
    assert KC.passed(m, PB_LIM), KC.fmt_metrics(m, PB_LIM)
    # dconv rows are the masked dE rows, bit for bit (every kept row written once)
    assert torch.equal(_bits(dconv), _bits(d3[:, 1:].reshape(-1, D).to(torch.bfloat16)))
    if never:  # exact zeros where no sample kept the patch
        assert bool((gpos[torch.tensor(never, device=DEV) + 1] == 0).all())
    kept_pos = torch.tensor(sorted(set(keep.reshape(-1).tolist())), device=DEV) + 1
    assert bool((gpos[kept_pos].abs().sum(1) > 0).all())
    # accumulation: a second call adds the same sums again
    ext.patch_bwd(dE, B, ntok, D, gpos.view(-1), gcls, None, gb, seed, 3 << 32, p, inv=inv, n_keep=n_keep)
    assert KC.errs(gpos, 2 * ref_pos)[0] <= PB_LIM["sums_l2"]
    with pytest.raises(RuntimeError, match="patch_bwd"):
        ext.patch_bwd(dE, B, ntok, D, gpos.view(-1), gcls, None, gb, seed, 3 << 32, p, inv=inv[:, :-1], n_keep=n_keep)
    with pytest.raises(RuntimeError, match="patch_bwd"):
        ext.patch_bwd(dE[:-1], B, ntok, D, gpos.view(-1), gcls, None, gb, seed, 3 << 32, p, inv=inv, n_keep=n_keep)


# ----------------------------------------------------------------------------- whole model
# exactly the configuration and limits of tests/test_gpu_cls_last_block.py
CFG = dict(image_size=32, patch_size=8, num_heads=2, embedding_dim=128, mlp_size=256, num_classes=10,
           mlp_dropout=0.1, embedding_dropout=0.1)
RATE, N_P, N_KEEP = 0.5, 16, 8
NC = N_KEEP + 1  # the encoder's tokens per sample


def _reference_step_pd(mr, x, y, seed, B, drop_path=0.0):
    """fp32 PyTorch forward + backward of ``mr`` with the fused path's draws at counter value ``seed`` replayed:
    the keep table into ``PatchEmbedding._draw_patch_keep``, the dropout masks of the compact [B * N', .]
    tensors into every nn.Dropout, and (``drop_path``) the drop-path vectors into the blocks' draw."""
    KC = _kc()
    ext = _E().ext()
    c = mr.config
    D, M = c["embedding_dim"], c["mlp_size"]
    T = B * NC
    pe = mr.patch_embedding_block
    patched = []

    def replay(mod, site, p, cols):
        if p > 0:
            k = _site_mask(seed, site, p, T, cols) * _scale(p)
            mod.forward = lambda t, k=k: t * k.view_as(t)
            patched.append((mod, "forward"))

    replay(pe.dropout, 0, c["embedding_dropout"], D)
    for i, blk in enumerate(mr.transformer_encoder):
        replay(blk.mlp_block.mlp[2], 1 + 2 * i, c["mlp_dropout"], M)
        replay(blk.mlp_block.mlp[4], 2 + 2 * i, c["mlp_dropout"], D)
        if drop_path > 0:
            def draw(batch, p, branch, device, i=i):
                return ext.drop_path_scale(seed, (H.DROP_PATH_SITE + 2 * i + branch) << 32, p, batch) != 0

            blk._draw_drop_path = draw
            patched.append((blk, "_draw_drop_path"))
    pe._draw_patch_keep = lambda batch, n_p, n_keep, device: ext.patch_keep_table(seed, SITE_OFF, batch, n_p, n_keep)[0].long()
    patched.append((pe, "_draw_patch_keep"))
    try:
        mr.train()
        mr.zero_grad(set_to_none=True)
        logits = KC._reference_logits(mr, x)
        loss = F.cross_entropy(logits, y)
        loss.backward()
    finally:
        for mod, name in patched:
            delattr(mod, name)
    return loss.detach(), logits.detach(), {n: p.grad.detach().clone() for n, p in mr.named_parameters()}


@pytest.fixture(scope="module")
def pd_parity():
    cache = {}

    def get(depth, drop_path=0.0, B=8):
        if (depth, drop_path) in cache:
            return cache[depth, drop_path]
        from pytorch_vit_paper_replication_amd.models import ViT
        from tests import test_gpu_cls_last_block as CL

        torch.manual_seed(depth * 10 + B)
        cfg = dict(CFG, num_transformer_layer=depth)
        mf = ViT(**cfg).to(DEV).set_patch_dropout(RATE)
        mr = ViT(**cfg).to(DEV).set_patch_dropout(RATE)
        mp = ViT(**cfg).to(DEV)  # the same weights without the option
        if drop_path:
            mf.set_drop_path(drop_path, "constant")
            mr.set_drop_path(drop_path, "constant")
        mr.load_state_dict(mf.state_dict())
        mp.load_state_dict(mf.state_dict())
        assert mf.patch_embedding_block.patch_keep == N_KEEP
        x = torch.rand(B, 3, 32, 32, device=DEV)
        y = torch.randint(0, 10, (B,), device=DEV)
        assert mf._fused_supported(x)
        mf._dropout_seed(x.device)
        mp._dropout_seed(x.device)
        v = 31337 + depth
        if drop_path:  # a counter value at which every block drops and keeps a sample in each branch
            def mixed(s):
                ks = [H.rng_keep(H.site_seed(s, H.DROP_PATH_SITE + k), np.arange(B), H.thr16(drop_path)) for k in range(2 * depth)]
                return all(0 < int(k.sum()) < B for k in ks)

            v = next(s for s in range(v, v + 10000) if mixed(s))
        mf._pvr_rng.fill_(v)
        mp._pvr_rng.fill_(v)
        rng0 = mf._pvr_rng.clone()
        out = {"B": B, "seed": v}
        out["ref"] = _reference_step_pd(mr, x, y, rng0, B, drop_path)
        for name, on in (("cls", True), ("full", False)):
            out[name] = CL._fused_step(mf, x, y, rng0, on)
            out[name + "_eval"] = CL._fused_step(mf, x, y, rng0, on, train=False)
            out[name + "_plain_eval"] = CL._fused_step(mp, x, y, rng0, on, train=False)
        out["plain"] = CL._fused_step(mp, x, y, rng0, True)
        mf.set_patch_dropout(0.0)
        if drop_path:
            mf.set_drop_path(0.0)
        out["off"] = CL._fused_step(mf, x, y, rng0, True)
        cache[depth, drop_path] = out
        return out

    return get


@pytest.mark.parametrize("depth,drop_path", [(1, 0.0), (3, 0.0), (3, 0.5)])
def test_training_step_parity_with_patch_dropout(pd_parity, depth, drop_path):
    from tests import test_gpu_cls_last_block as CL

    r = pd_parity(depth, drop_path)
    B = r["B"]
    table = O.keep_table(r["seed"], B, N_P, N_KEEP)
    assert len({tuple(t) for t in table.tolist()}) > 1  # the samples keep different patches
    # the encoder ran at N' = 9 tokens per sample: the dgrad GEMMs' rows (class-token block: B rows, its qkv dgrad B * N')
    assert r["cls"][3][:4] == [(0, B), (1, B), (2, B), (3, B * NC)]
    assert all(rows == B * NC for _, rows in r["full"][3]) and len(r["full"][3]) == 4 * depth == len(r["cls"][3])
    for name in ("full", "cls"):
        m, limits = CL._arm_metrics(r[name], r["ref"])
        CL._report(f"vit depth {depth} batch {B} patch dropout (drop path {drop_path}) {name} arm vs fp32 with the same draws", m, limits)
    # the position-embedding gradient is exactly zero where no sample kept the patch (none such need exist at B = 8)
    never = sorted(set(range(N_P)) - set(table.reshape(-1).tolist()))
    gpos = r["full"][2]["patch_embedding_block.position_embedding"][0]
    if never:
        assert bool((gpos[torch.tensor(never, device=DEV) + 1] == 0).all())
    # non-vacuity: the option changes the training logits; rate 0 restores the plain model's step bit for bit
    assert not torch.equal(r["plain"][1], r["cls"][1])
    assert torch.equal(r["plain"][1], r["off"][1]) and all(torch.equal(r["plain"][2][n], r["off"][2][n]) for n in r["plain"][2])
    # eval never drops: the logits of the same weights without the option, bit for bit
    for name in ("full", "cls"):
        assert torch.equal(r[name + "_eval"][1], r[name + "_plain_eval"][1])


def test_grad_mode_off_never_drops_and_the_backbone_returns_the_kept_tokens():
    from pytorch_vit_paper_replication_amd.models import ViT
    from pytorch_vit_paper_replication_amd.models.vit_no_classifier import ViT as ViTNoClassifier

    torch.manual_seed(2)
    cfg = dict(CFG, num_transformer_layer=2, mlp_dropout=0.0, embedding_dropout=0.0)
    m = ViT(**cfg).to(DEV).train()
    x = torch.rand(4, 3, 32, 32, device=DEV)
    with torch.no_grad():
        plain = m(x).clone()
    m.set_patch_dropout(RATE)
    for ctx in (torch.no_grad, torch.inference_mode):
        with ctx():
            assert torch.equal(m(x), plain)  # training mode, grad mode off: every patch
    assert not torch.equal(m(x).detach(), plain)
    nc = ViTNoClassifier(**{k: v for k, v in cfg.items() if k != "num_classes"}).to(DEV).set_patch_dropout(RATE).train()
    nc._dropout_seed(x.device)
    seed = nc._pvr_rng.clone()
    out = nc(x)
    assert out.shape == (4, NC, 128)
    out.square().mean().backward()
    # against the reference path with the same table
    pe = nc.patch_embedding_block
    pe._draw_patch_keep = lambda b, n_p, n_keep, dev: _E().ext().patch_keep_table(seed, SITE_OFF, b, n_p, n_keep)[0].long()
    try:
        ref = _kc()._reference_logits(nc, x)
    finally:
        del pe._draw_patch_keep
    assert ref.shape == out.shape
    a, b = _kc().errs(out, ref)
    assert a <= 2.1e-2 and b <= 2.8e-2, (a, b)  # the whole-model output limits of test_gpu_cls_last_block.LIMITS
    nc.eval()
    with torch.no_grad():
        assert nc(x).shape == (4, N_P + 1, 128)


def test_uint8_input_path_takes_the_table():
    """``set_device_input`` + patch dropout: the uint8 patchify kernel gathers the same patches, so the step equals
    the float path's on the preprocessed batch bit for bit (same counter value, deterministic mode)."""
    from pytorch_vit_paper_replication_amd.data import DeviceInput
    from pytorch_vit_paper_replication_amd.data.device_input import preprocess_reference
    from pytorch_vit_paper_replication_amd.models import ViT

    torch.manual_seed(6)
    m = ViT(**dict(CFG, num_transformer_layer=1)).to(DEV).set_patch_dropout(RATE).train()
    spec = DeviceInput()
    xu = torch.randint(0, 256, (4, 3, 32, 32), dtype=torch.uint8, device=DEV)
    mean, std = spec.mean_std(3)
    xf = preprocess_reference(xu, mean, std)
    m._dropout_seed(xu.device)
    rng0 = m._pvr_rng.clone()
    with _E().deterministic_mode():
        a = m(xf)
        a.square().mean().backward()
        ga = m.patch_embedding_block.position_embedding.grad.clone()
        m.zero_grad(set_to_none=True)
        m.set_device_input(spec)
        m._pvr_rng.copy_(rng0)
        b = m(xu)
        b.square().mean().backward()
        gb = m.patch_embedding_block.position_embedding.grad.clone()
    assert a.shape == (4, 10) and torch.equal(a, b) and torch.equal(ga, gb)


# ----------------------------------------------------------------------------- counter behaviour
TRAIN_CFG = dict(image_size=64, patch_size=16, num_transformer_layer=2, num_heads=2, embedding_dim=128, mlp_size=256,
                 num_classes=10, mlp_dropout=0.1, embedding_dropout=0.1)  # n_p = 16


def test_counter_fresh_tables_and_reproducible():
    from pytorch_vit_paper_replication_amd.models import ViT

    E = _E()
    ext = E.ext()
    torch.manual_seed(0)
    m = ViT(**dict(TRAIN_CFG, mlp_dropout=0.0, embedding_dropout=0.0)).to(DEV).set_patch_dropout(RATE).train()
    x = torch.rand(16, 3, 64, 64, device=DEV)
    m._dropout_seed(x.device)
    rng0 = m._pvr_rng.clone()
    with E.deterministic_mode():
        a = m(x).detach().clone()
        seed_a = m._pvr_rng.clone() - 1  # the value the forward snapshotted
        b = m(x).detach().clone()
        seed_b = m._pvr_rng.clone() - 1
        m._pvr_rng.copy_(rng0)
        c = m(x).detach().clone()
    # the option alone needs the counter (every dropout rate is 0 here): it advances once per forward
    assert torch.equal(seed_a, rng0) and torch.equal(seed_b, rng0 + 1)
    ka = ext.patch_keep_table(seed_a, SITE_OFF, 16, 16, 8)[0]
    kb = ext.patch_keep_table(seed_b, SITE_OFF, 16, 16, 8)[0]
    assert not torch.equal(ka, kb) and not torch.equal(a, b)  # two forwards, two tables
    assert torch.equal(a, c)  # the same counter value, the same bits
    assert np.array_equal(ka.cpu().numpy(), O.keep_table(int(rng0.item()), 16, 16, 8))


def test_resume_is_bit_exact_with_patch_dropout(tmp_path):
    from pytorch_vit_paper_replication_amd.models import ViT
    from pytorch_vit_paper_replication_amd.ops.fused_vit import cross_entropy
    from pytorch_vit_paper_replication_amd.optim import FusedAdam, param_groups_weight_decay, warmup_linear_decay
    from pytorch_vit_paper_replication_amd.utils.checkpoint import load_checkpoint, save_checkpoint
    from tests.test_gpu_train import _resume_check

    xs = [torch.rand(8, 3, 64, 64, device=DEV) for _ in range(4)]
    ys = [torch.randint(0, 10, (8,), device=DEV) for _ in range(4)]

    def make(seed):
        torch.manual_seed(seed)
        m = ViT(**TRAIN_CFG).to(DEV).set_patch_dropout(RATE)
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


def test_graphed_step_draws_a_fresh_table_each_replay():
    """Two hipGraph replays against two eager steps started from the same counter value (the tolerance of
    tests/test_gpu_train.test_graphed_train_step_matches_eager). The learning rate is 0 and element dropout
    is off, so the loss of a step depends on its keep table alone: a graph that replayed the captured table
    would give both replays the same loss."""
    from pytorch_vit_paper_replication_amd.models import ViT
    from pytorch_vit_paper_replication_amd.ops.fused_vit import cross_entropy
    from pytorch_vit_paper_replication_amd.optim import FusedAdam, param_groups_weight_decay
    from pytorch_vit_paper_replication_amd.runtime.graph import GraphedTrainStep

    B, WARM, v = 8, 3, 4242
    t0, t1 = (O.keep_table(v + WARM + j, B, 16, 8) for j in (0, 1))
    assert all(not np.array_equal(t0[b], t1[b]) for b in range(B))  # the two replays' tables differ in every sample
    torch.manual_seed(0)
    cfg = dict(TRAIN_CFG, mlp_dropout=0.0, embedding_dropout=0.0)
    ma = ViT(**cfg).to(DEV).set_patch_dropout(RATE)
    mb = ViT(**cfg).to(DEV).set_patch_dropout(RATE)
    mb.load_state_dict(ma.state_dict())
    oa = FusedAdam(param_groups_weight_decay(ma, 0.03), lr=0.0)
    ob = FusedAdam(param_groups_weight_decay(mb, 0.03), lr=0.0)
    x = torch.rand(B, 3, 64, 64, device=DEV)
    y = torch.randint(0, 10, (B,), device=DEV)
    ma._dropout_seed(x.device)
    mb._dropout_seed(x.device)
    ma._pvr_rng.fill_(v)
    mb._pvr_rng.fill_(v)
    rng0 = ma._pvr_rng.clone()
    la = []
    for _ in range(WARM + 2):
        ma.train()
        loss = cross_entropy(ma(x), y)
        oa.zero_grad()
        loss.backward()
        oa.step(clip_norm=1.0)
        la.append(loss.item())
    g = GraphedTrainStep(mb, ob, cross_entropy, x, y, clip_norm=1.0, warmup=WARM)
    lb = [g().item() for _ in range(2)]
    torch.cuda.synchronize()
    assert torch.equal(ma._pvr_rng, rng0 + 5) and torch.equal(mb._pvr_rng, rng0 + 5)  # one value per step, replays included
    print(f"eager losses {la}, replay losses {lb}")
    for a, b in zip(la[WARM:], lb):
        assert abs(a - b) < 2e-2 * max(1.0, abs(a)), (la, lb)
    ext = _E().ext()
    for j, want in ((0, t0), (1, t1)):  # the device's tables at the two replays' counter values are the oracle's
        assert np.array_equal(ext.patch_keep_table(rng0 + WARM + j, SITE_OFF, B, 16, 8)[0].cpu().numpy(), want)
    assert lb[0] != lb[1] and la[WARM] != la[WARM + 1], (la, lb)  # fresh tables: the only thing that differs between the steps


def test_fp8_with_patch_dropout_raises_on_the_gpu():
    from pytorch_vit_paper_replication_amd.models import ViT

    m = ViT(**TRAIN_CFG).to(DEV).set_patch_dropout(RATE).enable_fp8().train()
    with pytest.raises(NotImplementedError, match="enable_fp8.*set_patch_dropout"):
        m(torch.rand(4, 3, 64, 64, device=DEV))
    m.eval()
    with torch.no_grad():
        assert m(torch.rand(4, 3, 64, 64, device=DEV)).shape == (4, 10)  # eval never drops: fp8 inference is unaffected
