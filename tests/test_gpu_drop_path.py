"""Stochastic depth (drop path) on the fused path.

* the row-scale term of the residual GEMM epilogue at every code site (tiles 0, 6, 12, 13 with the
  register-direct and the staged ping-pong epilogue, and the split-K tail), against the numpy replica of the counter hash (tests/test_drop_path_cpu.py) for the
  keep decisions and an fp32 product for the kept rows;
* the LayerNorm-backward ``dz`` output and the column-sum kernel with the row scale;
* the host checks of the unsupported combinations;
* one training step of a small ViT (class-token last block on and off) against the fp32 reference
  model with the dropout masks and the drop-path vectors replayed;
* the device counter: fresh draws every forward, reproducible from the counter, bit-exact resume, and
  hipGraph replays.

Seeds are chosen on the CPU with the numpy replica so that every case has dropped and kept samples;
each test asserts that condition itself.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import test_drop_path_cpu as H  # the numpy oracle of the keep decisions

pytestmark = pytest.mark.gpu

DEV = "cuda"
P = 0.5  # thr16 = 32768, scale = 2 exactly


def _kc():
    from tests import kernel_checks as KC

    return KC


def _ext():
    from pytorch_vit_paper_replication_amd import _ext

    return _ext


def _seed_tensor(v):
    return torch.tensor([v], dtype=torch.int64, device=DEV)


def pick_seed(cond, start=1000):
    """The first counter value >= start for which ``cond(value)`` holds (host only, numpy oracle)."""
    for v in range(start, start + 10000):
        if cond(v):
            return v
    raise AssertionError("no seed found")


def keep_of(seed, site, batch, p=P):
    return H.rng_keep(H.site_seed(seed, site), np.arange(batch), H.thr16(p))


def _mixed(k, lo=2):
    return int(k.sum()) >= lo and int((~k).sum()) >= lo


# ----------------------------------------------------------------------------- the scale vector binding
def test_drop_path_scale_binding_matches_the_numpy_oracle():
    ext = _ext().ext()
    for seed, site, p, B in [(5, 0, 0.5, 8), (123456789012345, H.DROP_PATH_SITE + 3, 0.1, 257), (2 ** 62 + 17, 7, 0.9, 33)]:
        s = ext.drop_path_scale(_seed_tensor(seed), site << 32, p, B)
        keep = H.rng_keep(H.site_seed(seed, site), np.arange(B), H.thr16(p))
        want = torch.from_numpy(np.where(keep, H.keep_scale(p), np.float32(0)).astype(np.float32))
        assert s.dtype == torch.float32 and torch.equal(s.cpu(), want)
    assert torch.equal(ext.drop_path_scale(_seed_tensor(1), 0, 0.0, 4).cpu(), torch.ones(4))


# ----------------------------------------------------------------------------- GEMM epilogue
SITE = H.DROP_PATH_SITE + 4
# the limits kernel_checks.check_gemm_fwd applies to the residual GEMM
GEMM_LIM = dict(l2=3.5e-3, max=7e-3)


def _epilogue_case(B, N, K, C, seed):
    torch.manual_seed(B * 7 + N)
    T = B * N
    x = (torch.randn(T, K, device=DEV) + 0.5).to(torch.bfloat16)
    w = (0.1 * torch.randn(C, K, device=DEV)).to(torch.bfloat16)
    bias = torch.randn(C, device=DEV) + 3.0  # keeps kept outputs away from their residual
    resid = torch.randn(T, C, device=DEV).to(torch.bfloat16)
    st = _seed_tensor(seed)
    return x, w, bias, resid, st


def _check_epilogue(out, x, w, bias, resid, keep, N, name):
    """Rows equal to the residual bit for bit are exactly the dropped samples' rows; kept rows are
    bf16(resid + 2 * (x w^T + bias)) within the residual GEMM's limits."""
    KC = _kc()
    rowkeep = torch.from_numpy(np.repeat(keep, N)).to(DEV)
    same = (out == resid).all(dim=1) & (out.view(torch.int16) == resid.view(torch.int16)).all(dim=1)
    assert torch.equal(same, ~rowkeep), f"{name}: rows equal to the residual are not the dropped samples' rows"
    ref = resid.float() + 2.0 * (x.float() @ w.float().t() + bias)
    m = KC.worst((out[rowkeep], ref[rowkeep].to(torch.bfloat16)))
    print(f"{name}: {KC.fmt_metrics(m, GEMM_LIM)}")
    assert KC.passed(m, GEMM_LIM), f"{name}: {KC.fmt_metrics(m, GEMM_LIM)}"


def _epilogue_assertions(run, B, N, K, C, name):
    """``run(x, w, bias, resid, drop, dp)`` is one residual GEMM (``drop`` / ``dp`` None: without): drop path
    alone, then with element dropout against the same call without drop path."""
    KC = _kc()
    seed = pick_seed(lambda v: _mixed(keep_of(v, SITE, B)))
    keep = keep_of(seed, SITE, B)
    assert _mixed(keep)
    x, w, bias, resid, st = _epilogue_case(B, N, K, C, seed)
    dp = (st, SITE << 32, P, N)
    out = run(x, w, bias, resid, None, dp)
    _check_epilogue(out, x, w, bias, resid, keep, N, f"{name} drop path")
    # with element dropout: inside kept rows the zero pattern (out == resid) is that of the call without drop path
    drop = (st, 9 << 32, P)
    both = run(x, w, bias, resid, drop, dp)
    plain = run(x, w, bias, resid, drop, None)
    rowkeep = torch.from_numpy(np.repeat(keep, N)).to(DEV)
    # (an element reads as dropped when out == resid. A kept one whose branch value is below half a bf16
    # ulp of its residual reads so too, at 2 v or at 4 v: only values that cannot vanish, |v| > 0.05 against
    # residuals below 8, are compared. The dropout mask does not depend on v, so nothing is lost.)
    v = x.float() @ w.float().t() + bias
    sure = (v.abs() > 0.05) & (resid.float().abs() < 8) & rowkeep.view(-1, 1)
    assert sure.float().mean().item() > 0.9 * rowkeep.float().mean().item()
    assert torch.equal((both == resid)[sure], (plain == resid)[sure])
    frac = (plain == resid)[sure].float().mean().item()
    assert 0.4 < frac < 0.6
    assert torch.equal(both[~rowkeep].view(torch.int16), resid[~rowkeep].view(torch.int16))
    # kept elements of kept rows: resid + 4 * (x w^T + bias), the folded factor drop_scale * dp_scale
    ref = resid.float() + 4.0 * v
    sel = sure & (plain != resid)
    m = KC.worst((both[sel], ref[sel].to(torch.bfloat16)))
    assert KC.passed(m, GEMM_LIM), KC.fmt_metrics(m, GEMM_LIM)


@pytest.mark.parametrize("tile,B,N,K,C", [(12, 11, 197, 128, 320), (13, 11, 197, 128, 320), (0, 6, 5, 64, 128), (0, 11, 197, 128, 320),
                                          (6, 11, 197, 192, 320)])
def test_epilogue_row_scale(tile, B, N, K, C):
    """T = 2167 rows: a partial last row tile, and sample boundaries inside the 16-row fragments. Tile 6 (the
    BK-32 ring) gets K = 192, a multiple of 64 (the binding takes no other K for row-major operands) but
    not of the 128 its two-stage neighbours prefer: an odd number of 64-deep K-tiles. At these sizes tiles 12
    and 13 take their register-direct epilogue; the staged one has the test below."""
    from pytorch_vit_paper_replication_amd.ops import gemm as G

    def run(x, w, bias, resid, drop, dp):
        with _kc().tile(tile):
            return G.linear_fwd(x, w, bias, resid=resid, drop=drop, drop_path=dp)

    _epilogue_assertions(run, B, N, K, C, f"tile {tile}")


@pytest.mark.parametrize("tile", [12, 13])
def test_epilogue_row_scale_staged(tile):
    """The ping-pong kernels' LDS-staged epilogue, which a production call reaches only where the
    register-direct one cannot address the output (2^31 bytes and more): forced here with the kernel's
    ``epi_staged`` argument, 128 rows per pass on the one-tile kernel (12) and 32 on the persistent one (13)."""
    from pytorch_vit_paper_replication_amd.ops import gemm as G

    ext = _ext().ext()
    B, N, K, C = 11, 197, 128, 320

    def run(x, w, bias, resid, drop, dp):
        out = torch.empty_like(resid)
        seed, soff, p = G._drop_args(drop)
        ext.gemm(x, True, w, True, out, B * N, C, K, G.EPI_BF16, bias, resid, None, 0, None, 0, 0, 0, seed, soff, p, 0, tile,
                 epi_staged=1, **G._drop_path_kw(dp))
        return out

    _epilogue_assertions(run, B, N, K, C, f"tile {tile} staged")


def test_epilogue_compact_class_rows_equal_the_full_call():
    """Tile 0, ``dp_rows = 1`` with ``drop_row_mul = N``: B compact rows draw what rows b * N of the full call draw."""
    from pytorch_vit_paper_replication_amd.ops import gemm as G

    KC = _kc()
    B, N, K, C = 6, 5, 64, 128
    seed = pick_seed(lambda v: _mixed(keep_of(v, SITE, B)))
    keep = keep_of(seed, SITE, B)
    assert _mixed(keep)
    x, w, bias, resid, st = _epilogue_case(B, N, K, C, seed)
    drop = (st, 9 << 32, P)
    with KC.tile(0):
        full = G.linear_fwd(x, w, bias, resid=resid, drop=drop, drop_path=(st, SITE << 32, P, N))
        comp = G.linear_fwd(x[::N].contiguous(), w, bias, resid=resid.view(B, N, C)[:, 0], drop=drop, drop_row_mul=N,
                            drop_path=(st, SITE << 32, P, 1))
        comp_nodrop = G.linear_fwd(x[::N].contiguous(), w, bias, resid=resid.view(B, N, C)[:, 0],
                                   drop_path=(st, SITE << 32, P, 1))
    assert comp.shape == (B, C)
    assert torch.equal(full[::N].view(torch.int16), comp.view(torch.int16))
    _check_epilogue(comp_nodrop, x[::N], w, bias, resid[::N].contiguous(), keep, 1, "tile 0 compact rows")


def test_epilogue_row_scale_on_the_split_k_tail():
    """The last dispatch round of a long-K GEMM runs as K-parts; the part that arrives last runs the same
    epilogue (ViT-B/16 b256 token count, K = 2304: three parts of 12 K-tiles)."""
    from pytorch_vit_paper_replication_amd.ops import gemm as G

    KC = _kc()
    B, N, K, C = 256, 197, 2304, 768
    S = _ext().ext().gemm_tail_split(B * N, C, K, 2)
    assert S >= 2, "this shape no longer takes the split-K tail"
    seed = pick_seed(lambda v: _mixed(keep_of(v, SITE, B), 64))
    keep = keep_of(seed, SITE, B)
    x, w, bias, resid, st = _epilogue_case(B, N, K, C, seed)
    w = w * 0.2
    with KC.tile(12):
        out = G.linear_fwd(x, w, bias, resid=resid, drop_path=(st, SITE << 32, P, N))
    _check_epilogue(out, x, w, bias, resid, keep, N, f"tile 12 split-K tail ({S} parts)")


# ----------------------------------------------------------------------------- LayerNorm backward
LN_SITE = H.DROP_PATH_SITE + 9


def _ln_inputs(B, N, D):
    ext = _ext().ext()
    torch.manual_seed(B * 1000 + N + D)
    T = B * N
    x = torch.randn(T, D, device=DEV).to(torch.bfloat16)
    dy = torch.randn(T, D, device=DEV).to(torch.bfloat16)
    w, b = torch.randn(D, device=DEV), torch.randn(D, device=DEV)
    _, mean, rstd = ext.layernorm_fwd(x, w, b, 1e-5, T, D)
    return x, dy, w, mean, rstd


def _ln_bwd(inp, dres, every, T, D, **kw):
    ext = _ext().ext()
    x, dy, w, mean, rstd = inp
    dx = torch.empty(T, D, dtype=torch.bfloat16, device=DEV)
    dz = torch.empty_like(dx) if kw.pop("want_dz", True) else None
    dw, db, ds = (torch.zeros(D, device=DEV) for _ in range(3))
    ext.layernorm_bwd(dy, D, x, D, mean, rstd, w, dres, D, dx, D, dw, db, T, dsum=ds, dz=dz, dres_every=every, **kw)
    return dx, dz, dw, db, ds


@pytest.mark.parametrize("sparse", [False, True])
@pytest.mark.parametrize("B,N,D,want", [(3, 5, 128, None), (2, 197, 768, None), (1, 1, 256, True), (1, 1, 256, False)])
def test_layernorm_bwd_dz_row_scale(B, N, D, want, sparse):
    """``want``: for the single-sample shape, whether that sample is kept (both cases run)."""
    E = _ext()
    T = B * N
    if want is None:
        seed = pick_seed(lambda v: _mixed(keep_of(v, LN_SITE, B), 1))
    else:
        seed = pick_seed(lambda v: bool(keep_of(v, LN_SITE, B)[0]) == want)
    keep = keep_of(seed, LN_SITE, B)
    assert (0 < keep.sum() < B) if want is None else bool(keep[0]) == want
    rowkeep = torch.from_numpy(np.repeat(keep, N)).to(DEV)
    inp = _ln_inputs(B, N, D)
    if sparse:
        dres, every = torch.randn(B, D, device=DEV).to(torch.bfloat16), N
    else:
        dres, every = torch.randn(T, D, device=DEV).to(torch.bfloat16), 0
    st = _seed_tensor(seed)
    dpkw = dict(dp_seed=st, dp_offset=LN_SITE << 32, dp_p=P, dp_rows=N)
    dropkw = dict(seed=st, seed_offset=4 << 32, drop_p=P)
    with E.deterministic_mode():
        base = _ln_bwd(inp, dres, every, T, D, want_dz=False)
        only = _ln_bwd(inp, dres, every, T, D, **dpkw)  # the drop-path-only dz
        drop = _ln_bwd(inp, dres, every, T, D, **dropkw)
        both = _ln_bwd(inp, dres, every, T, D, **dropkw, **dpkw)
    torch.cuda.synchronize()
    for name, r in (("drop path only", only), ("dropout + drop path", both)):
        dx, dz, dw, db, ds = r
        # dx, dgamma, dbeta do not see the row scale
        assert torch.equal(dx, base[0]) and torch.equal(dw, base[2]) and torch.equal(db, base[3]), name
        assert (dz[~rowkeep] == 0).all(), name
        torch.testing.assert_close(ds, dz.float().sum(0), rtol=1e-5, atol=1e-4)
    # drop path only: dz = 2 * dx on kept rows, bit for bit (doubling a bf16 is exact)
    assert torch.equal(only[1][rowkeep].view(torch.int16), (2 * base[0][rowkeep]).view(torch.int16))
    # with dropout (scale 2 at p = 0.5): kept rows are twice the dropout-only dz, so the same zero pattern
    assert torch.equal(both[1][rowkeep].view(torch.int16), (2 * drop[1][rowkeep]).view(torch.int16))
    if rowkeep.any():
        z = (drop[1][rowkeep] == 0).float().mean().item()
        assert 0.3 < z < 0.7


# ----------------------------------------------------------------------------- column sums
CS_SITE = H.DROP_PATH_SITE + 1


def test_colsum_row_scale_plain_and_compact():
    from pytorch_vit_paper_replication_amd.ops import gemm as G

    B, N, C = 6, 5, 128
    seed = pick_seed(lambda v: _mixed(keep_of(v, CS_SITE, B)))
    keep = keep_of(seed, CS_SITE, B)
    assert _mixed(keep)
    st = _seed_tensor(seed)
    drop = (st, 7 << 32, P)
    torch.manual_seed(5)
    dy = (torch.randn(B * N, C, device=DEV) + 3.0).to(torch.bfloat16)
    rowkeep = torch.from_numpy(np.repeat(keep, N)).to(DEV)
    bkeep = torch.from_numpy(keep).to(DEV)

    def run(src, rows_keep, **kw):
        dz, db = torch.empty_like(src), torch.zeros(C, device=DEV)
        G.bias_grad(src, db, dz=dz, **kw)
        if "drop_path" in kw:
            assert (dz[~rows_keep] == 0).all()
        torch.testing.assert_close(db, dz.float().sum(0), rtol=1e-5, atol=1e-4)
        return dz

    with _ext().deterministic_mode():
        # every token row: N rows per sample
        only = run(dy, rowkeep, drop_path=(st, CS_SITE << 32, P, N))
        assert torch.equal(only[rowkeep].view(torch.int16), (2 * dy[rowkeep]).view(torch.int16))
        plain = run(dy, rowkeep, drop=drop)
        both = run(dy, rowkeep, drop=drop, drop_path=(st, CS_SITE << 32, P, N))
        assert torch.equal(both[rowkeep].view(torch.int16), (2 * plain[rowkeep]).view(torch.int16))
        assert 0.3 < (plain == 0).float().mean().item() < 0.7
        # the compact class-token rows: the dropout mask of rows b * N (row_mul), one row per sample (dp_rows = 1)
        dyc = dy[::N].contiguous()
        comp = run(dyc, bkeep, drop=drop, row_mul=N, drop_path=(st, CS_SITE << 32, P, 1))
        assert torch.equal(comp.view(torch.int16), both[::N].view(torch.int16))
        comp_only = run(dyc, bkeep, drop_path=(st, CS_SITE << 32, P, 1))
        assert torch.equal(comp_only.view(torch.int16), only[::N].view(torch.int16))
    # and it is the mask the forward epilogue of the same site draws
    s = _ext().ext().drop_path_scale(st, CS_SITE << 32, P, B)
    assert torch.equal(s != 0, bkeep)


# ----------------------------------------------------------------------------- host checks
def test_host_checks_name_drop_path():
    from pytorch_vit_paper_replication_amd.ops import gemm as G

    ext = _ext().ext()
    x = torch.zeros(8, 64, dtype=torch.bfloat16, device=DEV)
    w = torch.zeros(128, 64, dtype=torch.bfloat16, device=DEV)
    out = torch.empty(8, 128, dtype=torch.bfloat16, device=DEV)
    seed = _seed_tensor(1)
    dp = dict(dp_seed=seed, dp_offset=0, dp_p=0.5, dp_rows=2)

    def gemm(epi=0, resid=out, tile=0, row_group=0, **kw):
        ext.gemm(x, True, w, True, out, 8, 128, 64, epi, None, resid, None, 0, None, row_group, row_group, 0, None, 0, 0.0, 0, tile,
                 **dict(dp, **kw))

    with pytest.raises(RuntimeError, match="drop_path"):  # the wave-specialised tile has no row-scale term
        gemm(tile=15)
    with pytest.raises(RuntimeError, match="drop_path"):  # nor the split-K partial-store tile
        gemm(tile=14)
    with pytest.raises(RuntimeError, match="drop_path"):  # it scales a residual branch: a residual is required
        gemm(resid=None)
    with pytest.raises(RuntimeError, match="drop_path"):
        gemm(epi=1)
    with pytest.raises(RuntimeError, match="drop_path"):
        gemm(row_group=4)
    with pytest.raises(RuntimeError, match="drop_path"):
        gemm(dp_rows=0)
    with pytest.raises(RuntimeError, match="drop_path"):
        gemm(dp_seed=None)
    with pytest.raises(ValueError, match="drop_path"):
        G.linear_fwd(x, w, None, drop_path=(seed, 0, 0.5, 2))
    with pytest.raises(ValueError, match="drop_path"):
        G.linear_fwd(x, w, None, resid=out, gelu=True, drop_path=(seed, 0, 0.5, 2))
    # LayerNorm backward / column sums: the row scale is a property of dz, and not of the fp8 copies
    d = torch.zeros(8, 128, dtype=torch.bfloat16, device=DEV)
    f = torch.zeros(128, device=DEV)
    q = torch.empty(8, 128, dtype=torch.uint8, device=DEV)
    amax = torch.zeros(1, dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError, match="drop_path"):
        ext.layernorm_bwd(d, 128, d, 128, f[:8], f[:8], f, None, 0, torch.empty_like(d), 128, None, None, 8, **dp)
    with pytest.raises(RuntimeError, match="drop_path"):
        ext.layernorm_bwd(d, 128, d, 128, f[:8], f[:8], f, None, 0, torch.empty_like(d), 128, None, None, 8, dz=torch.empty_like(d),
                          q_out=q, q_scale=f[:1], q_amax=amax, **dp)
    with pytest.raises(RuntimeError, match="drop_path"):
        ext.colsum(d, 8, 128, f, torch.empty_like(d), None, 0, 0.0, q_out=q, q_scale=f[:1], q_amax=amax, **dp)
    with pytest.raises(ValueError, match="drop_path"):
        G.bias_grad(d, f, quant=(None, 0), drop_path=(seed, 0, 0.5, 2))


# ----------------------------------------------------------------------------- whole model
# exactly the configuration and limits of tests/test_gpu_cls_last_block.py
CFG = dict(image_size=32, patch_size=8, num_heads=2, embedding_dim=128, mlp_size=256, num_classes=10,
           mlp_dropout=0.1, embedding_dropout=0.1)
LIMITS = dict(logits_l2=2.1e-2, logits_max=2.8e-2, grad_l2=2.5e-2, grad_max=3.6e-2)


def _model_keeps(seed, depth, B):
    return [[keep_of(seed, H.DROP_PATH_SITE + 2 * i + br, B) for br in (0, 1)] for i in range(depth)]


def _reference_step_dp(mr, x, y, seed, B, train=True):
    """tests/test_gpu_cls_last_block._reference_step with the drop-path vectors of ``ext.drop_path_scale``
    replayed into the blocks' draw function as well."""
    from tests import test_gpu_cls_last_block as CL

    ext = _ext().ext()
    patched = []
    if train:
        for i, blk in enumerate(mr.transformer_encoder):
            def draw(batch, p, branch, device, i=i):
                s = ext.drop_path_scale(seed, (H.DROP_PATH_SITE + 2 * i + branch) << 32, p, batch)
                return s != 0

            blk._draw_drop_path = draw
            patched.append(blk)
    try:
        return CL._reference_step(mr, x, y, seed, B, train=train)
    finally:
        for blk in patched:
            del blk._draw_drop_path


@pytest.fixture(scope="module")
def dp_parity():
    cache = {}

    def get(depth, B=8):
        if depth in cache:
            return cache[depth]
        from pytorch_vit_paper_replication_amd.models import ViT
        from tests import test_gpu_cls_last_block as CL

        torch.manual_seed(depth * 10 + B)
        cfg = dict(CFG, num_transformer_layer=depth)
        mf = ViT(**cfg).to(DEV).set_drop_path(P, "constant")
        mr = ViT(**cfg).to(DEV).set_drop_path(P, "constant")
        mp = ViT(**cfg).to(DEV)  # the same weights without the option
        mr.load_state_dict(mf.state_dict())
        mp.load_state_dict(mf.state_dict())
        x = torch.rand(B, 3, 32, 32, device=DEV)
        y = torch.randint(0, 10, (B,), device=DEV)
        assert mf._fused_supported(x)
        # a counter value at which every block has a dropped and a kept sample in each branch
        v = pick_seed(lambda s: all(_mixed(k, 1) for blk in _model_keeps(s, depth, B) for k in blk), start=31337)
        mf._dropout_seed(x.device)
        mf._pvr_rng.fill_(v)
        mp._dropout_seed(x.device)
        mp._pvr_rng.fill_(v)
        rng0 = mf._pvr_rng.clone()
        out = {"N": mr.patch_embedding_block.number_of_patches + 1, "B": B, "seed": v}
        out["ref"] = _reference_step_dp(mr, x, y, rng0, B) + ({n: p.grad.detach().clone() for n, p in mr.named_parameters()},)
        for name, on in (("cls", True), ("full", False)):
            out[name] = CL._fused_step(mf, x, y, rng0, on)
            out[name + "_eval"] = CL._fused_step(mf, x, y, rng0, on, train=False)
            out[name + "_plain_eval"] = CL._fused_step(mp, x, y, rng0, on, train=False)
        cache[depth] = out
        return out

    return get


@pytest.mark.parametrize("depth", [1, 3])
def test_training_step_parity_with_drop_path(dp_parity, depth):
    from tests import test_gpu_cls_last_block as CL

    r = dp_parity(depth)
    B, N = r["B"], r["N"]
    keeps = _model_keeps(r["seed"], depth, B)
    assert all(0 < k.sum() < B for blk in keeps for k in blk)  # every block drops and keeps in each branch
    # the class-token block ran: its fc2 / fc1 / out dgrads have B rows, its qkv dgrad B * N
    assert r["cls"][3][:4] == [(0, B), (1, B), (2, B), (3, B * N)]
    assert all(rows == B * N for _, rows in r["full"][3]) and len(r["full"][3]) == 4 * depth == len(r["cls"][3])
    for name in ("full", "cls"):
        m, limits = CL._arm_metrics(r[name], r["ref"])
        CL._report(f"vit depth {depth} batch {B} drop path {name} arm vs fp32 with the same masks", m, limits)
    # eval never drops: the logits of the same weights without the option, bit for bit
    for name in ("full", "cls"):
        assert torch.equal(r[name + "_eval"][1], r[name + "_plain_eval"][1])


def test_drop_path_changes_the_step_and_rate_zero_does_not():
    """Guards the parity test against a vacuous pass: with the option on the training logits differ from the
    plain model's, and ``set_drop_path(0)`` restores them bit for bit (today's code path)."""
    from pytorch_vit_paper_replication_amd.models import ViT
    from tests import test_gpu_cls_last_block as CL

    torch.manual_seed(4)
    cfg = dict(CFG, num_transformer_layer=2)
    m = ViT(**cfg).to(DEV)
    x = torch.rand(8, 3, 32, 32, device=DEV)
    y = torch.randint(0, 10, (8,), device=DEV)
    m._dropout_seed(x.device)
    rng0 = m._pvr_rng.clone()
    plain = CL._fused_step(m, x, y, rng0, True)
    m.set_drop_path(P, "constant")
    on = CL._fused_step(m, x, y, rng0, True)
    m.set_drop_path(0.0)
    off = CL._fused_step(m, x, y, rng0, True)
    assert not torch.equal(plain[1], on[1])
    assert torch.equal(plain[1], off[1]) and all(torch.equal(plain[2][n], off[2][n]) for n in plain[2])
    # a rate below the 16-bit resolution (thr16 = 0) can drop nothing: such a block runs as one without the
    # option, forward and backward; block 1 of the second model has thr16 = 1 and keeps the term
    m.set_drop_path(1e-6, "constant")
    tiny = CL._fused_step(m, x, y, rng0, True)
    assert torch.equal(plain[1], tiny[1]) and all(torch.equal(plain[2][n], tiny[2][n]) for n in plain[2])
    m.set_drop_path(1e-5)
    assert [H.thr16(p) for p in m.drop_path_rates()] == [0, 1]
    mixed = CL._fused_step(m, x, y, rng0, True)
    assert all(torch.isfinite(g).all() for g in mixed[2].values())


# ----------------------------------------------------------------------------- counter behaviour
TRAIN_CFG = dict(image_size=64, patch_size=16, num_transformer_layer=2, num_heads=2, embedding_dim=128, mlp_size=256,
                 num_classes=10, mlp_dropout=0.1, embedding_dropout=0.1)


def test_counter_fresh_draws_and_reproducible():
    from pytorch_vit_paper_replication_amd.models import ViT

    E = _ext()
    ext = E.ext()
    torch.manual_seed(0)
    m = ViT(**dict(TRAIN_CFG, mlp_dropout=0.0, embedding_dropout=0.0)).to(DEV).set_drop_path(P, "constant").train()
    x = torch.rand(16, 3, 64, 64, device=DEV)
    m._dropout_seed(x.device)
    rng0 = m._pvr_rng.clone()
    with E.deterministic_mode(), torch.no_grad():
        a = m(x).clone()
        seed_a = m._pvr_rng.clone() - 1  # the value the forward snapshotted
        b = m(x).clone()
        seed_b = m._pvr_rng.clone() - 1
        m._pvr_rng.copy_(rng0)
        c = m(x).clone()
    assert torch.equal(seed_a, rng0) and torch.equal(seed_b, rng0 + 1)  # need_seed: the counter advances per forward
    ka = ext.drop_path_scale(seed_a, H.DROP_PATH_SITE << 32, P, 16)
    kb = ext.drop_path_scale(seed_b, H.DROP_PATH_SITE << 32, P, 16)
    assert not torch.equal(ka, kb) and not torch.equal(a, b)  # two forwards, two keep vectors
    assert torch.equal(a, c)  # the same counter value, the same bits


def test_resume_is_bit_exact_with_drop_path(tmp_path):
    from pytorch_vit_paper_replication_amd.models import ViT
    from pytorch_vit_paper_replication_amd.ops.fused_vit import cross_entropy
    from pytorch_vit_paper_replication_amd.optim import FusedAdam, param_groups_weight_decay, warmup_linear_decay
    from pytorch_vit_paper_replication_amd.utils.checkpoint import load_checkpoint, save_checkpoint
    from tests.test_gpu_train import _resume_check

    xs = [torch.rand(8, 3, 64, 64, device=DEV) for _ in range(4)]
    ys = [torch.randint(0, 10, (8,), device=DEV) for _ in range(4)]

    def make(seed):
        torch.manual_seed(seed)
        m = ViT(**TRAIN_CFG).to(DEV).set_drop_path(0.3)
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

    with _ext().deterministic_mode():
        _resume_check(make, run, False, tmp_path, save_checkpoint, load_checkpoint)


def test_graphed_step_draws_fresh_masks_from_the_counter():
    """Two hipGraph replays against two eager steps started from the same counter value (the tolerance
    of tests/test_gpu_train.test_graphed_train_step_matches_eager): every replay reads the advancing
    device counter, so it draws the keep vectors the eager step draws.

    The learning rate is 0 and element dropout is off, so the weights stay as they are and the loss of a
    step depends on its keep vectors alone: a graph that replayed the captured draws would give both
    replays the same loss, which the last assertion excludes. The starting counter value is chosen so that
    the two replays' keep vectors differ at every site."""
    from pytorch_vit_paper_replication_amd.models import ViT
    from pytorch_vit_paper_replication_amd.ops.fused_vit import cross_entropy
    from pytorch_vit_paper_replication_amd.optim import FusedAdam, param_groups_weight_decay
    from pytorch_vit_paper_replication_amd.runtime.graph import GraphedTrainStep

    B, WARM = 8, 3
    sites = range(H.DROP_PATH_SITE, H.DROP_PATH_SITE + 4)  # two blocks, two branches
    v = pick_seed(lambda s: all(_mixed(keep_of(s + WARM + j, site, B), 1) for site in sites for j in (0, 1))
                  and all((keep_of(s + WARM, site, B) != keep_of(s + WARM + 1, site, B)).any() for site in sites), start=4242)
    torch.manual_seed(0)
    cfg = dict(TRAIN_CFG, mlp_dropout=0.0, embedding_dropout=0.0)
    ma = ViT(**cfg).to(DEV).set_drop_path(P, "constant")
    mb = ViT(**cfg).to(DEV).set_drop_path(P, "constant")
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
    # the keep vectors of the two replays' counter values, from the device: the oracle's, and not each other's
    ext = _ext().ext()
    for site in sites:
        k = [ext.drop_path_scale(rng0 + WARM + j, site << 32, P, B) for j in (0, 1)]
        for j in (0, 1):
            assert torch.equal((k[j] != 0).cpu(), torch.from_numpy(keep_of(v + WARM + j, site, B)))
        assert not torch.equal(k[0], k[1])
    assert lb[0] != lb[1] and la[WARM] != la[WARM + 1], (la, lb)  # fresh draws: the only thing that differs between the steps


def test_fp8_with_drop_path_raises_on_the_gpu():
    from pytorch_vit_paper_replication_amd.models import ViT

    m = ViT(**TRAIN_CFG).to(DEV).set_drop_path(0.1).enable_fp8().train()
    with pytest.raises(NotImplementedError, match="enable_fp8.*set_drop_path"):
        m(torch.rand(4, 3, 64, 64, device=DEV))
    m.eval()
    with torch.no_grad():
        assert m(torch.rand(4, 3, 64, 64, device=DEV)).shape == (4, 10)  # eval never drops: fp8 inference is unaffected
