"""Host-side validation of the two argument groups every binding shares (csrc/bindings.cpp
``drop_args`` and ``fp8_copy``): a dropout site without its seed, or an fp8 copy without its scale /
with its amax record on the host, raises before any launch; the same call with the argument supplied
runs and passes the existing numerics check of that op (tests/kernel_checks.py, its reference and
limits unchanged) at the same small shape."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from tests import kernel_checks as KC

DEV = "cuda"
P = 0.1
OFF = 3 << 32


def _ext():
    from pytorch_vit_paper_replication_amd import _ext

    return _ext.ext()


def _seed():
    return torch.tensor([4242], dtype=torch.int64, device=DEV)


def _passes(result):
    name, metrics, limits = result
    torch.cuda.synchronize()
    assert KC.passed(metrics, limits), f"{name}: {KC.fmt_metrics(metrics, limits)}"


def test_cls_rows_needs_its_seed():
    """The CLS rows of the token matrix, rows b * ntok of [B * ntok, D]: dropout(cls + pos[0]).

    Reference: the keep mask of the same counter hash from the column-sum kernel on ones (as
    check_patch_bwd draws it), the kept values (cls + pos) * scale in fp32 with the kernel's scale
    65536 / (65536 - thr), rounded to bf16 once. The kernel performs the same fp32 operations, so the
    only difference allowed is the final rounding: one bf16 ulp, 2^-8 relative (l2 and max)."""
    ext = _ext()
    B, ntok, D = 2, 5, 64
    torch.manual_seed(0)
    cls, pos = torch.randn(D, device=DEV), torch.randn(D, device=DEV)
    out = torch.full((B * ntok, D), 7.0, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(RuntimeError):
        ext.cls_rows(cls, pos, out, B, D, ntok * D, None, OFF, P)
    assert bool((out == 7.0).all().item()), "a rejected call must not launch"
    ext.cls_rows(cls, pos, out, B, D, ntok * D, _seed(), OFF, P)
    mask = torch.empty(B * ntok, D, dtype=torch.bfloat16, device=DEV)
    ext.colsum(torch.ones(B * ntok, D, dtype=torch.bfloat16, device=DEV), B * ntok, D, None, mask, _seed(), OFF, P)
    thr = min(int(round(P * 65536)), 65535)
    keep = (mask.float() != 0).view(B, ntok, D)[:, 0]
    ref = ((cls + pos) * keep.float() * (65536.0 / (65536.0 - thr))).to(torch.bfloat16)
    got = out.view(B, ntok, D)
    l2, mx = KC.errs(got[:, 0], ref)
    print(f"cls_rows B{B} D{D} p{P}: l2={l2:.2e} max={mx:.2e} (limit 2^-8 = {2.0 ** -8:.2e})")
    assert torch.equal(got[:, 0] == 0, ~keep | (ref == 0)), "dropout mask differs from the shared hash"
    assert l2 <= 2.0 ** -8 and mx <= 2.0 ** -8
    assert bool((got[:, 1:] == 7.0).all().item()), "rows other than the CLS rows were written"
    # without dropout the seed stays optional
    ext.cls_rows(cls, pos, out, B, D, ntok * D, None, 0, 0.0)
    assert torch.equal(got[:, 0], (cls + pos).to(torch.bfloat16).expand(B, D))


def test_patch_bwd_needs_its_seed():
    ext = _ext()
    B, ntok, D = 2, 5, 64
    dE = torch.randn(B * ntok, D, device=DEV).to(torch.bfloat16)
    gpos, gcls, gb = torch.zeros(ntok * D, device=DEV), torch.zeros(D, device=DEV), torch.zeros(D, device=DEV)
    dconv = torch.empty(B * (ntok - 1), D, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(RuntimeError):
        ext.patch_bwd(dE, B, ntok, D, gpos, gcls, dconv, gb, None, OFF, P)
    assert not bool(gpos.any().item() or gcls.any().item() or gb.any().item()), "a rejected call must not launch"
    torch.manual_seed(1)
    _passes(KC.check_patch_bwd(B, ntok, D, P))


def test_colsum_copy_needs_its_scale():
    ext = _ext()
    T, N = 8, 64
    dy = torch.randn(T, N, device=DEV).to(torch.bfloat16)
    db = torch.zeros(N, device=DEV)
    q = torch.zeros(T, N, dtype=torch.uint8, device=DEV)
    amax = torch.zeros(1, dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError):
        ext.colsum(dy, T, N, db, None, None, 0, 0.0, q, None, amax, 1)
    assert not bool(db.any().item() or q.any().item() or amax.any().item()), "a rejected call must not launch"
    torch.manual_seed(2)
    _passes(KC.check_colsum_q8(T, N, 1))


def test_attn_fwd_copy_needs_a_device_amax():
    ext = _ext()
    B, N, H, dh = 2, 17, 1, 64
    qkv = torch.randn(B * N, 3 * H * dh, device=DEV).to(torch.bfloat16)
    q = torch.zeros(B * N, H * dh, dtype=torch.uint8, device=DEV)
    scale = torch.full((1,), 300.0, device=DEV)
    amax_cpu = torch.zeros(1, dtype=torch.int32)
    with pytest.raises(RuntimeError):
        ext.attn_fwd(qkv, B, N, H, 1.0 / math.sqrt(dh), None, 0, 0.0, q, scale, amax_cpu)
    assert not bool(q.any().item() or amax_cpu.any().item()), "a rejected call must not launch"
    torch.manual_seed(3)
    _passes(KC.check_attn_fwd_q8(B, N, H, dh))
