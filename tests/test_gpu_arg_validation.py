"""Host-side validation of the two argument groups every binding shares (csrc/bindings.cpp
``drop_args`` and ``fp8_copy``): a dropout site without its seed, or an fp8 copy without its scale /
with its amax record on the host, raises before any launch; the same call with the argument supplied
runs and passes the existing numerics check of that op (tests/kernel_checks.py, its reference and
limits unchanged) at the same small shape. The optimizer bindings (``adam``, ``adam_t``, ``grad_norm``)
pass raw pointers and counts: each argument their kernels dereference is rejected here unless it is
what the kernel assumes (device, dtype, contiguity, alignment, element count)."""
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


# ----------------------------------------------------------------------------- optimizer bindings
# adam / adam_t / grad_norm hand raw pointers and counts to their kernels: every argument a kernel
# dereferences is rejected on the host (csrc/bindings.cpp flat_f32, flat_bf16, clip_triple, the segment
# and group table checks) unless it is what the kernel assumes. Each case below is one such check.
def _adam_args(n=8):
    """A valid ext.adam call on sentinel buffers: n = 8, two 4-element segments (a one-element table
    counts as contiguous whatever its stride, so the strided cases need two)."""
    import numpy as np

    full = lambda dt=torch.float32: torch.full((n,), KC.SENTINEL, dtype=dt, device=DEV)  # noqa: E731
    table = torch.from_numpy(KC._adam_table(1, 3))
    assert table.dtype == torch.float32 and tuple(table.shape) == (3, 10) and np.isfinite(table.numpy()).all()
    return dict(p=full(), g=full(), m=full(), v=full(), shadow=full(torch.bfloat16),
                seg_start=torch.tensor([0, 4], dtype=torch.int64, device=DEV), seg_group=torch.ones(2, dtype=torch.int32, device=DEV),
                groups=table, clip=torch.tensor([1.0, 0.5, 0.0], device=DEV), skip_nonfinite=True)


def _strided(t):
    return torch.stack([t, t], dim=1)[:, 0]  # same values, stride 2


def _misaligned(t):
    return torch.cat([t[:1], t])[1:]  # same values, 4 (fp32) or 2 (bf16) bytes off a 16-byte boundary


def _message(who, case):
    """Pattern of the message of the one host check that must reject ``case``: '<who>: ... <fragment>'
    (a failed launch would say "pvr kernel '<who>' failed" instead)."""
    import re

    first = case.split()[0]
    rules = [("unequal", "same number"), ("empty segment", "same number"), ("seg_", "seg_start / seg_group must be contiguous"),
             ("clip", "clip must be a contiguous float32 tensor of at least 3"),
             ("out ", "out must be a contiguous float32 tensor of at least 3"), ("workspace", "workspace must be a contiguous float32"),
             ("shadow of another", "size mismatch" if who == "adam_t" else "shadow must hold"),
             ("tmeta", "tmeta int64"), ("fmeta", "fmeta int64"), ("multiple of 4", "multiple of 4"), ("9 rows", "1..8 groups"),
             (" strided", f"{first} must be a contiguous"), (" misaligned", f"{first} must be 16-byte aligned")]
    frag = next(f for key, f in rules if key in case)
    return re.escape(f"{who}: ") + ".*" + re.escape(frag)


ADAM_BAD = {
    "seg_start on the host": lambda a: a.update(seg_start=a["seg_start"].cpu()),
    "seg_group on the host": lambda a: a.update(seg_group=a["seg_group"].cpu()),
    "seg_start strided": lambda a: a.update(seg_start=_strided(a["seg_start"])),
    "seg_group strided": lambda a: a.update(seg_group=_strided(a["seg_group"])),
    "segment tables of unequal length": lambda a: a.update(seg_group=torch.ones(3, dtype=torch.int32, device=DEV)),
    "empty segment tables": lambda a: a.update(seg_start=a["seg_start"][:0], seg_group=a["seg_group"][:0]),
    "clip on the host": lambda a: a.update(clip=a["clip"].cpu()),
    "clip of 2 elements": lambda a: a.update(clip=a["clip"][:2]),
    "clip strided": lambda a: a.update(clip=_strided(a["clip"])),
    "clip float64": lambda a: a.update(clip=a["clip"].double()),
    "shadow of another element count": lambda a: a.update(shadow=torch.full((12,), KC.SENTINEL, dtype=torch.bfloat16, device=DEV)),
    "p strided": lambda a: a.update(p=_strided(a["p"])),
    "g strided": lambda a: a.update(g=_strided(a["g"])),
    "m strided": lambda a: a.update(m=_strided(a["m"])),
    "v strided": lambda a: a.update(v=_strided(a["v"])),
    "p misaligned": lambda a: a.update(p=_misaligned(a["p"])),
    "g misaligned": lambda a: a.update(g=_misaligned(a["g"])),
    "m misaligned": lambda a: a.update(m=_misaligned(a["m"])),
    "v misaligned": lambda a: a.update(v=_misaligned(a["v"])),
    "numel not a multiple of 4": lambda a: a.update({k: torch.full((6,), KC.SENTINEL, dtype=a[k].dtype, device=DEV) for k in ("p", "g", "m", "v", "shadow")}),
    "host group table of 9 rows": lambda a: a.update(groups=torch.from_numpy(KC._adam_table(1, 9))),
}


@pytest.mark.parametrize("case", list(ADAM_BAD), ids=[c.replace(" ", "_") for c in ADAM_BAD])
def test_adam_rejects_what_its_kernel_cannot_take(case):
    ext = _ext()
    a = _adam_args()
    ADAM_BAD[case](a)
    outs = [a[k] for k in ("p", "g", "m", "v", "shadow")]
    with pytest.raises(RuntimeError, match=_message("adam", case)):
        ext.adam(a["p"], a["g"], a["m"], a["v"], a["shadow"], a["seg_start"], a["seg_group"], a["groups"], a["clip"], a["skip_nonfinite"])
    torch.cuda.synchronize()
    assert all(bool((t.float() == KC.SENTINEL).all().item()) for t in outs), "a rejected call must not launch"


def test_adam_with_valid_arguments_runs_and_meets_its_numerics():
    ext = _ext()
    a = _adam_args()
    a["g"].normal_()
    ext.adam(a["p"], a["g"], a["m"], a["v"], a["shadow"], a["seg_start"], a["seg_group"], a["groups"], a["clip"], a["skip_nonfinite"])
    torch.cuda.synchronize()
    assert not bool((a["p"] == KC.SENTINEL).any().item()), "the valid call must launch"
    torch.manual_seed(4)
    _passes(KC.check_adam_kernel("host", 3, clip=True, tiny=True))


def _adam_t_args():
    """A valid ext.adam_t call on sentinel buffers: one 64x64 matrix and one 4-element flat range."""
    n = 64 * 64 + 4
    full = lambda k=n, dt=torch.float32: torch.full((k,), KC.SENTINEL, dtype=dt, device=DEV)  # noqa: E731
    return dict(p=full(), g=full(), m=full(), v=full(), shadow=full(n, torch.bfloat16), shadow_t=full(64 * 64, torch.bfloat16),
                tmeta=torch.tensor([[0, 0, 64, 64, 0, 0]], dtype=torch.int64, device=DEV), ntiles=1,
                fmeta=torch.tensor([[64 * 64, 4, 1, 0]], dtype=torch.int64, device=DEV), flat4=1,
                groups=torch.from_numpy(KC._adam_table(1, 3)), clip=torch.tensor([1.0, 0.5, 0.0], device=DEV), skip_nonfinite=True)


ADAM_T_BAD = {
    "clip on the host": lambda a: a.update(clip=a["clip"].cpu()),
    "clip of 2 elements": lambda a: a.update(clip=a["clip"][:2]),
    "clip strided": lambda a: a.update(clip=_strided(a["clip"])),
    "shadow of another element count": lambda a: a.update(shadow=torch.full((64 * 64,), KC.SENTINEL, dtype=torch.bfloat16, device=DEV)),
    "p strided": lambda a: a.update(p=_strided(a["p"])),
    "v misaligned": lambda a: a.update(v=_misaligned(a["v"])),
    "shadow_t misaligned": lambda a: a.update(shadow_t=_misaligned(a["shadow_t"])),
    "tmeta on the host": lambda a: a.update(tmeta=a["tmeta"].cpu()),
    "fmeta empty": lambda a: a.update(fmeta=a["fmeta"][:0]),
    "host group table of 9 rows": lambda a: a.update(groups=torch.from_numpy(KC._adam_table(1, 9))),
}


def _call_adam_t(ext, a):
    ext.adam_t(a["p"], a["g"], a["m"], a["v"], a["shadow"], a["shadow_t"], a["tmeta"], a["ntiles"], a["fmeta"], a["flat4"], a["groups"],
               a["clip"], a["skip_nonfinite"])


@pytest.mark.parametrize("case", list(ADAM_T_BAD), ids=[c.replace(" ", "_") for c in ADAM_T_BAD])
def test_adam_t_rejects_what_its_kernel_cannot_take(case):
    ext = _ext()
    a = _adam_t_args()
    ADAM_T_BAD[case](a)
    outs = [a[k] for k in ("p", "g", "m", "v", "shadow", "shadow_t")]
    with pytest.raises(RuntimeError, match=_message("adam_t", case)):
        _call_adam_t(ext, a)
    torch.cuda.synchronize()
    assert all(bool((t.float() == KC.SENTINEL).all().item()) for t in outs), "a rejected call must not launch"


def test_adam_t_with_valid_arguments_runs():
    """The corrected call launches: the matrix and the range move, W^T is the shadow's transpose."""
    ext = _ext()
    a = _adam_t_args()
    a["g"].normal_()
    _call_adam_t(ext, a)
    torch.cuda.synchronize()
    assert not bool((a["p"] == KC.SENTINEL).any().item())
    assert torch.equal(a["shadow_t"].view(64, 64), a["shadow"][:64 * 64].view(64, 64).t())
    from tests import optim_reference as R

    assert torch.equal(R.bf16_bits(a["shadow"]), R.bf16_rne_bits(a["p"]))


GRAD_NORM_BAD = {
    "out on the host": lambda a: a.update(out=a["out"].cpu()),
    "out of 2 elements": lambda a: a.update(out=a["out"][:2]),
    "out strided": lambda a: a.update(out=_strided(a["out"])),
    "out float64": lambda a: a.update(out=a["out"].double()),
    "workspace too small": lambda a: a.update(ws=a["ws"][:-1]),
    "workspace on the host": lambda a: a.update(ws=a["ws"].cpu()),
    "g strided": lambda a: a.update(g=_strided(a["g"])),
    "g misaligned": lambda a: a.update(g=_misaligned(a["g"])),
}


@pytest.mark.parametrize("case", list(GRAD_NORM_BAD), ids=[c.replace(" ", "_") for c in GRAD_NORM_BAD])
def test_grad_norm_rejects_what_its_kernels_cannot_take(case):
    ext = _ext()
    a = dict(g=torch.ones(8, device=DEV), ws=torch.full((ext.norm_partial_blocks(),), KC.SENTINEL, device=DEV),
             out=torch.full((3,), KC.SENTINEL, device=DEV))
    ws, out = a["ws"], a["out"]
    GRAD_NORM_BAD[case](a)
    with pytest.raises(RuntimeError, match=_message("grad_norm", case)):
        ext.grad_norm(a["g"], 1.0, a["ws"], a["out"])
    torch.cuda.synchronize()
    assert bool((ws == KC.SENTINEL).all().item()) and bool((out == KC.SENTINEL).all().item()), "a rejected call must not launch"
    torch.manual_seed(5)
    _passes(KC.check_grad_norm(5, 1.0))


@pytest.mark.parametrize("case", ["in misaligned", "out misaligned", "out of another length"])
def test_cast_f32_bf16_rejects_what_its_kernel_cannot_take(case):
    """The cast reads float4 and writes four bf16 at a time: 16- and 8-byte aligned bases."""
    ext = _ext()
    x = torch.ones(8, device=DEV)
    out = torch.full((8,), KC.SENTINEL, dtype=torch.bfloat16, device=DEV)
    if case == "in misaligned":
        args, why = (_misaligned(x), out), "16-byte aligned"
    elif case == "out misaligned":
        whole = torch.full((9,), KC.SENTINEL, dtype=torch.bfloat16, device=DEV)
        args, why, out = (x, whole[1:]), "8-byte aligned", whole
    else:
        args, why = (x, out[:7]), "shape/contiguity"
    with pytest.raises(RuntimeError, match="cast: .*" + why):
        ext.cast_f32_bf16(*args)
    torch.cuda.synchronize()
    assert bool((out.float() == KC.SENTINEL).all().item()), "a rejected call must not launch"
    torch.manual_seed(6)
    _passes(KC.check_cast_f32_bf16(5))


XENT_BAD = {
    "labels on the host": lambda a: a.update(labels=a["labels"].cpu()),
    "labels shorter than the batch": lambda a: a.update(labels=a["labels"][:-1]),
    "labels longer than the batch": lambda a: a.update(labels=torch.cat([a["labels"], a["labels"]])),
    "labels int32": lambda a: a.update(labels=a["labels"].int()),
    "labels strided": lambda a: a.update(labels=_strided(a["labels"])),
    "logits with no class": lambda a: a.update(logits=a["logits"][:, :0], dlogits=a["dlogits"][:, :0].contiguous()),
    "dlogits on the host": lambda a: a.update(dlogits=torch.full((4, 7), KC.SENTINEL)),
}


@pytest.mark.parametrize("case", list(XENT_BAD), ids=[c.replace(" ", "_") for c in XENT_BAD])
def test_xent_rejects_what_its_kernel_cannot_take(case):
    """``xent`` reads labels[b] for every logits row and writes dlogits through a raw pointer: labels
    of another length or device, logits without a class and a host dlogits are refused before any
    launch, as ``xent_soft`` refuses them."""
    ext = _ext()
    B, C = 4, 7
    a = dict(logits=torch.zeros(B, C, device=DEV), labels=torch.arange(B, dtype=torch.int64, device=DEV),
             dlogits=torch.full((B, C), KC.SENTINEL, device=DEV))
    dl, corr, mean = a["dlogits"], torch.full((B,), 7, dtype=torch.int32, device=DEV), torch.full((1,), KC.SENTINEL, device=DEV)
    XENT_BAD[case](a)
    with pytest.raises(RuntimeError, match="xent: .*(labels must be contiguous int64|logits must be|dlogits f32)"):
        ext.xent(a["logits"], a["labels"], a["dlogits"], corr, 1.0 / B, mean)
    torch.cuda.synchronize()
    assert bool((dl == KC.SENTINEL).all().item()) and bool((corr == 7).all().item()) and bool((mean == KC.SENTINEL).all().item()), \
        "a rejected call must not launch"
    torch.manual_seed(7)
    _passes(KC.check_xent(B, C))


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
