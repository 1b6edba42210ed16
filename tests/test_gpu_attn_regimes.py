"""The attention kernels on peaked, shifted, ramped, uniform and one-hot score rows.

Every other attention check draws qkv ~ N(0, 1): near-uniform softmax rows, scores within 5 nat,
lse about log N. Here each route of csrc/attention.hip (tests/attn_reference.py SHAPES: the smallest
shapes that reach it) runs on the regimes of ``attn_reference.make``; ``ext.attn_fwd`` and then
``ext.attn_bwd`` on the kernel's own O and lse, as ``kernel_checks.check_attn_bwd`` does.

For every case
* every output is finite;
* for O, dQ, dK, dV (and dbias where asked for) the global relative L2 and the row figure
  (``attn_reference.figures``) of the kernel against float64 are at most 4 x the figure of the
  bf16-staged emulation on the same inputs, computed here, with a floor of 2^-9 (one bf16 half-ulp)
  where the emulation is exact. No absolute limit is fixed in advance;
* per row, |lse - ref| <= 4e-7 max(1, max_k |score|): five fp32 roundings (c = scale log2e, m = s c,
  log2 l, the sum, the multiply by ln2) are 5 x 2^-24 = 3e-7, plus a margin for v_exp / v_log.
onehot, in addition: O = V[perm] and dV = dO[perm^-1] bit for bit (P of the matching key is exp2 of
at most half an ulp of 185, i.e. 1 +- 5e-6, which packs to bf16 1.0; l = 1 +- 5e-6 and a bf16 value
times 1 +- 1e-5 rounds back to itself; every other P is at most 2^-75), and max |dQ|, max |dK| at
most 2 dh^2 2^-24 max|dO| max|V| 4 scale (the worst-case fp32 error of dP - delta over dh terms,
times one K or Q entry and the scale), where a wrong key, query or delta row gives O(1). (The
class-token kernels see dO = 0 on every query but row 0: dV equals dO_0 bit for bit on key perm[0],
and on the other keys, where no dO row absorbs it, holds P dO_0 <= exp(-40) max|dO|.)
uniform, in addition: dK is exactly zero and lse = log N within the bound above.

tests/test_attn_reference_cpu.py proves the conditions on these inputs (onehot gaps, ramp reaching
both branches of the tiled forward's lazy rescale) without a GPU.

Measured on MI355X (profiles/attn_regimes/test_gpu_attn_regimes.log; the full table per path is in
profiles/attn_regimes/README.md). Worst kernel / emulation ratio of any figure (limit 4), over all paths:

    regime     O, dQ, dK, dV   dbias   where
    gauss          1.29         1.41   O.row N272 dh64; dbias.row N400 dh64 (accumulator path)
    sharp          1.86         1.51   dQ.row N577 dh64; class-token dbias.row N197
    shift_pos      2.14         1.58   dQ.row N100 dh96
    shift_neg      3.43         3.95   class-token dq0 N65 dh128; dbias.row N257 dh80 (lastkey path)
    ramp           1.56         1.95   dK.row N370 dh64; dbias.l2 N577 dh64 (tail split)
    uniform        1.04         2.00   dbias.l2 N400 dh64: 2 x the floor, the emulation is at 1.2e-4
    onehot         0.92 x floor        dQ.l2 B300 (absolute: the reference is zero); O and dV exact

The whole-head forward with the pipelined or one-block backward sits at 1.00-1.06 on every regime; the
tiled forward's O rows are 1.1-1.9 x the emulation (its P is rounded against a running, partly stale
max). dQ of shift_* is 1.4-2.3e-2 in global L2 for kernel and emulation alike: the cancellation of
dS rows against a common offset in K, not a fault. Worst |lse - ref|: 0.72 of its bound (gauss);
onehot max |dQ|, |dK|: 4e-4 of theirs.

Two faults these inputs found, both fixed in csrc/: shift_neg made every dQ row of the generic backward
NaN (P of a padded key is exp2(-lse log2e) = inf at lse = -130 nat, and met a zero K row as inf * 0), and
lse = (m + log2 l) ln2 carried 2-3 fp32 roundings at the size of the result, 1.0-1.2 x the bound on gauss
and uniform rows, where lse = log N exceeds every score.
"""
import math

import pytest
import torch

from tests import attn_reference as AR

pytestmark = pytest.mark.gpu

DEV = "cuda"
SEED_VAL, SEED_OFF = 987654321, 77 << 32  # the dropout counter of kernel_checks.check_attn_dropout
WORST = {}  # (path, regime) -> (ratio, what)


def _ext():
    from pytorch_vit_paper_replication_amd import _ext

    return _ext.ext()


@pytest.fixture(scope="module", autouse=True)
def _worst_ratio_table():
    yield
    if WORST:
        print("\nworst kernel / emulation ratio (figure over max(emulation, 2^-11)) per path and regime:")
        for (path, regime), (ratio, what) in sorted(WORST.items()):
            print(f"  {path:22s} {regime:9s} {ratio:5.2f}  ({what})")


class _Judge:
    """Collects one case's figures beside their limits, prints them in one line, then asserts."""

    def __init__(self, path, regime, B, H, N, dh):
        self.key = (path, regime)
        self.name = f"{path} {regime} B{B} H{H} N{N} dh{dh}"
        self.dh = dh
        self.rows = []  # (label, value, limit)

    def finite(self, **tensors):
        for k, t in tensors.items():
            self.rows.append((f"{k}.nonfinite", float((~torch.isfinite(t)).sum().item()), 0.0))

    def figures(self, label, out, ref, emu, dh=None):
        dh = dh or self.dh
        for kind, f, fe in zip(("l2", "row"), AR.figures(out, ref, dh), AR.figures(emu, ref, dh)):
            self.rows.append((f"{label}.{kind}", f, max(4.0 * fe, AR.FLOOR)))
            ratio = f / max(fe, AR.FLOOR / 4)
            if ratio > WORST.get(self.key, (-1.0, ""))[0]:
                WORST[self.key] = (ratio, f"{label}.{kind} {self.name.split(' ', 2)[2]}")

    def lse(self, lse, ref, peak):
        """Worst |lse - ref| in units of its bound 4e-7 max(1, max_k |score|)."""
        u = ((lse.double() - ref).abs() / (4e-7 * peak.clamp_min(1.0))).max().item()
        self.rows.append(("lse/bound", u, 1.0))

    def flag(self, label, bad):
        self.rows.append((label, float(bad), 0.0))

    def bound(self, label, value, limit):
        self.rows.append((label, float(value), float(limit)))

    def done(self):
        line = f"attn_regimes {self.name}: " + " ".join(f"{k}={v:.2e}/{l:.1e}" for k, v, l in self.rows)
        print(line)
        bad = [f"{k}={v:.3e}/{l:.3e}" for k, v, l in self.rows if not v <= l]
        assert not bad, f"{self.name}: {' '.join(bad)}"


def _onehot_checks(j, c, B, N, H, dh, o, dqkv, do_full, rows=None):
    """O = V[perm], dV = dO[perm^-1] bit for bit; dQ and dK within the fp32 error of dP - delta.
    ``rows``: compare O on these token rows only (the class-token kernels: row 0 of each image)."""
    D = H * dh
    o_exact = AR.gather_rows(c.qkv[:, 2 * D:], c.perm, B, N, H)
    if rows is not None:
        o_exact = o_exact[rows]
    j.flag("O!=V[perm]", (o != o_exact).sum().item())
    dv, dv_exact = dqkv[:, 2 * D:], AR.gather_rows(do_full, AR.inverse_perm(c.perm), B, N, H)
    if rows is None:
        j.flag("dV!=dO[inv]", (dv != dv_exact).sum().item())
    else:
        # dO is zero off row 0, so only key perm[0] of a pair has a dO row to equal; on every other key
        # nothing absorbs P <= exp(-gap) times dO_0: at most exp(-40) max|dO| (the gap the CPU test asserts)
        hit = AR.heads(dv_exact, B, N, H).ne(0).any(-1, keepdim=True).expand(B, H, N, dh)
        hit = AR.merge_heads(hit)
        j.flag("dV!=dO[inv]", ((dv != dv_exact) & hit).sum().item())
        j.bound("max|dV|off", dv.float().abs().masked_fill(hit, 0).max().item(), math.exp(-40.0) * do_full.float().abs().max().item())
    lim = 2 * dh * dh * 2.0 ** -24 * do_full.float().abs().max().item() * c.qkv[:, 2 * D:].float().abs().max().item() * 4 / math.sqrt(dh)
    j.bound("max|dQ|", dqkv[:, :D].float().abs().max().item(), lim)
    j.bound("max|dK|", dqkv[:, D:2 * D].float().abs().max().item(), lim)


def _run(path, regime, B, H, N, dh, *, dbias=False, p=0.0, calls=1, det=False):
    from tests import kernel_checks as KC

    ext = _ext()
    D = H * dh
    scale = 1.0 / math.sqrt(dh)
    c = AR.make(regime, B, N, H, dh, device=DEV)
    keep, drop = None, (None, 0, 0.0)
    if p > 0:
        keep = KC.attn_keep_mask(SEED_VAL, SEED_OFF, B * H, N, p)
        drop = (torch.tensor([SEED_VAL], dtype=torch.int64, device=DEV), SEED_OFF, p)
    r = AR.ref64(c.qkv, c.do, B, N, H, keep, p)
    e = AR.emulate(c.qkv, c.do, B, N, H, keep, p)
    peak = AR.scores64(c.qkv, B, N, H).abs().amax(-1)

    o, lse = ext.attn_fwd(c.qkv, B, N, H, scale, *drop)
    outs = []
    was = ext.deterministic()
    if det:
        ext.set_deterministic(True)
    try:
        for _ in range(calls):
            db = torch.zeros(3 * D, device=DEV) if dbias else None
            outs.append((ext.attn_bwd(c.do, c.qkv, o, lse, B, N, H, scale, db, None, *drop), db))
    finally:
        if det:
            ext.set_deterministic(was)
    torch.cuda.synchronize()

    j = _Judge(path, regime, B, H, N, dh)
    j.finite(O=o, lse=lse)
    j.figures("O", o, r.o, e.o)
    j.lse(lse, r.lse, peak)
    for i, (dqkv, db) in enumerate(outs):
        tag = "" if i == 0 else f"#{i + 1}"
        j.finite(**{f"dqkv{tag}": dqkv})
        for s, name in enumerate(("dQ", "dK", "dV")):
            sl = slice(s * D, (s + 1) * D)
            j.figures(name + tag, dqkv[:, sl], r.dqkv[:, sl], e.dqkv[:, sl])
        if db is not None:
            j.finite(**{f"dbias{tag}": db})
            j.figures("dbias" + tag, db, r.dbias, e.dbias)
        if regime == "onehot":
            _onehot_checks(j, c, B, N, H, dh, o, dqkv, c.do)
        if regime == "uniform":
            j.flag("dK!=0" + tag, (dqkv[:, D:2 * D] != 0).sum().item())
    if regime == "uniform":
        j.bound("|lse-logN|", (lse.double() - math.log(N)).abs().max().item(), 4e-7)
    if det:
        j.flag("not_bitwise_repeatable", not torch.equal(outs[0][0], outs[1][0]))
    j.done()


def _id(s):
    return f"{s[0]}-B{s[1]}H{s[2]}N{s[3]}dh{s[4]}"


@pytest.mark.parametrize("regime", AR.REGIMES)
@pytest.mark.parametrize("shape", AR.SHAPES, ids=_id)
def test_routes(shape, regime):
    path, B, H, N, dh = shape
    # the dQ accumulator shape runs twice: the second call finds the accumulator the first re-zeroed
    _run(path, regime, B, H, N, dh, calls=2 if path == "dqacc" else 1)


@pytest.mark.parametrize("regime", AR.REGIMES)
@pytest.mark.parametrize("shape", AR.DBIAS_SHAPES, ids=_id)
def test_fused_dbias(shape, regime):
    path, B, H, N, dh = shape
    _run(path, regime, B, H, N, dh, dbias=True)


@pytest.mark.parametrize("regime", AR.REGIMES)
def test_deterministic_slabs(regime):
    path, B, H, N, dh = AR.DET_SHAPE
    _run(path, regime, B, H, N, dh, calls=2, det=True)


@pytest.mark.parametrize("regime", ["sharp", "ramp"])
@pytest.mark.parametrize("shape", AR.DROP_SHAPES, ids=_id)
def test_attention_dropout(shape, regime):
    path, B, H, N, dh = shape
    _run(path, regime, B, H, N, dh, p=0.1)


def test_pair_handoff_onehot():
    """600 pairs: every persistent workgroup hands over 2-3 times; a stale K/V image is a wrong V row."""
    path, B, H, N, dh = AR.HANDOFF_SHAPE
    _run(path, "onehot", B, H, N, dh)


@pytest.mark.parametrize("regime", AR.REGIMES)
@pytest.mark.parametrize("shape", AR.CLS_SHAPES, ids=_id)
def test_class_token_kernels(shape, regime):
    """attn_cls_fwd / attn_cls_bwd / attn_cls_dbias against query row 0 of the reference: dO is zero on
    every other row."""
    path, B, H, N, dh = shape
    ext = _ext()
    D = H * dh
    scale = 1.0 / math.sqrt(dh)
    c = AR.make(regime, B, N, H, dh, device=DEV)
    rows0 = torch.arange(B, device=DEV) * N
    do0 = c.do[rows0].contiguous()
    do_full = torch.zeros_like(c.do)
    do_full[rows0] = do0
    r = AR.ref64(c.qkv, do_full, B, N, H)
    e = AR.emulate(c.qkv, do_full, B, N, H)
    peak = AR.scores64(c.qkv, B, N, H).abs().amax(-1)[:, 0]

    o0, lse0 = ext.attn_cls_fwd(c.qkv, B, N, H, scale)
    dqkv, dq0 = ext.attn_cls_bwd(do0, c.qkv, o0, lse0, B, N, H, scale)
    dbias = torch.zeros(3 * D, device=DEV)
    ext.attn_cls_dbias(dq0, do0, dbias)
    torch.cuda.synchronize()
    assert o0.shape == (B, D) and lse0.shape == (B * H,) and dqkv.shape == (B * N, 3 * D) and dq0.shape == (B, D)

    j = _Judge(path, regime, B, H, N, dh)
    j.finite(O=o0, lse=lse0, dqkv=dqkv, dq0=dq0, dbias=dbias)
    j.figures("O", o0, r.o[rows0], e.o[rows0])
    j.lse(lse0, r.lse[:, 0], peak)
    for s, name in enumerate(("dQ", "dK", "dV")):
        sl = slice(s * D, (s + 1) * D)
        j.figures(name, dqkv[:, sl], r.dqkv[:, sl], e.dqkv[:, sl])
    j.figures("dq0", dq0, r.dqkv[rows0, :D], e.dqkv[rows0, :D])
    j.figures("dbias", dbias, r.dbias, e.dbias)
    j.flag("dq_other_rows_nonzero", (dqkv.view(B, N, 3 * D)[:, 1:, :D] != 0).sum().item())
    if regime == "onehot":
        _onehot_checks(j, c, B, N, H, dh, o0, dqkv, do_full, rows=rows0)
    if regime == "uniform":
        j.flag("dK!=0", (dqkv[:, D:2 * D] != 0).sum().item())
        j.bound("|lse-logN|", (lse0.double() - math.log(N)).abs().max().item(), 4e-7)
    j.done()
