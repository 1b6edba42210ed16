"""The LayerNorm, head, cross-entropy and GELU kernels off the Gaussian regime.

Every other check of these kernels draws its inputs from one Gaussian and compares whole tensors. Here
each route of csrc/layernorm.hip (every forward MAXCH, every backward (MAXCH, W) pair, with and without
a partial last chunk, and each grid-stride path), csrc/head.hip, csrc/xent.hip and each call site of
``gelu_and_grad`` / ``gelu_and_grad2`` runs on the regimes of tests/rowwise_reference.py, which also
holds the float64 references, the fp32 emulations and the shape tables.

LayerNorm and head: every output is finite; the global relative L2 and the row figure
(``rowwise_reference.figures``) of the kernel against float64 are at most 4 x the figure of the fp32
emulation on the same inputs, with a floor where the emulation is exact: 2^-9 for bf16 outputs, the limit
kernel_checks holds Gaussian inputs to for fp32 sums (1e-6 dgamma / dbeta, 5e-6 dsum, 1.5e-6 / 2e-6 the
head's). No absolute limit is fixed in advance. mean within max(4 x emulation, 2^-22 max|x|), rstd within
max(4 x emulation, 2^-22) relative. constant rows, in addition: y = bf16(beta) bit for bit, rstd =
rsqrt(eps) within an fp32 ulp, dgamma exactly 0. Grid-stride cases, in addition: the rows of the second
pass equal the same rows run alone, bit for bit.

Cross-entropy, per row: |loss - ref| <= k 2^-24 max(1, max|x|, |ref|) and |dlogits - ref| <= k_g 2^-24
grad_scale with k, k_g counted from the kernel's roundings (``rowwise_reference.xent_roundings``: 24 / 21 at
C <= 256 up to 109 / 106 at C = 21843, the serial part of the exponential sum); flags by the explicit
first-argmax rule; ignored rows exactly zero; masked classes exactly zero gradient; xent_soft at lam = 1,
eps = 0, yb = ya keeps xent's bits on every regime. With eps > 0 a masked class makes the row loss +inf in
the reference and in the kernel alike (smoothing puts mass on an impossible class): those rows are
compared as equal infinities, their gradients as everywhere.

GELU, per element through the real GEMM epilogues, with f = gelu_formula64(u):
|h - f| <= 2^-8 |f| + 4 |gelu_emulate(u) - f| + 2^-126, the same for the stored derivative. The distance of
the formula from erfc is owned by tests/test_rowwise_reference_cpu.py and only printed here.

Measured on MI355X (profiles/rowwise_regimes/test_gpu_rowwise_regimes.log; the table per route and
regime is in profiles/rowwise_regimes/README.md). Worst kernel / emulation ratio of any figure (limit 4):

    ln_bwd grid stride   2.35   dgamma.l2, T 4101 D 1024 (2.3-2.4 from run to run: 1024 workgroups' atomics)
    head                 2.28   rstd, D 1040, offset
    ln_fwd               2.26   rstd, D 2048, offset
    every other route    below 2.3

Cross-entropy: at most 0.09 of the loss and gradient bounds, 0.48 of the batch mean's, on every regime.
GELU: every element within its limit on every tile (worst 0.996: the bf16 rounding of the output).

One fault these inputs found, fixed in csrc/xent.hip: xent_soft returned NaN losses on every row with a
masked (-inf) class, also without smoothing, because the smoothing term was formed as (eps / C) sum_c x_c =
0 * -inf. The term is now taken only where eps / C is not zero.

One property written down instead of a fix: exp(-u^2 / 2) in the GELU comes from one v_exp_f32, which returns
0 where the result is an fp32 subnormal (|u| > 13.2). The stored derivative is then 0 where the function is up
to 5.3 * 2^-126 in size (0 for -3.96e-38 at u = -13.25: 3.3 x the limit with torch's exp2, which keeps
subnormals). ``gelu_emulate`` flushes as the instruction does; tests/test_rowwise_reference_cpu.py states it.

Not thinned: every variant x regime x D product of the list runs (581 cases with the argument checks, 9 s).
"""
import math
import re

import numpy as np
import pytest
import torch

from tests import rowwise_reference as RR

pytestmark = pytest.mark.gpu

DEV = "cuda"
U = 2.0 ** -24
P = 0.1
SEED_VAL, SEED_OFF, DP_OFF = 31337, 11 << 32, 23 << 32
WORST = {}  # (route, regime) -> (ratio, what)


def _ext():
    from pytorch_vit_paper_replication_amd import _ext

    return _ext.ext()


@pytest.fixture(scope="module", autouse=True)
def _worst_ratio_table():
    yield
    if WORST:
        print("\nworst kernel / emulation ratio (figure over max(emulation, floor / 4); limit 4) per route, by regime:")
        routes = sorted({k[0] for k in WORST})
        for route in routes:
            cells = {reg: WORST[(route, reg)] for (rt, reg) in WORST if rt == route}
            top = max(cells.values())
            print(f"  {route:28s} " + " ".join(f"{reg}={v[0]:.2f}" for reg, v in cells.items()) + f"  (worst: {top[1]})")


class _Judge:
    """Collects one case's figures beside their limits, prints them in one line, then asserts."""

    def __init__(self, route, regime, shape):
        self.key = (route, regime)
        self.shape = shape
        self.name = f"{route} {regime} {shape}"
        self.rows = []  # (label, value, limit)

    def finite(self, **tensors):
        for k, t in tensors.items():
            if t is not None:
                self.rows.append((f"{k}.nonfinite", float((~torch.isfinite(t.float())).sum().item()), 0.0))

    def _ratio(self, label, f, fe, floor):
        ratio = f / max(fe, floor / 4)
        if ratio > WORST.get(self.key, (-1.0, ""))[0]:
            WORST[self.key] = (ratio, f"{label} {self.shape}")

    def figures(self, label, out, ref, emu, floors=(RR.FLOOR, RR.FLOOR)):
        kinds = ("l2", "row") if ref.dim() >= 2 else ("l2",)  # a vector is one row: its row figure is its l2
        for kind, f, fe, floor in zip(kinds, RR.figures(out, ref), RR.figures(emu, ref), floors):
            self.rows.append((f"{label}.{kind}", f, max(4.0 * fe, floor)))
            self._ratio(f"{label}.{kind}", f, fe, floor)

    def scalar(self, label, f, fe, floor):
        """A single error figure against 4 x the emulation's, with a floor."""
        self.rows.append((label, f, max(4.0 * fe, floor)))
        self._ratio(label, f, fe, floor)

    def flag(self, label, bad):
        self.rows.append((label, float(bad), 0.0))

    def bound(self, label, value, limit):
        self.rows.append((label, float(value), float(limit)))

    @staticmethod
    def _num(x):
        return f"{x:.1e}".replace("e-0", "e-").replace("e+0", "e+")

    def done(self):
        """One line: every figure beside its limit. Exact checks (limit 0) that hold are counted, not
        listed; a figure in units of its bound (limit 1) is printed alone; the xent_soft variants of a case
        are printed as the worst variant per figure (all of them are asserted)."""
        shown, exact, soft = [], 0, {}
        for k, v, l in self.rows:
            m = re.match(r"soft\[(.*?)\]\.(.*)$", k)
            if l == 0 and v == 0:
                exact += 1
            elif m and (m.group(2) not in soft or not v <= soft[m.group(2)][0]):
                soft[m.group(2)] = (v, l, m.group(1))
            elif not m:
                shown.append((k, v, l))
        shown += [(f"soft.{kind}@[{var}]", v, l) for kind, (v, l, var) in soft.items()]
        text = " ".join(f"{k}={v:.2f}" if l == 1 else f"{k}={self._num(v)}/{self._num(l)}" for k, v, l in shown)
        print(f"rowwise_regimes {self.name}: {text} exact_ok={exact}")
        bad = [f"{k}={v:.3e}/{l:.3e}" for k, v, l in self.rows if not v <= l]
        assert not bad, f"{self.name}: {' '.join(bad)}"


def _bits(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32)


def _ulps32(a, b):
    return (a.view(torch.int32).long() - b.view(torch.int32).long()).abs().max().item()


# ============================================================================= LayerNorm
QSCALE_FWD = 8.0


def _judge_stats(j, c, mean, rstd, r, e, regime):
    xmax = c.x.float().abs().max().item()
    j.scalar("mean", (mean.double() - r.mean).abs().max().item(), (e.mean.double() - r.mean).abs().max().item(), 2.0 ** -22 * xmax)
    j.scalar("rstd", (rstd.double() / r.rstd - 1).abs().max().item(), (e.rstd.double() / r.rstd - 1).abs().max().item(), 2.0 ** -22)
    if regime == "constant":
        want = torch.rsqrt(torch.full_like(rstd, RR.EPS))
        j.bound("rstd_ulps", _ulps32(rstd, want), 1)


def _ln_fwd_case(regime, T, D, route):
    from tests import fp8_reference as FR
    from tests import kernel_checks as KC

    ext = _ext()
    c = RR.make_ln(regime, T, D, device=DEV)
    r = RR.ln_ref64(c.x, c.gamma, c.beta, c.dy)
    e = RR.ln_emulate(c.x, c.gamma, c.beta, c.dy)
    y, mean, rstd = ext.layernorm_fwd(c.x, c.gamma, c.beta, RR.EPS, T, D)
    q = torch.zeros(T, D, dtype=torch.uint8, device=DEV)
    qs = torch.full((1,), QSCALE_FWD, device=DEV)
    amax = torch.zeros(1, dtype=torch.int32, device=DEV)
    yq, mq, rq = ext.layernorm_fwd_q8(c.x, c.gamma, c.beta, RR.EPS, T, D, q, qs, amax, False)
    torch.cuda.synchronize()
    j = _Judge(route, regime, f"T{T} D{D}")
    j.finite(y=y, mean=mean, rstd=rstd)
    j.figures("y", y, r.y, e.y)
    _judge_stats(j, c, mean, rstd, r, e, regime)
    if regime == "constant":
        j.flag("y!=bf16(beta)", (_bits(y) != _bits(c.beta.to(torch.bfloat16).expand(T, D).contiguous())).sum().item())
    # the forward with the e4m3 copy: the same y, mean, rstd; the copy against the reference quantiser of the
    # emulated fp32 precursor (check_layernorm_fwd_q8's allowance: one code step, 5 % of the codes); amax
    j.flag("q8_y_differs", not (torch.equal(_bits(yq), _bits(y)) and torch.equal(mq, mean) and torch.equal(rq, rstd)))
    want = torch.from_numpy(FR.encode((e.pre * QSCALE_FWD).cpu().numpy(), FR.E4M3)).to(DEV)
    j.bound("fp8_steps", KC._fp8_code_dist(q, want), 1)
    j.bound("fp8_mismatch", (q != want).float().mean().item(), 0.05)
    a_k, a_e, a_r = amax.view(torch.float32).item(), e.pre.abs().max().item(), r.y.abs().max().item()
    # amax = max |fp32 y|: four roundings and the statistics' 2^-22 per element, doubled
    j.scalar("amax", abs(a_k - a_r) / a_r, abs(a_e - a_r) / a_r, 2.0 ** -20)
    j.bound("amax_bits!=emu", float(np.float32(a_k) != np.float32(a_e)), 1)  # reported, not held
    j.done()
    return y, q


@pytest.mark.parametrize("regime", RR.LN_REGIMES)
@pytest.mark.parametrize("D", RR.LN_FWD_DS)
def test_layernorm_forward(D, regime):
    """ln_fwd_kernel<MAXCH> and ln_fwd_q8_kernel<MAXCH>, MAXCH = 1..4, full and partial last chunk."""
    full = "full" if (D // 8) % 64 == 0 else "part"
    _ln_fwd_case(regime, RR.LN_T, D, f"ln_fwd<{RR.ln_fwd_route(D)}>{full}")


def _keep_mask(T, D, seed, off, p):
    """The keep mask of the shared counter hash, as kernel_checks.check_layernorm_linked obtains it."""
    from pytorch_vit_paper_replication_amd.ops import gemm as G

    keep = torch.empty(T, D, dtype=torch.bfloat16, device=DEV)
    G.bias_grad(torch.ones(T, D, dtype=torch.bfloat16, device=DEV), torch.zeros(D, device=DEV), drop=(seed, off, p), dz=keep)
    return keep.float() != 0


def _ln_bwd_run(ext, c, T, D, mean, rstd, dres, **kw):
    dx = torch.full((T, D), float("nan"), dtype=torch.bfloat16, device=DEV)
    dz = torch.full((T, D), float("nan"), dtype=torch.bfloat16, device=DEV) if kw.pop("want_dz", False) else None
    dw, db, ds = (torch.zeros(D, device=DEV) for _ in range(3))
    ext.layernorm_bwd(c.dy, D, c.x, D, mean, rstd, c.gamma, dres, D, dx, D, dw, db, T, dsum=ds, dz=dz, **kw)
    return dx, dz, dw, db, ds


SUM_FLOORS = dict(dw=(1e-6,), db=(1e-6,), dsum=(5e-6,))  # kernel_checks' limits on Gaussian inputs


def _judge_bwd(j, outs, r, e, regime, tag=""):
    dx, dz, dw, db, ds = outs
    j.finite(**{"dx" + tag: dx, "dz" + tag: dz, "dw" + tag: dw, "db" + tag: db, "dsum" + tag: ds})
    j.figures("dx" + tag, dx, r.dx, e.dx)
    if dz is not None:
        j.figures("dz" + tag, dz, r.dz, e.dz)
    j.figures("dw" + tag, dw, r.dgamma, e.dgamma, SUM_FLOORS["dw"])
    j.figures("db" + tag, db, r.dbeta, e.dbeta, SUM_FLOORS["db"])
    j.figures("dsum" + tag, ds, r.dsum, e.dsum, SUM_FLOORS["dsum"])
    if regime == "constant":
        j.flag("dgamma!=0" + tag, (dw != 0).sum().item())


def _bwd_route(D):
    m, w = RR.ln_bwd_route(D)
    return f"ln_bwd<{m},{w}>{'part' if (D // w) % 64 else 'full'}"


@pytest.mark.parametrize("regime", RR.LN_REGIMES)
@pytest.mark.parametrize("D", RR.LN_BWD_DS)
def test_layernorm_backward(D, regime):
    """ln_bwd_kernel<MAXCH, W> with dres, dgamma, dbeta and the column sums, every (MAXCH, W) pair."""
    ext = _ext()
    T = RR.LN_T
    c = RR.make_ln(regime, T, D, device=DEV)
    r = RR.ln_ref64(c.x, c.gamma, c.beta, c.dy, c.dres)
    e = RR.ln_emulate(c.x, c.gamma, c.beta, c.dy, c.dres)
    _, mean, rstd = ext.layernorm_fwd(c.x, c.gamma, c.beta, RR.EPS, T, D)
    outs = _ln_bwd_run(ext, c, T, D, mean, rstd, c.dres)
    torch.cuda.synchronize()
    j = _Judge(_bwd_route(D), regime, f"T{T} D{D}")
    _judge_bwd(j, outs, r, e, regime)
    j.done()


DP_ROWS = 5
VARIANTS = ("dz", "compact", "dpath", "dpath+drop", "compact+dpath", "q8_e5m2", "q8_e4m3", "q8_e5m2_dz", "q8_e4m3_dz", "q8_e5m2_nostore",
            "q8_e4m3_nostore", "det")


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("regime", RR.LN_VARIANT_REGIMES)
@pytest.mark.parametrize("D", RR.LN_VARIANT_DS)
def test_layernorm_backward_variants(D, regime, variant):
    """The instantiations beside the plain one: SP (compact residual), DP (drop path), Q8 (fp8 copy), the
    linked dropout backward, and the deterministic partial rows."""
    from pytorch_vit_paper_replication_amd import _ext as E
    from tests import fp8_reference as FR
    from tests import kernel_checks as KC

    ext = _ext()
    T = RR.LN_T
    c = RR.make_ln(regime, T, D, device=DEV)
    _, mean, rstd = ext.layernorm_fwd(c.x, c.gamma, c.beta, RR.EPS, T, D)
    seed = torch.tensor([SEED_VAL], dtype=torch.int64, device=DEV)
    drop = variant in ("dz", "dpath+drop") or variant.endswith(("_dz", "_nostore"))
    dpath = "dpath" in variant
    every = 5 if "compact" in variant else 0
    dres = c.dres[::every].contiguous() if every else c.dres
    ref_kw, kw = dict(dres_every=every), dict(dres_every=every)
    if drop:
        ref_kw.update(keep=_keep_mask(T, D, seed, SEED_OFF, P), p=P)
        kw.update(want_dz=True, seed=seed, seed_offset=SEED_OFF, drop_p=P)
    if dpath:
        nb = (T + DP_ROWS - 1) // DP_ROWS
        s = ext.drop_path_scale(seed, DP_OFF, 0.3, nb)
        assert 0 < (s == 0).sum().item() < nb
        ref_kw.update(row_scale=s[torch.arange(T, device=DEV) // DP_ROWS])
        kw.update(want_dz=True, dp_seed=seed, dp_offset=DP_OFF, dp_p=0.3, dp_rows=DP_ROWS)
    r = RR.ln_ref64(c.x, c.gamma, c.beta, c.dy, dres, **ref_kw)
    e = RR.ln_emulate(c.x, c.gamma, c.beta, c.dy, dres, **ref_kw)
    j = _Judge(f"{_bwd_route(D)}+{variant}", regime, f"T{T} D{D}")
    if variant == "det":
        with E.deterministic_mode():
            a = _ln_bwd_run(ext, c, T, D, mean, rstd, dres, **dict(kw))
            b = _ln_bwd_run(ext, c, T, D, mean, rstd, dres, **dict(kw))
        atomic = _ln_bwd_run(ext, c, T, D, mean, rstd, dres, **dict(kw))
        torch.cuda.synchronize()
        j.flag("not_bitwise_repeatable", not all(torch.equal(_bits(p), _bits(q)) for p, q in zip(a, b) if p is not None))
        _judge_bwd(j, a, r, e, regime)
        _judge_bwd(j, atomic, r, e, regime, "@atomic")
    elif variant.startswith("q8"):
        fmt = 1 if "e5m2" in variant else 0
        plain = _ln_bwd_run(ext, c, T, D, mean, rstd, dres, **dict(kw))
        q = torch.zeros(T, D, dtype=torch.uint8, device=DEV)
        qs = torch.full((1,), 2.0, device=DEV)
        amax = torch.zeros(1, dtype=torch.int32, device=DEV)
        nostore = variant.endswith("_nostore")
        outs = _ln_bwd_run(ext, c, T, D, mean, rstd, dres, q_out=q, q_scale=qs, q_amax=amax, q_fmt=fmt, dz_nostore=nostore, **dict(kw))
        torch.cuda.synchronize()
        last = plain[1] if drop else plain[0]  # the gradient written last: dz with the linked dropout backward
        # the stand-alone quantiser of the bf16 gradient (tests/fp8_reference.py, which test_gpu_fp8_edges holds
        # ext.fp8_quant to; the kernel itself takes only 16-byte row strides, which D = 1032 is not)
        want = torch.from_numpy(FR.quant_reference(last.view(torch.int16).cpu().numpy().view(np.uint16), 2.0, fmt)).to(DEV)
        j.flag("dx_differs", not torch.equal(_bits(outs[0]), _bits(plain[0])))
        if drop and not nostore:
            j.flag("dz_differs", not torch.equal(_bits(outs[1]), _bits(plain[1])))
        if nostore:  # dz is not stored: the buffer keeps its NaN fill; judged from the plain run's dz
            j.flag("dz_written", (~torch.isnan(outs[1].float())).sum().item())
            outs = (outs[0], plain[1]) + outs[2:]
        # check_layernorm_bwd_q8's allowance: one code step, 5 % of the codes, amax to bf16 rounding
        j.bound("fp8_steps", KC._fp8_code_dist(q, want), 1)
        j.bound("fp8_mismatch", (q != want).float().mean().item(), 0.05)
        lm = last.float().abs().max().item()
        j.bound("amax_rel", abs(amax.view(torch.float32).item() - lm) / lm, 8e-3)
        _judge_bwd(j, outs, r, e, regime)
    else:
        outs = _ln_bwd_run(ext, c, T, D, mean, rstd, dres, **kw)
        torch.cuda.synchronize()
        _judge_bwd(j, outs, r, e, regime)
        if dpath:  # dsum == dz.sum(0) up to the order of the adds: the bias gradient of the tensor dz itself
            j.bound("dsum-dz.sum", RR.figures(outs[4], outs[1].double().sum(0))[0], 1e-6)
    j.done()


@pytest.mark.parametrize("regime", RR.LN_STRIDE_REGIMES)
@pytest.mark.parametrize("D", [768, 1024, 1280])
def test_layernorm_backward_grid_stride(D, regime):
    """More rows than the grid holds: 1024 workgroups (4096 rows) at D = 1024 and 1280, 3 per CU at D = 768.
    The rows past the cap are a second trip of the first workgroups, fed by the next-row prefetch: they
    must equal the same rows run alone (a small T, no second trip), bit for bit."""
    ext = _ext()
    first = 12 * ext.num_cus() if D == 768 else 4096
    T = first + 5
    c = RR.make_ln(regime, T, D, device=DEV)
    r = RR.ln_ref64(c.x, c.gamma, c.beta, c.dy, c.dres)
    e = RR.ln_emulate(c.x, c.gamma, c.beta, c.dy, c.dres)
    _, mean, rstd = ext.layernorm_fwd(c.x, c.gamma, c.beta, RR.EPS, T, D)
    outs = _ln_bwd_run(ext, c, T, D, mean, rstd, c.dres)
    tail = RR.LnCase(c.x[first:].contiguous(), c.dy[first:].contiguous(), c.dres[first:].contiguous(), c.gamma, c.beta)
    alone = _ln_bwd_run(ext, tail, 5, D, mean[first:].contiguous(), rstd[first:].contiguous(), tail.dres)
    torch.cuda.synchronize()
    j = _Judge(f"{_bwd_route(D)}+stride", regime, f"T{T} D{D}")
    _judge_bwd(j, outs, r, e, regime)
    j.flag("second_trip_rows_differ", (_bits(outs[0][first:]) != _bits(alone[0])).sum().item())
    j.done()


@pytest.mark.parametrize("regime", RR.LN_STRIDE_REGIMES)
@pytest.mark.parametrize("D", [768, 1032])
def test_layernorm_forward_q8_grid_stride(D, regime):
    """ln_fwd_q8_kernel's row loop: one workgroup per CU, so 4 CUs + 5 rows make a second trip."""
    ext = _ext()
    first = 4 * ext.num_cus()
    T = first + 5
    ext.set_ln_fwd_q8_grid(1)
    try:
        y, q = _ln_fwd_case(regime, T, D, f"ln_fwd_q8<{RR.ln_fwd_route(D)}>+stride")
        c = RR.make_ln(regime, T, D, device=DEV)
        q1 = torch.zeros(5, D, dtype=torch.uint8, device=DEV)
        y1, _, _ = ext.layernorm_fwd_q8(c.x[first:].contiguous(), c.gamma, c.beta, RR.EPS, 5, D, q1, torch.full((1,), QSCALE_FWD, device=DEV),
                                        torch.zeros(1, dtype=torch.int32, device=DEV), False)
        torch.cuda.synchronize()
    finally:
        ext.set_ln_fwd_q8_grid(4)
    assert torch.equal(_bits(y[first:]), _bits(y1)) and torch.equal(q[first:], q1), "second-trip rows differ from the rows run alone"


# ============================================================================= classifier head
@pytest.mark.parametrize("frozen_w", [False, True], ids=["train_w", "frozen_w"])
@pytest.mark.parametrize("regime", RR.HEAD_REGIMES)
@pytest.mark.parametrize("shape", RR.HEAD_SHAPES, ids=lambda s: "B%dN%dD%dC%d" % s)
def test_head(shape, regime, frozen_w):
    ext = _ext()
    B, N, D, C = shape
    c = RR.make_head(regime, B, N, D, C, device=DEV)
    r, e = RR.head_ref64(c, B, N), RR.head_emulate(c, B, N)
    logits, xhat, rstd = ext.head_fwd(c.tok, B, N, c.gamma, c.beta, RR.EPS, c.W, c.bias)
    dW, db, dg, dbt = (torch.zeros_like(t) for t in (c.W, c.bias, c.gamma, c.beta))
    dtok = ext.head_bwd(c.dl.contiguous(), xhat, rstd, c.gamma, c.beta, c.W, B, N, None if frozen_w else dW, db, dg, dbt)
    torch.cuda.synchronize()
    dt = dtok.view(B, N, D)
    j = _Judge("head", regime, f"B{B} N{N} D{D} C{C}{' frozen_w' if frozen_w else ''}")
    j.finite(logits=logits, xhat=xhat, rstd=rstd, dW=dW, db=db, dgamma=dg, dbeta=dbt, dtok=dtok)
    f32 = (1.5e-6, 2e-6)  # kernel_checks.check_head's limits
    j.figures("logits", logits, r.logits, e.logits, f32)
    j.figures("xhat", xhat, r.xhat, e.xhat, f32)
    j.scalar("rstd", (rstd.double() / r.rstd - 1).abs().max().item(), (e.rstd.double() / r.rstd - 1).abs().max().item(), 2.0 ** -22)
    if not frozen_w:
        j.figures("dW", dW, r.dW, e.dW, f32)
    j.figures("db", db, r.db, e.db, f32)
    j.figures("dgamma", dg, r.dgamma, e.dgamma, f32)
    j.figures("dbeta", dbt, r.dbeta, e.dbeta, f32)
    j.figures("dtok_cls", dt[:, 0], r.dcls, e.dcls)
    j.flag("other_rows_nonzero", (dt[:, 1:] != 0).sum().item())
    if frozen_w:
        j.flag("dW_written", (dW != 0).sum().item())
    if regime == "constant":
        j.flag("xhat!=0", (xhat != 0).sum().item())
        j.flag("dgamma!=0", (dg != 0).sum().item())
    j.done()


# ============================================================================= cross-entropy
EPS32 = float(np.float32(0.1))  # the binding narrows eps to fp32: the reference takes the same number
SOFT_CASES = [(1.0, 0.0), (0.0, 0.0), (0.3, 0.0), (1.0, EPS32), (0.0, EPS32), (0.3, EPS32)]


def _judge_xent(j, tag, x, c, r, k, loss, dl, corr, mean, B, eps):
    k_loss, k_grad = k
    finite_x = torch.where(torch.isfinite(x), x.abs(), torch.zeros_like(x)).amax(1).double()
    lk = loss.double()
    inf_rows = torch.isinf(r.loss)
    j.flag(f"{tag}.inf_rows_differ", (lk[inf_rows] != r.loss[inf_rows]).sum().item())
    ok = ~inf_rows
    scale = torch.maximum(torch.maximum(finite_x, r.loss.abs().masked_fill(inf_rows, 0)), torch.ones_like(finite_x))
    j.bound(f"{tag}.loss/bound", ((lk - r.loss).abs()[ok] / (k_loss * U * scale[ok])).max().item() if ok.any() else 0.0, 1.0)
    j.bound(f"{tag}.dl/bound", ((dl.double() - r.dlogits).abs().max().item()) / (k_grad * U / B), 1.0)
    j.flag(f"{tag}.flags", (corr.bool() != r.correct).sum().item())
    j.flag(f"{tag}.ignored_nonzero", (lk[~r.valid] != 0).sum().item() + (dl[~r.valid] != 0).sum().item())
    if c.masked is not None and eps == 0:
        j.flag(f"{tag}.masked_grad", (dl[c.masked] != 0).sum().item())
        j.finite(**{f"{tag}.loss": loss})
    j.finite(**{f"{tag}.dl": dl})
    if ok.all():  # the batch mean of the kernel's own rows, in float64
        j.bound(f"{tag}.mean/bound", abs(mean.item() - lk.mean().item()) / max(B * U * lk.abs().max().item(), 1e-300), 1.0)
    else:
        j.flag(f"{tag}.mean_not_inf", not math.isinf(mean.item()))


@pytest.mark.parametrize("strided", [False, True], ids=["contig", "strided"])
@pytest.mark.parametrize("regime", RR.LOGIT_REGIMES)
@pytest.mark.parametrize("shape", RR.XENT_SHAPES, ids=lambda s: "B%dC%d" % s)
def test_cross_entropy(shape, regime, strided):
    """xent_kernel and xent_soft_kernel (lam in {1, 0, 0.3} x eps in {0, 0.1}, and ya == yb); ``strided``:
    the logits are the leading C columns of a wider matrix (the kernels take a row stride)."""
    ext = _ext()
    B, C = shape
    c = RR.make_logits(regime, B, C, device=DEV)
    x = c.logits
    if strided:
        big = torch.full((B, C + 13), 1e30, device=DEV)
        big[:, :C] = c.logits
        x = big[:, :C]
        assert x.stride(0) == C + 13 and not x.is_contiguous() or B == 1
    j = _Judge("xent", regime, f"B{B} C{C}{' strided' if strided else ''}")

    def run(fn, *args):
        dl = torch.full((B, C), float("nan"), device=DEV)
        corr = torch.full((B,), 7, dtype=torch.int32, device=DEV)
        mean = torch.full((1,), float("nan"), device=DEV)
        loss = fn(x, *args, dl, corr, 1.0 / B, mean)
        return loss, dl, corr, mean

    hard = run(ext.xent, c.labels)
    torch.cuda.synchronize()
    _judge_xent(j, "xent", c.logits, c, RR.xent_ref64(c.logits, c.labels, grad_scale=1.0 / B), RR.xent_roundings(C), *hard, B, 0.0)
    for lam, eps in SOFT_CASES:
        for same in (False, True):
            if same and lam != 0.3:
                continue
            yb = c.labels if same else c.other
            lam_t = torch.full((B,), lam, device=DEV)
            soft = run(ext.xent_soft, c.labels, yb, lam_t, eps)
            torch.cuda.synchronize()
            r = RR.xent_ref64(c.logits, c.labels, yb, lam_t, eps, 1.0 / B)
            tag = f"soft[{lam:g},{0.1 if eps else 0:g}{',ya=yb' if same else ''}]"
            _judge_xent(j, tag, c.logits, c, r, RR.xent_roundings(C, eps, soft=True), *soft, B, eps)
    # lam = 1, eps = 0, yb = ya: xent's bits
    same = run(ext.xent_soft, c.labels, c.labels, torch.ones(B, device=DEV), 0.0)
    torch.cuda.synchronize()
    j.flag("soft(1,0,ya)!=xent", sum(int(not torch.equal(a.view(torch.int32), b.view(torch.int32))) for a, b in zip(same, hard)))
    j.done()


# ============================================================================= GELU probe
def _gelu_bias(N, kind):
    if kind == "zero":
        return torch.zeros(N, device=DEV)
    return ((torch.arange(N, device=DEV) % 7) - 3).float()  # small integers, exact in fp32


def _judge_gelu(j, u, h, d=None):
    """h (and the stored derivative d) per element against the float64 formula at the fp32 pre-activation u."""
    g64, d64, _ = RR.gelu_formula64(u)
    g32, d32, _ = RR.gelu_emulate(u)
    gr, dr, _ = RR.gelu_ref64(u)
    for name, out, f, emu, ref in (("h", h, g64, g32, gr), ("d", d, d64, d32, dr)):
        if out is None:
            continue
        o = out.double()
        j.flag(f"{name}.nan", torch.isnan(o).sum().item())
        lim = 2.0 ** -8 * f.abs() + 4.0 * (emu.double() - f).abs() + RR.BF16_MIN_NORMAL
        j.bound(f"{name}/limit", ((o - f).abs() / lim).max().item(), 1.0)
        j.bound(f"{name}_formula-erfc", (f - ref).abs().max().item(), math.inf)  # reported: the CPU test owns it
    zero = u == 0
    if zero.any():
        j.flag("h(0)!=0", (h[zero] != 0).sum().item())
        if d is not None:
            j.flag("d(0)!=0.5", (d[zero].float() != 0.5).sum().item())
    far_neg, far_pos = u <= -40, u >= 40
    j.flag("h(u<=-40)!=0", (h[far_neg] != 0).sum().item())
    j.flag("h(u>=40)!=bf16(u)", (_bits(h[far_pos]) != _bits(u[far_pos].to(torch.bfloat16))).sum().item())
    if d is not None:
        j.flag("d(u>=40)!=1", (d[far_pos].float() != 1).sum().item())
    tiny = u.abs() == 2.0 ** -100
    if tiny.any():  # the sign select of the two-lane form: Phi = 1/2 on either side of zero
        j.flag("h(+-2^-100)!=u/2", (h[tiny].float() != (u[tiny] * 0.5).to(torch.bfloat16).float()).sum().item())


@pytest.mark.parametrize("bias", ["zero", "ints"])
@pytest.mark.parametrize("t", RR.GELU_TILES)
def test_gelu_epilogues(t, bias):
    """gelu_and_grad (tile 0 / 6 epilogue of gemm.hip), gelu_and_grad2 (the ping-pong epilogues of tiles 12
    and 13 in gemm.hip, the wave-specialised tile 15 of gemm_ws.hip), each with the stored derivative."""
    from pytorch_vit_paper_replication_amd.ops import gemm as G
    from tests import kernel_checks as KC

    M, N, K = RR.GELU_PROBE
    x, w = RR.gelu_probe_operands(M, N, K, device=DEV)
    b = _gelu_bias(N, bias)
    aux = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
    with KC.tile(t):
        h = G.linear_fwd(x, w, b, gelu_aux=aux)
    torch.cuda.synchronize()
    u = RR.gelu_probe_product(w, M) + b  # fp32: one rounding, as in the epilogue
    j = _Judge(f"gelu tile {t}", f"bias_{bias}", f"M{M} N{N} K{K}")
    _judge_gelu(j, u, h, aux)
    j.done()


@pytest.mark.parametrize("bias", ["zero", "ints"])
def test_gelu_splitk_epilogue(bias):
    """gelu_and_grad in elementwise.hip's split-K reduction pass: the smallest M and K the route takes."""
    from pytorch_vit_paper_replication_amd.ops import gemm as G

    M, N, K = 2048, 256, 256
    assert G._small_splitk(M, N, K) >= 2 and G._small_splitk(M - 1, N, K) == 0 and G._small_splitk(M, N, K - 128) == 0
    x, w = RR.gelu_probe_operands(M, N, K, device=DEV)
    b = _gelu_bias(N, bias)
    h = G.linear_fwd(x, w, b, gelu=True)
    torch.cuda.synchronize()
    j = _Judge("gelu split-K epilogue", f"bias_{bias}", f"M{M} N{N} K{K}")
    _judge_gelu(j, RR.gelu_probe_product(w, M) + b, h)
    j.done()


@pytest.mark.parametrize("wt,t", [(False, None), (False, 12), (True, 12), (True, 13), (True, 15)])
def test_dgelu_dgrad_takes_the_stored_derivative(wt, t):
    """The dGELU dgrad epilogue multiplies the product by the stored derivative: with an exact product
    (one-hot dy rows select rows of w) and the derivative tile 0 stored for the grid, every element is one
    fp32 product rounded to bf16."""
    from pytorch_vit_paper_replication_amd.ops import gemm as G
    from tests import kernel_checks as KC

    M, N, K = RR.GELU_PROBE  # the forward probe: aux [M, N]
    x, w = RR.gelu_probe_operands(M, N, K, device=DEV)
    aux = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
    with KC.tile(0):
        G.linear_fwd(x, w, torch.zeros(N, device=DEV), gelu_aux=aux)
    # dgrad: dx [M, N] = (dy [M, K] . wd [K, N]) * aux, dy one-hot: the product is wd[i % K, :]
    dy = x
    wd = w.t().contiguous()  # [K, N], grid values
    with KC.tile(t if wt else None):
        dx = G.linear_dgrad(dy, wd, dgelu_aux=aux, wt=w.contiguous() if wt else None, tile=t)
    torch.cuda.synchronize()
    prod = wd.float()[torch.arange(M, device=DEV) % K]
    want = prod.double() * aux.double()
    j = _Judge(f"dgelu dgrad tile {t}{' wt' if wt else ''}", "grid", f"M{M} N{K} K{N}")
    j.flag("nan", torch.isnan(dx.float()).sum().item())
    fin = torch.isfinite(want) & (want.abs() < 3e38)
    j.bound("dx/limit", ((dx.double() - want).abs()[fin] / (2.0 ** -8 * want.abs()[fin] + RR.BF16_MIN_NORMAL)).max().item(), 1.0)
    j.done()
