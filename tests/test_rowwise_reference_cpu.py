"""Conditions on the inputs and yardsticks of tests/test_gpu_rowwise_regimes.py, proved on the CPU
before any GPU figure is trusted (tests/rowwise_reference.py):

* the fp32 emulations of LayerNorm, the head and the GELU formula agree with their float64 references
  on Gaussian inputs to what bf16 and fp32 rounding allow (each bound derived where it is asserted);
* every regime is what its name says, on every shape the GPU test runs: constant rows have an exact
  fp32 sum, xhat = 0, y = bf16(beta) and rstd = rsqrt(eps); tiny rows have a variance of at most eps / 4;
  tie rows have exactly two classes at the maximum; no label of a masked row is masked; the outlier
  columns of massive rows carry more than 99 % of the row's variance (97 % at D = 8 and 98.8 % at
  D = 2048, where +-300 cannot give more: the arithmetic is at the assertion);
* the error of the GELU formula itself, in float64, against erfc: the absolute error of Phi times
  max(1, |u|), and its relative error through the tail. The GPU test holds the kernels to the formula,
  so this file owns the formula's distance from the function;
* the exact-operand GEMM input of the GELU probe returns the chosen w entries bit for bit.
"""
import math

import pytest
import torch

from tests import rowwise_reference as RR

U = 2.0 ** -24  # half an fp32 ulp, relative
ALL_DS = sorted(set(RR.LN_FWD_DS + RR.LN_BWD_DS))


def _sum_l2(n, abs_terms, ref):
    """Relative L2 an fp32 sum of n terms may be off by: (n + 16) roundings of 2^-24, each at most at
    the size of the sum of the absolute terms (16: the roundings inside a term)."""
    return (n + 16) * U * abs_terms.double().norm().item() / ref.double().norm().item()


# ----------------------------------------------------------------------------- emulation against reference
@pytest.mark.parametrize("D", ALL_DS)
def test_ln_emulation_meets_float64_on_gauss(D):
    T = RR.LN_T
    c = RR.make_ln("gauss", T, D)
    r = RR.ln_ref64(c.x, c.gamma, c.beta, c.dy, c.dres)
    e = RR.ln_emulate(c.x, c.gamma, c.beta, c.dy, c.dres)
    fy, fdx = RR.figures(e.y, r.y), RR.figures(e.dx, r.dx)
    mean_err = (e.mean.double() - r.mean).abs().max().item()
    rstd_err = (e.rstd.double() / r.rstd - 1).abs().max().item()
    print(f"ln gauss D{D}: y {fy[0]:.2e}/{fy[1]:.2e} dx {fdx[0]:.2e}/{fdx[1]:.2e} mean {mean_err:.2e} rstd {rstd_err:.2e}")
    # y and dx: each element is the fp32 value (within a few 2^-24 of float64) rounded to bf16: half an
    # ulp, which is 2^-9 of the element at a significand near 2 and 2^-8 at a significand of 1. So no
    # row's relative L2 exceeds 2^-8 (1 %: the fp32 part), a row of uniform significands sits near
    # 2^-9 / sqrt 3 * 1.4 = 1.6e-3, and anything under 2^-11 would mean the rounding is missing
    for f in (fy, fdx):
        assert 2.0 ** -11 <= f[0] <= 1.01 * 2.0 ** -8 and f[1] <= 1.01 * 2.0 ** -8
    # mean: an fp32 sum of D terms, at most D roundings at the size of the sum of |x|, divided by D
    assert mean_err <= D * U * c.x.float().abs().mean().item()
    # rstd: var carries the same D roundings relative to itself (all terms positive) plus 4 for the
    # differences' squares; rsqrt halves a relative error and adds its own ulp (2 U)
    assert rstd_err <= (D / 2 + 4) * U
    xh, dy = r.xhat, c.dy.double()
    for name, out, ref, terms in (("dgamma", e.dgamma, r.dgamma, (dy * xh).abs().sum(0)), ("dbeta", e.dbeta, r.dbeta, dy.abs().sum(0)),
                                  ("dsum", e.dsum, r.dsum, r.dx.abs().sum(0))):
        l2 = RR.figures(out, ref)[0]
        lim = _sum_l2(T, terms, ref)
        print(f"   {name} l2 {l2:.2e} / {lim:.2e}")
        assert l2 <= lim


@pytest.mark.parametrize("keep,scale,every", [(True, False, 0), (False, True, 0), (True, True, 5), (False, False, 5)])
def test_ln_emulation_variants_meet_float64(keep, scale, every):
    """dz = factor * dx with the keep mask and the row scale, the compact residual: same bounds."""
    T, D, p = RR.LN_T, 768, 0.1
    c = RR.make_ln("gauss", T, D)
    g = RR._gen(5)
    kw = dict(dres_every=every)
    if keep:
        kw.update(keep=torch.rand(T, D, generator=g) >= p, p=p)
    if scale:
        kw.update(row_scale=(torch.rand(T, generator=g) >= 0.3).float() / 0.7)
    dres = c.dres[::every].contiguous() if every else c.dres
    r, e = RR.ln_ref64(c.x, c.gamma, c.beta, c.dy, dres, **kw), RR.ln_emulate(c.x, c.gamma, c.beta, c.dy, dres, **kw)
    assert RR.figures(e.dx, r.dx)[1] <= 1.01 * 2.0 ** -8
    if every:
        assert torch.equal(r.dx[1] - RR.ln_ref64(c.x, c.gamma, c.beta, c.dy, None).dx[1], torch.zeros(D, dtype=torch.float64))
    if keep or scale:
        assert RR.figures(e.dz, r.dz)[1] <= 1.01 * 2.0 ** -8
        # with a row scale the sums run over the stored bf16 dz: one more half-ulp per term
        lim = _sum_l2(T, r.dz.abs().sum(0), r.dsum) + (2.0 ** -8 * r.dz.abs().sum(0).norm() / r.dsum.norm()).item() * scale
        assert RR.figures(e.dsum, r.dsum)[0] <= lim
    else:
        assert e.dz is None and r.dz is None


@pytest.mark.parametrize("B,N,D,C", RR.HEAD_SHAPES)
def test_head_emulation_meets_float64_on_gauss(B, N, D, C):
    c = RR.make_head("gauss", B, N, D, C)
    r, e = RR.head_ref64(c, B, N), RR.head_emulate(c, B, N)
    xc = (r.xhat * c.gamma.double() + c.beta.double()).abs()
    dy = c.dl.double() @ c.W.double()
    dya = c.dl.double().abs() @ c.W.double().abs()
    checks = (("logits", e.logits, r.logits, D, xc @ c.W.double().abs().t() + c.bias.double().abs()),
              ("dW", e.dW, r.dW, B, c.dl.double().abs().t() @ xc), ("db", e.db, r.db, B, c.dl.double().abs().sum(0)),
              # dgamma, dbeta: sums over B of dy (a sum over C) times xhat (D roundings in its statistics)
              ("dgamma", e.dgamma, r.dgamma, B + C + D, (dya * r.xhat.abs()).sum(0)), ("dbeta", e.dbeta, r.dbeta, B + C, dya.sum(0)))
    for name, out, ref, n, terms in checks:
        l2, lim = RR.figures(out, ref)[0], _sum_l2(n, terms, ref)
        print(f"head B{B} N{N} D{D} C{C} {name}: {l2:.2e} / {lim:.2e}")
        assert l2 <= lim
    f = RR.figures(e.dcls, r.dcls)
    assert 2.0 ** -11 <= f[0] <= 1.01 * 2.0 ** -8 and f[1] <= 1.01 * 2.0 ** -8  # bf16 rows, as LayerNorm's dx
    assert dy.shape == (B, D)


def test_gelu_emulation_meets_the_float64_formula():
    u = RR.gelu_grid()
    g64, d64, _ = RR.gelu_formula64(u)
    g32, d32, _ = RR.gelu_emulate(u)
    assert torch.isfinite(g32).all() and torch.isfinite(d32).all()
    ud = u.double()
    pdf = torch.exp(-0.5 * ud * ud) / math.sqrt(2 * math.pi)
    cdf = RR.gelu_ref64(u)[2]
    # exp2's argument w = -u^2 log2(e) / 2 is rounded twice in fp32: a relative error of |w| ln 2 * 2 U
    # = u^2 U in the exponential; 16 more roundings in the reciprocal, the polynomial and the products.
    # Each is relative to the sizes of the terms: |u| Phi for g, Phi + |u| phi for g'. For u > 0, Phi
    # is 1 - half_erfc, exact to U at the size of 1.
    k = (ud * ud + 16) * U
    eg = (g32.double() - g64).abs()
    ed = (d32.double() - d64).abs()
    lim_g = k * ud.abs() * torch.maximum(cdf, torch.full_like(cdf, 0.0)) + ud.abs() * U * (ud > 0)
    lim_d = k * (cdf + ud.abs() * pdf) + U * (ud > 0)
    worst_g, worst_d = (eg / lim_g.clamp_min(1e-300)).max().item(), (ed / lim_d.clamp_min(1e-300)).max().item()
    print(f"gelu_emulate vs gelu_formula64: worst g {worst_g:.2f}, g' {worst_d:.2f} of the fp32 bound")
    big = ud.abs() >= 40  # exp2 underflows in both: identical
    assert torch.equal(g32[big].double(), g64[big]) and torch.equal(d32[big].double(), d64[big])
    assert (eg[~big] <= lim_g[~big] + 1e-45).all() and (ed[~big] <= lim_d[~big]).all()


# ----------------------------------------------------------------------------- regime conditions
@pytest.mark.parametrize("D", ALL_DS)
def test_constant_rows_are_exact(D):
    T = RR.LN_T
    c = RR.make_ln("constant", T, D)
    xf = c.x.float()
    assert (xf == xf[:, :1]).all() and (xf[:, 0] == 0).any() and xf[:, 0].unique().numel() == len(RR.CONSTANT_VALUES)
    # D times an 8-bit significand fits in 24 bits for D <= 2048: every partial sum k v is an fp32 number
    assert D <= 2048
    assert torch.equal(xf.sum(1).double(), xf.double().sum(1)) and torch.equal(xf.cumsum(1).double(), xf.double().cumsum(1))
    e = RR.ln_emulate(c.x, c.gamma, c.beta, c.dy, c.dres)
    assert torch.equal(e.mean, xf[:, 0])
    assert (e.xhat == 0).all()
    assert torch.equal(e.rstd, torch.rsqrt(torch.full((T,), RR.EPS)))
    assert torch.equal(e.y, c.beta.to(torch.bfloat16).expand(T, D))
    assert (e.dgamma == 0).all()
    r = RR.ln_ref64(c.x, c.gamma, c.beta, c.dy, c.dres)
    assert (r.dgamma == 0).all() and torch.equal(r.y, c.beta.double().expand(T, D))


@pytest.mark.parametrize("D", ALL_DS)
def test_ln_regimes_are_what_their_names_say(D):
    T = RR.LN_T
    stat = lambda x: (x.double().mean(1), x.double().var(1, unbiased=False))  # noqa: E731
    _, var = stat(RR.make_ln("tiny", T, D).x)
    assert var.max().item() <= RR.EPS / 4
    mean, var = stat(RR.make_ln("offset", T, D).x)
    assert (mean.abs() / var.sqrt()).min().item() >= 20 and (mean > 0).any() and (mean < 0).any()
    x = RR.make_ln("massive", T, D).x.double()
    cols = list(RR.massive_columns(D))
    assert len(set(cols)) == 3
    dev2 = (x - x.mean(1, keepdim=True)) ** 2
    share = (dev2[:, cols].sum(1) / dev2.sum(1)).min().item()
    # two columns at +-300 carry 2 * 300^2 = 180000 of a sum of squared deviations of 180000 + D, which is
    # more than 99 % up to D = 1818. Two of the shapes here cannot reach 99 % with these inputs, by
    # arithmetic: the forward's D = 2048 (180000 / 182048 = 98.9 %), and D = 8, where the third outlier
    # moves the row mean to 300 / 8 and the five ordinary columns then hold 5 * 37.5^2 of 258000 (97.2 %).
    print(f"massive D{D}: outlier share of the variance >= {share:.4f}")
    assert share > (0.97 if D == 8 else 0.99 if D <= 1544 else 0.988)
    assert (x[::3, cols[2]] == RR.MASSIVE).all() and (x[1::3, cols[2]].abs() < 10).all()
    assert RR.make_ln("large", T, D).x.float().abs().max().item() >= 2.0 ** 20
    g = RR.make_ln("gamma_edge", T, D).gamma
    assert (g == 0).any() and (g < 0).any() and (g == 1e-4).any()
    dy = RR.make_ln("dy_sparse", T, D).dy
    live = dy.float().abs().sum(1) != 0
    assert torch.equal(live, torch.arange(T) % RR.SPARSE_EVERY == 0)
    dyo = RR.make_ln("dy_offset", T, D).dy.double()
    assert (dyo.mean(1) - 8).abs().max().item() < 1.0
    assert RR.ln_fwd_route(D) in (1, 2, 3, 4)


def test_the_shape_tables_reach_every_route():
    fwd = {(RR.ln_fwd_route(D), (D // 8) % 64 == 0) for D in RR.LN_FWD_DS}
    assert fwd == {(m, full) for m in (1, 2, 3, 4) for full in (True, False)}
    bwd = {RR.ln_bwd_route(D) for D in RR.LN_BWD_DS}
    assert bwd == {(1, 4), (3, 4), (5, 4), (1, 8), (2, 8), (3, 8)}
    partial = {RR.ln_bwd_route(D) for D in RR.LN_BWD_DS if (D // RR.ln_bwd_route(D)[1]) % 64}
    assert partial == {(1, 8), (2, 8), (3, 8)}  # the 4-column routes are taken only where they tile the row
    assert {RR.ln_bwd_route(D) for D in RR.LN_VARIANT_DS} == {(3, 4), (3, 8), (5, 4)}


@pytest.mark.parametrize("B,C", RR.XENT_SHAPES)
def test_logit_regimes_are_what_their_names_say(B, C):
    c = RR.make_logits("tie", B, C)
    top = (c.logits == c.logits.amax(1, keepdim=True))
    if C >= 2:
        assert (top.sum(1) == 2).all() and top.gather(1, c.labels[:, None]).all()
        first = RR.first_argmax(c.logits)
        assert torch.equal(first == c.labels, torch.arange(B) % 2 == 1)  # the lower index is the argmax
    c = RR.make_logits("masked", B, C)
    assert not c.masked.gather(1, c.labels[:, None]).any() and not c.masked.gather(1, c.other[:, None]).any()
    assert torch.equal(torch.isinf(c.logits), c.masked)
    if C >= 3:
        assert 0.2 < c.masked.float().mean().item() < 0.45
    r = RR.xent_ref64(c.logits, c.labels)
    assert torch.isfinite(r.loss).all() and (r.dlogits[c.masked] == 0).all()
    c = RR.make_logits("confident", B, C)
    assert torch.equal(RR.first_argmax(c.logits), c.labels)
    if C >= 2:
        rest = c.logits.scatter(1, c.labels[:, None], -math.inf).amax(1)
        assert (c.logits.gather(1, c.labels[:, None])[:, 0] - rest >= 29.99).all()
        w = RR.make_logits("wrong", B, C)
        assert (RR.first_argmax(w.logits) != w.labels).all()
    c = RR.make_logits("ignore", B, C)
    r = RR.xent_ref64(c.logits, c.labels)
    assert (c.labels == -100).any() and (c.labels == C).any()
    assert (r.loss[~r.valid] == 0).all() and (r.dlogits[~r.valid] == 0).all() and (~r.valid).sum() >= 2
    c = RR.make_logits("uniform", B, C)
    assert (c.logits == c.logits[0, 0]).all() and (c.labels == 0).any()
    for s, sign in (("shift_pos", 1), ("shift_neg", -1)):
        assert (RR.make_logits(s, B, C).logits * sign > 9.9e3).all()
    # the reference against torch's own cross-entropy where that is defined
    c = RR.make_logits("gauss", B, C)
    r = RR.xent_ref64(c.logits, c.labels, grad_scale=1.0 / B)
    x = c.logits.double().requires_grad_(True)
    ref = torch.nn.functional.cross_entropy(x, c.labels)
    ref.backward()
    assert abs(r.mean.item() - ref.item()) <= 1e-12 * max(1, abs(ref.item())) and (r.dlogits - x.grad).abs().max().item() <= 1e-15
    lam = torch.full((B,), 0.3)
    rs = RR.xent_ref64(c.logits, c.labels, c.other, lam, 0.1)
    q = 0.9 * (0.3 * torch.nn.functional.one_hot(c.labels, C) + 0.7 * torch.nn.functional.one_hot(c.other, C)).double() + 0.1 / C
    want = -(q * torch.log_softmax(c.logits.double(), 1)).sum(1)
    assert (rs.loss - want).abs().max().item() <= 1e-12 * max(1.0, want.abs().max().item())


# ----------------------------------------------------------------------------- the formula's own error
# relative error of the formula's Phi(u) for u < 0, per stretch of the tail: the figures found in float64
# (4.7e-4 at -4, 1.6e-3 at -5, 3.6e-3 at -6, 1.0e-2 at -8, 3.1e-2 at -12; it grows with |u|, so each
# stretch is bounded by its far end), with 5 % for the two digits they are quoted to
GELU_TAIL_REL = ((-4.0, -3.0, 4.7e-4), (-5.0, -4.0, 1.6e-3), (-6.0, -5.0, 3.6e-3), (-8.0, -6.0, 1.0e-2), (-12.0, -8.0, 3.1e-2))
GELU_ABS_BOUND = 2.5e-7  # |dPhi| max(1, |u|): 2.1e-7 found (at u = 3)


def test_gelu_formula_error_in_float64():
    u = RR.gelu_grid()
    ud = u.double()
    _, _, cdf_f = RR.gelu_formula64(u)
    _, _, cdf = RR.gelu_ref64(u)
    err = (cdf_f - cdf).abs()
    scaled = err * ud.abs().clamp_min(1.0)
    i = scaled.argmax().item()
    print(f"gelu formula: max |dPhi| max(1, |u|) = {scaled[i].item():.3e} at u = {ud[i].item():.3f}; max |dPhi| = {err.max().item():.3e}")
    assert scaled.max().item() <= GELU_ABS_BOUND
    for lo, hi, lim in GELU_TAIL_REL:
        m = (ud >= lo) & (ud <= hi)
        rel = (err[m] / cdf[m]).max().item()
        print(f"gelu formula: relative error of Phi on [{lo}, {hi}]: {rel:.3e} (limit {1.05 * lim:.2e})")
        assert m.sum() >= 20 and rel <= 1.05 * lim
        assert rel >= 0.2 * lim  # the table describes this formula, not a better one
    # the functions built on it
    g, d, _ = RR.gelu_formula64(u)
    gr, dr, _ = RR.gelu_ref64(u)
    assert ((g - gr).abs() <= GELU_ABS_BOUND).all()                     # |u| |dPhi|
    assert ((d - dr).abs() <= GELU_ABS_BOUND * (1 + 1e-6)).all()        # |dPhi| alone: u phi(u) is exact here
    assert g[0] == 0 and g[1] == 0 and d[0] == d[1] and abs(d[0].item() - 0.5) <= 1e-9


def test_gelu_branch_at_zero_cannot_be_seen_in_bf16():
    """``u >= 0 ? 1 - he : he`` at u = +-0: the Abramowitz-Stegun coefficients sum to 1 - 1e-9, so he(0) is
    1/2 within an fp32 ulp and both branches give Phi(0) = 1/2 to bf16 (and g = 0 Phi = 0 exactly).
    Whether the comparison is >= or > therefore changes no bf16 output: no test of the kernels can tell."""
    assert abs(sum(RR.GELU_A) - 1.0) <= 2e-9
    a = [torch.tensor(v, dtype=torch.float32) for v in RR.GELU_A]
    t = torch.tensor(1.0)  # 1 / (1 + p |0|)
    poly = t * a[4] + a[3]
    for c in (a[2], a[1], a[0]):
        poly = t * poly + c
    he = 0.5 * t * poly * torch.exp2(torch.tensor(0.0))
    assert abs(he.item() - 0.5) <= 2.0 ** -24
    assert he.to(torch.bfloat16) == (1.0 - he).to(torch.bfloat16) == 0.5


def test_gelu_emulation_flushes_where_the_hardware_exponential_does():
    """The kernels take exp(-u^2 / 2) from one v_exp_f32, which returns 0 where the result would be an fp32
    subnormal: u^2 log2(e) / 2 > 126, |u| > 13.22. There g' = u phi(u) + Phi(u) is lost, up to
    13.22 * 0.39894 * 2^-126 = 5.3 * 2^-126 = 6.2e-38 in size; the emulation does the same."""
    u = torch.tensor([-13.25, -13.2, 13.25], dtype=torch.float32)
    g32, d32, _ = RR.gelu_emulate(u)
    _, d64, _ = RR.gelu_formula64(u)
    assert d32[0] == 0 and d32[1] != 0 and g32[0] == 0
    assert 0 < -d64[0].item() <= 5.3 * 2.0 ** -126


def test_gelu_grid_holds_what_it_says():
    u = RR.gelu_grid()
    assert u.dtype == torch.float32 and u.numel() == 4 + 4096 + 209 + 6
    assert math.copysign(1.0, u[1].item()) == -1.0 and u[0] == 0 and u[1] == 0
    tail = u[4 + 4096:4 + 4096 + 209]
    assert tail[0] == -3.0 and tail[-1] == -9.0 and torch.equal(tail, tail.to(torch.bfloat16).float())
    assert (tail[1:] < tail[:-1]).all()  # consecutive bf16 patterns


# ----------------------------------------------------------------------------- the exact GEMM operand
def test_gelu_probe_operand_is_exact():
    M, N, K = RR.GELU_PROBE
    x, w = RR.gelu_probe_operands(M, N, K)
    assert (x.float().sum(1) == 1).all() and (x.float().abs().sum(1) == 1).all()
    grid = RR.gelu_grid().to(torch.bfloat16)
    assert N * K >= grid.numel() and M >= K  # every grid value is in w, every column of w is selected
    assert torch.equal(w.flatten()[:grid.numel()].view(torch.int16), grid.view(torch.int16))
    prod = x.float() @ w.float().t()
    want = RR.gelu_probe_product(w, M)
    # bit for bit, but for the sign of zero: the sum of 0 * w and 1 * (-0) is +0
    assert torch.equal(prod, want)
    nz = want != 0
    assert torch.equal(prod[nz].view(torch.int32), want[nz].view(torch.int32))
    assert (prod[~nz].view(torch.int32) == 0).all() and (want[~nz].view(torch.int32) != 0).any()
    # and in bf16 accumulate-then-round form (tile 15 rounds the product): the same values
    assert torch.equal(prod.to(torch.bfloat16).float(), prod)
