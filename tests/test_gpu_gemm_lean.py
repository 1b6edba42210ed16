"""Lean instantiations of the 256x256 ping-pong GEMM kernels (csrc/gemm_lean.h) against the general
kernels they specialise.

Every case runs the same launch with ``set_gemm_lean(True)`` and ``(False)`` and requires bit-identical
outputs (C, the GELU aux, the dGELU column sums, the weight-gradient fp32 result), and checks through
``ext.gemm_lean_last()`` which instantiation the launcher took: the expected GemmLean bits with the
switch on, the general kernel (0) with it off and for every launch outside the list. The one-tile
residual + bias and plain forms and the weight gradient measured no faster on a lean kernel and are
not on the list (profiles/gemm_lean/README.md): their cases stay, and assert the general kernel. One comparison
per epilogue kind against an fp32 reference uses the tolerances tests/kernel_checks.py has for that
kind (check_gemm_fwd, check_gemm_gelu, check_gemm_dgelu, check_gemm_wgrad).

Shapes are the smallest that reach each path: M = 528 is two row tiles, the second with 16 live rows;
the split tail needs just over one dispatch round of tiles and K = 1536 for two K-parts; the persistent
kernels take more than one tile per workgroup at 4 * CUs / 3 + 1 row tiles of 3 column tiles.

The N = 772 fallback case of the one-tile shapes cannot reach a kernel: ``ext.gemm`` refuses an N
that is no multiple of 8 before it plans the launch. The test asserts that refusal under both
settings; tests/cpp/test_gemm_lean.cpp checks that the chooser itself sends N = 772 to the general
kernel.
"""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"
ON, BIAS, DROP, RES, TAIL, AUX, COLSUM = 1, 2, 4, 8, 16, 32, 64  # csrc/gemm_lean.h GemmLean


def _kc():
    from tests import kernel_checks as KC

    return KC


def _ext():
    from pytorch_vit_paper_replication_amd import _ext

    return _ext.ext()


def _G():
    from pytorch_vit_paper_replication_amd.ops import gemm as G

    return G


def _bits(t):
    """The tensor's bits as integers (bit-identical comparison: -0 != +0, NaN payloads count)."""
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def ab(fn, want, tile=None):
    """Run ``fn`` (returns a tuple of output tensors) with the lean kernels on and off; assert the
    instantiation taken (``want`` GemmLean bits with the switch on, 0 with it off) and bit-identical
    outputs. Returns the lean-on outputs."""
    ext, KC = _ext(), _kc()
    outs = {}
    try:
        for on in (True, False):
            ext.set_gemm_lean(on)
            with KC.tile(tile):
                outs[on] = fn()
            torch.cuda.synchronize()
            assert ext.gemm_lean_last() == (want if on else 0), (on, ext.gemm_lean_last(), want)
    finally:
        ext.set_gemm_lean(True)
    assert len(outs[True]) == len(outs[False])
    for i, (a, b) in enumerate(zip(outs[True], outs[False])):
        assert _same(a, b), f"output {i}: {(_bits(a) != _bits(b)).sum().item()} elements differ between lean and general"
    return outs[True]


def _close(name, pairs, limits, extra=None):
    KC = _kc()
    m = KC.worst(*pairs)
    m.update(extra or {})
    print(f"{name}: {KC.fmt_metrics(m, limits)}")
    assert KC.passed(m, limits), f"{name}: {KC.fmt_metrics(m, limits)}"


def _seed():
    return torch.tensor([20240607], dtype=torch.int64, device=DEV)


@pytest.fixture(scope="module")
def small():
    """One-tile shapes: M = 528 (two row tiles, 16 live rows in the second), N = 768, K = 128."""
    KC = _kc()
    torch.manual_seed(11)
    M, N, K = 528, 768, 128
    return dict(M=M, N=N, K=K, x=KC.bf(KC.rnd(M, K)), w=KC.bf(KC.rnd(N, K, scale=0.05)), b=KC.rnd(N), r=KC.bf(KC.rnd(M, N)))


# ----------------------------------------------------------------------------- one tile per workgroup
def test_one_tile_residual_bias(small):
    G, s = _G(), small
    # (measured no faster than the general kernel at the out-proj shape: not on the list, general kernel)
    (y,) = ab(lambda: (G.linear_fwd(s["x"], s["w"], s["b"], resid=s["r"]),), 0, tile=12)
    ref = s["x"].float() @ s["w"].float().t() + s["b"] + s["r"].float()
    _close("one-tile resid+bias vs fp32", [(y, ref)], _kc().lim(3.5e-3, 7e-3))  # check_gemm_fwd


def test_one_tile_residual_bias_dropout(small):
    G, s = _G(), small
    drop = (_seed(), 4 << 32, 0.1)
    ab(lambda: (G.linear_fwd(s["x"], s["w"], s["b"], resid=s["r"], drop=drop),), ON | BIAS | RES | DROP, tile=12)
    # with a zero residual the zeros of the output are exactly the dropped elements: the mask's rate,
    # and the kept values against fp32 (check_gemm_fwd's limits)
    r0 = torch.zeros_like(s["r"])
    (y,) = ab(lambda: (G.linear_fwd(s["x"], s["w"], s["b"], resid=r0, drop=drop),), ON | BIAS | RES | DROP, tile=12)
    keep = (y != 0).float()
    rate = 1.0 - keep.mean().item()
    assert abs(rate - 0.1) <= _kc().rate_limit(0.1, s["M"] * s["N"]), rate
    ref = (s["x"].float() @ s["w"].float().t() + s["b"]) * keep / 0.9
    _close("lean one-tile resid+bias+dropout vs fp32", [(y, ref)], _kc().lim(3.5e-3, 7e-3))


def test_one_tile_plain(small):
    G, s = _G(), small
    # (the plain dgrads measured no faster on a lean kernel: not on the list, general kernel)
    (y,) = ab(lambda: (G.linear_fwd(s["x"], s["w"], None),), 0, tile=12)
    _close("one-tile plain vs fp32", [(y, s["x"].float() @ s["w"].float().t())], _kc().lim(3.5e-3, 7e-3))


def test_one_tile_negative_zero_products(small):
    """Products that are exactly -0 (zero activations times negative weights, -0 activations times
    positive ones): an accumulator of such products is +0, and the epilogues (the general form adds
    the 0.0f it loads for a missing bias; a lean form without a bias keeps that add) write +0."""
    G, s = _G(), small
    x = s["x"].clone()
    x[::3] = 0.0
    x[1::3] = -0.0
    w = s["w"].clone()
    w[::2] = -w[::2].abs()
    w[1::2] = w[1::2].abs()
    (y,) = ab(lambda: (G.linear_fwd(x, w, None),), 0, tile=12)
    zero_rows = torch.cat([y[::3], y[1::3]])
    assert (_bits(zero_rows) == 0).all(), "a sum of -0 products must be stored as +0"
    # the lean residual + bias + dropout form on the same operands, with a zero bias and a -0 residual:
    # kept and dropped elements of the zero rows are +0 + -0 = +0 in both forms
    b0, rneg = torch.zeros_like(s["b"]), torch.full_like(s["r"], -0.0)
    drop = (_seed(), 4 << 32, 0.1)
    (yd,) = ab(lambda: (G.linear_fwd(x, w, b0, resid=rneg, drop=drop),), ON | BIAS | RES | DROP, tile=12)
    assert (_bits(torch.cat([yd[::3], yd[1::3]])) == 0).all()


def test_fallback_addend_and_odd_n_take_the_general_kernel(small):
    G, s, ext = _G(), small, _ext()
    pos = _kc().rnd(16, s["N"])  # position addend, period 16 rows
    drop = (_seed(), 4 << 32, 0.1)
    # the option set of the lean one-tile kernel (residual + bias + dropout) plus an addend: general
    ab(lambda: (G.linear_fwd(s["x"], s["w"], s["b"], resid=s["r"], drop=drop, addend=pos, addend_period=16),), 0, tile=12)
    (y,) = ab(lambda: (G.linear_fwd(s["x"], s["w"], s["b"], resid=s["r"], addend=pos, addend_period=16),), 0, tile=12)
    ref = s["x"].float() @ s["w"].float().t() + s["b"] + pos.repeat(s["M"] // 16, 1) + s["r"].float()
    _close("general kernel with an addend vs fp32", [(y, ref)], _kc().lim(3.5e-3, 7e-3))
    # N = 772: refused by the binding under both settings, so no kernel (lean or general) runs
    w772, b772, r772 = _kc().bf(_kc().rnd(772, s["K"], scale=0.05)), _kc().rnd(772), _kc().bf(_kc().rnd(s["M"], 772))
    try:
        for on in (True, False):
            ext.set_gemm_lean(on)
            with _kc().tile(12), pytest.raises(RuntimeError, match="multiple of 8"):
                G.linear_fwd(s["x"], w772, b772, resid=r772, drop=drop)
    finally:
        ext.set_gemm_lean(True)


# ----------------------------------------------------------------------------- split tail
def test_split_tail_two_k_parts():
    """Tile count just above the CU count, K = 1536: the leftover tiles run as two K-parts each. Two
    launches in a row show that the arrival counters re-arm."""
    G, KC, ext = _G(), _kc(), _ext()
    cus = int(ext.num_cus())
    M, N, K = 256 * ((cus + 2) // 3 + 1), 768, 1536
    assert ext.gemm_tail_split(M, N, K, 2, 0) == 2
    torch.manual_seed(12)
    x, w, b, r = KC.bf(KC.rnd(M, K)), KC.bf(KC.rnd(N, K, scale=0.05)), KC.rnd(N), KC.bf(KC.rnd(M, N))
    drop = (_seed(), 4 << 32, 0.1)

    def twice(f):
        a = f()
        return a, f()

    y0, y1 = ab(lambda: twice(lambda: G.linear_fwd(x, w, b, resid=r, drop=drop)), ON | BIAS | RES | DROP | TAIL)
    assert _same(y0, y1), "second launch differs: the tail counters did not re-arm"
    p0, p1 = ab(lambda: twice(lambda: G.linear_fwd(x, w, None)), 0)  # plain: the general kernel's split tail
    assert _same(p0, p1)
    _close("split-tail plain vs fp32", [(p0[-512:], x[-512:].float() @ w.float().t())], KC.lim(3.5e-3, 7e-3))


# ----------------------------------------------------------------------------- persistent kernels
@pytest.fixture(scope="module")
def pers():
    KC, ext = _kc(), _ext()
    cus = int(ext.num_cus())
    M, N, K = 256 * (4 * cus // 3 + 1), 768, 256
    torch.manual_seed(13)
    return dict(M=M, N=N, K=K, x=KC.bf(KC.rnd(M, K)), w=KC.bf(KC.rnd(N, K, scale=0.05)), b=KC.rnd(N), g=KC.bf(KC.rnd(M, N)))


def test_persistent_bias(pers):
    G, s = _G(), pers
    assert G._tile(s["M"], s["N"], s["K"], "fwd") == 13
    ab(lambda: (G.linear_fwd(s["x"], s["w"], s["b"]),), ON | BIAS)


def test_persistent_gelu_dropout_aux(pers):
    G, s = _G(), pers

    def run():
        u = torch.empty(s["M"], s["N"], dtype=torch.bfloat16, device=DEV)
        h = G.linear_fwd(s["x"], s["w"], s["b"], gelu_aux=u, drop=(_seed(), 3 << 32, 0.1))
        return h, u

    ab(run, ON | BIAS | DROP | AUX)


def test_persistent_dgelu_colsum(pers):
    """dx is bit-identical. The column sums are one float atomic per row tile and column, added in
    arrival order, so two runs of one kernel already differ in the last bits: here they are held to
    the fp32 bound of re-ordering a sum of n terms, |a - b| <= 2 (n - 1) 2^-24 sum |terms|, with
    sum |terms| <= the column's sum of |dx| (from the bf16 dx, 1 % added for its rounding). The case
    with one row tile below has no such freedom and is compared bit for bit."""
    G, s, ext = _G(), pers, _ext()
    dy, wt = s["x"], s["w"]  # dx = dy [M, K] . w [K, N], through W^T [N, K]
    w = wt.t().contiguous()
    res = {}
    try:
        for on in (True, False):
            ext.set_gemm_lean(on)
            cs = torch.zeros(s["N"], device=DEV)
            res[on] = (G.linear_dgrad(dy, w, dgelu_aux=s["g"], wt=wt, colsum=cs), cs)
            torch.cuda.synchronize()
            assert ext.gemm_lean_last() == ((ON | AUX | COLSUM) if on else 0)
    finally:
        ext.set_gemm_lean(True)
    assert _same(res[True][0], res[False][0])
    n = s["M"] // 256
    bound = 2.0 * (n - 1) * 2.0 ** -24 * 1.01 * res[True][0].float().abs().sum(0)
    diff = (res[True][1] - res[False][1]).abs()
    print(f"dGELU column sums, lean vs general: max |diff| / bound = {(diff / bound).max().item():.3f}")
    assert (diff <= bound).all()


def test_persistent_one_row_tile_column_sums_are_bit_identical():
    """One row tile (M = 256): every column's sum is one atomic add onto zero, so the column sums have
    no reordering freedom and must match bit for bit; also the fp32-reference comparison of the GELU
    and dGELU epilogues (check_gemm_gelu / check_gemm_dgelu limits) on M = 1328 (48 live rows in the
    last row tile)."""
    G, KC = _G(), _kc()
    torch.manual_seed(14)
    N, K = 768, 256
    for M, exact in ((256, True), (1328, False)):
        x, w, b, g = KC.bf(KC.rnd(M, K)), KC.bf(KC.rnd(N, K, scale=0.05)), KC.rnd(N), KC.bf(KC.rnd(M, N))
        wt = w  # [N, K] = W^T of the dgrad's w [K, N]

        def dg():
            cs = torch.zeros(N, device=DEV)
            return G.linear_dgrad(x, wt.t().contiguous(), dgelu_aux=g, wt=wt, colsum=cs), cs

        if exact:
            ab(dg, ON | AUX | COLSUM, tile=13)
            continue
        ext = _ext()
        with KC.tile(13):
            dx, cs = dg()
        assert ext.gemm_lean_last() == (ON | AUX | COLSUM)
        ref = (x.float() @ wt.float().t()) * g.float()
        l2c, mxc = KC.errs(cs, ref.double().sum(0))
        _close("lean persistent dGELU vs fp32", [(dx, ref)], KC.lim(3.5e-3, 7e-3, colsum_l2=1.5e-6, colsum_max=1.5e-6),
               dict(colsum_l2=l2c, colsum_max=mxc))

        def ge():
            u = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
            return G.linear_fwd(x, w, b, gelu_aux=u, drop=(_seed(), 3 << 32, 0.1)), u

        h, u = ab(ge, ON | BIAS | DROP | AUX, tile=13)
        uref = (x.float() @ w.float().t() + b).requires_grad_(True)
        gp = torch.autograd.grad(F.gelu(uref), uref, torch.ones_like(uref))[0]
        keep = ((u != 0) | (h != 0)).float() / 0.9
        rate = 1.0 - (keep != 0).float().mean().item()
        assert abs(rate - 0.1) <= KC.rate_limit(0.1, M * N), rate
        _close("lean persistent GELU+dropout vs fp32", [(u, gp * keep), (h, F.gelu(uref.detach()) * keep)], KC.lim(4e-3, 7e-3))


# ----------------------------------------------------------------------------- weight gradient
def test_weight_gradient_partial_stores():
    G, KC = _G(), _kc()
    torch.manual_seed(15)
    T, N, K = 1024, 768, 768
    assert G.wgrad_splits(T, N, K, 12) == 4
    dy, x = KC.bf(KC.rnd(T, N)), KC.bf(KC.rnd(T, K))

    def run():
        out = torch.zeros(N, K, device=DEV)
        G.linear_wgrad(dy, x, out)
        return (out,)

    # (measured no faster on a lean kernel: not on the list, the general kernel under both settings)
    (out,) = ab(run, 0, tile=12)
    _close("weight gradient vs fp32", [(out, dy.float().t() @ x.float())], KC.lim(1e-6, 4e-6))  # check_gemm_wgrad
