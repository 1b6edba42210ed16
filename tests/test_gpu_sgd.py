"""FusedSGD on the GPU: csrc/sgd.hip on raw buffers (segment-table and tile form, host and device group table,
with and without a clip coefficient and a model EMA), through a real ParamStore against float64
``torch.optim.SGD``, under hipGraph, in ``engine.train``, its host-side argument checks, and a model whose
resolution was changed with ``ViT.set_image_size`` on the fused path.

The numerics rule is the project's (tests/kernel_checks.py): every launch starts from the kernel's own fp32
state and is compared with the float64 step (tests/sgd_reference.py) from that state. The yardstick is the fp32
torch-ops step, ``FusedSGD`` off the fused path on the same inputs; per segment (parameter) the kernel's rel-L2
and max error may be ``max(4 x yardstick, floor)``, the floor being the fp32 rounding cost of the formula's
operation count (``sgd_rounding_floors``). Both figures are printed for the worst segment of each run."""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from tests import optim_reference as R  # noqa: E402
from tests import sgd_reference as S  # noqa: E402
from tests.test_gpu_model_ema import BUCKET_LAYOUT, CFG, DEV, NODROP, _check_update, _encoder_weights, _masks  # noqa: E402

if torch.cuda.is_available():
    from tests import kernel_checks as KC
    from tests.test_gpu_optim import _check_shadow, _model, _trainable, _write_grads

NESTEROV_BIT = 4  # csrc/kernels.h SGD_NESTEROV
# (lr, momentum, weight decay, nesterov): lr 10x apart, so an element updated with another group's row is a gross
# error; momentum with decay, no momentum (its buffer must stay as it is), Nesterov without decay
SPECS = ((1e-2, 0.9, 0.03, False), (1e-3, 0.0, 0.1, False), (1e-4, 0.8, 0.0, True))
NO_MOMENTUM = 1
COEF = 0.37


def _ext():
    from pytorch_vit_paper_replication_amd import _ext as E

    return E.ext()


def _f32(x) -> float:
    return float(np.float32(x))


def _spec_at(spec, step):
    """The spec's hyper-parameters at ``step`` as the fp32 values the table carries (lr follows a schedule)."""
    lr, mom, wd, nest = SPECS[spec]
    return _f32(lr / math.sqrt(step)), _f32(mom), _f32(wd), nest


def _table(step, G=3):
    """float32 [G, 10] group table (csrc/kernels.h AdamGroup as csrc/sgd.hip reads it); rows no segment names hold
    lr 1e3."""
    arr = np.zeros((G, 10), dtype=np.float32)
    arr[:, 0], arr[:, 1], arr[:, 4] = 1e3, 0.5, 0.5
    for k in range(len(SPECS)):
        lr, mom, wd, nest = _spec_at(k, step)
        row = KC._adam_rows(G)[k]
        arr[row, :] = 0.0
        arr[row, 0], arr[row, 1], arr[row, 4] = lr, mom, wd
        arr.view(np.int32)[row, 7] = NESTEROV_BIT if nest else 0
    return arr


class Layout:
    """One flat buffer: ``segments`` [(start, elements, spec)] of the trainable and frozen (-1) pieces, everything
    else a gap; optionally the tile tables over the same pieces."""

    def __init__(self, n, segments, trows=None, frows=None, nt=0):
        self.n, self.segments, self.trows, self.frows, self.nt = n, segments, trows, frows, nt
        self.elem_spec = torch.full((n,), -1, dtype=torch.int64)
        for start, e, spec in segments:
            self.elem_spec[start:start + e] = spec
        self.elem_spec = self.elem_spec.to(DEV)
        self.upd = self.elem_spec >= 0

    def seg_table(self, G):
        """(seg_start, seg_group) lists covering [0, n): the pieces, and -1 for every gap between them."""
        starts, groups, pos = [], [], 0
        for start, e, spec in sorted(self.segments):
            if start > pos:
                starts.append(pos)
                groups.append(-1)
            starts.append(start)
            groups.append(-1 if spec < 0 else KC._adam_rows(G)[spec])
            pos = start + e
        if pos < self.n:
            starts.append(pos)
            groups.append(-1)
        return starts, groups

    def tables(self, form, G):
        ext = _ext()
        rowof = lambda s: -1 if s < 0 else KC._adam_rows(G)[s]  # noqa: E731
        if form == "seg":
            starts, groups = self.seg_table(G)
            return ext.sgd_segments(torch.tensor(starts, dtype=torch.int64), torch.tensor(groups, dtype=torch.int32), self.n,
                                    torch.device(DEV, 0))
        tmeta = torch.tensor([r[:5] + [rowof(r[5])] for r in self.trows], dtype=torch.int64)
        fmeta = torch.tensor([[r[0], r[1], rowof(r[2]), r[3]] for r in self.frows], dtype=torch.int64)
        return ext.sgd_tiles(tmeta, fmeta, self.n, self.nt, torch.device(DEV, 0))


def seg_layout():
    """The layout of check_adam_kernel for this kernel's grid cap: a 4-element segment, a large one, a frozen one in
    the middle, a boundary 512 elements into the second grid-stride trip, a frozen segment at the end; the total
    is one trip of ``sgd_blocks() x 256`` float4 and 3 x 256 + 5 more."""
    blocks = _ext().sgd_blocks()
    trip = 4 * blocks * 256
    n = trip + 4 * (3 * 256 + 5)
    starts, specs = [0, 4, 5_000_000, 5_000_400, trip + 512, n - 200], [0, 1, -1, 2, 0, -1]
    assert starts == sorted(starts) and starts[3] < trip < starts[4] < starts[5] < n
    if blocks == 8192:
        assert n == KC.ADAM_N and (n, starts, specs) == KC.adam_kernel_layout()
    return Layout(n, [(a, b - a, s) for a, b, s in zip(starts, starts[1:] + [n], specs)])


def tile_layout():
    """The matrices and flat ranges of check_adam_t_kernel: 64x128, 64x64 (frozen), 192x64 (R != C); flat ranges of
    262,144 + 300 float4 in all, the flat blocks' second trip."""
    n, nt, trows, frows, ntiles, flat4 = KC.adam_t_layout()
    assert flat4 > 1024 * 256
    segs = [(r[0], r[2] * r[3], r[5]) for r in trows] + [(r[0], r[1], r[2]) for r in frows]
    lay = Layout(n, segs, trows, frows, nt)
    lay.ntiles, lay.flat4 = ntiles, flat4
    return lay


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _buffers(lay, ema, gen):
    n, upd = lay.n, lay.upd
    sent = torch.full((n,), KC.SENTINEL, device=DEV)
    bufs = {"p": torch.where(upd, R.adam_inputs(n, gen, DEV), sent), "g": sent.clone(),
            "buf": torch.where(upd, torch.zeros_like(sent), sent), "shadow": sent.to(torch.bfloat16)}
    # the group without momentum has no buffer: whatever lies there, a NaN included, is neither read nor written
    nomom = lay.elem_spec == NO_MOMENTUM
    bufs["buf"][nomom] = 3.0
    idx = nomom.nonzero().squeeze(1)
    bufs["buf"][idx[::7]] = float("nan")
    noise = torch.randn(n, device=DEV, generator=gen)  # drawn with or without an EMA: the gradients that follow are the same
    if ema:
        bufs["ema"] = torch.where(upd, bufs["p"] + 0.01 * noise, sent)
    if lay.trows is not None:
        bufs["shadow_t"] = torch.full((lay.nt,), KC.SENTINEL, dtype=torch.bfloat16, device=DEV)
    return bufs


def _yardstick(p0, g0s, b0, hyper):
    """The fp32 torch-ops step: FusedSGD off the fused path (these tensors are in no ParamStore)."""
    from pytorch_vit_paper_replication_amd.optim import FusedSGD

    lr, mom, wd, nest = hyper
    tp = torch.nn.Parameter(p0.clone())
    tp.grad = g0s.clone()
    opt = FusedSGD([tp], lr=lr, momentum=mom, weight_decay=wd, nesterov=nest)
    if mom != 0:
        opt.state[tp] = {"momentum_buffer": b0.clone()}
    opt.step()
    assert opt._fused is None
    return tp.detach(), (opt.state[tp]["momentum_buffer"] if mom != 0 else None)


class Worst:
    """Per metric, the segment and step where kernel error / limit is largest (a NaN counts as largest)."""

    def __init__(self):
        self.best = {}

    def add(self, key, kernel, yard, floor, where):
        limit = max(4.0 * yard, floor)
        ratio = 0.0 if kernel == 0.0 else (math.inf if limit == 0.0 else kernel / limit)
        old = self.best.get(key)
        if old is None or (old[0] == old[0] and not ratio <= old[0]):
            self.best[key] = (ratio, kernel, yard, floor, where)

    def report(self, name):
        txt = " ".join(f"{k}: kernel {b[1]:.2e} / fp32 torch {b[2]:.2e} / floor {b[3]:.2e} [{b[4]}]" for k, b in sorted(self.best.items()))
        print(f"{name}: {txt}")
        bad = {k: b for k, b in self.best.items() if not b[0] <= 1.0}
        assert not bad, f"{name}: over max(4 x yardstick, floor): {bad}"


def run_kernel(lay, form, table="host", clip=False, ema_pair=None, check=True, steps=None, seed=11):
    """``len(steps)`` launches on fresh gradients from one seeded input set; returns the buffers. ``check``: every
    launch against the float64 step per segment, and the exact properties."""
    ext = _ext()
    steps = KC.ADAM_STEPS if steps is None else steps
    G = 3 if table == "host" else 12
    gen = torch.Generator(device=DEV).manual_seed(seed)
    bufs = _buffers(lay, ema_pair is not None, gen)
    tabs = lay.tables(form, G)
    clip_t = torch.tensor([123.0, COEF, 0.0], device=DEV) if clip else None
    gscale = _f32(COEF) if clip else 1.0
    ema_kw = {}
    if ema_pair is not None:
        ema_kw = dict(ema=bufs["ema"], ema_pair=torch.from_numpy(np.array(ema_pair, dtype=np.float32)))
    upd, n = lay.upd, lay.n
    name = f"sgd {form} form n{n} {table} table G{G}" + (f" clip coef {COEF}" if clip else " no clip") + (" +ema" if ema_kw else "")
    worst = Worst()

    def launch(tab, clip_arg=clip_t, skip=True):
        t = torch.from_numpy(tab)
        t = t if table == "host" else t.to(DEV)
        if form == "seg":
            ext.sgd(bufs["p"], bufs["g"], bufs["buf"], bufs["shadow"], tabs, t, clip_arg, skip, **ema_kw)
        else:
            ext.sgd_t(bufs["p"], bufs["g"], bufs["buf"], bufs["shadow"], bufs["shadow_t"], tabs, t, clip_arg, skip, **ema_kw)
        torch.cuda.synchronize()

    def check_transposed(before_t, written_specs=True):
        if form != "tile":
            return
        written = torch.zeros(lay.nt, dtype=torch.bool, device=DEV)
        for soff, doff, R_, C_, _, spec in lay.trows:
            if spec < 0 or not written_specs:
                continue
            written[doff:doff + R_ * C_] = True
            w = bufs["shadow"][soff:soff + R_ * C_].view(R_, C_)
            assert torch.equal(bufs["shadow_t"][doff:doff + R_ * C_].view(C_, R_), w.t()), f"{name}: W^T of the {R_}x{C_} matrix"
        assert _same_bits(bufs["shadow_t"][~written], before_t[~written]), f"{name}: shadow_t written outside the trained matrices"

    for step in steps:
        bufs["g"].copy_(torch.where(upd, R.adam_grad(n, gen, DEV), torch.full_like(bufs["g"], KC.SENTINEL)))
        before = {k: t.clone() for k, t in bufs.items()}
        launch(_table(step, G))
        if not check:
            continue
        for start, e, spec in lay.segments:
            if spec < 0:
                continue
            sl = slice(start, start + e)
            hyper = _spec_at(spec, step)
            p0, g0, b0 = before["p"][sl], before["g"][sl], before["buf"][sl]
            b0z = torch.zeros_like(b0) if hyper[1] == 0 else b0
            pr, br = S.sgd_step64(p0, g0, b0z, *hyper, gscale)
            fl = S.sgd_rounding_floors(p0, g0, b0z, *hyper, gscale)
            py, by = _yardstick(p0, g0 * gscale, b0z, hyper)
            base = p0.double().cpu().numpy()
            pairs = [("dp", bufs["p"][sl].double().cpu().numpy() - base, py.double().cpu().numpy() - base, pr - base, fl["dp"])]
            if hyper[1] != 0:
                pairs.append(("buf", bufs["buf"][sl], by, br, fl["buf"]))
            for key, kv, yv, ref, floor in pairs:
                for suffix, a, b, c in zip(("l2", "max"), S.errs64(kv, ref), S.errs64(yv, ref), S.floor_metrics(floor, ref)):
                    worst.add(f"{key}_{suffix}", a, b, c, f"step {step} segment {start}+{e} spec {spec}")
        # exact: frozen segments and gaps of every buffer, g everywhere, the buffer of the group without momentum
        for k in ("p", "buf", "shadow", "g") + (("ema",) if ema_kw else ()):
            keep = torch.ones_like(upd) if k == "g" else ~upd
            assert _same_bits(bufs[k][keep], before[k][keep]), f"{name} step {step}: {k} changed where nothing may"
        nomom = lay.elem_spec == NO_MOMENTUM
        assert _same_bits(bufs["buf"][nomom], before["buf"][nomom]), f"{name} step {step}: the buffer of the momentum-0 group was written"
        assert bool(torch.isnan(bufs["buf"][nomom]).any()) and bool(torch.isfinite(bufs["p"][upd]).all())
        assert torch.equal(R.bf16_bits(bufs["shadow"])[upd], R.bf16_rne_bits(bufs["p"])[upd]), f"{name} step {step}: shadow is not RNE(p)"
        assert torch.equal(bufs["shadow"][upd], bufs["p"][upd].to(torch.bfloat16))
        check_transposed(before["shadow_t"] if form == "tile" else None)
        if ema_kw:
            _check_update(bufs["ema"], before["ema"], bufs["p"], ema_pair, upd, f"{name} step {step}")
    final = {k: t.clone() for k, t in bufs.items()}  # what the steps left (the flag runs below go on from it)
    if check:
        worst.report(name)
        # a flagged non-finite step: skipped (every buffer bit-identical) or, with skip_nonfinite off, taken
        bad = torch.tensor([float("inf"), 0.5, 1.0], device=DEV)
        bufs["g"].copy_(torch.where(upd, R.adam_grad(n, gen, DEV), torch.full_like(bufs["g"], KC.SENTINEL)))
        before = {k: t.clone() for k, t in bufs.items()}
        launch(_table(3, G), bad, True)
        for k in bufs:
            assert _same_bits(bufs[k], before[k]), f"{name}: a skipped non-finite step wrote {k}"
        launch(_table(3, G), bad, False)
        mom = upd & (lay.elem_spec != NO_MOMENTUM)
        assert not torch.equal(bufs["p"][upd], before["p"][upd]) and not torch.equal(bufs["buf"][mom], before["buf"][mom])
        assert _same_bits(bufs["p"][~upd], before["p"][~upd])
        check_transposed(before["shadow_t"] if form == "tile" else None)
    return final


# ----------------------------------------------------------------------------- raw buffers
@pytest.fixture(scope="module")
def seg_lay():
    return seg_layout()


@pytest.fixture(scope="module")
def tile_lay():
    return tile_layout()


@pytest.mark.parametrize("clip", [False, True], ids=["no_clip", "clip"])
@pytest.mark.parametrize("table", ["host", "dev"])
def test_segment_form_against_float64(seg_lay, table, clip):
    run_kernel(seg_lay, "seg", table, clip)


@pytest.mark.parametrize("clip", [False, True], ids=["no_clip", "clip"])
@pytest.mark.parametrize("table", ["host", "dev"])
def test_tile_form_against_float64_and_its_transposed_shadow(tile_lay, table, clip):
    run_kernel(tile_lay, "tile", table, clip)


@pytest.mark.parametrize("clip", [False, True], ids=["no_clip", "clip"])
def test_tile_form_and_segment_form_give_the_same_bits(tile_lay, clip):
    a = run_kernel(tile_lay, "tile", "host", clip, check=False)
    b = run_kernel(tile_lay, "seg", "dev", clip, check=False)
    for k in ("p", "buf", "shadow", "g"):
        assert _same_bits(a[k], b[k]), k
    assert not torch.equal(a["p"][tile_lay.upd], _buffers(tile_lay, False, torch.Generator(device=DEV).manual_seed(11))["p"][tile_lay.upd])


@pytest.mark.parametrize("form", ["seg", "tile"])
def test_ema_instantiation(tile_lay, form):
    """The EMA instantiation writes the bits of the default one and the EMA follows decay * ema + (1 - decay) * p_new;
    decay 0 gives p_new and decay 1 leaves the EMA, exactly."""
    pair = (np.float32(0.99), np.float32(1.0 - 0.99))
    plain = run_kernel(tile_lay, form, "host", True, check=False)
    with_ema = run_kernel(tile_lay, form, "host", True, ema_pair=pair, check=True)
    for k in ("p", "buf", "shadow") + (("shadow_t",) if form == "tile" else ()):
        assert _same_bits(plain[k], with_ema[k]), k
    upd = tile_lay.upd
    zero = run_kernel(tile_lay, form, "dev", False, ema_pair=(np.float32(0.0), np.float32(1.0)), check=False, steps=(1,))
    assert torch.equal(zero["ema"][upd], zero["p"][upd]) and bool((zero["ema"][~upd] == KC.SENTINEL).all())
    start = _buffers(tile_lay, True, torch.Generator(device=DEV).manual_seed(11))["ema"]
    one = run_kernel(tile_lay, form, "dev", False, ema_pair=(np.float32(1.0), np.float32(0.0)), check=False, steps=(1,))
    assert torch.equal(one["ema"], start) and not torch.equal(one["p"][upd], start[upd])


# ----------------------------------------------------------------------------- argument validation
def _valid_args(n=64):
    full = lambda k=n, dt=torch.float32: torch.full((k,), KC.SENTINEL, dtype=dt, device=DEV)  # noqa: E731
    return dict(p=full(), g=full(), buf=full(), shadow=full(n, torch.bfloat16), groups=torch.from_numpy(_table(1, 3)),
                clip=torch.tensor([1.0, 0.5, 0.0], device=DEV))


def test_arguments_are_checked_on_the_host_before_any_launch():
    """Wrong dtypes, a misaligned segment, short tables and tables that do not fit the buffers raise on the host:
    the segment and tile tables when they are built (``sgd_segments`` / ``sgd_tiles`` take them as CPU tensors and
    hand back the only thing ``sgd`` / ``sgd_t`` accept), the buffers at the call. Nothing is launched."""
    ext = _ext()
    dev = torch.device(DEV, 0)
    i64 = lambda v: torch.tensor(v, dtype=torch.int64)  # noqa: E731
    i32 = lambda v: torch.tensor(v, dtype=torch.int32)  # noqa: E731
    n = 64
    bad_tables = [
        ("not a multiple of 4", lambda: ext.sgd_segments(i64([0, 6]), i32([0, 1]), n, dev)),  # a misaligned segment
        ("begin at 0 and rise", lambda: ext.sgd_segments(i64([4, 8]), i32([0, 1]), n, dev)),
        ("begin at 0 and rise", lambda: ext.sgd_segments(i64([0, 8, 8]), i32([0, 1, 0]), n, dev)),
        ("of 64", lambda: ext.sgd_segments(i64([0, 64]), i32([0, 1]), n, dev)),  # a segment past the end
        ("same number", lambda: ext.sgd_segments(i64([0, 8]), i32([0]), n, dev)),  # a short table
        ("seg_start must be a contiguous int64 CPU", lambda: ext.sgd_segments(i32([0, 8]), i32([0, 1]), n, dev)),
        ("seg_start must be a contiguous int64 CPU", lambda: ext.sgd_segments(i64([0, 8]).to(DEV), i32([0, 1]), n, dev)),
        ("seg_group must be a contiguous int32 CPU", lambda: ext.sgd_segments(i64([0, 8]), i64([0, 1]), n, dev)),
        ("names group", lambda: ext.sgd_segments(i64([0, 8]), i32([0, -2]), n, dev)),
        ("multiple of 4 elements", lambda: ext.sgd_segments(i64([0]), i32([0]), 62, dev)),
        ("tmeta must be", lambda: ext.sgd_tiles(i64([[0, 0, 64, 64, 0]]), i64([[4096, 4, 1, 0]]), 4100, 4096, dev)),  # 5 columns
        ("not multiples of 64", lambda: ext.sgd_tiles(i64([[0, 0, 64, 96, 0, 0]]), i64([[6144, 4, 1, 0]]), 6148, 6144, dev)),
        ("inside the 4096 elements", lambda: ext.sgd_tiles(i64([[4, 0, 64, 64, 0, 0]]), i64([[0, 4, 1, 0]]), 4096, 4096, dev)),
        ("multiple of 4 and lie inside", lambda: ext.sgd_tiles(i64([[2, 0, 64, 64, 0, 0]]), i64([[4100, 4, 1, 0]]), 4104, 4096, dev)),
        ("elements of shadow_t", lambda: ext.sgd_tiles(i64([[0, 8, 64, 64, 0, 0]]), i64([[4096, 4, 1, 0]]), 4100, 4096, dev)),
        ("multiple of 8", lambda: ext.sgd_tiles(i64([[0, 4, 64, 64, 0, 0]]), i64([[4096, 4, 1, 0]]), 4100, 8192, dev)),
        ("first tile", lambda: ext.sgd_tiles(i64([[0, 0, 64, 64, 1, 0]]), i64([[4096, 4, 1, 0]]), 4100, 4096, dev)),
        ("range 0", lambda: ext.sgd_tiles(i64([[0, 0, 64, 64, 0, 0]]), i64([[4096, 8, 1, 0]]), 4100, 4096, dev)),  # past the end
        ("range 0", lambda: ext.sgd_tiles(i64([[0, 0, 64, 64, 0, 0]]), i64([[4098, 4, 1, 0]]), 4104, 4096, dev)),  # misaligned
        ("first float4", lambda: ext.sgd_tiles(i64([[0, 0, 64, 64, 0, 0]]), i64([[4096, 4, 1, 1]]), 4100, 4096, dev)),
    ]
    for text, call in bad_tables:
        with pytest.raises(RuntimeError, match=text):
            call()
    tabs = ext.sgd_segments(i64([0, 8]), i32([0, 2]), n, dev)
    assert not tabs.tiles and tabs.numel == n
    a = _valid_args(n)
    outs = [a[k] for k in ("p", "g", "buf", "shadow")]

    def call(**kw):
        b = dict(a, **kw)
        return ext.sgd(b["p"], b["g"], b["buf"], b["shadow"], b.get("tables", tabs), b["groups"], b["clip"], True, **b.get("ema", {}))

    mis = torch.full((n + 4,), KC.SENTINEL, device=DEV)[1:n + 1]
    bad_calls = [
        ("p must be a contiguous float32", dict(p=a["p"].double())),  # a wrong dtype
        ("buf must be a contiguous float32", dict(buf=a["buf"].half())),
        ("g must be a contiguous float32", dict(g=torch.full((2 * n,), KC.SENTINEL, device=DEV)[::2])),
        ("buf must be 16-byte aligned", dict(buf=mis)),
        ("size mismatch", dict(g=torch.full((n + 4,), KC.SENTINEL, device=DEV))),
        ("built for buffers of 64", dict(p=a["p"][:32], g=a["g"][:32], buf=a["buf"][:32], shadow=a["shadow"][:32])),
        ("shadow must be a contiguous bfloat16", dict(shadow=a["shadow"].float())),
        ("shadow must hold", dict(shadow=a["shadow"][:32])),
        ("group table holds 2", dict(groups=a["groups"][:2].contiguous())),  # a short group table
        ("groups must be contiguous float32", dict(groups=a["groups"][:, :8].contiguous())),
        ("1..8 groups", dict(groups=torch.from_numpy(_table(1, 9)))),
        ("clip must be", dict(clip=a["clip"][:2])),
        ("ema needs ema_pair", dict(ema=dict(ema=torch.zeros(n, device=DEV)))),
        ("go to sgd_t", dict(tables=ext.sgd_tiles(i64([[0, 0, 64, 64, 0, 0]]), i64([[4096, 4, 1, 0]]), 4100, 4096, dev))),
    ]
    for text, kw in bad_calls:
        with pytest.raises(RuntimeError, match=text):
            call(**kw)
    with pytest.raises(RuntimeError, match="go to sgd"):
        ext.sgd_t(a["p"], a["g"], a["buf"], a["shadow"], a["shadow"], tabs, a["groups"], a["clip"], True)
    t = ext.sgd_tiles(i64([[0, 0, 64, 64, 0, 0]]), i64([[4096, 4, 1, 0]]), 4100, 4096, dev)
    assert t.tiles and t.ntiles == 1 and t.flat4 == 1
    b = _valid_args(4100)
    st = torch.full((4096,), KC.SENTINEL, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(RuntimeError, match="shadow_t of 4096"):
        ext.sgd_t(b["p"], b["g"], b["buf"], b["shadow"], st[:2048], t, b["groups"], b["clip"], True)
    with pytest.raises(RuntimeError, match="shadow_t must be 16-byte aligned"):
        ext.sgd_t(b["p"], b["g"], b["buf"], b["shadow"], torch.full((4100,), KC.SENTINEL, dtype=torch.bfloat16, device=DEV)[4:], t,
                  b["groups"], b["clip"], True)
    torch.cuda.synchronize()
    assert all(bool((x.float() == KC.SENTINEL).all()) for x in outs + [b[k] for k in ("p", "g", "buf", "shadow")] + [st]), \
        "a rejected call must not launch"
    # the valid calls launch
    a["g"].fill_(1.0)
    call()
    b["g"].fill_(1.0)
    ext.sgd_t(b["p"], b["g"], b["buf"], b["shadow"], st, t, b["groups"], b["clip"], True)
    torch.cuda.synchronize()
    assert not bool((a["p"] == KC.SENTINEL).any()) and not bool((b["p"] == KC.SENTINEL).any())
    assert torch.equal(st.view(64, 64), b["shadow"][:4096].view(64, 64).t())


# ----------------------------------------------------------------------------- through a real ParamStore
LAYOUTS = pytest.mark.parametrize("transposed,layout", [(False, None), (True, None), (True, BUCKET_LAYOUT), (False, BUCKET_LAYOUT)],
                                  ids=["sgd_kernel", "sgd_t_kernel", "sgd_t_kernel-buckets", "sgd_kernel-buckets"])


def _sgd_groups(m):
    """Momentum with decay on the matrices, Nesterov without decay on everything else."""
    from pytorch_vit_paper_replication_amd.optim import param_groups_weight_decay

    decay, rest = param_groups_weight_decay(m, 0.03)
    return [dict(decay, momentum=0.9), dict(rest, momentum=0.8, nesterov=True, lr=3e-3)]


@LAYOUTS
def test_store_steps_against_float64_torch_sgd(transposed, layout):
    """3 clipped steps under a cosine schedule through a real ParamStore, both kernels, with and without padding
    between segments, against ``torch.optim.SGD`` on a float64 twin fed the clip coefficient the step computed on
    the device (itself held to the float64 norm); afterwards the shadows are fresh."""
    from pytorch_vit_paper_replication_amd.models import ViT
    from pytorch_vit_paper_replication_amd.optim import FusedSGD, warmup_cosine_decay

    m, st = _model(transposed, layout, freeze=True)
    twin64 = ViT(**NODROP).to(DEV).double()
    twin32 = ViT(**NODROP).to(DEV)
    for t in (twin64, twin32):
        t.transformer_encoder[1].mlp_block.mlp[0].weight.requires_grad_(False)
        t.transformer_encoder[0].msa_block.layer_norm.bias.requires_grad_(False)
    opt = FusedSGD(_sgd_groups(m), lr=1e-2)
    o64 = torch.optim.SGD(_sgd_groups(twin64), lr=1e-2, foreach=False)
    o32 = FusedSGD(_sgd_groups(twin32), lr=1e-2)  # the yardstick: torch ops in fp32
    scheds = [warmup_cosine_decay(o, 10, 0.2) for o in (opt, o64, o32)]
    fp, p64, p32 = _trainable(m), _trainable(twin64), _trainable(twin32)
    train, frozen, pad = _masks(st)
    frozen_bits = st.flat[frozen].clone()
    lrs, worst = [], Worst()
    for it in range(3):
        with torch.no_grad():
            for a, b, c in zip(m.parameters(), twin64.parameters(), twin32.parameters()):
                b.copy_(a.double())
                c.copy_(a)
        if it > 0:
            for a, b, c in zip(fp, p64, p32):
                o64.state[b] = {"momentum_buffer": opt.state[a]["momentum_buffer"].double()}
                o32.state[c] = {"momentum_buffer": opt.state[a]["momentum_buffer"].clone()}
        _write_grads((m, twin32), it)
        before = [(a.detach().clone(), opt.state[a]["momentum_buffer"].clone() if it > 0 else torch.zeros_like(a)) for a in fp]
        assert [g["lr"] for g in opt.param_groups] == [g["lr"] for g in o64.param_groups] == [g["lr"] for g in o32.param_groups]
        lrs.append(opt.param_groups[0]["lr"])
        opt.step(clip_norm=1.0)
        torch.cuda.synchronize()
        assert (opt._tmeta_key is not None) == transposed, "the other kernel ran"
        norm, coef, flag = (float(x) for x in opt._fused[6].cpu())
        want = R.norm64(torch.cat([a.grad.reshape(-1) for a in fp]))
        assert flag == 0.0 and abs(norm - want) <= 1e-6 * want and abs(coef - min(1.0, 1.0 / (want + 1e-6))) <= 2e-6 and coef < 1.0
        for a, b, c in zip(fp, p64, p32):
            b.grad = a.grad.double() * coef
            c.grad.mul_(coef)
        o64.step()
        o32.step()
        assert o32._fused is None
        for tg in o64.param_groups:
            hyper = (tg["lr"], tg["momentum"], tg["weight_decay"], tg["nesterov"])
            for b in tg["params"]:
                k = next(i for i, x in enumerate(p64) if x is b)
                a, c = fp[k], p32[k]
                p0, b0 = before[k]
                fl = S.sgd_rounding_floors(p0, a.grad, b0, *hyper, coef)
                base = p0.double()
                for key, kv, yv, ref, floor in (
                        ("dp", a.detach().double() - base, c.detach().double() - base, b.detach() - base, fl["dp"]),
                        ("buf", opt.state[a]["momentum_buffer"], o32.state[c]["momentum_buffer"], o64.state[b]["momentum_buffer"], fl["buf"])):
                    for suffix, x, y, z in zip(("l2", "max"), S.errs64(kv, ref), S.errs64(yv, ref), S.floor_metrics(floor, ref)):
                        # the table's fp32 lr / momentum / decay against the user's doubles: one more rounding each
                        worst.add(f"{key}_{suffix}", x, y, z + 3 * S.EPS32, f"step {it + 1} {tuple(a.shape)}")
        # the shadows are fresh: refreshing launches nothing and the version key is unchanged
        key, gen = st._shadow_key, st.generation
        assert key == st._version_key()
        _check_shadow(st, train)
        st.shadow[pad] = 5.0  # (padding: nothing reads it; a refresh would rewrite it to the master's zeros)
        st.refresh_shadow()
        torch.cuda.synchronize()
        assert st._shadow_key == key == st._version_key() and st.generation == gen and bool((st.shadow[pad] == 5.0).all())
        st.shadow[pad] = 0.0
        if transposed:
            assert not st._t_dirty and all(torch.equal(st.bf16_t(w), st.bf16(w).t()) for w in _encoder_weights(m))
        for s in scheds:
            s.step()
    worst.report(f"FusedSGD through the store ({'sgd_t_kernel' if transposed else 'sgd_kernel'}, layout {layout})")
    assert len(set(lrs)) == 3
    assert _same_bits(st.flat[frozen], frozen_bits) and bool((st.flat[pad] == 0).all()) and bool((opt._fused[1][pad] == 0).all())
    assert set(opt.state) == set(fp) and all(opt.state[a]["momentum_buffer"].data_ptr() != 0 for a in fp)


def test_state_dict_round_trip_on_the_fused_path():
    """The flat buffer is the state: a state dict from torch.optim.SGD is carried into it, and comes back out."""
    from pytorch_vit_paper_replication_amd.optim import FusedSGD

    m, st = _model(True)
    opt = FusedSGD([{"params": [p for p in m.parameters() if p.ndim > 1], "momentum": 0.9},
                    {"params": [p for p in m.parameters() if p.ndim <= 1], "momentum": 0.0}], lr=1e-2)
    _write_grads((m,), 0)
    opt.step()
    _write_grads((m,), 1)
    opt.step()
    sd = opt.state_dict()
    with_mom = [p for p in m.parameters() if p.ndim > 1]
    assert len(sd["state"]) == len(with_mom) and set(opt.state) == set(with_mom)
    import copy

    m2, st2 = _model(True)
    with torch.no_grad():
        st2.flat.copy_(st.flat)
    st2.refresh_shadow(force=True)
    opt2 = FusedSGD([{"params": [p for p in m2.parameters() if p.ndim > 1], "momentum": 0.9},
                     {"params": [p for p in m2.parameters() if p.ndim <= 1], "momentum": 0.0}], lr=1e-2)
    opt2.load_state_dict(copy.deepcopy(sd))
    _write_grads((m, m2), 2)
    opt.step()
    opt2.step()
    torch.cuda.synchronize()
    assert opt2._fused is not None and torch.equal(st.flat, st2.flat) and torch.equal(opt._fused[1], opt2._fused[1])
    assert torch.equal(st.shadow, st2.shadow)


# ----------------------------------------------------------------------------- hipGraph and training
TRAIN_CFG = dict(image_size=64, patch_size=16, num_transformer_layer=2, num_heads=2, embedding_dim=128, mlp_size=256, num_classes=10,
                 mlp_dropout=0.0, embedding_dropout=0.0)


def _train_pair():
    from pytorch_vit_paper_replication_amd.models import ViT
    from pytorch_vit_paper_replication_amd.optim import FusedSGD, param_groups_weight_decay, warmup_cosine_decay

    torch.manual_seed(0)
    ma, mb = ViT(**TRAIN_CFG).to(DEV), ViT(**TRAIN_CFG).to(DEV)
    mb.load_state_dict(ma.state_dict())
    oa, ob = (FusedSGD(param_groups_weight_decay(m, 1e-4), lr=0.03, momentum=0.9, nesterov=True) for m in (ma, mb))
    return ma, mb, oa, ob, warmup_cosine_decay(oa, 20, 0.1), warmup_cosine_decay(ob, 20, 0.1)


def test_graph_replay_leaves_the_eager_steps_bits():
    from pytorch_vit_paper_replication_amd import _ext as E
    from pytorch_vit_paper_replication_amd.ops.fused_vit import cross_entropy
    from pytorch_vit_paper_replication_amd.optim import ModelEma
    from pytorch_vit_paper_replication_amd.runtime.graph import GraphedTrainStep

    with E.deterministic_mode():
        ma, mb, oa, ob, sa, sb = _train_pair()
        ea, eb = ModelEma(ma, decay=0.99).attach(oa), ModelEma(mb, decay=0.99).attach(ob)
        x = torch.rand(8, 3, 64, 64, device=DEV)
        y = torch.randint(0, 10, (8,), device=DEV)
        for _ in range(3 + 2):
            ma.train()
            loss = cross_entropy(ma(x), y)
            oa.zero_grad()
            loss.backward()
            oa.step(clip_norm=1.0)
            sa.step()
        g = GraphedTrainStep(mb, ob, cross_entropy, x, y, clip_norm=1.0, warmup=3, scheduler=sb)
        for _ in range(2):
            g()
        torch.cuda.synchronize()
    assert oa.step_count == ob.step_count == 5 and ob._tmeta_key is not None
    sta, stb = oa._fused[0], ob._fused[0]
    assert torch.equal(sta.flat, stb.flat) and torch.equal(oa._fused[1], ob._fused[1])
    assert torch.equal(sta.shadow, stb.shadow) and torch.equal(sta.shadow_t, stb.shadow_t)
    assert torch.equal(ea.fused_buffer(), eb.fused_buffer()) and not torch.equal(ea.fused_buffer(), sta.flat)
    for p1, p2 in zip(ma.parameters(), mb.parameters()):
        assert torch.equal(p1, p2)


def test_engine_train_runs_an_epoch_and_the_loss_falls():
    from pytorch_vit_paper_replication_amd import engine
    from pytorch_vit_paper_replication_amd.data import create_synthetic_dataloaders
    from pytorch_vit_paper_replication_amd.models import ViT
    from pytorch_vit_paper_replication_amd.ops.fused_vit import cross_entropy
    from pytorch_vit_paper_replication_amd.optim import FusedSGD, param_groups_weight_decay, warmup_cosine_decay

    tr, te, _ = create_synthetic_dataloaders(batch_size=4, train_len=12, test_len=8, image_size=32, num_classes=10)
    torch.manual_seed(0)
    m = ViT(**CFG).to(DEV)
    opt = FusedSGD(param_groups_weight_decay(m, 0.0), lr=0.01, momentum=0.9)
    before = [p.detach().clone() for p in m.parameters()]
    res = engine.train(m, tr, te, opt, torch.nn.CrossEntropyLoss(), warmup_cosine_decay(opt, 3, 0.0), epochs=1, device=DEV)
    assert list(res) == ["train_loss", "train_acc", "test_loss", "test_acc"] and all(math.isfinite(v[0]) for v in res.values())
    assert opt._fused is not None and opt.step_count == 3 and opt._tmeta_key is not None
    assert any(not torch.equal(a, b) for a, b in zip(before, m.parameters()))
    assert all(bool(opt.state[p]["momentum_buffer"].abs().sum() > 0) for p in m.parameters())
    # a fixed batch is learnable: 20 clipped steps at a constant lr
    torch.manual_seed(1)
    m = ViT(**NODROP).to(DEV)
    opt = FusedSGD(param_groups_weight_decay(m, 0.0), lr=0.02, momentum=0.9)
    x = torch.rand(8, 3, 32, 32, device=DEV)
    y = torch.randint(0, 10, (8,), device=DEV)
    losses = []
    for _ in range(20):
        loss = cross_entropy(m(x), y)
        opt.zero_grad()
        loss.backward()
        opt.step(clip_norm=1.0)
        losses.append(loss.item())
    print(f"FusedSGD(momentum=0.9) on a fixed batch: loss {losses[0]:.4f} -> {losses[-1]:.4f}")
    assert all(math.isfinite(v) for v in losses) and losses[-1] < losses[0]


# ----------------------------------------------------------------------------- a resized model on the fused path
def test_a_resized_model_trains_on_the_fused_path():
    """image 32 -> 48 (5 -> 10 tokens) with ``set_image_size``, then one training step: the fused path against the
    ``PVR_DISABLE_FUSED=1`` path of the same weights. Tolerances are those of tests/test_gpu_train.py at this model
    size (D 128, 2 heads): the loss to ``3e-2 * max(1, |reference|)`` (test_fused_training_tracks_fp32_reference),
    applied to the logits against their largest reference magnitude too, and every gradient to rel-L2 5e-2
    (test_odd_patch_size_fused_matches_reference)."""
    from pytorch_vit_paper_replication_amd import _ext as E
    from pytorch_vit_paper_replication_amd.models import ViT
    from pytorch_vit_paper_replication_amd.ops.fused_vit import cross_entropy
    from pytorch_vit_paper_replication_amd.optim import FusedSGD, param_groups_weight_decay

    torch.manual_seed(0)
    mf, mr = ViT(**NODROP), ViT(**NODROP)
    mr.load_state_dict(mf.state_dict())
    for m in (mf, mr):
        m.set_image_size(48).to(DEV)
    assert mf.patch_embedding_block.position_embedding.shape == (1, 10, 128)
    assert torch.equal(mf.patch_embedding_block.position_embedding, mr.patch_embedding_block.position_embedding)
    opt = FusedSGD(param_groups_weight_decay(mf, 0.0), lr=0.01, momentum=0.9)
    x = torch.rand(16, 3, 48, 48, device=DEV)
    y = torch.randint(0, 10, (16,), device=DEV)
    assert E.use_fused(x) and mf._fused_supported(x)
    logits = mf(x)
    lf = cross_entropy(logits, y)
    opt.zero_grad()
    lf.backward()
    grads = {n: p.grad.detach().clone() for n, p in mf.named_parameters()}
    p0 = mf.patch_embedding_block.position_embedding.detach().clone()
    opt.step(clip_norm=1.0)
    torch.cuda.synchronize()
    st = getattr(mf, "_pvr_store", None)
    assert st is not None and opt._fused is not None and opt._fused[0] is st, "the fused path did not run"
    assert not torch.equal(mf.patch_embedding_block.position_embedding, p0), "the resized position grid did not train"
    with pytest.raises(RuntimeError, match="ParamStore"):
        mf.set_image_size(64)
    os.environ["PVR_DISABLE_FUSED"] = "1"
    try:
        ref_logits = mr(x).float()
        lr_ = F.cross_entropy(ref_logits, y)
        lr_.backward()
    finally:
        os.environ["PVR_DISABLE_FUSED"] = "0"
    assert getattr(mr, "_pvr_store", None) is None
    dl = float((logits.detach().float() - ref_logits.detach()).abs().max())
    scale = max(1.0, float(ref_logits.abs().max()))
    print(f"resized 32 -> 48: loss {lf.item():.5f} vs {lr_.item():.5f}; max logit difference {dl:.3e} (limit {3e-2 * scale:.3e})")
    assert abs(lf.item() - lr_.item()) < 3e-2 * max(1.0, abs(lr_.item()))
    assert dl < 3e-2 * scale
    for n, pr in mr.named_parameters():
        g, gr = grads[n].float(), pr.grad.float()
        rel = float((g - gr).norm() / gr.norm().clamp_min(1e-12))
        assert rel < 5e-2, f"{n}: rel-L2 {rel:.3e}"
