"""FusedLamb on the GPU: the three kernels of csrc/lamb.hip on raw buffers against the float64 step of
tests/lamb_reference.py, then through a real ParamStore (segment-table and tile forms, bucket layout),
and the plumbing FusedLamb inherits from FusedAdam (clip, non-finite skip, model EMA, hipGraph, engine).

The yardstick is the project's rule for the Adam kernels: the fp32 torch-ops step (FusedLamb off the
fused path) from the same inputs is measured against the same float64 values, and the kernels' error may
be 4x its error on rel-L2 and on max, per segment. Two fp32 evaluations of one element differ by luck, and
with gradients over eight decades one element carries the norm of a small segment: so a figure that is
within what the fp32 operations of the formula may cost (lamb_rounding_floors, derived from operation
counts and the inputs) passes as well, whatever the yardstick's luck: limit = max(4 x yardstick, floor)."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import lamb_reference as L  # noqa: E402
from tests import optim_reference as R  # noqa: E402
from tests.kernel_checks import ADAM_STEPS, SENTINEL, _adam_bufs, errs64  # noqa: E402
from tests.test_gpu_model_ema import BUCKET_LAYOUT, CFG, DEV, _check_update, _encoder_weights, _masks  # noqa: E402
from tests.test_gpu_optim import _check_shadow, _fused, _model, _trainable, _twin, _write_grads  # noqa: E402

FORMS = pytest.mark.parametrize("transposed", [False, True], ids=["segments", "tiles"])
FORMS_LAYOUTS = pytest.mark.parametrize(
    "transposed,layout", [(False, None), (True, None), (True, BUCKET_LAYOUT), (False, BUCKET_LAYOUT)],
    ids=["segments", "tiles", "tiles-buckets", "segments-buckets"])

CHUNK = 4096  # csrc/kernels.h LAMB_CHUNK (asserted against the extension below)
# (lr, betas, eps, weight decay, always_adapt): adapting with decay, plain Adam steps, adapting without decay;
# lr 10x apart, the betas of tests/optim_reference.py
SPECS = ((1e-2, (0.9, 0.999), 1e-6, 0.03, False), (1e-3, (0.8, 0.95), 1e-6, 0.0, False), (1e-4, (0.0, 0.5), 1e-5, 0.0, True))
LONG = 257 * CHUNK + 8  # 258 chunks: the ratio kernel's threads 0 and 1 take a second trip (1,052,680 elements)
# (elements, spec or -1 frozen / None gap, kind)
SEGMENTS = ((4, 0, ""), (64, None, ""), (128, 1, ""), (CHUNK, 0, ""), (64, None, ""), (CHUNK + 4, 2, ""), (LONG, 0, ""),
            (2048, 1, ""), (256, -1, ""), (1024, 0, "zero_p"), (64, None, ""), (512, 2, "zero_g"), (64, None, ""))

# Every bound below is tests/lamb_reference.py lamb_rounding_floors': what fp32 arithmetic alone may cost a step,
# worked out from the formula's operation counts, the chunked summation and the step's inputs.


def _table(step):
    rows = [R.group_row(lr, betas, eps, wd, step, False) for lr, betas, eps, wd, _ in SPECS]
    tab = R.table_f32(rows)
    tab.view(np.int32)[:, 7] = [2 if s[4] else 0 for s in SPECS]  # LAMB_ALWAYS_ADAPT
    return tab


def _torch_lamb_step32(p, g_scaled, m, v, spec, step):
    """The yardstick: one fp32 torch-ops FusedLamb step of one tensor from the given state."""
    from pytorch_vit_paper_replication_amd.optim import FusedLamb

    lr, betas, eps, wd, always = spec
    tp = torch.nn.Parameter(p.clone())
    tp.grad = g_scaled.clone()
    opt = FusedLamb([tp], lr=lr, betas=betas, eps=eps, weight_decay=wd, always_adapt=always)
    opt.state[tp] = {"step": torch.tensor(float(step - 1)), "exp_avg": m.clone(), "exp_avg_sq": v.clone()}
    opt.step()
    assert opt._fused is None
    return tp.detach(), opt.state[tp]["exp_avg"], opt.state[tp]["exp_avg_sq"]


def _raw_layout():
    starts, groups, chunks, seg_chunks, off = [], [], [], [], 0
    for i, (n, spec, _) in enumerate(SEGMENTS):
        starts.append(off)
        gi = -1 if spec is None else spec
        groups.append(gi)
        first = len(chunks)
        if gi >= 0:
            chunks.extend([off + c, min(CHUNK, n - c), i] for c in range(0, n, CHUNK))
        seg_chunks.append([first, len(chunks) - first])
        off += n
    return off, starts, groups, chunks, seg_chunks


@pytest.mark.parametrize("table,coef", [("host", None), ("dev", 0.37)], ids=["host_table-no_clip", "device_table-clip"])
def test_kernels_on_raw_buffers(table, coef):
    from pytorch_vit_paper_replication_amd import _ext

    ext = _ext.ext()
    assert ext.lamb_chunk() == CHUNK
    torch.manual_seed(11)
    n, starts, groups, chunks, seg_chunks = _raw_layout()
    assert seg_chunks[6][1] == 258 and n % 4 == 0
    elem_group = R.expand_segments(starts, groups, n).to(DEV)
    upd = elem_group >= 0
    bufs = _adam_bufs(n, upd, shadow=True)
    p, g, m, v, shadow = (bufs[k] for k in ("p", "g", "m", "v", "shadow"))
    seg_start = torch.tensor(starts, dtype=torch.int64, device=DEV)
    seg_group = torch.tensor(groups, dtype=torch.int32, device=DEV)
    chunks_t = torch.tensor(chunks, dtype=torch.int64, device=DEV)
    seg_chunks_t = torch.tensor(seg_chunks, dtype=torch.int64, device=DEV)
    partial = torch.full((len(chunks), 2), float("nan"), device=DEV)  # stale contents: every row is overwritten
    trust = torch.full((len(starts), 3), SENTINEL, device=DEV)
    clip_t = torch.tensor([123.0, coef, 0.0], device=DEV) if coef is not None else None
    gscale = float(clip_t[1]) if coef is not None else 1.0  # the fp32 coefficient the kernels read

    def launch(tab, clip=clip_t, skip=True):
        t = torch.from_numpy(tab)
        t = t if table == "host" else t.to(DEV)
        ext.lamb_moments(p, g, m, v, chunks_t, seg_group, partial, t, clip, skip)
        ext.lamb_ratio(partial, seg_chunks_t, seg_group, trust, t, clip, skip)
        ext.lamb_update(p, m, v, shadow, trust, t, clip, skip, seg_start=seg_start, seg_group=seg_group)
        torch.cuda.synchronize()

    spans = [(a, a + s[0]) for a, s in zip(starts, SEGMENTS)]
    worst = {}
    for step in ADAM_STEPS:
        tab = _table(step)
        g.copy_(torch.where(upd, R.adam_grad(n, None, DEV), torch.full_like(g, SENTINEL)))
        for (a, b), (_, _, kind) in zip(spans, SEGMENTS):
            if kind == "zero_p":
                p[a:b] = 0.0
            if kind == "zero_g":
                g[a:b] = 0.0
                assert bool((m[a:b] == 0).all()) and bool((v[a:b] == 0).all())
        before = {k: t.clone() for k, t in bufs.items()}
        trust0 = trust.clone()
        launch(tab)
        assert not bool(torch.isnan(partial).any()), "a chunk's partial sums were not written"
        tr = trust.cpu().double()
        pooled = {}
        for i, ((a, b), (cnt, spec, kind)) in enumerate(zip(spans, SEGMENTS)):
            if spec is None or spec < 0:
                assert torch.equal(trust[i], trust0[i]), f"trust row {i} of a frozen segment written"
                continue
            adapt = SPECS[spec][3] != 0 or SPECS[spec][4]
            p0, g0, m0, v0 = (before[k][a:b] for k in ("p", "g", "m", "v"))
            pr, mr, vr, wn, un, r = L.lamb_step64(p0, g0, m0, v0, tab[spec], adapt, gscale)
            floors, bounds = L.lamb_rounding_floors(p0, g0, m0, v0, tab[spec], adapt, gscale)
            py, my, vy = _torch_lamb_step32(p0, g0 * gscale, m0, v0, SPECS[spec], step)
            base = p0.double()
            for key, k_t, r_t, y_t in zip(("dp", "m", "v"), (p[a:b].double() - base, m[a:b], v[a:b]), (pr - base, mr, vr),
                                          (py.double() - base, my, vy)):
                ek, ey = errs64(k_t, r_t), errs64(y_t, r_t)
                fl = L.floor_metrics(floors[key], r_t)
                print(f"step {step} segment {i} ({cnt} elements, spec {spec} {kind}) {key}: kernel l2 {ek[0]:.2e} max {ek[1]:.2e}; "
                      f"fp32 torch l2 {ey[0]:.2e} max {ey[1]:.2e}; fp32 floor l2 {fl[0]:.2e} max {fl[1]:.2e} (limit: 4x torch or the floor)")
                assert ek[0] <= max(4.0 * ey[0], fl[0]) and ek[1] <= max(4.0 * ey[1], fl[1]), \
                    f"step {step} segment {i} {key}: {ek} vs 4 x {ey} and the floor {fl}"
                pooled.setdefault((spec, key), []).append((k_t.double().reshape(-1), r_t.reshape(-1), y_t.double().reshape(-1)))
            got = tr[i].tolist()
            rel = [abs(x - y) / y if y != 0.0 else abs(x) for x, y in zip(got, (wn, un, r))]
            print(f"step {step} segment {i} trust {got} float64 {(wn, un, r)} rel {rel[0]:.2e} {rel[1]:.2e} {rel[2]:.2e} "
                  f"(bounds {bounds[0]:.2e} {bounds[1]:.2e} {bounds[2]:.2e})")
            for k in range(3):
                worst[k] = max(worst.get(k, 0.0), rel[k])
            assert all(x <= y for x, y in zip(rel, bounds)), f"step {step} segment {i}: trust {got} vs {(wn, un, r)}"
            assert (r != 1.0) == (adapt and not kind)
            if kind == "zero_p":
                assert got[0] == 0.0 and got[1] > 0.0 and got[2] == 1.0
            if kind == "zero_g":
                assert got[0] > 0.0 and got[1] == 0.0 and got[2] == 1.0
                assert torch.equal(p[a:b], before["p"][a:b]), "a zero update moved p"
        # and the 4x rule alone as tests/kernel_checks.py _adam_driver applies it, per step and per param group
        # over that group's segments together
        for (spec, key), parts in sorted(pooled.items()):
            k_t, r_t, y_t = (torch.cat([x[j] for x in parts]) for j in range(3))
            ek, ey = errs64(k_t, r_t), errs64(y_t, r_t)
            print(f"step {step} group {spec} {key}: kernel l2 {ek[0]:.2e} max {ek[1]:.2e}; fp32 torch l2 {ey[0]:.2e} max {ey[1]:.2e} (limit 4x)")
            assert ek[0] <= 4.0 * ey[0] and ek[1] <= 4.0 * ey[1], f"step {step} group {spec} {key}: {ek} vs 4 x {ey}"
        for k, t in bufs.items():  # frozen segments and gaps: bit-unchanged (g everywhere)
            keep = torch.ones_like(upd) if k == "g" else ~upd
            assert torch.equal(t[keep], before[k][keep]), f"step {step}: {k} changed outside the trainable segments"
        assert torch.equal(R.bf16_bits(shadow)[upd], R.bf16_rne_bits(p)[upd])
    print(f"worst trust errors: ||w|| {worst[0]:.2e} ||u|| {worst[1]:.2e} r {worst[2]:.2e}")

    # a flagged non-finite step: skipped (every buffer bit-unchanged), or taken with skip_nonfinite off
    bad = torch.tensor([float("inf"), 0.5, 1.0], device=DEV)
    g.copy_(torch.where(upd, R.adam_grad(n, None, DEV), torch.full_like(g, SENTINEL)))
    before = {k: t.clone() for k, t in bufs.items()}
    trust0 = trust.clone()
    launch(_table(3), clip=bad, skip=True)
    for k, t in bufs.items():
        assert torch.equal(t, before[k]), f"a skipped step wrote {k}"
    assert torch.equal(trust, trust0)
    launch(_table(3), clip=bad, skip=False)
    a, b = spans[6]
    for k in ("p", "m", "v", "shadow"):
        assert not torch.equal(bufs[k][a:b], before[k][a:b]), f"an unskipped step left {k}"
    assert not torch.equal(trust, trust0)


def _lamb(m, **kw):
    from pytorch_vit_paper_replication_amd.optim import FusedLamb, param_groups_weight_decay

    return FusedLamb(param_groups_weight_decay(m, 0.03), lr=1e-2, **kw)


@FORMS_LAYOUTS
def test_three_steps_through_a_param_store(transposed, layout):
    """Fused steps against the torch-ops FusedLamb on a twin that is loaded with the fused parameters and
    moments before every step; one weight (a tile segment) and one LayerNorm bias are frozen."""
    m, st = _model(transposed, layout, freeze=True)
    twin = _twin(m, freeze=True)
    opt, topt = _lamb(m), _lamb(twin)
    fp, tp = _trainable(m), _trainable(twin)
    train, frozen, pad = _masks(st)
    assert int(frozen.sum()) == 256 * 128 + 128 and int(pad.sum()) > 0
    flat0, shadow0 = st.flat.clone(), st.shadow.clone()
    wt0 = st.shadow_t.clone() if transposed else None
    seg_of = {id(p): i for i, p in enumerate(st.params)}
    for it in range(3):
        with torch.no_grad():
            for a, b in zip(m.parameters(), twin.parameters()):
                b.copy_(a)
        if it > 0:
            for a, b in zip(fp, tp):
                topt.state[b] = {"step": torch.tensor(float(it)), "exp_avg": opt.state[a]["exp_avg"].clone(),
                                 "exp_avg_sq": opt.state[a]["exp_avg_sq"].clone()}
        _write_grads((m, twin), it)
        before = {id(b): (b.detach().clone(), b.grad.clone(),
                          topt.state[b]["exp_avg"].clone() if it > 0 else torch.zeros_like(b),
                          topt.state[b]["exp_avg_sq"].clone() if it > 0 else torch.zeros_like(b)) for b in tp}
        opt.step()
        topt.step()
        torch.cuda.synchronize()
        assert opt._fused is not None and topt._fused is None
        assert (opt._tmeta_key is not None) == transposed, "the other form ran"
        trust = opt.last_trust.cpu().double()
        assert tuple(trust.shape) == (len(st.params), 3)
        got, yard, ref = [[], [], []], [[], [], []], [[], [], []]
        index = {id(b): a for a, b in zip(fp, tp)}
        for tg in topt.param_groups:
            row = R.group_row(tg["lr"], tg["betas"], tg["eps"], tg["weight_decay"], it + 1, False)  # the user's doubles
            for b in tg["params"]:
                a = index[id(b)]
                p0, g0, m0, v0 = before[id(b)]
                r = L.lamb_step64(p0, g0, m0, v0, row, tg["weight_decay"] != 0)
                for k, (x, y, z) in enumerate(((a.detach(), b.detach(), r[0]), (opt.state[a]["exp_avg"], topt.state[b]["exp_avg"], r[1]),
                                               (opt.state[a]["exp_avg_sq"], topt.state[b]["exp_avg_sq"], r[2]))):
                    base = p0.double() if k == 0 else 0.0
                    got[k].append((x.double() - base).reshape(-1))
                    yard[k].append((y.double() - base).reshape(-1))
                    ref[k].append((z - base).reshape(-1))
                row_t = trust[seg_of[id(a)]].tolist()
                bounds = L.lamb_rounding_floors(p0, g0, m0, v0, row, tg["weight_decay"] != 0)[1]
                for x, y, bound in zip(row_t, r[3:], bounds):
                    assert abs(x - y) <= bound * y, f"step {it + 1} trust {row_t} vs {r[3:]}"
                assert (r[5] != 1.0) == (tg["weight_decay"] != 0)
        for k, name in enumerate(("p_after - p_before", "m", "v")):
            rr = torch.cat(ref[k])
            ek, ey = errs64(torch.cat(got[k]), rr), errs64(torch.cat(yard[k]), rr)
            print(f"step {it + 1} {name}: fused l2 {ek[0]:.2e} max {ek[1]:.2e}; fp32 torch l2 {ey[0]:.2e} max {ey[1]:.2e} (limit 4x)")
            assert ek[0] <= 4.0 * ey[0] and ek[1] <= 4.0 * ey[1], f"step {it + 1} {name}: {ek} vs 4 x {ey}"
    flat, mm, vv, shadow = _fused(st, opt)
    for name, t in (("flat", flat), ("m", mm), ("v", vv), ("shadow", shadow.float())):
        assert bool((t[pad] == 0).all()), f"{name}: padding moved"
    assert torch.equal(flat[frozen], flat0[frozen]) and torch.equal(shadow[frozen], shadow0[frozen])
    assert bool((mm[frozen] == 0).all()) and bool((vv[frozen] == 0).all())
    assert not torch.equal(flat[train], flat0[train])
    for p in st.params:
        if not p.requires_grad:
            assert bool((opt.last_trust[seg_of[id(p)]] == 0).all()), "trust row of a frozen segment written"
    _check_shadow(st, train)
    if transposed:
        w = m.transformer_encoder[1].mlp_block.mlp[0].weight  # the frozen one
        off = st._t_views[id(w)].storage_offset()
        assert torch.equal(st.shadow_t[off:off + w.numel()], wt0[off:off + w.numel()])
        for x in _encoder_weights(m):
            assert torch.equal(st.bf16_t(x), st.bf16(x).t())
        assert not torch.equal(st.shadow_t, wt0)


def _pair(transposed, **kw):
    out = []
    for _ in range(2):
        m, st = _model(transposed)
        out.append((m, st, _lamb(m, **kw)))
    assert torch.equal(out[0][1].flat, out[1][1].flat)
    return out


def _assert_same(a, b, transposed):
    for x, y in zip(_fused(a[1], a[2]), _fused(b[1], b[2])):
        assert torch.equal(x, y)
    if transposed:
        assert torch.equal(a[1].shadow_t, b[1].shadow_t)
    assert torch.equal(a[2].last_trust, b[2].last_trust)


@FORMS
def test_steps_are_bitwise_repeatable(transposed):
    a, b = _pair(transposed)
    for it in range(3):
        _write_grads((a[0], b[0]), it)
        a[2].step(clip_norm=1.0)
        b[2].step(clip_norm=1.0)
        torch.cuda.synchronize()
        _assert_same(a, b, transposed)
    assert not torch.equal(a[1].flat, _model(transposed)[1].flat)
    assert bool((a[2].last_trust[:, 2] > 0).all()) and bool((a[2].last_trust[:, 2] != 1).any())


@FORMS
def test_clip_grad_norm_then_bare_step_equals_step_with_clip_norm(transposed):
    a, b = _pair(transposed)
    for it in range(3):
        _write_grads((a[0], b[0]), it)
        na = a[2].clip_grad_norm_(1.0)
        assert a[2]._pending_clip
        a[2].step()
        assert not a[2]._pending_clip
        b[2].step(clip_norm=1.0)
        torch.cuda.synchronize()
        assert float(na) > 1.0, "the clip must bite"
        assert torch.equal(a[2].last_grad_norm, b[2].last_grad_norm) and torch.equal(a[2]._fused[6], b[2]._fused[6])
        _assert_same(a, b, transposed)


def _randn_step(m, opt, it, **kw):
    g = torch.Generator(device=DEV).manual_seed(1000 + it)
    for p in m.parameters():
        if p.requires_grad:
            p.grad.copy_(torch.randn(p.shape, device=DEV, generator=g) * (it + 1))
    opt.step(clip_norm=1.0, **kw)


@FORMS
def test_nonfinite_gradient(transposed):
    from pytorch_vit_paper_replication_amd.optim import ModelEma

    for skip in (True, False):
        m, st = _model(transposed)
        opt = _lamb(m, skip_nonfinite=skip)
        ema = ModelEma(m, decay=0.9).attach(opt)
        _randn_step(m, opt, 0)
        torch.cuda.synchronize()

        def state():
            ts = [st.flat, opt._fused[1], opt._fused[2], st.shadow, opt.last_trust, ema.fused_buffer()]
            return ts + ([st.shadow_t] if transposed else [])

        before = [t.clone() for t in state()]
        g = torch.Generator(device=DEV).manual_seed(7)
        for p in m.parameters():
            p.grad.copy_(torch.randn(p.shape, device=DEV, generator=g))
        m.classifier[0].weight.grad[0, 0] = float("inf")
        opt.step(clip_norm=1.0)
        torch.cuda.synchronize()
        assert not torch.isfinite(opt.last_grad_norm).item()
        same = [torch.equal(a, b) for a, b in zip(before, state())]
        if skip:
            assert all(same), same
        else:
            assert not any(same), same


@FORMS
def test_model_ema_in_the_update_pass(transposed):
    from pytorch_vit_paper_replication_amd.optim import ModelEma

    m1, s1 = _model(transposed, freeze=True)
    m2, s2 = _model(transposed, freeze=True)
    o1, o2 = _lamb(m1), _lamb(m2)
    ema = ModelEma(m1, decay=0.99).attach(o1)
    buf = ema.fused_buffer()
    init = buf.clone()
    train, frozen, pad = _masks(s1)
    for it in range(3):
        old = buf.clone()
        pair = ema.pair_at(ema.num_updates)
        _randn_step(m1, o1, it)
        _randn_step(m2, o2, it)
        torch.cuda.synchronize()
        assert ema.fused_buffer() is buf
        _check_update(buf, old, s1.flat, pair, train, f"step {it}")
        assert torch.equal(buf[frozen], init[frozen]) and bool((buf[pad] == 0).all())
    assert ema.num_updates == 3 and (o1._tmeta_key is not None) == transposed
    assert torch.equal(s1.flat, s2.flat) and torch.equal(s1.shadow, s2.shadow)
    assert torch.equal(o1._fused[1], o2._fused[1]) and torch.equal(o1._fused[2], o2._fused[2])
    assert torch.equal(o1.last_trust, o2.last_trust)
    if transposed:
        assert not s1._t_dirty and torch.equal(s1.shadow_t, s2.shadow_t)


def test_captured_step_replays_under_an_lr_schedule():
    """graph_mode(): lr, the bias corrections and the EMA's warm-up pair come from the device table that
    graph_prepare() uploads, not from arguments frozen at capture: three replays equal three eager steps."""
    from pytorch_vit_paper_replication_amd.optim import ModelEma, warmup_linear_decay

    (ma, sa, oa), (mb, sb, ob) = _pair(True)
    scha, schb = warmup_linear_decay(oa, 20, 0.1), warmup_linear_decay(ob, 20, 0.1)
    ea = ModelEma(ma, decay=0.9999, warmup=True).attach(oa)
    eb = ModelEma(mb, decay=0.9999, warmup=True).attach(ob)
    _write_grads((ma, mb), 0)
    for o, s in ((oa, scha), (ob, schb)):  # one eager step each: tables, W^T and the EMA buffer exist before the capture
        o.step(clip_norm=1.0)
        s.step()
    torch.cuda.synchronize()
    oa.graph_mode(True)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        oa.step(clip_norm=1.0)
    torch.cuda.synchronize()
    assert oa.step_count == 1
    lrs = []
    for it in range(1, 4):
        _write_grads((ma, mb), it)
        lrs.append(oa.param_groups[0]["lr"])
        assert ob.param_groups[0]["lr"] == lrs[-1]
        oa.graph_prepare()
        graph.replay()
        scha.step()
        ob.step(clip_norm=1.0)
        schb.step()
        torch.cuda.synchronize()
        _assert_same((ma, sa, oa), (mb, sb, ob), True)
        assert torch.equal(ea.fused_buffer(), eb.fused_buffer())
    assert len(set(lrs)) == 3 and oa.step_count == ob.step_count == 4 and ea.num_updates == eb.num_updates == 4
    assert not torch.equal(ea.fused_buffer(), sa.flat)


def test_graphed_train_step_with_lamb():
    """GraphedTrainStep (forward, loss, backward, clip, LAMB, lr schedule, EMA warm-up in one hipGraph): every
    replay's parameters, moments and trust rows against the float64 step from the state before it, the
    gradients it left in the store and the clip coefficient it computed, within the fp32 floors; the EMA
    against its formula as test_warmup_decays_eager_and_graph_replay checks it."""
    from pytorch_vit_paper_replication_amd.ops.fused_vit import cross_entropy
    from pytorch_vit_paper_replication_amd.optim import ModelEma, warmup_linear_decay
    from pytorch_vit_paper_replication_amd.runtime.graph import GraphedTrainStep

    m, st = _model(False)  # the model's first forward registers the W^T shadow itself
    opt = _lamb(m)
    sched = warmup_linear_decay(opt, 20, 0.1)
    ema = ModelEma(m, decay=0.9999, warmup=True).attach(opt)
    x = torch.rand(4, 3, 32, 32, device=DEV)
    y = torch.randint(0, 10, (4,), device=DEV)
    g = GraphedTrainStep(m, opt, cross_entropy, x, y, clip_norm=1.0, warmup=3, scheduler=sched)
    assert ema.num_updates == 3 and opt._tmeta_key is not None and opt.step_count == 3
    buf = ema.fused_buffer()
    train, _, _ = _masks(st)
    seg_of = {id(p): i for i, p in enumerate(st.params)}
    lrs = []
    for it in range(3):
        torch.cuda.synchronize()
        old = buf.clone()
        pair = ema.pair_at(ema.num_updates)
        before = {id(p): (p.detach().clone(), opt.state[p]["exp_avg"].clone(), opt.state[p]["exp_avg_sq"].clone()) for p in _trainable(m)}
        rows = [R.group_row(tg["lr"], tg["betas"], tg["eps"], tg["weight_decay"], 4 + it, False) for tg in opt.param_groups]
        lrs.append(opt.param_groups[0]["lr"])
        g()
        torch.cuda.synchronize()
        assert opt.step_count == 4 + it and ema.num_updates == 4 + it and ema.fused_buffer() is buf
        _check_update(buf, old, st.flat, pair, train, f"replay {it}")
        clip = opt._fused[6].cpu()
        assert float(clip[2]) == 0.0 and 0.0 < float(clip[1]) <= 1.0
        trust = opt.last_trust.cpu().double()
        for tg, row in zip(opt.param_groups, rows):
            adapt = tg["weight_decay"] != 0
            for p in tg["params"]:
                p0, m0, v0 = before[id(p)]
                ref = L.lamb_step64(p0, p.grad, m0, v0, row, adapt, float(clip[1]))
                floors, bounds = L.lamb_rounding_floors(p0, p.grad, m0, v0, row, adapt, float(clip[1]))
                for key, got, want in (("dp", p.detach().double() - p0.double(), ref[0] - p0.double()),
                                       ("m", opt.state[p]["exp_avg"], ref[1]), ("v", opt.state[p]["exp_avg_sq"], ref[2])):
                    ek, fl = errs64(got, want), L.floor_metrics(floors[key], want)
                    assert ek[0] <= fl[0] and ek[1] <= fl[1], f"replay {it} {key} {tuple(p.shape)}: {ek} over the fp32 floor {fl}"
                for a, b, bound in zip(trust[seg_of[id(p)]].tolist(), ref[3:], bounds):
                    assert abs(a - b) <= bound * b, f"replay {it} trust {tuple(p.shape)}: {a} vs {b} (bound {bound})"
    assert len(set(lrs)) == 3 and opt.step_count == 6


def test_engine_train_takes_the_fused_path():
    from pytorch_vit_paper_replication_amd import engine
    from pytorch_vit_paper_replication_amd.data import create_synthetic_dataloaders
    from pytorch_vit_paper_replication_amd.models import ViT
    from pytorch_vit_paper_replication_amd.optim import warmup_linear_decay

    tr, te, _ = create_synthetic_dataloaders(batch_size=4, train_len=12, test_len=8, image_size=32, num_classes=10)
    torch.manual_seed(0)
    m = ViT(**CFG).to(DEV)
    opt = _lamb(m)
    sched = warmup_linear_decay(opt, 3, 0.1)
    before = [p.detach().clone() for p in m.parameters()]
    res = engine.train(m, tr, te, opt, torch.nn.CrossEntropyLoss(), sched, epochs=1, device=DEV)
    assert list(res) == ["train_loss", "train_acc", "test_loss", "test_acc"] and all(len(v) == 1 for v in res.values())
    assert all(math.isfinite(v[0]) for v in res.values())
    assert opt._fused is not None and opt.step_count == 3
    st = opt._fused[0]
    trust = opt.last_trust
    assert trust.is_cuda and tuple(trust.shape) == (len(st.params), 3)
    assert bool(torch.isfinite(trust).all()) and bool((trust[:, 2] > 0).all()) and bool((trust[:, 2] != 1).any())
    assert any(not torch.equal(a, b) for a, b in zip(before, m.parameters()))


def test_host_validation_of_the_launch_arguments():
    """What the kernels assume of every tensor whose pointer they follow is checked before any launch."""
    from pytorch_vit_paper_replication_amd import _ext

    ext = _ext.ext()
    n = 64
    p, g, m, v = (torch.zeros(n, device=DEV) for _ in range(4))
    shadow = torch.zeros(n, dtype=torch.bfloat16, device=DEV)
    chunks = torch.tensor([[0, 64, 0]], dtype=torch.int64, device=DEV)
    seg_chunks = torch.tensor([[0, 1]], dtype=torch.int64, device=DEV)
    seg_start = torch.zeros(1, dtype=torch.int64, device=DEV)
    seg_group = torch.zeros(1, dtype=torch.int32, device=DEV)
    partial = torch.zeros(1, 2, device=DEV)
    trust = torch.zeros(1, 3, device=DEV)
    tab = torch.from_numpy(_table(1))
    ext.lamb_moments(p, g, m, v, chunks, seg_group, partial, tab, None, True)  # the well-formed calls pass
    ext.lamb_ratio(partial, seg_chunks, seg_group, trust, tab, None, True)
    ext.lamb_update(p, m, v, shadow, trust, tab, None, True, seg_start=seg_start, seg_group=seg_group)
    torch.cuda.synchronize()
    big = torch.zeros(n + 4, device=DEV)
    bad_calls = [
        ("size mismatch", lambda: ext.lamb_moments(p, big[:60], m, v, chunks, seg_group, partial, tab, None, True)),
        ("16-byte aligned", lambda: ext.lamb_moments(big[1:n + 1], g, m, v, chunks, seg_group, partial, tab, None, True)),
        ("chunks", lambda: ext.lamb_moments(p, g, m, v, chunks.int(), seg_group, partial, tab, None, True)),
        ("chunks", lambda: ext.lamb_moments(p, g, m, v, chunks.cpu(), seg_group, partial, tab, None, True)),
        ("one row per chunk", lambda: ext.lamb_moments(p, g, m, v, chunks, seg_group, torch.zeros(2, 2, device=DEV), tab, None, True)),
        ("groups", lambda: ext.lamb_moments(p, g, m, v, chunks, seg_group, partial, tab[:, :8].contiguous(), None, True)),
        ("1..8 groups", lambda: ext.lamb_moments(p, g, m, v, chunks, seg_group, partial, tab.repeat(3, 1), None, True)),
        ("clip", lambda: ext.lamb_moments(p, g, m, v, chunks, seg_group, partial, tab, torch.zeros(2, device=DEV), True)),
        ("same number", lambda: ext.lamb_ratio(partial, seg_chunks, seg_group, torch.zeros(2, 3, device=DEV), tab, None, True)),
        ("seg_chunks", lambda: ext.lamb_ratio(partial, seg_chunks.view(-1), seg_group, trust, tab, None, True)),
        ("trust", lambda: ext.lamb_update(p, m, v, shadow, trust.view(-1), tab, None, True, seg_start=seg_start, seg_group=seg_group)),
        ("shadow", lambda: ext.lamb_update(p, m, v, shadow.float(), trust, tab, None, True, seg_start=seg_start, seg_group=seg_group)),
        ("needs seg_start", lambda: ext.lamb_update(p, m, v, shadow, trust, tab, None, True)),
        ("same number", lambda: ext.lamb_update(p, m, v, shadow, trust, tab, None, True, seg_start=torch.zeros(2, dtype=torch.int64, device=DEV),
                                                seg_group=torch.zeros(2, dtype=torch.int32, device=DEV))),
        ("tile form needs", lambda: ext.lamb_update(p, m, v, shadow, trust, tab, None, True,
                                                    tmeta=torch.zeros(1, 7, dtype=torch.int64, device=DEV), ntiles=1)),
        ("ema_pair", lambda: ext.lamb_update(p, m, v, shadow, trust, tab, None, True, seg_start=seg_start, seg_group=seg_group,
                                             ema=torch.zeros(n, device=DEV))),
    ]
    for text, call in bad_calls:
        with pytest.raises(RuntimeError, match=text):
            call()
    torch.cuda.synchronize()
    assert bool((p == 0).all()) and bool((trust[:, :2] == 0).all())
