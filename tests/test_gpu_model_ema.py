"""ModelEma on the fused path: the EMA instantiation of adam_kernel / adam_t_kernel, the store swap,
hipGraph stepping, checkpoints and the engine. Every test uses the smallest model that reaches every
branch (5 tokens; 384x128, 256x128 and 128x256 tile weights; a 10x128 head and a 10-element bias that
the store pads)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

CFG = dict(image_size=32, patch_size=16, num_transformer_layer=2, num_heads=2, embedding_dim=128, mlp_size=256,
           num_classes=10)
NODROP = dict(CFG, mlp_dropout=0.0, embedding_dropout=0.0)
DEV = "cuda"
# a parameter in the middle of the model starts a 4096-element block: padding between segments
BUCKET_LAYOUT = ((9,), 4096)


def _encoder_weights(m):
    return [w for blk in m.transformer_encoder for w in blk.fused_params()[2:12:2] if w.dim() == 2]


def _setup(transposed, layout=None, freeze=False, seed=0, cfg=NODROP, **opt_kw):
    """(model, store, FusedAdam) with weight-decay groups; ``transposed``: the encoder weights are
    registered, so steps run adam_t_kernel (else adam_kernel). ``freeze``: one registered weight (a tile
    segment) and one LayerNorm bias (a flat segment) are frozen."""
    from pytorch_vit_paper_replication_amd.models import ViT
    from pytorch_vit_paper_replication_amd.optim import FusedAdam, param_groups_weight_decay
    from pytorch_vit_paper_replication_amd.runtime.param_store import get_store

    torch.manual_seed(seed)
    m = ViT(**cfg).to(DEV)
    if freeze:
        m.transformer_encoder[1].mlp_block.mlp[0].weight.requires_grad_(False)
        m.transformer_encoder[0].msa_block.layer_norm.bias.requires_grad_(False)
    st = get_store(m, torch.device(DEV), layout=layout)
    if transposed:
        st.register_transposed(_encoder_weights(m))
        st.ensure_transposed()
    opt = FusedAdam(param_groups_weight_decay(m, 0.03), lr=1e-2, **opt_kw)
    return m, st, opt


def _synthetic_step(m, opt, it):
    """The gradients of tests/kernel_checks.py _adam_steps, written into p.grad, then a clipped step."""
    g = torch.Generator(device=DEV).manual_seed(1000 + it)
    for p in m.parameters():
        if p.requires_grad:
            p.grad.copy_(torch.randn(p.shape, device=DEV, generator=g) * (it + 1))
    opt.step(clip_norm=1.0)


def _masks(st):
    """(trainable, frozen, padding) boolean masks over the store's flat layout."""
    train = torch.zeros(st.numel, dtype=torch.bool, device=st.flat.device)
    frozen = torch.zeros_like(train)
    for p, off in zip(st.params, st.offsets):
        (train if p.requires_grad else frozen)[off:off + p.numel()] = True
    return train, frozen, ~(train | frozen)


def _check_update(ema_new, ema_old, p_new, pair, mask, what):
    """ema_new vs decay * ema_old + omd * p_new in float64 from the fp32 pair. Two products and a sum
    are at most three fp32 roundings of 2**-24 each on intermediates no larger than max(|ema_old|,
    |p_new|) (decay + omd <= 1 + 2**-24): the bound is 2**-22 of that maximum, elementwise."""
    d, w = float(pair[0]), float(pair[1])
    want = d * ema_old.double() + w * p_new.double()
    bound = 2.0 ** -22 * torch.maximum(ema_old.abs(), p_new.abs()).double() + 1e-30
    err = (ema_new.double() - want).abs()
    worst = float((err / bound)[mask].max())
    print(f"{what}: decay {d!r} worst error / bound {worst:.3f}")
    assert bool((err <= bound)[mask].all()), f"{what}: worst error / bound {worst}"
    assert not torch.equal(ema_new[mask], ema_old[mask]) or d == 1.0, f"{what}: the EMA did not move"


@pytest.mark.parametrize("transposed", [False, True], ids=["adam_kernel", "adam_t_kernel"])
def test_adam_is_untouched_by_an_attached_ema(transposed):
    """The EMA instantiation writes the same master weights, moments and shadows as the default one."""
    from pytorch_vit_paper_replication_amd.optim import ModelEma

    m1, s1, o1 = _setup(transposed)
    m2, s2, o2 = _setup(transposed)
    assert torch.equal(s1.flat, s2.flat)
    ema = ModelEma(m1, decay=0.99).attach(o1)
    for it in range(3):
        _synthetic_step(m1, o1, it)
        _synthetic_step(m2, o2, it)
    torch.cuda.synchronize()
    assert (o1._tmeta_key is not None) == transposed and (o2._tmeta_key is not None) == transposed
    assert ema.num_updates == 3 and ema.fused_buffer(s1) is not None
    assert torch.equal(s1.flat, s2.flat)
    assert torch.equal(o1._fused[1], o2._fused[1]) and torch.equal(o1._fused[2], o2._fused[2])
    assert torch.equal(s1.shadow, s2.shadow)
    if transposed:
        assert not s1._t_dirty and torch.equal(s1.shadow_t, s2.shadow_t)
    assert not torch.equal(ema.fused_buffer(), s1.flat)


@pytest.mark.parametrize("transposed,layout", [(False, None), (True, None), (True, BUCKET_LAYOUT), (False, BUCKET_LAYOUT)],
                         ids=["adam_kernel", "adam_t_kernel", "adam_t_kernel-buckets", "adam_kernel-buckets"])
def test_ema_values_frozen_segments_and_padding(transposed, layout):
    from pytorch_vit_paper_replication_amd.optim import ModelEma

    m, st, opt = _setup(transposed, layout=layout, freeze=True)
    ema = ModelEma(m, decay=0.99).attach(opt)
    buf = ema.fused_buffer()
    assert buf is not None and buf.shape == st.flat.shape and buf.dtype == torch.float32
    init = buf.clone()
    assert torch.equal(init, st.flat)
    train, frozen, pad = _masks(st)
    assert int(frozen.sum()) == 256 * 128 + 128 and int(pad.sum()) > 0
    if layout is not None:  # padding between segments, not only at the end of a segment's last 64
        k = layout[0][0]
        assert st.offsets[k] % 4096 == 0 and st.offsets[k] - (st.offsets[k - 1] + st.params[k - 1].numel()) >= 64
    for it in range(3):
        old = buf.clone()
        pair = ema.pair_at(ema.num_updates)
        assert pair == (np.float32(0.99), np.float32(1.0 - 0.99))
        _synthetic_step(m, opt, it)
        torch.cuda.synchronize()
        assert ema.fused_buffer() is buf
        _check_update(buf, old, st.flat, pair, train, f"step {it}")
        assert torch.equal(buf[frozen], init[frozen])
        assert bool((buf[pad] == 0).all())
    assert (opt._tmeta_key is not None) == transposed


@pytest.mark.parametrize("transposed", [False, True], ids=["adam_kernel", "adam_t_kernel"])
def test_exact_ends(transposed):
    """decay 0: the EMA is the new weights; decay 1: it never moves. Bit for bit (two-product form)."""
    from pytorch_vit_paper_replication_amd.optim import ModelEma

    for decay in (0.0, 1.0):
        m, st, opt = _setup(transposed, freeze=True)
        ema = ModelEma(m, decay=decay).attach(opt)
        init = ema.fused_buffer().clone()
        train, frozen, pad = _masks(st)
        for it in range(2):
            _synthetic_step(m, opt, it)
        torch.cuda.synchronize()
        buf = ema.fused_buffer()
        assert not torch.equal(st.flat[train], init[train])
        if decay == 0.0:
            assert torch.equal(buf[train], st.flat[train])
        else:
            assert torch.equal(buf, init)
        assert torch.equal(buf[frozen], init[frozen]) and bool((buf[pad] == 0).all())


def test_warmup_decays_eager_and_graph_replay():
    """warmup=True: update n uses min(decay, (1 + n) / (10 + n)). Eager steps take the pair by value; a
    captured step must read the pair graph_prepare() uploads, not an argument frozen at capture."""
    from pytorch_vit_paper_replication_amd.ops.fused_vit import cross_entropy
    from pytorch_vit_paper_replication_amd.optim import ModelEma, warmup_linear_decay
    from pytorch_vit_paper_replication_amd.runtime.graph import GraphedTrainStep

    m, st, opt = _setup(True)
    ema = ModelEma(m, decay=0.9999, warmup=True).attach(opt)
    buf = ema.fused_buffer()
    train, _, _ = _masks(st)
    for it, d in enumerate((1 / 10, 2 / 11, 3 / 12)):
        old = buf.clone()
        pair = ema.pair_at(ema.num_updates)
        assert pair == (np.float32(d), np.float32(1.0 - d))
        _synthetic_step(m, opt, it)
        torch.cuda.synchronize()
        _check_update(buf, old, st.flat, pair, train, f"eager step {it}")

    # the set-up of test_graphed_train_step_matches_eager: its own 3 warm-up steps, then replays
    m, st, opt = _setup(False)  # the model's first forward registers the W^T shadow itself
    sched = warmup_linear_decay(opt, 20, 0.1)
    ema = ModelEma(m, decay=0.9999, warmup=True).attach(opt)
    x = torch.rand(4, 3, 32, 32, device=DEV)
    y = torch.randint(0, 10, (4,), device=DEV)
    g = GraphedTrainStep(m, opt, cross_entropy, x, y, clip_norm=1.0, warmup=3, scheduler=sched)
    assert ema.num_updates == 3 and opt._tmeta_key is not None
    buf = ema.fused_buffer()
    train, _, _ = _masks(st)
    for it, d in enumerate((4 / 13, 5 / 14, 6 / 15)):
        torch.cuda.synchronize()
        old = buf.clone()
        pair = ema.pair_at(ema.num_updates)
        assert pair == (np.float32(d), np.float32(1.0 - d))
        g()
        torch.cuda.synchronize()
        assert ema.num_updates == 4 + it and ema.fused_buffer() is buf
        _check_update(buf, old, st.flat, pair, train, f"replay {it}")
    assert opt.step_count == 6


def test_nonfinite_step_leaves_the_ema_alone():
    """The skip path of test_nonfinite_gradient_skips_step: the kernel returns before any element."""
    from pytorch_vit_paper_replication_amd.optim import ModelEma

    for transposed in (False, True):
        m, st, opt = _setup(transposed, skip_nonfinite=True)
        ema = ModelEma(m, decay=0.9).attach(opt)
        _synthetic_step(m, opt, 0)
        torch.cuda.synchronize()
        before = [t.clone() for t in (ema.fused_buffer(), st.flat, opt._fused[1], opt._fused[2])]
        g = torch.Generator(device=DEV).manual_seed(7)
        for p in m.parameters():
            p.grad.copy_(torch.randn(p.shape, device=DEV, generator=g))
        m.classifier[0].weight.grad[0, 0] = float("inf")
        opt.step(clip_norm=1.0)
        torch.cuda.synchronize()
        assert not torch.isfinite(opt.last_grad_norm).item()
        for a, b in zip(before, (ema.fused_buffer(), st.flat, opt._fused[1], opt._fused[2])):
            assert torch.equal(a, b)
        assert ema.num_updates == 2  # the host counter cannot see the skip


def _train_steps(m, opt, xs, ys, steps, sched=None):
    from pytorch_vit_paper_replication_amd.ops import fused_vit

    for i in steps:
        m.train()
        loss = fused_vit.cross_entropy(m(xs[i]), ys[i])
        opt.zero_grad()
        fused_vit.backward(loss)
        opt.step(clip_norm=1.0)
        if sched is not None:
            sched.step()
    torch.cuda.synchronize()


@pytest.mark.parametrize("decay", [0.5, 0.0])
def test_applied_computes_with_the_averaged_weights(decay):
    from pytorch_vit_paper_replication_amd.models import ViT
    from pytorch_vit_paper_replication_amd.optim import ModelEma

    m, st, opt = _setup(False, cfg=CFG)
    ema = ModelEma(m, decay=decay).attach(opt)
    torch.manual_seed(1)
    xs = [torch.rand(4, 3, 32, 32, device=DEV) for _ in range(4)]
    ys = [torch.randint(0, 10, (4,), device=DEV) for _ in range(4)]
    _train_steps(m, opt, xs, ys, range(3))
    assert st.shadow_t is not None and opt._tmeta_key is not None
    buf = ema.fused_buffer()
    before = [t.clone() for t in (st.flat, st.shadow, st.shadow_t, buf)]
    m.eval()
    with torch.inference_mode():
        outside = m(xs[3]).clone()
    gen0 = st.generation
    with ema.applied(), torch.inference_mode():
        assert torch.equal(st.flat, before[3]) and torch.equal(buf, before[0])
        inside = m(xs[3]).clone()
    torch.cuda.synchronize()
    assert st.generation > gen0
    for a, b in zip(before, (st.flat, st.shadow, st.shadow_t, buf)):
        assert torch.equal(a, b)
    fresh = ViT(**CFG)
    fresh.load_state_dict(ema.state_dict(), strict=True)
    fresh = fresh.to(DEV).eval()
    with torch.inference_mode():
        want = fresh(xs[3])
    assert getattr(fresh, "_pvr_store", None) is not None
    assert torch.equal(inside, want)
    if decay == 0.0:
        assert torch.equal(inside, outside)
    else:
        assert not torch.equal(inside, outside)
    with torch.inference_mode():
        assert torch.equal(m(xs[3]), outside)
    _train_steps(m, opt, xs, ys, [3])
    assert not st._t_dirty and ema.num_updates == 4
    with pytest.raises(ValueError):
        with st.swapped(buf[:-64]):
            pass


def test_swapped_refuses_a_stream_capture(monkeypatch):
    """The exchange is full-buffer copies and a generation bump: nothing a captured graph may hold."""
    m, st, opt = _setup(True)
    other = st.flat.clone() + 1.0
    keep = st.flat.clone()
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(RuntimeError, match="capture"):
        with st.swapped(other):
            pass
    monkeypatch.undo()
    assert torch.equal(st.flat, keep) and torch.equal(other, keep + 1.0)


def test_resume_restores_the_ema_bit_for_bit(tmp_path):
    """The bf16 setting of test_resume_is_bit_exact with an EMA whose warm-up makes the counter matter."""
    from pytorch_vit_paper_replication_amd import _ext
    from pytorch_vit_paper_replication_amd.optim import ModelEma, warmup_linear_decay
    from pytorch_vit_paper_replication_amd.utils.checkpoint import load_checkpoint, save_checkpoint

    cfg = dict(CFG, mlp_dropout=0.1, embedding_dropout=0.1)
    torch.manual_seed(5)
    xs = [torch.rand(4, 3, 32, 32, device=DEV) for _ in range(4)]
    ys = [torch.randint(0, 10, (4,), device=DEV) for _ in range(4)]

    def make(seed):
        m, _, o = _setup(False, seed=seed, cfg=cfg)
        return m, o, warmup_linear_decay(o, 10, 0.2), ModelEma(m, decay=0.9999, warmup=True).attach(o)

    with _ext.deterministic_mode():
        ma, oa, sa, ea = make(0)
        torch.manual_seed(123)
        _train_steps(ma, oa, xs, ys, range(4), sa)

        mb, ob, sb, eb = make(0)
        torch.manual_seed(123)
        _train_steps(mb, ob, xs, ys, range(2), sb)
        path = save_checkpoint(str(tmp_path), mb, ob, sb, epoch=1, model_ema=eb)
        del mb, ob, sb, eb
        mc, oc, sc, ec = make(1)  # different init: everything must come from the checkpoint
        load_checkpoint(str(path), mc, oc, sc, model_ema=ec)
        assert ec.num_updates == 2
        _train_steps(mc, oc, xs, ys, range(2, 4), sc)
    assert ea.num_updates == ec.num_updates == 4
    assert torch.equal(ma._pvr_store.flat, mc._pvr_store.flat)
    assert torch.equal(ea.fused_buffer(), ec.fused_buffer())
    assert not torch.equal(ea.fused_buffer(), ma._pvr_store.flat)


def test_engine_train_evaluates_the_averaged_weights():
    from pytorch_vit_paper_replication_amd import engine
    from pytorch_vit_paper_replication_amd.data import create_synthetic_dataloaders
    from pytorch_vit_paper_replication_amd.optim import ModelEma, warmup_linear_decay

    tr, te, _ = create_synthetic_dataloaders(batch_size=4, train_len=12, test_len=8, image_size=32, num_classes=10)
    m, st, opt = _setup(False, cfg=CFG)
    sched = warmup_linear_decay(opt, 3, 0.1)
    ema = ModelEma(m, decay=0.5)
    loss_fn = torch.nn.CrossEntropyLoss()
    res = engine.train(m, tr, te, opt, loss_fn, sched, epochs=1, device=DEV, model_ema=ema)
    assert list(res) == ["train_loss", "train_acc", "test_loss", "test_acc"] and all(len(v) == 1 for v in res.values())
    assert ema.updated_by(opt) and ema.num_updates == 3 and ema.fused_buffer() is not None
    with ema.applied():
        want = engine.test_step(m, te, loss_fn, DEV)
    assert (res["test_loss"][0], res["test_acc"][0]) == want
    assert engine.test_step(m, te, loss_fn, DEV)[0] != want[0]
