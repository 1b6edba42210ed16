"""Fused GPU autograd Functions for the ViT hot path (bf16 activations, fp32 accumulation).

Token tensors are 2-D ``[B*N, D]`` bf16 row-major (token-major), the layout every kernel reads and
writes in place. Each Function writes its parameter gradients straight into the flat fp32
gradient store (``runtime.param_store``) and returns ``None`` for them, then signals the store so
the data-parallel bucketer can launch all-reduces while the rest of backward runs.

Reference semantics (models/vit.py):
  PatchEmbedding  :45-67   conv(P, stride P) -> flatten -> cat(CLS) -> +pos -> dropout
  TransformerEncoderBlock :166-169  x = MSA(LN(x)) + x ;  x = MLP(LN(x)) + x
  MLPBlock        :118-126 Linear -> GELU(erf) -> Dropout -> Linear -> Dropout
  ViT head        :232-235 LayerNorm on all tokens, classifier on token 0 (here: LN of token 0 only,
                           identical output since LayerNorm is per token)
"""
from __future__ import annotations

import math
from typing import List, Optional

import torch
import torch.nn.functional as F

from .. import _ext
from . import gemm

SITE_SHIFT = 32
ATTN_SITE = 1 << 20  # dropout site of block i's attention probabilities: ATTN_SITE + i
# stochastic depth (drop path): block i's attention branch draws its per-sample keep decisions at site
# DROP_PATH_SITE + 2 i, its MLP branch at DROP_PATH_SITE + 2 i + 1 (disjoint from 0 .. 2 L and ATTN_SITE + i)
DROP_PATH_SITE = 1 << 21
# patch dropout: the keys that rank a sample's patches (csrc/elementwise.hip patch_keep_kernel) are the
# hashes of site PATCH_DROP_SITE (disjoint from 0 .. 2 L, ATTN_SITE + i and DROP_PATH_SITE + k)
PATCH_DROP_SITE = 1 << 22
# random erasing: the "pixel" fill's normals (csrc/elementwise.hip erase_normal) are drawn from the hashes of
# site ERASE_SITE (disjoint from 0 .. 2 L, ATTN_SITE + i, DROP_PATH_SITE + k and PATCH_DROP_SITE)
ERASE_SITE = 1 << 23


# Test hook: called as DGRAD_TAP(which, output) after every encoder-block dgrad GEMM (which = 0 fc2,
# 1 fc1, 2 out-proj, 3 qkv), so numerics checks can compare the dgrad outputs themselves.
DGRAD_TAP = None


def site_drop(seed: Optional[torch.Tensor], site: int, p: float, training: bool):
    if seed is None or not training or p <= 0.0:
        return None
    return (seed, site << SITE_SHIFT, float(p))


def _dp(site, rows: int):
    """A drop-path site ``(seed, offset, p)`` (``site_drop`` of a DROP_PATH_SITE site; None: none) as the
    ``drop_path`` argument of the GEMM / column-sum front ends, for a tensor with ``rows`` rows per sample."""
    return None if site is None else (site[0], site[1], site[2], int(rows))


def _split_drops(drops):
    """(fc1 dropout, fc2 dropout, attention dropout, attention-branch drop path, MLP-branch drop path)
    from a block's ``drops`` (the two drop-path sites are optional: a 3-tuple means none)."""
    drops = tuple(drops)
    return drops + (None,) * (5 - len(drops))


def _patch_geometry(C, H, W, patch):
    n_p = (H // patch) * (W // patch)
    kc = C * patch * patch
    return n_p, kc, (kc + 63) // 64 * 64


def patch_keep(seed, B: int, n_p: int, n_keep: int):
    """Patch dropout's table for a step: ``(keep, inv)`` of ``ext.patch_keep_table`` at the counter value
    ``seed`` (None when ``n_keep`` is 0 = off). ``keep`` int32 [B, n_keep]: the kept patches of each sample,
    ascending; ``inv`` int32 [B, n_p]: a patch's row in ``keep``, -1 if dropped."""
    if not n_keep:
        return None
    if n_p > 4096 or B * n_p >= 2 ** 32:
        raise ValueError(f"patch dropout takes at most 4096 patches per image and B * n_p < 2^32, got {B} x {n_p}")
    return _ext.ext().patch_keep_table(seed, PATCH_DROP_SITE << SITE_SHIFT, B, n_p, n_keep)


def _keep_arg(table):
    """The patchify kernels' ``keep`` argument for a :func:`patch_keep` table ({}: none, today's call)."""
    return {} if table is None else dict(keep=table[0])


def _patch_embed_fwd(ctx, patches, B, n_p, kc, kp, store, seed, p_drop, training, conv_w, conv_b, cls, pos, table=None):
    """Patch rows [B*n_p, kp] bf16 -> tokens [B*(n_p+1), D]: the embedding GEMM with the position
    addend and dropout, the CLS rows, and what the backward needs. Shared by the float and the
    uint8 entry (PatchEmbedFn / PatchEmbedU8Fn), which differ only in how ``patches`` is built.

    ``table`` (patch dropout, :func:`patch_keep`): ``patches`` holds the kept rows only, [B*n_keep, kp], and
    the tokens are the compact [B*(n_keep+1), D]; the position addend is gathered per row (one fp32
    [B*(n_keep+1), D] tensor), and the dropout masks are those of the compact element index."""
    ext = _ext.ext()
    dev = patches.device
    D = conv_w.shape[0]
    ntok = n_p + 1
    rows = ntok if table is None else table[0].shape[1] + 1  # token rows per sample
    w16 = store.bf16(conv_w).reshape(D, kc)
    if kp != kc:
        if kc % 4 == 0:
            w16p = torch.empty(D, kp, dtype=torch.bfloat16, device=dev)
            ext.pad_cols_bf16(w16, w16p)  # 8-B column groups
            w16 = w16p
        else:  # odd patch sizes (kc = 3 * P * P odd): plain zero padding
            w16 = torch.nn.functional.pad(w16, (0, kp - kc))
    tokens = torch.empty(B * rows, D, dtype=torch.bfloat16, device=dev)
    drop = site_drop(seed, 0, p_drop, training)
    if table is None:
        addend, period = pos.reshape(ntok, D), ntok
    else:
        addend, period = ext.pos_gather(pos.reshape(ntok, D), table[0]), B * rows
    gemm.linear_fwd(patches, w16, conv_b, addend=addend, addend_period=period,
                    row_remap=(rows - 1, rows, 1), drop=drop, out=tokens)
    dseed, doff, dp = gemm._drop_args(drop)
    ext.cls_rows(cls.reshape(D), pos.reshape(ntok, D)[0].contiguous(), tokens, B, D, rows * D, dseed, doff, dp)
    ctx.save_for_backward(patches)
    ctx.meta = (store, drop, B, ntok, D, kc, kp, conv_w, conv_b, cls, pos, None if table is None else table[1])
    return tokens


def _patch_embed_bwd(ctx, dtokens) -> None:
    ext = _ext.ext()
    (patches,) = ctx.saved_tensors
    store, drop, B, ntok, D, kc, kp, conv_w, conv_b, cls, pos, inv = ctx.meta
    dtokens = dtokens.contiguous()
    gpos = store.grad_dest(pos)
    gcls = store.grad_dest(cls)
    gb = store.grad_dest(conv_b)
    gw = store.grad_dest(conv_w)
    n_keep = patches.shape[0] // B if inv is not None else 0  # patch dropout: dtokens / dconv are the compact tensors
    dconv = torch.empty(patches.shape[0], D, dtype=torch.bfloat16, device=dtokens.device) if gw is not None else None
    dseed, doff, dp = gemm._drop_args(drop)
    ext.patch_bwd(dtokens, B, ntok, D, None if gpos is None else gpos.view(-1),
                  None if gcls is None else gcls.view(-1), dconv, gb, dseed, doff, dp,
                  **({} if inv is None else dict(inv=inv, n_keep=n_keep)))
    if gw is not None:  # K padded to kp in patches; the reduction writes the first kc columns
        gemm.linear_wgrad(dconv, patches, gw.view(D, kc))
    store.grad_ready([conv_w, conv_b, cls, pos])


def _mix_args(mix, B, size, device):
    """The patchify kernels' ``mix`` / ``mix_host`` arguments for a ``data.batch_mix.MixPlan`` (None: none):
    the device table and the host copy the binding validates."""
    if mix is None:
        return {}
    mix.check(B, size)
    return dict(mix=mix.on(device)[0], mix_host=mix.rows)


def _erase_args(erase, B, C, size, device, seed):
    """The patchify kernels' erase arguments for a ``data.random_erasing.ErasePlan`` (None: none, today's
    call): the device table, the host copy the binding validates, mode and value, and for the "pixel"
    mode the step's counter ``seed`` with the offset of ``ERASE_SITE``."""
    if erase is None:
        return {}
    erase.check(B, size)
    kw = dict(erase=erase.on(device), erase_host=erase.rows, erase_mode=erase.mode)
    if erase.mode == "pixel":
        if seed is None:
            raise ValueError("a \"pixel\" ErasePlan needs the step's dropout counter (seed)")
        kw.update(erase_seed=seed, erase_offset=ERASE_SITE << SITE_SHIFT)
    else:
        kw.update(erase_value=list(erase.channel_values(C)))
    return kw


def erase_noise(seed, B: int, C: int, H: int, W: int):
    """The "pixel" fill of a ``[B, C, H, W]`` batch at the counter value ``seed``: what the patchify kernels
    write inside the erase boxes of that step (``ext.erase_noise`` at ``ERASE_SITE``)."""
    return _ext.ext().erase_noise(seed, ERASE_SITE << SITE_SHIFT, B, C, H, W)


def color_u8(x, plan):
    """The colour stage of a ``data.color_augment.ColorPlan`` on a raw uint8 ``[B, 3, Hs, Ws]`` GPU batch (contiguous or
    ``channels_last``): a new uint8 batch of the same shape and layout from the kernels of ``csrc/color.hip``; ``x``
    is untouched. No autograd: images carry no gradient."""
    if x.dim() != 4:
        raise ValueError(f"color_u8: expected [B, 3, Hs, Ws], got {tuple(x.shape)}")
    plan.check(x.shape[0])
    return _ext.ext().color_u8(x, plan.on(x.device), plan.rows)


class PatchEmbedFn(torch.autograd.Function):
    """``mix`` (optional ``MixPlan``): mixup / CutMix inside the gather, here and in PatchEmbedU8Fn.
    ``erase`` (optional ``ErasePlan``): random erasing of each sample before the mix, likewise."""

    @staticmethod
    def forward(ctx, img, patch, store, seed, p_drop, training, conv_w, conv_b, cls, pos, mix=None, n_keep=0, erase=None):
        img = img.float().contiguous()
        B, C, H, W = img.shape
        n_p, kc, kp = _patch_geometry(C, H, W, patch)
        table = patch_keep(seed, B, n_p, n_keep)
        patches = torch.empty(B * (n_keep or n_p), kp, dtype=torch.bfloat16, device=img.device)
        _ext.ext().im2col(img, patches, patch, kp, **_mix_args(mix, B, (H, W), img.device), **_keep_arg(table),
                          **_erase_args(erase, B, C, (H, W), img.device, seed))
        return _patch_embed_fwd(ctx, patches, B, n_p, kc, kp, store, seed, p_drop, training, conv_w, conv_b, cls, pos, table)

    @staticmethod
    def backward(ctx, dtokens):
        _patch_embed_bwd(ctx, dtokens)
        return (None,) * 13


class PatchEmbedU8Fn(torch.autograd.Function):
    """PatchEmbedFn for a raw uint8 image batch [B, C, Hs, Ws] (contiguous or channels_last, read in
    place): ``im2col_u8`` scales to [0, 1], normalises with ``mean`` / ``std`` (per-channel tuples) and,
    with ``geom`` [B, 4] float32 on the device, crops / resizes / flips each sample to ``size`` = (H, W)
    while it writes the patch rows (data/device_input.py). ``geom`` None needs Hs x Ws == H x W."""

    @staticmethod
    def forward(ctx, img, geom, mean, std, size, patch, store, seed, p_drop, training, conv_w, conv_b, cls, pos, mix=None, n_keep=0,
                erase=None):
        B, C = img.shape[0], img.shape[1]
        H, W = size
        n_p, kc, kp = _patch_geometry(C, H, W, patch)
        table = patch_keep(seed, B, n_p, n_keep)
        patches = torch.empty(B * (n_keep or n_p), kp, dtype=torch.bfloat16, device=img.device)
        _ext.ext().im2col_u8(img, patches, list(mean), list(std), geom, H, W, patch, kp, **_mix_args(mix, B, (H, W), img.device),
                             **_keep_arg(table), **_erase_args(erase, B, C, (H, W), img.device, seed))
        return _patch_embed_fwd(ctx, patches, B, n_p, kc, kp, store, seed, p_drop, training, conv_w, conv_b, cls, pos, table)

    @staticmethod
    def backward(ctx, dtokens):
        _patch_embed_bwd(ctx, dtokens)
        return (None,) * 17


# test hook: bf16 outputs left unwritten on the fp8 path (only their fp8 copies are consumed) are
# filled with NaN, so any reader of one would poison the loss / gradients (tests/kernel_checks.py)
POISON_SKIPPED = False


def _poison(t: torch.Tensor, skipped: bool) -> None:
    if skipped and POISON_SKIPPED:
        t.fill_(float("nan"))


def _ln_grad_quant(f8d, which: int, shape, device):
    """Producer-side fp8 copy (the gradient slot's format) of a LayerNorm-backward output for gradient slot ``which`` of the fp8
    block ``f8d = (Fp8State, block)``: (layernorm_bwd kwargs, (copy, dequant scale)) once the slot is
    calibrated, else ({}, None) (the first step calibrates it through the quantize pass)."""
    if f8d is None:
        return {}, None
    prod = f8d[0].grad_producer(f8d[1], which)
    if prod is None:
        return {}, None
    meta, slot = prod
    q = torch.empty(shape, dtype=torch.uint8, device=device)
    kw = dict(q_out=q, q_scale=meta.qscale[slot:slot + 1], q_amax=meta.amax[slot:slot + 1], q_fmt=meta.fmt)
    return kw, (q, meta.dscale[slot:slot + 1])


def _needs_grad(*params) -> bool:
    return any(p is not None and p.requires_grad for p in params)


def _bias_scratch(R: int, device) -> torch.Tensor:
    """Zeroed fp32 [R]: the destination of a folded bias's gradient (LayerScale), read by the unfold."""
    return torch.zeros(R, dtype=torch.float32, device=device)


def _scaled_operands(store, ls, w, b):
    """(bf16 W, bf16 W^T or None, fp32 bias) that the GEMMs of a branch's last Linear read: with LayerScale
    (``ls`` the branch's scale) the store's folded copies ``diag(g) W`` and ``g * b``, else W's shadows and b."""
    if ls is None:
        return store.bf16(w), store.bf16_t(w), b
    w16, wt16 = store.folded_w(w)
    return w16, wt16, (store.folded_b(b) if b is not None else None)  # (the dgrads pass no bias)


def _scaled_wgrad(wgrad, dy, x, w, b, ls, db_hat, dests):
    """Weight gradient of a LayerScale branch's last Linear (runs inside the side-stream closure): the GEMM
    accumulates ``dy^T x`` into a zeroed scratch (allocated here, so the side stream's allocator owns it),
    which with ``db_hat`` (the folded bias's gradient, a scratch of the main stream that the closure's
    caller holds) is unfolded into ``dests`` = the gradient views of (W, b, scale), None for a frozen one."""
    dw_hat = torch.zeros(w.shape, dtype=torch.float32, device=dy.device)
    wgrad(dy, x, dw_hat)
    _ext.ext().layerscale_unfold(dw_hat, db_hat, w, b, ls, *dests)


class BlockLink:
    """Backward hand-off between consecutive encoder blocks. Block i's final LayerNorm backward
    produces dx for block i-1 and, in the same pass, block i-1's fc2 dropout backward (dz2) and fc2
    bias gradient; block i-1's backward then starts from dz2 instead of re-reading dx with a
    column-sum kernel. ``dp2``: block i-1's MLP-branch drop-path site, whose row scale the same pass
    folds into dz2."""

    __slots__ = ("drop2", "b2", "w2", "dz2", "dz2_q", "done", "dp2", "ls2", "db2")

    def __init__(self, drop2, b2, w2=None, dp2=None, ls2=None):
        self.drop2, self.b2, self.w2, self.dz2, self.dz2_q, self.done, self.dp2 = drop2, b2, w2, None, None, False, dp2
        # LayerScale: block i-1's MLP-branch scale (None: none). Its fc2 bias gradient is then that of the folded
        # bias: the producing pass sums it into the zeroed scratch ``db2``, which block i-1's unfold reads
        self.ls2, self.db2 = ls2, None

    def bias_dest(self, store, D: int, device):
        """Where the pass that produces this block's fc2 bias gradient sums it: the gradient view, or with
        LayerScale a zeroed fp32 scratch [D] kept in ``db2`` (None: nothing needs it)."""
        if self.ls2 is None:
            return store.grad_dest(self.b2)
        self.db2 = _bias_scratch(D, device) if _needs_grad(self.w2, self.b2, self.ls2) else None
        return self.db2


def block_links(blocks, drops2, dps2=None):
    """(own link, previous block's link) per block, for EncoderBlockFn's ``links`` argument."""
    dps2 = dps2 if dps2 is not None else [None] * len(drops2)
    own = [BlockLink(d, blk.mlp_block.mlp[3].bias, blk.mlp_block.mlp[3].weight, dp, getattr(blk, "layer_scale_2", None))
           for blk, d, dp in zip(blocks, drops2, dps2)]
    return [(own[i], own[i - 1] if i else None) for i in range(len(own))]


class EncoderBlockFn(torch.autograd.Function):
    """One pre-LN transformer encoder block, forward and hand-written backward."""

    @staticmethod
    def forward(ctx, x, B, N, H, eps1, eps2, store, drops, f8, links, *params):
        ext = _ext.ext()
        # fc1 (after GELU), fc2, attention probabilities; drop path of the attention / MLP branch
        drop1, drop2, dropa, dpa, dpm = _split_drops(drops)
        if f8 is not None and (dpa is not None or dpm is not None):
            raise NotImplementedError("enable_fp8() does not combine with set_drop_path(): the fp8 gradient copies "
                                      "would have to be taken from the drop-path-scaled gradients")
        aseed, aoff, ap = gemm._drop_args(dropa)
        ln1w, ln1b, wqkv, bqkv, wo, bo, ln2w, ln2b, w1, b1, w2, b2 = params[:12]
        ls1, ls2 = params[12:] if len(params) > 12 else (None, None)  # LayerScale: the branches' scales
        if f8 is not None and ls1 is not None:
            raise NotImplementedError("enable_fp8() does not combine with set_layer_scale(): the fp8 weight copies "
                                      "would have to be taken from the folded weights")
        T, D = x.shape
        ctx.links = links if links is not None else (None, None)
        # fp8 dgrad GEMMs (e5m2 gradients x e4m3 W^T) only if the model asked for them:
        # ViT.enable_fp8(dgrad=True), the default (+5 % ViT-H/14, profiles/fp8_dgrad_ab.log)
        ctx.f8d = f8 if f8 is not None and f8[0].dgrad else None
        M = w1.shape[0]
        scale = 1.0 / math.sqrt(D // H)
        # inference (grad mode off at the model call: eval under no_grad / inference_mode; a Function's
        # forward itself always runs with grad mode off, and ctx.needs_input_grad ignores the caller's
        # mode): the fc1 epilogue stores no GELU derivative and nothing is saved for a backward
        need_bwd = getattr(store, "grad_enabled", True) and any(ctx.needs_input_grad)
        u = (torch.empty(T, M, dtype=torch.bfloat16, device=x.device)  # receives mask*scale*gelu'(pre-act)
             if need_bwd else None)
        q1 = f8[0].act_producer(f8[1], 0) if f8 is not None else None

        def fp8_only(which_grad: int, which_act: int) -> bool:
            # the bf16 activation is read by nothing but the weight gradient of (gradient slot, activation
            # slot), and that one is certain to run in fp8 from the activation's e4m3 copy (both slots
            # calibrated, so they stay so): the producer then stores only the fp8 copy (HBM writes saved).
            # Inference: the next GEMM reads the e4m3 copy and nothing is saved, so no bf16 copy either
            if not need_bwd:
                return T >= 256 and DGRAD_TAP is None
            return (ctx.f8d is not None and T >= 256 and DGRAD_TAP is None
                    and f8[0].wgrad_ready(f8[1], which_grad, which_act))

        if q1 is not None:  # fp8 forward, calibrated: xn1's e4m3 copy from the LayerNorm itself
            from . import fp8 as F8

            skip1 = fp8_only(3, 0)
            xn1, mean1, rstd1, xq1 = F8.layernorm_fwd_q8(x, ln1w, ln1b, eps1, q1, skip_y=skip1)
            _poison(xn1, skip1)
        else:
            xn1, mean1, rstd1 = ext.layernorm_fwd(x, ln1w, ln1b, eps1, T, D)
        if f8 is None:
            qkv = gemm.linear_fwd(xn1, store.bf16(wqkv), bqkv)
            o, lse = ext.attn_fwd(qkv, B, N, H, scale, aseed, aoff, ap)
            wo16, _, bo_r = _scaled_operands(store, ls1, wo, bo)
            w2_16, _, b2_r = _scaled_operands(store, ls2, w2, b2)
            x1 = gemm.linear_fwd(o, wo16, bo_r, resid=x, drop_path=_dp(dpa, N))
            xn2, mean2, rstd2 = ext.layernorm_fwd(x1, ln2w, ln2b, eps2, T, D)
            h = gemm.linear_fwd(xn2, store.bf16(w1), b1, gelu_aux=u, gelu=True, drop=drop1)
            x2 = gemm.linear_fwd(h, w2_16, b2_r, resid=x1, drop=drop2, drop_path=_dp(dpm, N))
        else:
            # fp8 forward GEMMs (e4m3 x e4m3, per-tensor delayed scaling); everything the backward
            # saves stays bf16, so the backward below is unchanged
            from . import fp8 as F8

            st, blk = f8
            gen = store.generation
            lay = store.layout_key()
            wq = [st.weight(store.bf16(w), id(w), gen, lay) for w in (wqkv, wo, w1, w2)]
            acts8 = []  # the e4m3 operands xn1, o, xn2, h: kept for the fp8 weight gradients (byte transposes)
            a, s_ = xq1 if q1 is not None else st.act_quant(xn1, blk, 0)
            acts8.append(a)
            qkv = F8.linear_fwd_fp8(a, s_, *wq[0], bqkv)
            qo = st.act_producer(blk, 1)  # o's e4m3 copy from the attention forward (calibrated slot)
            if qo is not None:
                a = torch.empty(T, D, dtype=torch.uint8, device=x.device)
                # inference: only o's e4m3 copy is read (the out-proj GEMM); the bf16 o is not stored
                o_only = not need_bwd and T >= 256 and DGRAD_TAP is None
                o, lse = ext.attn_fwd(qkv, B, N, H, scale, aseed, aoff, ap, a, qo[0].qscale[qo[1]:qo[1] + 1],
                                      qo[0].amax[qo[1]:qo[1] + 1], q_only=o_only)
                _poison(o, o_only)
                s_ = qo[0].dscale[qo[1]:qo[1] + 1]
            else:
                o, lse = ext.attn_fwd(qkv, B, N, H, scale, aseed, aoff, ap)
                a, s_ = st.act_quant(o, blk, 1)
            acts8.append(a)
            x1 = F8.linear_fwd_fp8(a, s_, *wq[1], bo, resid=x)
            q2 = st.act_producer(blk, 2)
            if q2 is not None:
                skip2 = fp8_only(1, 2)
                xn2, mean2, rstd2, (a, s_) = F8.layernorm_fwd_q8(x1, ln2w, ln2b, eps2, q2, skip_y=skip2)
                _poison(xn2, skip2)
            else:
                xn2, mean2, rstd2 = ext.layernorm_fwd(x1, ln2w, ln2b, eps2, T, D)
                a, s_ = st.act_quant(xn2, blk, 2)
            acts8.append(a)
            hq = st.act_producer(blk, 3)  # h's e4m3 copy from the fc1 epilogue (calibrated slot)
            skip_h = hq is not None and fp8_only(0, 3)
            h = F8.linear_fwd_fp8(a, s_, *wq[2], b1, gelu_aux=u, drop=drop1, quant=hq, skip_out=skip_h, gelu=True)
            if hq is not None:
                h, (a, s_) = h
                _poison(h, skip_h)
            else:
                a, s_ = st.act_quant(h, blk, 3)
            acts8.append(a)
            x2 = F8.linear_fwd_fp8(a, s_, *wq[3], b2, resid=x1, drop=drop2)
            # for the fp8 weight gradients (only once every slot they use is calibrated)
            ctx.acts8 = acts8 if st.wgrad and need_bwd else None
        if need_bwd:
            ctx.save_for_backward(x, xn1, mean1, rstd1, qkv, o, lse, x1, xn2, mean2, rstd2, u, h)
        ctx.meta = (B, N, H, scale, store, drop1, drop2, dropa, params)
        ctx.dpath = (dpa, dpm)
        if f8 is None:
            ctx.acts8 = None
        return x2

    @staticmethod
    def backward(ctx, dx2):
        ext = _ext.ext()
        _ext.deterministic()  # native flag follows torch.use_deterministic_algorithms from this kernel on
        x, xn1, mean1, rstd1, qkv, o, lse, x1, xn2, mean2, rstd2, u, h = ctx.saved_tensors
        B, N, H, scale, store, drop1, drop2, dropa, params = ctx.meta
        dpa, dpm = ctx.dpath
        ln1w, ln1b, wqkv, bqkv, wo, bo, ln2w, ln2b, w1, b1, w2, b2 = params[:12]
        ls1, ls2 = params[12:] if len(params) > 12 else (None, None)
        scaled = {id(wo): ls1, id(w2): ls2}  # LayerScale: these two read the folded copies
        aseed, aoff, ap = gemm._drop_args(dropa)
        g = store.grad_dest
        dx2 = dx2.contiguous()
        T, D = dx2.shape
        own, prev = ctx.links
        f8d = ctx.f8d

        # (the "e5m2" gradient copies below are e4m3 by default since round 6: Fp8State.grad.fmt)
        pre_q = {}  # grad slot -> (e5m2 copy, dequant scale) written by the producing dgrad epilogue
        grads8 = {}  # grad slot -> the e5m2 copy a dgrad GEMM consumed (reused by the fp8 weight gradients)
        acts8 = ctx.acts8

        def grad8(which):  # the e5m2 copy of gradient slot `which`, consumed or pending (None: none yet)
            if which in grads8:
                return grads8[which]
            return pre_q[which][0] if which in pre_q else None

        def side8(*whichs):  # fp8 copies a side-stream weight gradient reads (held until the join)
            ts = [grad8(w) for w in whichs] + (list(acts8) if acts8 is not None else [])
            return tuple(t for t in ts if t is not None)

        def dgrad(dy, w, which, dgelu_aux=None, colsum=None, skip_out=False):
            w16, wt, _ = _scaled_operands(store, scaled.get(id(w)), w, None)
            if f8d is not None and wt is not None:
                from . import fp8 as F8

                st, blk = f8d
                gq, gs = pre_q.pop(which) if which in pre_q else st.grad_quant(dy, blk, which)
                grads8[which] = gq
                wq, ws = st.weight(wt, ~id(w), store.generation, store.layout_key())
                # the dGELU dgrad (fc2) also writes dU's e5m2 copy for the fc1 dgrad (grad slot 1)
                nq = st.grad_producer(blk, 1) if dgelu_aux is not None else None
                skip = skip_out and DGRAD_TAP is None and nq is not None
                out = F8.linear_dgrad_fp8(gq, gs, wq, ws, dgelu_aux=dgelu_aux, colsum=colsum, quant=nq, skip_out=skip,
                                          g_fmt=st.grad.fmt)
                if nq is not None:
                    out, pre_q[1] = out
                    _poison(out, skip)
            else:
                out = gemm.linear_dgrad(dy, w16, dgelu_aux=dgelu_aux, wt=wt, colsum=colsum)
            if DGRAD_TAP is not None:
                DGRAD_TAP(which, out)
            return out

        def wgrad(dy, x, gw, which_grad, which_act):
            # fp8 weight gradient (e5m2 dy^T x e4m3 x) once the slots are calibrated, else bf16
            if f8d is not None and f8d[0].wgrad_ready(f8d[1], which_grad, which_act) and dy.shape[0] >= 256:
                f8d[0].linear_wgrad(dy, x, gw, f8d[1], which_grad, which_act, grad8(which_grad),
                                    acts8[which_act] if acts8 is not None else None)
            else:
                gemm.linear_wgrad(dy, x, gw)

        # LayerScale: the gradients of a scaled Linear's folded pair go to zeroed scratch (the bias's here, on
        # this stream; the weight's inside the side-stream closure), and the unfold turns them into those of
        # W, b and the scale (None: the branch has no scale, or nothing of it trains)
        gb2 = g(b2) if ls2 is not None else None
        db2 = None
        # ---- MLP branch: x2 = x1 + drop2(h . W2^T + b2),  h = drop1(gelu(u)),  u = xn2 . W1^T + b1
        if own is not None and own.done:
            # the next block's LayerNorm backward already produced dz2 and d(b2) (and, on the fp8
            # path, dz2's e5m2 copy: no quantize pass before the fc2 dgrad)
            dz2 = own.dz2 if own.dz2 is not None else dx2
            own.dz2 = None
            if ls2 is not None:
                db2, own.db2 = own.db2, None
            if own.dz2_q is not None:
                if f8d is not None:
                    pre_q[0] = own.dz2_q
                own.dz2_q = None
        else:
            # last block: the column-sum pass that reduces d(b2) (and applies the fc2 dropout) also
            # writes dz2's e5m2 copy for the fp8 fc2 dgrad once that slot is calibrated
            prod = f8d[0].grad_producer(f8d[1], 0) if f8d is not None and store.bf16_t(w2) is not None else None
            if ls2 is None:
                db2 = g(b2)
            elif _needs_grad(w2, b2, ls2):
                db2 = _bias_scratch(D, dx2.device)
            if drop2 is not None or dpm is not None:
                # (drop path: dz2 = s_m * mask2 * dx2, the last block has no next block's LayerNorm backward to ride on)
                dz2 = torch.empty_like(dx2)
                r = gemm.bias_grad(dx2, db2, drop=drop2, dz=dz2, quant=prod, drop_path=_dp(dpm, N))
            else:
                dz2 = dx2
                r = gemm.bias_grad(dx2, db2, quant=prod) if (db2 is not None or prod is not None) else None
            if prod is not None:
                pre_q[0] = r
        # dU = (dz2 . W2) * mask*scale*gelu'(u), with d(b1) = colsum(dU) reduced in the same epilogue
        gb1 = g(b1)
        gw2, gw1 = g(w2), g(w1)
        # dU's bf16 copy is not stored when both of its readers take the e5m2 copy the dGELU epilogue
        # writes: the fc1 dgrad (fp8, W1^T shadow present) and the fc1 weight gradient (fp8, calibrated)
        det = _ext.deterministic()
        du_fp8_only = (f8d is not None and T >= 256 and store.bf16_t(w1) is not None and not det
                       and f8d[0].wgrad_ready(f8d[1], 1, 2) and f8d[0].grad_producer(f8d[1], 1) is not None)
        # deterministic mode: d(b1) from the column-sum kernel's ordered partials over dU (the bf16 dU,
        # as the reference's autocast bias gradient) instead of the epilogue's per-tile float atomics
        du = dgrad(dz2, w2, 0, dgelu_aux=u, colsum=None if det else gb1, skip_out=du_fp8_only)
        if det and gb1 is not None:
            gemm.bias_grad(du, gb1)

        gls2 = g(ls2) if ls2 is not None else None

        def mlp_wgrads():
            if ls2 is not None:
                if db2 is not None:
                    _scaled_wgrad(lambda dy, a, out: wgrad(dy, a, out, 0, 3), dz2, h, w2, b2, ls2, db2, (gw2, gb2, gls2))
            elif gw2 is not None:
                wgrad(dz2, h, gw2, 0, 3)
            if gw1 is not None:
                wgrad(du, xn2, gw1, 1, 2)

        # weight grads off the critical path
        store.on_side(mlp_wgrads, dz2, h, du, xn2, *side8(0, 1), *(() if ls2 is None or db2 is None else (db2,)))
        dxn2 = dgrad(du, w1, 1)
        dx1 = torch.empty_like(dx2)
        # dx1 = dx2 + LN2'(dxn2); d(bo) = colsum(dx1) reduced in the same kernel; on the fp8 path the
        # kernel also writes dx1's e5m2 copy for the out-proj dgrad (grad slot 2) once it is calibrated
        q_kw, q_dx1 = _ln_grad_quant(f8d, 2, dx1.shape, dx1.device)
        # drop path: the same pass also writes dz1 = s_a * dx1, the gradient of the attention branch
        # (out-projection dgrad / weight gradient operand), and d(bo) becomes colsum(dz1)
        dz1 = torch.empty_like(dx1) if dpa is not None else dx1
        gbo = g(bo)
        dbo = gbo if ls1 is None else (_bias_scratch(D, dx2.device) if _needs_grad(wo, bo, ls1) else None)
        ext.layernorm_bwd(dxn2, D, x1, D, mean2, rstd2, ln2w, dx2, D, dx1, D, g(ln2w), g(ln2b), T, dsum=dbo,
                          **(dict(dz=dz1, **gemm._drop_path_kw(_dp(dpa, N))) if dpa is not None else {}), **q_kw)
        if q_dx1 is not None:
            pre_q[2] = q_dx1
        # (without a bucket that ends on the scale's gradient being told of it, that bucket never completes)
        store.grad_ready([w2, b2, w1, b1, ln2w, ln2b] + ([ls2] if ls2 is not None else []))
        # ---- attention branch: x1 = x + s_a * (attn(qkv(xn1)) . Wo^T + bo)
        gwo, gwqkv = g(wo), g(wqkv)
        gls1 = g(ls1) if ls1 is not None else None
        do = dgrad(dz1, wo, 2)
        gbqkv = g(bqkv)
        side_db = False
        db_part = None
        prow = ext.attn_bwd_bias_rows(B, N, H, D, aseed is not None) if gbqkv is not None else 0
        # the qkv dgrad runs in fp8 (W^T shadow present); its weight gradient too once both slots are
        # calibrated and fp8 weight gradients are on (enable_fp8(wgrad=True), opt-in)
        fp8_qkv = f8d is not None and store.bf16_t(wqkv) is not None
        wgrad8_qkv = fp8_qkv and f8d[0].wgrad_ready(f8d[1], 3, 0)
        # fp8: dQKV's e5m2 copy (grad slot 3: the qkv dgrad operand, and the weight-gradient operand when
        # that runs in fp8) written by the attention backward's own stores once the slot is calibrated
        # (generic kernels) - with bf16 weight gradients too, instead of a separate quantize pass over dQKV
        q8kw, q8res = {}, None
        if fp8_qkv:
            prod = f8d[0].grad_producer(f8d[1], 3)
            if prod is not None and ext.attn_bwd_q8_ok(B, N, H, D, aseed is not None):
                meta, slot = prod
                q8 = torch.empty(T, 3 * D, dtype=torch.uint8, device=do.device)
                # dQKV's bf16 copy is not stored when every reader takes the e5m2 copy: the qkv dgrad
                # and weight gradient (both fp8) and the bias gradient (kernel partials, prow > 0)
                q8_only = wgrad8_qkv and prow > 0 and DGRAD_TAP is None and T >= 256
                q8kw = dict(q_out=q8, q_scale=meta.qscale[slot:slot + 1], q_amax=meta.amax[slot:slot + 1], q_only=q8_only,
                            q_fmt=meta.fmt)
                q8res = (q8, meta.dscale[slot:slot + 1])
        if prow > 0:
            # the attention backward emits per-(image, head, query block) column sums of dQ and dO
            # (= sum_k dV: the v-bias gradient; the k bias has none); only their small reduction
            # remains (side stream), no pass over dQKV
            db_part = torch.empty(B * H, prow, 3 * (D // H), dtype=torch.float32, device=do.device)
            dqkv = ext.attn_bwd(do, qkv, o, lse, B, N, H, scale, None, db_part, **q8kw)
            _poison(dqkv, q8kw.get("q_only", False))
        else:
            # other shapes: the in_proj bias gradient is a column sum of dQKV on the side stream
            dqkv = ext.attn_bwd(do, qkv, o, lse, B, N, H, scale, None, None, aseed, aoff, ap, **q8kw)
            side_db = gbqkv is not None

        def attn_wgrads():
            # the in_proj bias gradient (a memory-bound column sum, consumed only by the optimizer)
            # rides on the side stream with the weight gradients, off the dgrad chain
            if db_part is not None:
                ext.attn_dbias_reduce(db_part, B, H, gbqkv.view(-1))
            if side_db and aseed is None:
                # sum_k dK = 0 (softmax rows: sum_k dS = 0 per query) and sum_k dV = sum_q dO (rows of P
                # sum to 1): the k slice gets nothing, the v slice the column sums of dO, so two
                # [T, D] column sums replace one over [T, 3D]
                gemm.bias_grad(dqkv[:, :D], gbqkv[:D])
                gemm.bias_grad(do, gbqkv[2 * D:])
            elif side_db:
                gemm.bias_grad(dqkv, gbqkv)
            if ls1 is not None:
                if dbo is not None:
                    _scaled_wgrad(lambda dy, a, out: wgrad(dy, a, out, 2, 1), dz1, o, wo, bo, ls1, dbo, (gwo, gbo, gls1))
            elif gwo is not None:
                wgrad(dz1, o, gwo, 2, 1)
            if gwqkv is not None:
                wgrad(dqkv, xn1, gwqkv, 3, 0)

        if q8res is not None:
            pre_q[3] = q8res
        elif fp8_qkv:
            # dQKV's e5m2 copy now, so the side-stream qkv weight gradient transposes it (the dgrad uses it too).
            # With a column-sum in_proj bias gradient (generic attention path) and a calibrated slot, ONE
            # pass over dQKV writes both: the bias gradient (all three slices, exact with or without
            # attention dropout) and the e5m2 copy; the side stream then has no bias work
            prod = f8d[0].grad_producer(f8d[1], 3)
            if side_db and prod is not None:
                pre_q[3] = gemm.bias_grad(dqkv, gbqkv, quant=prod)
                side_db = False
            else:
                pre_q[3] = f8d[0].grad_quant(dqkv, f8d[1], 3)
        store.on_side(attn_wgrads, dz1, o, dqkv, xn1, do, *(() if db_part is None else (db_part,)), *side8(2, 3),
                      *(() if ls1 is None or dbo is None else (dbo,)))
        dxn1 = dgrad(dqkv, wqkv, 3)
        dx = torch.empty_like(dx2)
        if prev is not None:
            # the previous block's fc2 dropout backward and bias gradient ride along with dx
            seed, soff, p = gemm._drop_args(prev.drop2)
            dp_kw = gemm._drop_path_kw(_dp(prev.dp2, N))  # its MLP-branch drop path: dz = s_m * mask2 * dx
            dzp = torch.empty_like(dx2) if seed is not None or dp_kw else None
            # fp8: the previous block's dz2 (= dz, or dx without dropout) leaves as e5m2 too (its grad slot 0)
            pf8 = (f8d[0], f8d[1] - 1) if f8d is not None and f8d[1] > 0 else None
            q_kw, q_dz = _ln_grad_quant(pf8, 0, dx.shape, dx.device)
            # dz's bf16 copy is not stored when the previous block reads only its e5m2 copy: the fc2 dgrad
            # (fp8, W2^T shadow present) and the fc2 weight gradient (fp8, calibrated slots)
            dz_nostore = (q_dz is not None and dzp is not None and T >= 256 and DGRAD_TAP is None
                          and prev.w2 is not None and store.bf16_t(prev.w2) is not None
                          and pf8[0].wgrad_ready(pf8[1], 0, 3))
            ext.layernorm_bwd(dxn1, D, x, D, mean1, rstd1, ln1w, dx1, D, dx, D, g(ln1w), g(ln1b), T,
                              dsum=prev.bias_dest(store, D, dx.device), dz=dzp, seed=seed, seed_offset=soff, drop_p=p,
                              dz_nostore=dz_nostore, **dp_kw, **q_kw)
            if dzp is not None:
                _poison(dzp, dz_nostore)
            prev.dz2, prev.dz2_q, prev.done = dzp, q_dz, True
        else:
            ext.layernorm_bwd(dxn1, D, x, D, mean1, rstd1, ln1w, dx1, D, dx, D, g(ln1w), g(ln1b), T)
        store.grad_ready([bo, wo, bqkv, wqkv, ln1w, ln1b] + ([ls1] if ls1 is not None else []))
        return (dx,) + (None,) * (9 + len(params))


# The classifier reads token 0 of each image only, and after the last block's attention every
# operation is row-wise: with this switch on (default) ViT._forward_fused runs the last encoder block
# through EncoderBlockClsFn, which computes everything after the qkv GEMM for the B class-token rows
# alone. False selects the full last block (A/Bs, parity tests).
CLS_LAST_BLOCK = True


def cls_last_block_ok(N: int, H: int, D: int, f8, dropa) -> bool:
    """True if the last block of a classifier may run on its class-token rows: bf16 path (the fp8
    delayed-scaling statistics cover every token), no attention dropout in this step, a shape the
    class-token attention kernels take."""
    return (CLS_LAST_BLOCK and f8 is None and gemm._drop_args(dropa)[0] is None
            and D % H == 0 and bool(_ext.ext().attn_cls_ok(N, D // H)))


class EncoderBlockClsFn(torch.autograd.Function):
    """The last encoder block of a classifier: ``x [B*N, D]`` -> the block's output on the class-token
    rows only, ``[B, D]``. LN1 and the qkv GEMM (and, backward, the qkv dgrad / weight gradient and the
    LN1 backward) run on every token, since every token's K and V feed the class-token query; the
    attention (csrc/attention.hip attn_cls_*), out-projection, LN2 and the MLP run on B rows. Dropout
    masks are those of rows ``b * N`` of the full tensors, bit for bit (``drop_row_mul``); drop path draws
    per sample, so the B-row tensors take it with one row per sample. bf16 only, no attention dropout
    (``cls_last_block_ok``)."""

    @staticmethod
    def forward(ctx, x, B, N, H, eps1, eps2, store, drops, links, *params):
        ext = _ext.ext()
        drop1, drop2, _, dpa, dpm = _split_drops(drops)
        ln1w, ln1b, wqkv, bqkv, wo, bo, ln2w, ln2b, w1, b1, w2, b2 = params[:12]
        ls1, ls2 = params[12:] if len(params) > 12 else (None, None)  # LayerScale: the branches' scales
        T, D = x.shape
        ctx.links = links if links is not None else (None, None)
        M = w1.shape[0]
        scale = 1.0 / math.sqrt(D // H)
        need_bwd = getattr(store, "grad_enabled", True) and any(ctx.needs_input_grad)
        xn1, mean1, rstd1 = ext.layernorm_fwd(x, ln1w, ln1b, eps1, T, D)
        qkv = gemm.linear_fwd(xn1, store.bf16(wqkv), bqkv)
        o, lse = ext.attn_cls_fwd(qkv, B, N, H, scale)
        xc = x.view(B, N, D)[:, 0]  # the class-token rows, in place (row stride N * D)
        wo16, _, bo_r = _scaled_operands(store, ls1, wo, bo)
        w2_16, _, b2_r = _scaled_operands(store, ls2, w2, b2)
        x1 = gemm.linear_fwd(o, wo16, bo_r, resid=xc, drop_path=_dp(dpa, 1))
        xn2, mean2, rstd2 = ext.layernorm_fwd(x1, ln2w, ln2b, eps2, B, D)
        u = torch.empty(B, M, dtype=torch.bfloat16, device=x.device) if need_bwd else None
        h = gemm.linear_fwd(xn2, store.bf16(w1), b1, gelu_aux=u, gelu=True, drop=drop1, drop_row_mul=N)
        x2 = gemm.linear_fwd(h, w2_16, b2_r, resid=x1, drop=drop2, drop_row_mul=N, drop_path=_dp(dpm, 1))
        if need_bwd:
            ctx.save_for_backward(x, xn1, mean1, rstd1, qkv, o, lse, x1, xn2, mean2, rstd2, u, h)
        ctx.meta = (B, N, H, scale, store, drop2, params)
        ctx.dpath = (dpa, dpm)
        return x2

    @staticmethod
    def backward(ctx, dx2):
        ext = _ext.ext()
        det = _ext.deterministic()  # native flag follows torch.use_deterministic_algorithms from this kernel on
        x, xn1, mean1, rstd1, qkv, o, lse, x1, xn2, mean2, rstd2, u, h = ctx.saved_tensors
        B, N, H, scale, store, drop2, params = ctx.meta
        dpa, dpm = ctx.dpath
        ln1w, ln1b, wqkv, bqkv, wo, bo, ln2w, ln2b, w1, b1, w2, b2 = params[:12]
        ls1, ls2 = params[12:] if len(params) > 12 else (None, None)
        scaled = {id(wo): ls1, id(w2): ls2}  # LayerScale: see EncoderBlockFn.backward
        g = store.grad_dest
        dx2 = dx2.contiguous()  # [B, D]: the gradient of the class-token rows
        T, D = x.shape
        _, prev = ctx.links

        def dgrad(dy, w, which, dgelu_aux=None, colsum=None):
            w16, wt, _ = _scaled_operands(store, scaled.get(id(w)), w, None)
            out = gemm.linear_dgrad(dy, w16, dgelu_aux=dgelu_aux, wt=wt, colsum=colsum)
            if DGRAD_TAP is not None:
                DGRAD_TAP(which, out)
            return out

        # ---- MLP branch on B rows (see EncoderBlockFn.backward)
        gb2 = g(b2)
        db2 = gb2 if ls2 is None else (_bias_scratch(D, dx2.device) if _needs_grad(w2, b2, ls2) else None)
        if drop2 is not None or dpm is not None:
            dz2 = torch.empty_like(dx2)
            gemm.bias_grad(dx2, db2, drop=drop2, dz=dz2, row_mul=N, drop_path=_dp(dpm, 1))
        else:
            dz2 = dx2
            if db2 is not None:
                gemm.bias_grad(dx2, db2)
        gls2 = g(ls2) if ls2 is not None else None
        gb1 = g(b1)
        gw2, gw1 = g(w2), g(w1)
        du = dgrad(dz2, w2, 0, dgelu_aux=u, colsum=None if det else gb1)
        if det and gb1 is not None:
            gemm.bias_grad(du, gb1)

        def mlp_wgrads():  # reductions over B tokens
            if ls2 is not None:
                if db2 is not None:
                    _scaled_wgrad(gemm.linear_wgrad, dz2, h, w2, b2, ls2, db2, (gw2, gb2, gls2))
            elif gw2 is not None:
                gemm.linear_wgrad(dz2, h, gw2)
            if gw1 is not None:
                gemm.linear_wgrad(du, xn2, gw1)

        store.on_side(mlp_wgrads, dz2, h, du, xn2, *(() if ls2 is None or db2 is None else (db2,)))
        dxn2 = dgrad(du, w1, 1)
        dx1 = torch.empty_like(dx2)
        dz1 = torch.empty_like(dx1) if dpa is not None else dx1  # drop path: s_a * dx1 (see EncoderBlockFn.backward)
        gbo = g(bo)
        dbo = gbo if ls1 is None else (_bias_scratch(D, dx2.device) if _needs_grad(wo, bo, ls1) else None)
        ext.layernorm_bwd(dxn2, D, x1, D, mean2, rstd2, ln2w, dx2, D, dx1, D, g(ln2w), g(ln2b), B, dsum=dbo,
                          **(dict(dz=dz1, **gemm._drop_path_kw(_dp(dpa, 1))) if dpa is not None else {}))
        store.grad_ready([w2, b2, w1, b1, ln2w, ln2b] + ([ls2] if ls2 is not None else []))
        # ---- attention branch: the class-token query against every token's K and V
        gwo, gwqkv, gbqkv = g(wo), g(wqkv), g(bqkv)
        gls1 = g(ls1) if ls1 is not None else None
        do = dgrad(dz1, wo, 2)
        dqkv, dq0 = ext.attn_cls_bwd(do, qkv, o, lse, B, N, H, scale)

        def attn_wgrads():
            if gbqkv is not None:
                ext.attn_cls_dbias(dq0, do, gbqkv.view(-1))
            if ls1 is not None:
                if dbo is not None:
                    _scaled_wgrad(gemm.linear_wgrad, dz1, o, wo, bo, ls1, dbo, (gwo, gbo, gls1))
            elif gwo is not None:
                gemm.linear_wgrad(dz1, o, gwo)
            if gwqkv is not None:
                gemm.linear_wgrad(dqkv, xn1, gwqkv)

        store.on_side(attn_wgrads, dz1, o, dqkv, xn1, do, dq0, *(() if ls1 is None or dbo is None else (dbo,)))
        dxn1 = dgrad(dqkv, wqkv, 3)
        dx = torch.empty_like(x)
        # dx = LN1'(dxn1) on every row + dx1 on the class-token rows (compact: no zero-filled carrier)
        if prev is not None:
            # the previous block's fc2 dropout backward and bias gradient ride along with dx
            seed, soff, p = gemm._drop_args(prev.drop2)
            dp_kw = gemm._drop_path_kw(_dp(prev.dp2, N))  # every token row of the previous block: N rows per sample
            dzp = torch.empty_like(x) if seed is not None or dp_kw else None
            ext.layernorm_bwd(dxn1, D, x, D, mean1, rstd1, ln1w, dx1, D, dx, D, g(ln1w), g(ln1b), T,
                              dsum=prev.bias_dest(store, D, dx.device), dz=dzp, seed=seed, seed_offset=soff, drop_p=p,
                              dres_every=N, **dp_kw)
            prev.dz2, prev.dz2_q, prev.done = dzp, None, True
        else:
            ext.layernorm_bwd(dxn1, D, x, D, mean1, rstd1, ln1w, dx1, D, dx, D, g(ln1w), g(ln1b), T, dres_every=N)
        store.grad_ready([bo, wo, bqkv, wqkv, ln1w, ln1b] + ([ls1] if ls1 is not None else []))
        return (dx,) + (None,) * (8 + len(params))


class HeadFn(torch.autograd.Function):
    """Final LayerNorm (token 0 only) + classifier Linear in fp32 (csrc/head.hip: one forward launch;
    backward: dW / db / dgamma / dbeta and d(LN input) in two launches that also zero the other token
    rows of the returned gradient). ``N`` = 1: ``tokens`` holds the class-token rows alone ``[B, D]``
    (EncoderBlockClsFn), and so does the returned gradient: nothing to zero."""

    @staticmethod
    def forward(ctx, tokens, B, N, eps, store, ln_w, ln_b, head_w, head_b):
        ext = _ext.ext()
        logits, xhat, rstd = ext.head_fwd(tokens, B, N, ln_w, ln_b, eps, head_w, head_b)
        ctx.save_for_backward(xhat, rstd)
        ctx.meta = (B, N, store, ln_w, ln_b, head_w, head_b)
        return logits

    @staticmethod
    def backward(ctx, dlogits):
        ext = _ext.ext()
        _ext.deterministic()  # native flag follows torch.use_deterministic_algorithms from this kernel on
        xhat, rstd = ctx.saved_tensors
        B, N, store, ln_w, ln_b, head_w, head_b = ctx.meta
        g = store.grad_dest
        dlogits = dlogits.float().contiguous()
        dtokens = ext.head_bwd(dlogits, xhat, rstd, ln_w, ln_b, head_w, B, N, g(head_w), g(head_b), g(ln_w), g(ln_b))
        store.grad_ready([head_w, head_b, ln_w, ln_b])
        return (dtokens,) + (None,) * 8


class CrossEntropyFn(torch.autograd.Function):
    """Mean softmax cross-entropy with the gradient produced in the same kernel pass (and the per-row
    argmax == label flags the engine's accuracy metric reads: ``last_correct``)."""

    @staticmethod
    def forward(ctx, logits, target, correct):
        ext = _ext.ext()
        lf = logits.float().contiguous()
        B = lf.shape[0]
        dl = torch.empty_like(lf) if logits.requires_grad else None
        mean = torch.empty((), dtype=torch.float32, device=lf.device)
        ext.xent(lf, target.long().contiguous(), dl, correct, 1.0 / B, mean.view(1))
        ctx.save_for_backward(dl) if dl is not None else None
        ctx.in_dtype = logits.dtype
        return mean

    @staticmethod
    def backward(ctx, g):
        (dl,) = ctx.saved_tensors
        return _ext.ext().scale_by(dl, g.float().reshape(1).contiguous()).to(ctx.in_dtype), None, None


# int32 [B] argmax == label flags of the last fused cross_entropy call (device; read by the engine)
last_correct: Optional[torch.Tensor] = None


def cross_entropy(logits: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    global last_correct
    if _ext.use_fused(logits) and logits.dim() == 2 and target.dim() == 1:
        correct = torch.empty(logits.shape[0], dtype=torch.int32, device=logits.device)
        loss = CrossEntropyFn.apply(logits, target, correct)
        last_correct = correct
        return loss
    last_correct = None
    return F.cross_entropy(logits, target)


class SoftCrossEntropyFn(torch.autograd.Function):
    """CrossEntropyFn for soft target rows ``(1 - eps) * (lam * onehot(ya) + (1 - lam) * onehot(yb)) + eps / C``
    (csrc/xent.hip ``xent_soft_kernel``); ``correct`` flags ``argmax == ya``."""

    @staticmethod
    def forward(ctx, logits, ya, yb, lam, eps, correct):
        ext = _ext.ext()
        lf = logits.float().contiguous()
        B = lf.shape[0]
        dl = torch.empty_like(lf) if logits.requires_grad else None
        mean = torch.empty((), dtype=torch.float32, device=lf.device)
        ext.xent_soft(lf, ya, yb, lam, eps, dl, correct, 1.0 / B, mean.view(1))
        ctx.save_for_backward(dl) if dl is not None else None
        ctx.in_dtype = logits.dtype
        return mean

    @staticmethod
    def backward(ctx, g):
        (dl,) = ctx.saved_tensors
        return (_ext.ext().scale_by(dl, g.float().reshape(1).contiguous()).to(ctx.in_dtype),) + (None,) * 5


def soft_targets(target: torch.Tensor, num_classes: int, plan=None, label_smoothing: float = 0.0,
                 dtype=torch.float32) -> torch.Tensor:
    """The explicit target rows ``[B, C]`` of :func:`soft_cross_entropy` as torch ops."""
    ya = target.long()
    one_a = F.one_hot(ya, num_classes).to(dtype)
    if plan is None:
        q = one_a
    else:
        _, partner, lam = plan.on(target.device)
        lam = lam.to(dtype).view(-1, 1)
        q = lam * one_a + (1.0 - lam) * F.one_hot(ya.index_select(0, partner), num_classes).to(dtype)
    return (1.0 - label_smoothing) * q + label_smoothing / num_classes


_ONES: dict = {}


def soft_cross_entropy(logits: torch.Tensor, target: torch.Tensor, plan=None, label_smoothing: float = 0.0) -> torch.Tensor:
    """Mean cross-entropy against mixed and / or smoothed labels: sample ``b``'s target row is
    ``(1 - eps) * (lam_b * onehot(y_b) + (1 - lam_b) * onehot(y_partner[b])) + eps / C`` with ``lam`` =
    ``plan.lam_eff`` of a ``data.batch_mix.MixPlan`` (``plan=None``: no mixing) and ``eps`` = ``label_smoothing``.
    On the GPU one fused kernel (loss, gradient, and the ``last_correct`` flags ``argmax == y_b``); on the
    CPU ``F.cross_entropy`` on the explicit rows (torch's own ``label_smoothing`` when there is no plan)."""
    global last_correct
    eps = float(label_smoothing)
    if plan is not None and plan.batch != logits.shape[0]:
        raise ValueError(f"soft_cross_entropy: a plan for {plan.batch} samples with {logits.shape[0]} logit rows")
    if _ext.use_fused(logits) and logits.dim() == 2 and target.dim() == 1:
        B, dev = logits.shape[0], logits.device
        ya = target.long().contiguous()
        if plan is None:
            yb = ya
            lam = _ONES.get((dev, B))
            if lam is None:
                with torch.inference_mode(False):  # kept across calls: not an inference tensor
                    lam = _ONES[(dev, B)] = torch.ones(B, dtype=torch.float32, device=dev)
        else:
            _, partner, lam = plan.on(dev)
            yb = ya.index_select(0, partner)
        correct = torch.empty(B, dtype=torch.int32, device=dev)
        loss = SoftCrossEntropyFn.apply(logits, ya, yb, lam, eps, correct)
        last_correct = correct
        return loss
    last_correct = None
    if plan is None:
        return F.cross_entropy(logits, target, label_smoothing=eps)
    return F.cross_entropy(logits, soft_targets(target, logits.shape[1], plan, eps, logits.dtype))


class BinaryCrossEntropyFn(torch.autograd.Function):
    """SoftCrossEntropyFn's counterpart for the sigmoid loss (csrc/bce.hip ``bce_kernel``): mean over the rows of
    the binary cross-entropy against the same target rows, binarised at ``thr`` when ``thr >= 0``; the row loss is
    the mean over the classes, or their sum with ``sum_classes``. ``correct`` flags ``argmax == ya``."""

    @staticmethod
    def forward(ctx, logits, ya, yb, lam, eps, thr, sum_classes, correct):
        ext = _ext.ext()
        lf = logits.float().contiguous()
        B, C = lf.shape
        dl = torch.empty_like(lf) if logits.requires_grad else None
        mean = torch.empty((), dtype=torch.float32, device=lf.device)
        ext.bce(lf, ya, yb, lam, eps, thr, sum_classes, dl, correct, 1.0 / B if sum_classes else 1.0 / (B * C), mean.view(1))
        ctx.save_for_backward(dl) if dl is not None else None
        ctx.in_dtype = logits.dtype
        return mean

    @staticmethod
    def backward(ctx, g):
        (dl,) = ctx.saved_tensors
        return (_ext.ext().scale_by(dl, g.float().reshape(1).contiguous()).to(ctx.in_dtype),) + (None,) * 7


def binary_cross_entropy(logits: torch.Tensor, target: torch.Tensor, plan=None, label_smoothing: float = 0.0,
                         target_threshold: Optional[float] = None, sum_classes: bool = False) -> torch.Tensor:
    """Binary cross-entropy with logits against the target rows of :func:`soft_cross_entropy` (integer labels
    ``target`` ``[B]``, mixed by ``plan``, smoothed by ``label_smoothing``): the loss of DeiT-III and of timm's
    ``--bce-loss``. ``target_threshold`` (optional, below 1) binarises the rows, ``t = q > threshold``.
    The result is ``F.binary_cross_entropy_with_logits``'s ``mean`` over ``[B, C]``, or with ``sum_classes``
    the sum over the classes averaged over the batch. On the GPU one fused kernel (loss, gradient, and the
    ``last_correct`` flags ``argmax == y_b``); elsewhere the torch function on the explicit rows."""
    global last_correct
    eps = float(label_smoothing)
    if plan is not None and plan.batch != logits.shape[0]:
        raise ValueError(f"binary_cross_entropy: a plan for {plan.batch} samples with {logits.shape[0]} logit rows")
    if target_threshold is not None and not 0.0 <= target_threshold < 1.0:
        raise ValueError(f"binary_cross_entropy: target_threshold must be in [0, 1), got {target_threshold}")
    if _ext.use_fused(logits) and logits.dim() == 2 and target.dim() == 1:
        B, dev = logits.shape[0], logits.device
        ya = target.long().contiguous()
        if plan is None:
            yb = ya
            lam = _ONES.get((dev, B))
            if lam is None:
                with torch.inference_mode(False):  # kept across calls: not an inference tensor
                    lam = _ONES[(dev, B)] = torch.ones(B, dtype=torch.float32, device=dev)
        else:
            _, partner, lam = plan.on(dev)
            yb = ya.index_select(0, partner)
        correct = torch.empty(B, dtype=torch.int32, device=dev)
        thr = -1.0 if target_threshold is None else float(target_threshold)
        loss = BinaryCrossEntropyFn.apply(logits, ya, yb, lam, eps, thr, bool(sum_classes), correct)
        last_correct = correct
        return loss
    last_correct = None
    t = soft_targets(target, logits.shape[1], plan, eps, logits.dtype)
    if target_threshold is not None:
        t = t.gt(target_threshold).to(t.dtype)
    if sum_classes:
        return F.binary_cross_entropy_with_logits(logits, t, reduction="none").sum(-1).mean()
    return F.binary_cross_entropy_with_logits(logits, t)


_UNIT: dict = {}


def backward(loss: torch.Tensor) -> None:
    """``loss.backward()`` seeded from a persistent device 1.0 of the loss's shape: autograd's own
    seed is a fresh ``ones_like`` (an ATen fill kernel) on every step."""
    if not loss.is_cuda:
        loss.backward()
        return
    key = (loss.device, loss.dtype, tuple(loss.shape))
    u = _UNIT.get(key)
    if u is None:
        u = _UNIT[key] = torch.ones_like(loss)
    loss.backward(u)


class TokenLayerNormFn(torch.autograd.Function):
    """LayerNorm over every row of a bf16 token matrix [T, D] (used by the classifier-free ViT)."""

    @staticmethod
    def forward(ctx, tokens, eps, store, w, b):
        ext = _ext.ext()
        T, D = tokens.shape
        y, mean, rstd = ext.layernorm_fwd(tokens, w, b, eps, T, D)
        ctx.save_for_backward(tokens, mean, rstd)
        ctx.meta = (store, w, b)
        return y

    @staticmethod
    def backward(ctx, dy):
        ext = _ext.ext()
        _ext.deterministic()  # native flag follows torch.use_deterministic_algorithms from this kernel on
        tokens, mean, rstd = ctx.saved_tensors
        store, w, b = ctx.meta
        T, D = tokens.shape
        dy = dy.to(torch.bfloat16).contiguous()
        dx = torch.empty_like(tokens)
        ext.layernorm_bwd(dy, D, tokens, D, mean, rstd, w, None, 0, dx, D, store.grad_dest(w), store.grad_dest(b), T)
        store.grad_ready([w, b])
        return dx, None, None, None, None
