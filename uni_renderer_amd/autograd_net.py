"""The four networks as differentiable functions (SURVEY section 8a device op 11; reference train/train.py:1324-1354):
AttributeEncoderModel, UNet2DConditionModel, AttributeDecoderModel and ControlNetModel written over the autograd Functions
of ``autograd_ops``, so every forward AND backward kernel is this package's HIP code and torch.autograd only walks the graph.
``controlnet.py``'s module ``forward``s route here whenever autograd is recording; ``dual_stream_forward`` composes the three
networks of the training step (train_step.py) without the NCHW views in between.

The modules hold the fp32 master parameters (as under the reference's autocast).  Each network forward runs inside one
``param_stage.Stage``, which casts, merges (trainable LoRA) and packs them into the compute dtype up front, inside the graph,
so gradients arrive in fp32 on ``param.grad``.  Activations are NHWC / token matrices in the compute dtype.  Fused here: all
``time_emb_proj`` of a network phase are one GEMM, so are the to_k | to_v of its cross-attentions and q | k | v of each
self-attention (adjacent slices of the staged buffer, ``A.cat_adjacent``); attention keeps q, k, v, o and the row statistics
and runs the flash backward where its shapes allow; a pre-norm residual is one node with its LayerNorm.  GEGLU is its own
kernel, the up path's concatenation is materialised, resnets honour ``gradient_checkpointing`` (tests/test_train_gpu.py).
"""
from __future__ import annotations

from typing import Dict, List, Optional

import torch

from . import autograd_ops as A
from . import ops
from .controlnet import CIN_PAD
from .param_stage import Stage, lora_merged, w2 as _w2, wc as _wc
from .unet_2d_blocks import freeu_enabled


def _temb_projections(resnets, temb_act, dt):
    """All ``time_emb_proj`` of a network phase as ONE GEMM (what the inference path does too): the M = batch-size
    linears, their two backward GEMMs, three transposes and the bias column sum per resnet are launch-bound, ~25
    launches per resnet.  Returns {id(resnet): [B, C_out] column slice}; autograd splits the gradients back."""
    w = A.cat_adjacent([_wc(r.time_emb_proj.weight, dt) for r in resnets])
    b = torch.cat([r.time_emb_proj.bias for r in resnets], 0)
    t_all = A.linear(temb_act, w, b)
    # torch.split, not per-resnet slicing: its backward is ONE cat of the slice gradients, where every SliceBackward
    # allocates a zero-filled full-width tensor, copies its slice in and adds it to the running sum (3 launches each)
    parts = torch.split(t_all, [r.time_emb_proj.weight.shape[0] for r in resnets], dim=1)
    return {id(r): part for r, part in zip(resnets, parts)}


def _resnets_of(blocks, mid=None):
    rs = [r for blk in blocks for r in blk.resnets]
    return rs + (list(mid.resnets) if mid is not None else [])


def _resnet(r, x, temb, dt, x1=None, scw=None):
    """models/unet_2d_blocks.py:1100-1111 (ResnetBlock2D, time_embedding_norm='default'); ``temb``: the dict of
    _temb_projections; ``scw``: the [N, K] shortcut weight when the caller holds it (a LoRA-merged one under checkpointing)."""
    xin = torch.cat([x, x1], -1) if x1 is not None else x
    h = A.group_norm(xin, r.norm1.weight, r.norm1.bias, r.eps, r.groups, True)
    t = temb[id(r)]
    h = A.conv3x3(h, A.pack_conv_weight(r.conv1.weight, dt), r.conv1.bias, rowadd=t)
    h = A.group_norm(h, r.norm2.weight, r.norm2.bias, r.eps, r.groups, True)
    sc = xin if r.conv_shortcut is None else A.linear(xin, scw if scw is not None else _w2(r.conv_shortcut, dt), r.conv_shortcut.bias)
    if r.output_scale_factor != 1.0:
        raise NotImplementedError("output_scale_factor != 1 in the training path")
    return A.conv3x3(h, A.pack_conv_weight(r.conv2.weight, dt), r.conv2.bias, res=sc)


def _resnet_ckpt(blk, r, x, temb, dt, x1=None):
    """``_resnet``, recomputed in the backward when the block asks for it (unet_2d_blocks.py:1172-1197: training mode and
    ``gradient_checkpointing``; ``use_reentrant=False`` like the reference).  The recompute runs the same kernels on the same
    inputs, so the saved tensors -- and with them every gradient -- are bit-identical to the ones the plain forward keeps."""
    if getattr(blk, "gradient_checkpointing", False) and torch.is_grad_enabled() and blk.training:
        from torch.utils.checkpoint import checkpoint

        # a LoRA-merged shortcut weight exists only while its network forward runs: the recompute (in the backward, on the
        # unstaged look-ups) must be handed the very tensor; x1 / scw may be None
        scw = _w2(r.conv_shortcut, dt) if (r.conv_shortcut is not None and lora_merged(r.conv_shortcut.weight)) else None
        fn = lambda x_, t_, x1_, w_: _resnet(r, x_, {id(r): t_}, dt, x1=x1_, scw=w_)
        return checkpoint(fn, x, temb[id(r)], x1, scw, use_reentrant=False)
    return _resnet(r, x, temb, dt, x1=x1)


def _self_attn(a, xn, res, dt):
    """q | k | v as ONE projection (one forward and two backward GEMMs instead of three of each)."""
    qkv = A.linear(xn, A.cat_adjacent([_wc(a.to_q.weight, dt), _wc(a.to_k.weight, dt), _wc(a.to_v.weight, dt)]))
    o = A.AttentionQKV.apply(qkv, a.heads)
    return A.linear(o, _w2(a.to_out[0], dt), a.to_out[0].bias, res=res)


def _cross_attn(a, xn, kv, res, dt):
    """``kv`` [B, 77, 2C]: this block's columns of the phase-wide prompt projection (_context_projections)."""
    Cc = a.to_q.weight.shape[0]
    q = A.linear(xn, _w2(a.to_q, dt))
    k_, v_ = torch.split(kv, Cc, dim=-1)
    o = A.Attention.apply(q, k_, v_, a.heads)
    return A.linear(o, _w2(a.to_out[0], dt), a.to_out[0].bias, res=res)


def _context_projections(blocks, ehs, dt):
    """to_k | to_v of every cross-attention of a network phase applied to the prompt embedding as ONE GEMM (M = 77 B
    rows: per block these projections and their backward are launch-bound).  {id(block): [B, 77, 2C] column slice}."""
    tbs = [tb for blk in blocks for t in getattr(blk, "attentions", []) for tb in t.transformer_blocks]
    if not tbs:
        return {}
    w = A.cat_adjacent([_wc(w_, dt) for tb in tbs for w_ in (tb.attn2.to_k.weight, tb.attn2.to_v.weight)])
    kv_all = A.linear(ehs, w)
    parts = torch.split(kv_all, [2 * tb.attn2.to_k.weight.shape[0] for tb in tbs], dim=-1)  # one cat in the backward
    return {id(tb): part for tb, part in zip(tbs, parts)}


def _tblock(b, x, kvs, dt):
    # (x, LN(x)) as one autograd node: the residual's gradient is added inside the LayerNorm backward kernel
    xs, xn = A.layer_norm_skip(x, b.norm1.weight, b.norm1.bias, b.norm1.eps)
    x = _self_attn(b.attn1, xn, xs, dt)
    xs, xn = A.layer_norm_skip(x, b.norm2.weight, b.norm2.bias, b.norm2.eps)
    x = _cross_attn(b.attn2, xn, kvs[id(b)], xs, dt)
    proj, out = b.ff.net[0].proj, b.ff.net[2]
    xs, xn = A.layer_norm_skip(x, b.norm3.weight, b.norm3.bias, b.norm3.eps)
    h = A.linear(xn, _w2(proj, dt), proj.bias)
    return A.linear(A.GEGLU.apply(h), _w2(out, dt), out.bias, res=xs)


def _transformer(t, x, ehs, dt):
    B, H, W, Cc = x.shape
    h = A.group_norm(x, t.norm.weight, t.norm.bias, t.norm.eps, t.groups, False)
    h = A.linear(h.view(B, H * W, Cc), _w2(t.proj_in, dt), t.proj_in.bias)
    for blk in t.transformer_blocks:
        h = _tblock(blk, h, ehs, dt)
    return A.linear(h, _w2(t.proj_out, dt), t.proj_out.bias, res=x.view(B, H * W, Cc)).view(B, H, W, Cc)


def _conv(m, x, dt, stride=1, cin_pad=None):
    return A.conv3x3(x, A.pack_conv_weight(m.weight, dt, cin_pad), m.bias, stride=stride)


def _time(net, timesteps, B, dt, dev):
    t = torch.as_tensor(timesteps, device=dev, dtype=torch.float32).reshape(-1)
    t = t.expand(B).contiguous() if t.numel() == 1 else t.contiguous()
    c = net.config
    t_emb = ops.timestep_embedding(t, B, c["block_out_channels"][0], c["flip_sin_to_cos"], c["freq_shift"], dt)
    te = net.time_embedding
    emb = A.linear(A.SiLU.apply(A.linear(t_emb, _w2(te.linear_1, dt), te.linear_1.bias)), _w2(te.linear_2, dt),
                   te.linear_2.bias)
    return A.SiLU.apply(emb)  # every resnet applies SiLU to the embedding before its projection


def _down_mid(net, x, temb_act, ehs, dt):
    temb = _temb_projections(_resnets_of(net.down_blocks, net.mid_block), temb_act, dt)
    ehs = _context_projections(list(net.down_blocks) + [net.mid_block], ehs, dt)  # from here on: per-block K | V
    skips = [x]
    for blk in net.down_blocks:
        for i, r in enumerate(blk.resnets):
            x = _resnet_ckpt(blk, r, x, temb, dt)
            if getattr(blk, "has_cross_attention", False):
                x = _transformer(blk.attentions[i], x, ehs, dt)
            skips.append(x)
        if blk.downsamplers is not None:
            x = _conv(blk.downsamplers[0].conv, x, dt, stride=2)
            skips.append(x)
    m = net.mid_block
    x = _resnet(m.resnets[0], x, temb, dt)
    for a, r in zip(m.attentions, m.resnets[1:]):
        x = _resnet(r, _transformer(a, x, ehs, dt), temb, dt)
    return x, skips


FREEU_AUTOGRAD_MSG = ("FreeU is enabled on this network's up blocks, but the differentiable path has no backward for it: FreeU is a "
                      "sampling-time switch -- call disable_freeu() for training, or run the forward under torch.no_grad()")

LORA_AUTOGRAD_MSG = ("a LoRA adapter is loaded on this network that is not trainable (it is merged into the weights): train one made "
                     "with add_adapter() or loaded with load_attn_procs(..., trainable=True), call unload_lora() to train the "
                     "network itself, or run the forward under torch.no_grad()")


def _up_out(net, x, skips: List[torch.Tensor], temb_act, ehs, dt, extras=None, collect=None):
    """Up path + conv_out.  ``extras``: per-resnet tensors added after each resnet(/transformer) of an ``UpRes*`` block
    (unet_2d_blocks.py:2408, 2814); ``collect``: list that receives the per-layer outputs (the reference-modified
    blocks return them, 2584-2590 / 2697-2704)."""
    if freeu_enabled(net):
        raise NotImplementedError(FREEU_AUTOGRAD_MSG)
    temb = _temb_projections(_resnets_of(net.up_blocks), temb_act, dt)
    ehs = _context_projections(net.up_blocks, ehs, dt)
    skips = list(skips)
    k = 0
    for blk in net.up_blocks:
        for i, r in enumerate(blk.resnets):
            x = _resnet_ckpt(blk, r, x, temb, dt, x1=skips.pop())
            if getattr(blk, "has_cross_attention", False):
                x = _transformer(blk.attentions[i], x, ehs, dt)
            if extras is not None and getattr(blk, "adds_up_states", False):
                x = A.Add.apply(x, extras[k])
            k += 1
            if collect is not None:
                collect.append(x)
        if blk.upsamplers is not None:
            tgt = tuple(skips[-1].shape[1:3])  # the reference's upsample_size (controlnet.py:1129-1130)
            if tgt != (2 * x.shape[1], 2 * x.shape[2]):
                raise NotImplementedError("training path: latent sides must be multiples of 2**num_upsamplers")
            x = _conv(blk.upsamplers[0].conv, A.Up2x.apply(x), dt)
    n = net.conv_norm_out
    h = A.group_norm(x, n.weight, n.bias, n.eps, n.num_groups, True)
    return _conv(net.conv_out, h, dt)


def to_nhwc_grad(t: torch.Tensor, dt, cpad: Optional[int] = None) -> torch.Tensor:
    """NCHW (any strides / dtype, may carry a grad_fn) -> contiguous NHWC in the compute dtype, channels zero padded to
    ``cpad``; plain differentiable torch glue (a zero-copy view when ``t`` is one of this package's NCHW views)."""
    v = t.permute(0, 2, 3, 1)
    if v.dtype != dt:
        v = v.to(dt)
    if cpad is not None and v.shape[-1] != cpad:
        v = torch.nn.functional.pad(v, (0, cpad - v.shape[-1]))
    return v.contiguous()


def _prompt(ehs, B, dt):
    ehs = ehs.to(dt).contiguous()
    if ehs.shape[0] == 1 and B > 1:
        ehs = ehs.expand(B, -1, -1).contiguous()
    return ehs


def encoder_forward(enc, cond_nhwc, ehs, t_attr, dt, conditioning_scale: float = 1.0):
    """AttributeEncoderModel (controlnet.py:1657-1778).  ``cond_nhwc`` [B,H,W,CIN_PAD].  Returns
    (res[12], mid_res, raw_down[12], raw_mid), NHWC."""
    B, dev = cond_nhwc.shape[0], cond_nhwc.device
    with Stage(enc, dt):
        te = _time(enc, t_attr, B, dt, dev)
        xe = _conv(enc.conv_in, cond_nhwc, dt, cin_pad=CIN_PAD)
        res, mid_res, raw_enc, raw_mid_enc = _encoder_trunk(enc, xe, te, ehs, dt)
    if conditioning_scale != 1.0:  # ref 1773-1775
        res = [r * conditioning_scale for r in res]
        mid_res = mid_res * conditioning_scale
    return res, mid_res, raw_enc, raw_mid_enc


def _encoder_trunk(net, x, te, ehs, dt):
    """Down blocks, mid block and the 12 + 1 exchange (``controlnet_*``) convs of an encoder-shaped network, from the output of its
    input stage on: what AttributeEncoderModel and ControlNetModel share.  Inside the caller's ``Stage``."""
    raw_mid, raw = _down_mid(net, x, te, ehs, dt)
    res = [A.linear(s, _w2(z, dt), z.bias) for s, z in zip(raw, net.controlnet_down_blocks)]
    mid_res = A.linear(raw_mid, _w2(net.controlnet_mid_block, dt), net.controlnet_mid_block.bias)
    return res, mid_res, raw, raw_mid


def controlnet_forward(cn, x_nhwc, cond_nchw, ehs, t, dt, conditioning_scale: float = 1.0, guess_mode: bool = False):
    """ControlNetModel (ref 2530-3266) under autograd: the conditioning embedding on the direct narrow-channel kernels
    (layers.ControlNetConditioningEmbedding.forward_autograd), its ``conv_out`` as the residual operand of ``conv_in(sample)``,
    then the trunk of ``encoder_forward``.  ``x_nhwc`` [B,H,W,CIN_PAD]; ``cond_nchw`` the caller's image (no gradient).  The
    scales are host floats: ``conditioning_scale``, times ``logspace(-1, 0, 13)`` in ``guess_mode`` (ref 3245-3249).  Returns
    (res[12], mid_res), NHWC.  Not covered here: ``GraphedTrainStep`` (built around the three-network batch),
    ``parallel.GradientBuckets`` / ``GradSink`` for this network, and LoRA on it."""
    B, dev = x_nhwc.shape[0], x_nhwc.device
    emb = cn.controlnet_cond_embedding
    bgr = cn.config["controlnet_conditioning_channel_order"] == "bgr"
    with Stage(cn, dt):
        te = _time(cn, t, B, dt, dev)
        h = emb.forward_autograd(cond_nchw, dt, bgr=bgr)
        if tuple(h.shape[:3]) != tuple(x_nhwc.shape[:3]):
            raise ValueError(f"controlnet_cond {tuple(cond_nchw.shape)} embeds to a {tuple(h.shape[1:3])} map for a "
                             f"{tuple(x_nhwc.shape[1:3])} sample")
        e = _conv(emb.conv_out, h, dt)
        x = A.conv3x3(x_nhwc, A.pack_conv_weight(cn.conv_in.weight, dt, CIN_PAD), cn.conv_in.bias, res=e)  # ref 3201-3204
        res, mid_res, _, _ = _encoder_trunk(cn, x, te, ehs, dt)
    s, n = float(conditioning_scale), len(res) + 1
    scales = [10.0 ** (-1.0 + i / (n - 1)) * s for i in range(n)] if guess_mode else [s] * n
    res = [r if k == 1.0 else r * k for r, k in zip(res, scales)]
    mid_res = mid_res if scales[-1] == 1.0 else mid_res * scales[-1]
    return res, mid_res


def unet_forward(unet, x_nhwc, ehs, t_img, dt, res=None, mid_res=None, collect_up: bool = False, lora_scale=None):
    """UNet2DConditionModel (controlnet.py:781-1166).  ``x_nhwc`` [B,H,W,CIN_PAD]; ``res`` / ``mid_res``: the encoder's
    residuals (NHWC) or None.  Returns (img_pred, raw_down[12], raw_mid, up_res[13] | None), NHWC.
    ``lora_scale``: the scale of a trainable LoRA adapter (``cross_attention_kwargs["scale"]``; None: 1.0, or the pinned one)."""
    if getattr(unet, "_ip", None) is not None:
        from .ip_adapter import IP_AUTOGRAD_MSG

        raise NotImplementedError(IP_AUTOGRAD_MSG)  # this path has neither the forward nor a backward of the image attention
    plan = None
    if getattr(unet, "_lora", None) is not None:
        if torch.is_grad_enabled():
            plan = unet._lora_train_plan(lora_scale)  # raises for an adapter that cannot be trained
        else:
            unet._lora_apply(lora_scale)  # the parameters hold the merged weights, as on the inference path
    B, dev = x_nhwc.shape[0], x_nhwc.device
    with Stage(unet, dt, lora=plan):
        tu = _time(unet, t_img, B, dt, dev)
        xu = _conv(unet.conv_in, x_nhwc, dt, cin_pad=CIN_PAD)
        raw_mid_unet, raw_unet = _down_mid(unet, xu, tu, ehs, dt)
        skips, mid = raw_unet, raw_mid_unet
        if res is not None:  # ref 1078-1087, 1114-1115
            skips = [A.Add.apply(s, r) for s, r in zip(raw_unet, res)]
            mid = A.Add.apply(raw_mid_unet, mid_res)
        ups = [mid] if collect_up else None
        img = _up_out(unet, mid, skips, tu, ehs, dt, collect=ups)
    return img, raw_unet, raw_mid_unet, ups


def decoder_forward(dec, raw_mid_enc, raw_enc, ehs, t_attr, dt, raw_unet=None, raw_mid_unet=None, extras=None):
    """AttributeDecoderModel (controlnet.py:2342-2527): exchange skip_enc + conv1x1(skip_unet) (2446-2461, 2476-2477),
    up path on its own weights.  All NHWC; returns attr_pred [B,H,W,out_channels]."""
    B, dev = raw_mid_enc.shape[0], raw_mid_enc.device
    with Stage(dec, dt):
        td = _time(dec, t_attr, B, dt, dev)
        dskips = list(raw_enc)
        if raw_unet is not None:
            dskips = [A.linear(u, _w2(z, dt), z.bias, res=e) for u, e, z in zip(raw_unet, raw_enc, dec.control_down_blocks)]
        xd = A.linear(raw_mid_unet, _w2(dec.control_mid_block, dt), dec.control_mid_block.bias, res=raw_mid_enc)
        return _up_out(dec, xd, dskips, td, ehs, dt, extras=extras)


def dual_stream_forward(unet, enc, dec, x_t, cond, ehs, t_img, t_attr, dtype=torch.bfloat16, run_decoder: bool = True,
                        cond_nhwc: Optional[torch.Tensor] = None, cross_attention_kwargs=None) -> Dict[str, torch.Tensor]:
    """Differentiable dual-stream step (the call pattern of train.py:1324-1354): NCHW inputs, NHWC predictions
    ``img_pred`` [B,H,W,4] / ``attr_pred`` [B,H,W,28] in the compute dtype.  ``cond_nhwc`` ([B,H,W,28], compute dtype,
    may require grad) replaces ``cond``: the cycle-consistency pass feeds the decoder's own prediction back in.
    ``cross_attention_kwargs``: ``{"scale": s}``, the scale of the UNet's trainable LoRA adapter (lora.py)."""
    from .lora import scale_of

    B = x_t.shape[0]
    dt = dtype
    ehs = _prompt(ehs, B, dt)
    if cond_nhwc is not None:
        cin = torch.nn.functional.pad(cond_nhwc, (0, CIN_PAD - cond_nhwc.shape[-1])).contiguous()
    else:
        cin = ops.to_nhwc(cond, dt, CIN_PAD)
    res, mid_res, raw_enc, raw_mid_enc = encoder_forward(enc, cin, ehs, t_attr, dt)
    img, raw_unet, raw_mid_unet, _ = unet_forward(unet, ops.to_nhwc(x_t, dt, CIN_PAD), ehs, t_img, dt, res, mid_res,
                                                  lora_scale=scale_of(cross_attention_kwargs))
    out = {"img_pred": img}
    if run_decoder:
        out["attr_pred"] = decoder_forward(dec, raw_mid_enc, raw_enc, ehs, t_attr, dt, raw_unet, raw_mid_unet)
    return out
