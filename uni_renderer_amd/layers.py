"""L0 leaves of the hot path, MI355X-native.

The reference imports these from diffusers 0.24 (models/unet_2d_blocks.py:24-28, models/controlnet.py:24-34):
``ResnetBlock2D``, ``Transformer2DModel`` (-> ``BasicTransformerBlock`` -> ``Attention`` / ``FeedForward``),
``Downsample2D``, ``Upsample2D``, ``Timesteps``, ``TimestepEmbedding``.  Here each class is

  * a parameter holder whose ``state_dict`` keys and shapes are the diffusers ones (so SD-1.x /
    Uni-Renderer checkpoints load unchanged), and
  * a ``forward`` over NHWC tensors that only enqueues HIP kernels through ``ops`` (C ABI).  There is no
    PyTorch arithmetic on this path; parameter holders raise if someone calls their torch ``forward``.

Weights are re-laid-out ("packed") once per (dtype, parameter version) into the layouts the kernels read:
conv3x3 -> [Cout, (ky,kx,Cin)], q|k fused, GEGLU value/gate interleaved in groups of 4 columns.
"""
from __future__ import annotations

import math
from typing import Optional

import torch
import torch.nn as nn

from . import ops

_HOLDER_MSG = ("this nn.Module only holds parameters for the HIP path; its torch forward is disabled "
               "(no PyTorch fallback in uni_renderer_amd)")


class Conv2d(nn.Conv2d):
    def forward(self, *a, **k):  # pragma: no cover
        raise RuntimeError(_HOLDER_MSG)


class Linear(nn.Linear):
    def forward(self, *a, **k):  # pragma: no cover
        raise RuntimeError(_HOLDER_MSG)


class GroupNorm(nn.GroupNorm):
    def forward(self, *a, **k):  # pragma: no cover
        raise RuntimeError(_HOLDER_MSG)


class LayerNorm(nn.LayerNorm):
    def forward(self, *a, **k):  # pragma: no cover
        raise RuntimeError(_HOLDER_MSG)


def _ceil(v: int, m: int) -> int:
    return (v + m - 1) // m * m


LOG2E = 1.4426950408889634


def pack_conv3x3(weight: torch.Tensor, dtype, cin_pad: Optional[int] = None, cblock: int = 0) -> torch.Tensor:
    """[Co, Ci, 3, 3] -> [Co, 9 * Ci_pad] with k = (ky*3 + kx) * Ci_pad + c (zero padded channels), or with
    ``cblock`` > 0 in the block-outer order k = (c // cblock) * 9 * cblock + (ky*3 + kx) * cblock + c % cblock
    (``ops.conv_cblock``; the launch must pass the same ``cblock``)."""
    co, ci = weight.shape[:2]
    cp = ci if cin_pad is None else cin_pad
    w = weight.detach().permute(0, 2, 3, 1)  # [Co, ky, kx, Ci]
    if cp != ci:
        w = torch.nn.functional.pad(w, (0, cp - ci))
    if cblock:
        w = w.reshape(co, 9, cp // cblock, cblock).permute(0, 2, 1, 3)  # [Co, block, tap, c]
    return w.reshape(co, 9 * cp).to(dtype).contiguous()


def pack_matrix(weight: torch.Tensor, dtype) -> torch.Tensor:
    """Linear [N, K] or 1x1 conv [N, K, 1, 1] -> [N, K]."""
    return weight.detach().reshape(weight.shape[0], -1).to(dtype).contiguous()


def geglu_perm(n_half: int, device) -> torch.Tensor:
    """Row order the GEGLU epilogue expects: packed row p -> value row (p//8)*4 + p%4 if p%8 < 4 else the
    matching gate row (include/ur_kernels.h, UR_ACT_GEGLU)."""
    p = torch.arange(2 * n_half, device=device)
    col = (p // 8) * 4 + (p % 4)
    return torch.where((p % 8) < 4, col, n_half + col)


def f32(t: torch.Tensor) -> torch.Tensor:
    return t.detach().float().contiguous()


def pack_cond_conv3x3(weight: torch.Tensor, dtype, stride: int = 1, image: bool = False, bgr: bool = False) -> torch.Tensor:
    """[Co, Ci, 3, 3] -> the weight image ``ops.cond_conv3x3`` reads (include/ur_kernels.h, ur_cond_conv3x3):
    [Co / 16][Cp / CC][STEPS][64 lanes][8] with CC = ``ops.cond_conv_kchunk(Ci, stride, image)``, Cp = Ci rounded up to
    CC, STEPS = ceil(9 * CC / 32); element j of lane l of step s holds k = 32 s + 8 (l // 16) + j = tap * CC + c of output
    channel 16 nb + l % 16, zero where tap >= 9 or the channel is padding.  ``bgr``: the input-channel axis is flipped
    here, so the kernel reads a BGR image as it lies in memory."""
    co, ci = weight.shape[:2]
    cc = ops.cond_conv_kchunk(ci, stride, image)
    cp = _ceil(ci, cc)
    steps = _ceil(9 * cc, 32) // 32
    if co % 16:
        raise ValueError("pack_cond_conv3x3: output channels are a multiple of 16")
    w = weight.detach()
    if bgr:
        w = w.flip(1)
    w = torch.nn.functional.pad(w.permute(0, 2, 3, 1).reshape(co, 9, ci), (0, cp - ci))  # [Co, tap, Cp]
    w = w.reshape(co, 9, cp // cc, cc).permute(0, 2, 1, 3).reshape(co, cp // cc, 9 * cc)  # k = tap * CC + c per chunk
    w = torch.nn.functional.pad(w, (0, steps * 32 - 9 * cc))
    w = w.reshape(co // 16, 16, cp // cc, steps, 4, 8).permute(0, 2, 3, 4, 1, 5)            # lane = 16 * (k // 8 % 4) + n
    return w.to(dtype).contiguous()


def pack_cond_conv3x3_rot(weight: torch.Tensor, dtype) -> torch.Tensor:
    """[Co, Ci, 3, 3] -> the ``w_rot`` image ``ops.cond_conv3x3_dgrad`` reads (include/ur_kernels.h, ur_cond_conv3x3_dgrad): the
    rotated, channel-transposed weights W_rot[c][n][ky][kx] = W[n][c][2 - ky][2 - kx] in the forward's image of a stride-1
    layer with Co input and Ci output channels."""
    if weight.shape[0] % 16 or weight.shape[1] % 16:
        raise ValueError("pack_cond_conv3x3_rot: channels are multiples of 16 (the image-mode layer has no input gradient)")
    return pack_cond_conv3x3(weight.detach().flip(2, 3).transpose(0, 1), dtype, 1)


from . import packs as R  # noqa: E402 -- the recipes build on the primitives above
from .packs import PackCache, one  # noqa: E402,F401 -- PackCache is imported from here by its other users


class Ctx:
    """Per-forward context handed down the module tree."""

    __slots__ = ("dtype", "temb", "ehs", "B", "kc", "vtc", "ip")

    def __init__(self, dtype, B):
        self.dtype = dtype
        self.B = B
        self.temb = None  # [B, sum(Cout of all resnets)] = time_emb_proj(silu(emb)) of every resnet, batched
        self.ehs = None   # [B, 77, cross_dim] tokens in compute dtype
        self.kc = None    # [B, 77, sum(C)]   to_k(ehs) of every cross-attention of the network, one GEMM
        self.vtc = None   # [B, sum(C), 128]  to_v(ehs)^T of every cross-attention, one GEMM
        self.ip = None    # ip_adapter.IpContext: image K | V of every cross-attention of a UNet with an IP-Adapter, one GEMM


# ---------------------------------------------------------------------------------------------------
class TimestepEmbedding(nn.Module):
    """diffusers TimestepEmbedding (ctor controlnet.py:289-295): linear_1 -> SiLU -> linear_2."""

    def __init__(self, in_channels: int, time_embed_dim: int):
        super().__init__()
        self.linear_1 = Linear(in_channels, time_embed_dim)
        self.linear_2 = Linear(time_embed_dim, time_embed_dim)
        self._pk = PackCache()

    def forward(self, t_emb: torch.Tensor, silu_out: bool = True) -> torch.Tensor:
        """Returns SiLU(emb) when ``silu_out`` (every consumer of emb in this config is a resnet's
        ``time_emb_proj(SiLU(emb))``), computed in the GEMM epilogues."""
        dt = t_emb.dtype
        w1, b1 = one(self._pk, R.linear, self.linear_1, dt)
        w2, b2 = one(self._pk, R.linear, self.linear_2, dt)
        h = ops.linear(t_emb, w1, b1, act=ops.ACT_SILU)
        return ops.linear(h, w2, b2, act=ops.ACT_SILU if silu_out else ops.ACT_NONE)


class ResnetBlock2D(nn.Module):
    """GN+SiLU -> conv3x3 (+bias +temb) -> GN+SiLU -> conv3x3 (+bias, + shortcut(x), / output_scale_factor).
    ctor args as at unet_2d_blocks.py:1100-1111; time_embedding_norm="default", dropout 0."""

    def __init__(self, in_channels, out_channels, temb_channels, groups=32, eps=1e-5, output_scale_factor=1.0):
        super().__init__()
        self.in_channels, self.out_channels = in_channels, out_channels
        self.groups, self.eps, self.output_scale_factor = groups, eps, output_scale_factor
        self.norm1 = GroupNorm(groups, in_channels, eps=eps, affine=True)
        self.conv1 = Conv2d(in_channels, out_channels, 3, padding=1)
        self.time_emb_proj = Linear(temb_channels, out_channels)
        self.norm2 = GroupNorm(groups, out_channels, eps=eps, affine=True)
        self.conv2 = Conv2d(out_channels, out_channels, 3, padding=1)
        self.conv_shortcut = Conv2d(in_channels, out_channels, 1) if in_channels != out_channels else None
        self.temb_slice = None  # (offset, offset + out_channels) into Ctx.temb, set by the owning network
        self._pk = PackCache()

    def forward(self, x, ctx: Ctx, x1=None, extra_res=None):
        """x (and optional x1, concatenated on channels) NHWC -> NHWC [B,H,W,out_channels]."""
        dt, pk = x.dtype, self._pk
        g1, b1 = one(pk, R.affine, self.norm1, dt)
        g2, b2 = one(pk, R.affine, self.norm2, dt)
        w1, cb1 = one(pk, R.conv3x3, self.conv1, dt)
        lo, hi = self.temb_slice
        h = ops.groupnorm(x, g1, b1, self.eps, x1=x1, groups=self.groups, silu=True)
        h = ops.conv3x3(h, w1, cb1, rowadd=ctx.temb[:, lo:hi], cblock=ops.conv_cblock(h.shape[-1]))
        h = ops.groupnorm(h, g2, b2, self.eps, groups=self.groups, silu=True)
        if self.conv_shortcut is not None and ops.FOLD_SHORTCUT and extra_res is None:
            # conv_shortcut rides in conv2's K loop as its 1x1 tail (ops.conv3x3 ``tail``)
            w2s, cb2s = one(pk, R.fold, self, dt)
            return ops.conv3x3(h, w2s, cb2s, tail=(x, x1), out_scale=1.0 / self.output_scale_factor, hilo=ops.PRECISE_RESIDUAL,
                               cblock=ops.conv_cblock(h.shape[-1]))
        if self.conv_shortcut is not None:
            ws, bs = one(pk, R.linear, self.conv_shortcut, dt)
            sc = ops.linear(x, ws, bs, x1=x1)
        else:
            if x1 is not None:
                raise RuntimeError("concat input requires a conv_shortcut (in_channels != out_channels)")
            sc = x
        w2, cb2 = one(pk, R.conv3x3, self.conv2, dt)
        return ops.conv3x3(h, w2, cb2, res=sc, out_scale=1.0 / self.output_scale_factor, hilo=ops.PRECISE_RESIDUAL,
                           cblock=ops.conv_cblock(h.shape[-1]))


class Attention(nn.Module):
    """diffusers Attention / AttnProcessor2_0: q,k,v without bias; softmax(QK^T/sqrt(d))V; out proj + bias."""

    def __init__(self, query_dim, heads, dim_head, cross_attention_dim=None):
        super().__init__()
        inner = heads * dim_head
        self.heads, self.dim_head, self.inner = heads, dim_head, inner
        self.is_cross = cross_attention_dim is not None
        kv = cross_attention_dim if self.is_cross else query_dim
        self.to_q = Linear(query_dim, inner, bias=False)
        self.to_k = Linear(kv, inner, bias=False)
        self.to_v = Linear(kv, inner, bias=False)
        self.to_out = nn.ModuleList([Linear(inner, query_dim), nn.Dropout(0.0)])
        self.kv_slice = None  # rows of the network-wide batched K / V^T projection (cross-attention only)
        self._pk = PackCache()

    def forward(self, xn, ctx: Ctx, residual):
        """xn: normalised tokens [B,T,C]; returns residual + to_out(attention)."""
        dt, pk = xn.dtype, self._pk
        B, T, _ = xn.shape
        H, d, C = self.heads, self.dim_head, self.inner
        # The softmax scale and the change to base 2 are folded into the q (and, when q|k come from one GEMM, k)
        # projection epilogues in fp32 -- before the single rounding to fp16/bf16 -- so the attention kernel sees
        # scores in log2 units (ur_attention scale = 0) and spends no multiply-add per score.
        cs = d ** -0.5 * LOG2E
        wo, bo = one(pk, R.linear, self.to_out[0], dt)
        if self.is_cross and ctx.kc is not None and self.kv_slice is not None:
            # K / V^T of the prompt were projected once for the whole network (controlnet._begin)
            lo, hi = self.kv_slice
            wq = one(pk, R.matrix, self.to_q, dt)
            q = ops.linear(xn, wq, out_scale=cs)
            o = ops.attention(q, ctx.kc[:, :, lo:hi], ctx.vtc[:, lo:hi], B=B, H=H, Tq=T, Tk=ctx.kc.shape[1], d=d,
                              ldq=C, ldk=ctx.kc.stride(1), scale=0.0)
            self._ip_add(o, q, ctx, B, T)
            return ops.linear(o, wo, bo, res=residual, hilo=ops.PRECISE_RESIDUAL)
        wv = one(pk, R.matrix, self.to_v, dt)
        if not self.is_cross:
            wqk = one(pk, R.matrix_rows, (self.to_q, self.to_k), dt)
            qk = ops.linear(xn, wqk, out_scale=math.sqrt(cs))  # [B,T,2C] = q | k, each carrying sqrt(cs)
            vt = ops.vt_proj(xn, wv)                       # [B,C,Tpad]
            o = ops.attention(qk, qk, vt, B=B, H=H, Tq=T, Tk=T, d=d, ldq=2 * C, ldk=2 * C, q_off=0, k_off=C, scale=0.0)
        else:
            wq = one(pk, R.matrix, self.to_q, dt)
            wk = one(pk, R.matrix, self.to_k, dt)
            ehs = ctx.ehs
            Tk = ehs.shape[1]
            q = ops.linear(xn, wq, out_scale=cs)
            k = ops.linear(ehs, wk)                        # [B,Tk,C]
            vt = ops.vt_proj(ehs, wv)                      # [B,C,ceil64(Tk)]
            o = ops.attention(q, k, vt, B=B, H=H, Tq=T, Tk=Tk, d=d, ldq=C, ldk=C, scale=0.0)
            self._ip_add(o, q, ctx, B, T)
        return ops.linear(o, wo, bo, res=residual, hilo=ops.PRECISE_RESIDUAL)

    def _ip_add(self, o, q, ctx: Ctx, B, T):
        """IP-Adapter's decoupled cross-attention: ``o += scale * softmax(q k_ip^T) v_ip`` over the image tokens, one launch
        behind the prompt's attention (``ctx.ip``: only a UNet with an adapter loaded has one)."""
        kv = ctx.ip.of(self) if ctx.ip is not None else None
        if kv is not None:
            ops.ip_attention_add(o, q, kv[0], kv[1], ctx.ip.scale, B=B, H=self.heads, T=T, d=self.dim_head, ldq=self.inner)


class GEGLU(nn.Module):
    def __init__(self, dim_in, dim_out):
        super().__init__()
        self.proj = Linear(dim_in, dim_out * 2)


class FeedForward(nn.Module):
    """net.0.proj (GEGLU, erf GELU) -> net.2; keys ``ff.net.0.proj.*`` / ``ff.net.2.*`` as in diffusers."""

    def __init__(self, dim, mult=4):
        super().__init__()
        self.net = nn.ModuleList([GEGLU(dim, dim * mult), nn.Dropout(0.0), Linear(dim * mult, dim)])
        self._pk = PackCache()

    def forward(self, xn, residual):
        dt, pk = xn.dtype, self._pk
        w_in, b_in = one(pk, R.geglu, self.net[0].proj, dt)
        w_out, b_out = one(pk, R.linear, self.net[2], dt)
        g = ops.linear(xn, w_in, b_in, act=ops.ACT_GEGLU)   # [B,T,4C]
        return ops.linear(g, w_out, b_out, res=residual, hilo=ops.PRECISE_RESIDUAL)


class BasicTransformerBlock(nn.Module):
    def __init__(self, dim, heads, dim_head, cross_attention_dim):
        super().__init__()
        self.norm1 = LayerNorm(dim, eps=1e-5)
        self.attn1 = Attention(dim, heads, dim_head)
        self.norm2 = LayerNorm(dim, eps=1e-5)
        self.attn2 = Attention(dim, heads, dim_head, cross_attention_dim=cross_attention_dim)
        self.norm3 = LayerNorm(dim, eps=1e-5)
        self.ff = FeedForward(dim)
        self._pk = PackCache()

    def forward(self, x, ctx: Ctx):
        dt = x.dtype
        g, b = one(self._pk, R.affine, self.norm1, dt)
        x = self.attn1(ops.layernorm(x, g, b, self.norm1.eps), ctx, x)
        g, b = one(self._pk, R.affine, self.norm2, dt)
        x = self.attn2(ops.layernorm(x, g, b, self.norm2.eps), ctx, x)
        g, b = one(self._pk, R.affine, self.norm3, dt)
        return self.ff(ops.layernorm(x, g, b, self.norm3.eps), x)


class Transformer2DModel(nn.Module):
    """GN(32, eps 1e-6) -> 1x1 proj_in -> transformer block(s) -> 1x1 proj_out -> + input
    (ctor unet_2d_blocks.py:1115-1126; use_linear_projection=False).  NHWC makes the NCHW<->token
    permutes of the reference disappear: [B,H,W,C] *is* [B,HW,C]."""

    def __init__(self, heads, dim_head, in_channels, cross_attention_dim, norm_num_groups=32, num_layers=1):
        super().__init__()
        inner = heads * dim_head
        self.groups = norm_num_groups
        self.norm = GroupNorm(norm_num_groups, in_channels, eps=1e-6, affine=True)
        self.proj_in = Conv2d(in_channels, inner, 1)
        self.transformer_blocks = nn.ModuleList(
            [BasicTransformerBlock(inner, heads, dim_head, cross_attention_dim) for _ in range(num_layers)])
        self.proj_out = Conv2d(inner, in_channels, 1)
        self._pk = PackCache()

    def forward(self, x, ctx: Ctx):
        dt, pk = x.dtype, self._pk
        B, H, W, Cc = x.shape
        g, b = one(pk, R.affine, self.norm, dt)
        wi, bi = one(pk, R.linear, self.proj_in, dt)
        wo, bo = one(pk, R.linear, self.proj_out, dt)
        h = ops.groupnorm(x, g, b, self.norm.eps, groups=self.groups, silu=False)
        h = ops.linear(h.view(B, H * W, Cc), wi, bi, hilo=ops.PRECISE_RESIDUAL)
        for blk in self.transformer_blocks:
            h = blk(h, ctx)
        out = ops.linear(h, wo, bo, res=ops.view_hilo(x, B, H * W, Cc), hilo=ops.PRECISE_RESIDUAL)
        return ops.view_hilo(out, B, H, W, Cc)


class Downsample2D(nn.Module):
    """conv3x3 stride 2 pad 1 (ctor unet_2d_blocks.py:1143-1149); key ``downsamplers.0.conv``."""

    def __init__(self, channels, padding=1):
        super().__init__()
        if padding != 1:
            raise NotImplementedError("downsample_padding != 1")
        self.conv = Conv2d(channels, channels, 3, stride=2, padding=1)
        self._pk = PackCache()

    def forward(self, x):
        dt = x.dtype
        w, b = one(self._pk, R.conv3x3, self.conv, dt)
        return ops.conv3x3(x, w, b, stride=2, hilo=ops.PRECISE_RESIDUAL, cblock=ops.conv_cblock(x.shape[-1]))


class Upsample2D(nn.Module):
    """nearest x2 (F.interpolate) then conv3x3 (unet_2d_blocks.py:2501), fused into one gather-conv."""

    def __init__(self, channels):
        super().__init__()
        self.conv = Conv2d(channels, channels, 3, padding=1)
        self._pk = PackCache()

    def forward(self, x, output_size=None):
        dt = x.dtype
        w, b = one(self._pk, R.conv3x3, self.conv, dt)
        if output_size is not None and tuple(int(v) for v in output_size) != (2 * x.shape[1], 2 * x.shape[2]):
            # latent side not a multiple of 8 (controlnet.py:869-883, 1129-1130): F.interpolate(size=...), then the conv
            return ops.conv3x3(ops.resize_nearest(x, output_size), w, b, hilo=ops.PRECISE_RESIDUAL, cblock=ops.conv_cblock(x.shape[-1]))
        return ops.conv3x3(x, w, b, ups=True, hilo=ops.PRECISE_RESIDUAL, cblock=ops.conv_cblock(x.shape[-1]))


def zero_module(m: nn.Module) -> nn.Module:
    for p in m.parameters():
        nn.init.zeros_(p)
    return m


# ---------------------------------------------------------------------------------------------------
class ControlNetConditioningEmbedding(nn.Module):
    """diffusers' ``ControlNetConditioningEmbedding`` (reference models/controlnet.py, ``controlnet_cond_embedding``):
    conv_in, then per level a stride-1 and a stride-2 3x3 conv, SiLU after each, and a zero-initialised conv_out; parameter
    names ``conv_in``, ``blocks.0 ...``, ``conv_out`` as there.  ``forward`` takes the caller's NCHW image and runs the
    seven narrow convs as seven ``ops.cond_conv3x3`` launches; it returns the ``block_out_channels[-1]``-channel NHWC map,
    and the model that owns the embedding runs ``conv_out`` (whose result it needs as a residual operand)."""

    def __init__(self, conditioning_embedding_channels: int, conditioning_channels: int = 3,
                 block_out_channels=(16, 32, 96, 256)):
        super().__init__()
        boc = tuple(block_out_channels)
        if not 1 <= conditioning_channels <= 4 or any(c % 16 or c > 256 for c in boc):
            raise NotImplementedError("conditioning embedding: 1-4 image channels and widths that are multiples of 16 up to 256")
        self.conv_in = Conv2d(conditioning_channels, boc[0], 3, padding=1)
        self.blocks = nn.ModuleList()
        for i in range(len(boc) - 1):
            self.blocks.append(Conv2d(boc[i], boc[i], 3, padding=1))
            self.blocks.append(Conv2d(boc[i], boc[i + 1], 3, padding=1, stride=2))
        self.conv_out = zero_module(Conv2d(boc[-1], conditioning_embedding_channels, 3, padding=1))
        self._pk = PackCache()

    def forward(self, cond_nchw: torch.Tensor, dtype, bgr: bool = False) -> torch.Tensor:
        if cond_nchw.dtype not in ops.DT_ANY or not cond_nchw.is_contiguous():
            cond_nchw = cond_nchw.float().contiguous()  # boundary plumbing for exotic inputs
        convs = [self.conv_in] + list(self.blocks)
        x = cond_nchw
        for i, conv in enumerate(convs):
            s, img = conv.stride[0], i == 0
            w, b = one(self._pk, R.cond_conv3x3(img, bgr), conv, dtype)
            x = ops.cond_conv3x3(x, w, b, n_out=conv.out_channels, stride=s, act=ops.ACT_SILU, dtype=dtype, image=img)
        return x

    def forward_autograd(self, cond_nchw: torch.Tensor, dtype, bgr: bool = False) -> torch.Tensor:
        """The same map under autograd: seven ``autograd_ops.CondConv3x3`` (forward kernel without activation; backward on the
        direct narrow-channel dgrad / wgrad kernels) with ``autograd_ops.SiLU`` between them -- SiLU and its derivative are
        elementwise passes of their own here, not conv epilogues.  The parameters enter the Functions themselves,
        so each ``weight.grad`` / ``bias.grad`` arrives once, in the parameter's shape and dtype; the packed images come from
        the module's cache, which follows the parameters' versions.  The image gets no gradient."""
        from . import autograd_ops as A

        if cond_nchw.requires_grad:
            raise NotImplementedError(COND_IMAGE_GRAD_MSG)
        if cond_nchw.dtype not in ops.DT_ANY or not cond_nchw.is_contiguous():
            cond_nchw = cond_nchw.float().contiguous()
        convs = [self.conv_in] + list(self.blocks)
        x = cond_nchw
        for i, conv in enumerate(convs):
            s, img = conv.stride[0], i == 0
            w, b = one(self._pk, R.cond_conv3x3(img, bgr), conv, dtype)
            w_rot = None if img or not x.requires_grad else one(self._pk, R.cond_conv3x3_rot, conv, dtype)
            x = A.SiLU.apply(A.CondConv3x3.apply(x, conv.weight, conv.bias, w, b, w_rot, s, img, bgr and img, dtype))
        return x


COND_IMAGE_GRAD_MSG = ("controlnet_cond requires a gradient, but the conditioning embedding's first layer has no input gradient on "
                       "the MI355X path (it reads the caller's image as it lies in memory): pass the image without requires_grad")
