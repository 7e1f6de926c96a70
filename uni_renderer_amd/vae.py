"""``AutoencoderKL`` (the SD-1.x VAE) on the same HIP kernels as the denoiser.

The reference encodes 8 images per training step (``vae.encode(x).latent_dist.sample() * vae.config.scaling_factor``,
train/train.py:1266-1304), 2 per sampling call (models/pipeline.py:2533-2538) and decodes 5 per inference
(``vae.decode(latents / scaling_factor, return_dict=False)[0]``, 2755-2769) with diffusers' ``AutoencoderKL``
(train.py:40, 953).  This module is that network -- same class name, ``encode`` / ``decode`` surface, ``config``,
diffusers ``state_dict`` key names (an SD-1.x ``vae/`` folder loads) -- with every layer running on ``ur_igemm`` (3x3
convs incl. the encoder's asymmetric-pad stride-2 downsample and the decoder's fused nearest-2x upsample, 1x1 convs,
the attention GEMMs), ``ur_groupnorm*`` and ``ur_softmax_rows``.  The single-head attention of the mid blocks has head
dim = 512 channels, outside the flash kernel's head dims, so it runs GEMM -> row softmax -> GEMM (the score matrix is
T x T = 32 MB per sample at 512x512, nothing next to 288 GB).  NHWC throughout; NCHW only at the two ends.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Tuple

import torch
import torch.nn as nn

from . import _lib, ops
from ._lib import check
from . import packs as R
from .layers import Conv2d, GroupNorm, Linear, PackCache
from .packs import one
from .modeling_utils import ConfigModelMixin, register_to_config

CIN_PAD = 64
_CONV_IN = R.conv3x3_padded(CIN_PAD)
_POST_QUANT = R.linear_padded(CIN_PAD)  # 1x1 over the (zero padded) latent channels


@dataclass(frozen=True)
class TileAxis:
    """One axis of a tile grid: per tile its start and length on the input, its length on the output, the extent of the
    blend with its predecessor (0 for the first tile) and how much of it is kept; ``blend`` / ``limit`` as diffusers names
    them (``blend_extent`` / ``row_limit``)."""
    positions: Tuple[int, ...]
    lengths: Tuple[int, ...]
    out_lengths: Tuple[int, ...]
    extents: Tuple[int, ...]
    kept: Tuple[int, ...]
    blend: int
    limit: int


def tile_axis(length: int, tile_in: int, tile_out: int, factor: float, out_len) -> TileAxis:
    """The tiles diffusers 0.24 cuts along one axis of ``length`` (pure Python, no device): tiles of ``tile_in`` starting
    every ``overlap = int(tile_in * (1 - factor))``, each ``out_len(n)`` long on the output side, blended over ``blend =
    int(tile_out * factor)`` and cropped to ``limit = tile_out - blend``.  ``tiled_decode``: ``tile_in`` = the latent tile,
    ``tile_out`` = the sample tile, ``out_len`` = times the scale; ``tiled_encode`` is the mirror image (steps in pixels,
    blends in latents).  The fused stitch evaluates the sequential in-place blends as a closed form over the raw tiles,
    which holds while a tile's own blends stay clear of what it hands to its successor: ``NotImplementedError`` for a
    factor above 1/3 or a tile with a successor shorter than ``2 * blend``."""
    if not 0.0 <= factor <= 1.0 / 3.0:
        raise NotImplementedError(f"tile_overlap_factor = {factor}: the fused tile stitch supports 0 <= factor <= 1/3 (diffusers' default: 0.25)")
    overlap, blend = int(tile_in * (1 - factor)), int(tile_out * factor)
    limit = tile_out - blend
    if length < 1 or overlap < 1 or limit < 1:
        raise ValueError(f"tile_axis: nothing to cut (length {length}, tile {tile_in} -> {tile_out}, factor {factor})")
    positions = tuple(range(0, length, overlap))
    lengths = tuple(min(tile_in, length - p) for p in positions)
    out_lengths = tuple(out_len(n) for n in lengths)
    if min(out_lengths) < 1:
        raise ValueError(f"tile_axis: a tile of {lengths[out_lengths.index(min(out_lengths))]} has no output (length {length}, tile {tile_in})")
    if blend > 0 and any(n < 2 * blend for n in out_lengths[:-1]):
        raise NotImplementedError(f"tile_axis: a tile with a successor is shorter than 2 * blend = {2 * blend} (output lengths {out_lengths})")
    extents = (0,) + tuple(min(a, b, blend) for a, b in zip(out_lengths, out_lengths[1:]))
    return TileAxis(positions, lengths, out_lengths, extents, tuple(min(limit, n) for n in out_lengths), blend, limit)


class _Resnet(nn.Module):
    """diffusers ResnetBlock2D with ``temb_channels=None`` (no time embedding), eps 1e-6."""

    def __init__(self, cin, cout, groups, eps=1e-6):
        super().__init__()
        self.groups, self.eps = groups, eps
        self.norm1 = GroupNorm(groups, cin, eps=eps)
        self.conv1 = Conv2d(cin, cout, 3, padding=1)
        self.norm2 = GroupNorm(groups, cout, eps=eps)
        self.conv2 = Conv2d(cout, cout, 3, padding=1)
        self.conv_shortcut = Conv2d(cin, cout, 1) if cin != cout else None
        self._pk = PackCache()

    def forward(self, x):
        dt, pk = x.dtype, self._pk
        g1, b1 = one(pk, R.affine, self.norm1, dt)
        g2, b2 = one(pk, R.affine, self.norm2, dt)
        w1, c1 = one(pk, R.conv3x3_tap, self.conv1, dt)
        h = ops.groupnorm(x, g1, b1, self.eps, groups=self.groups, silu=True)
        h = ops.conv3x3(h, w1, c1)
        h = ops.groupnorm(h, g2, b2, self.eps, groups=self.groups, silu=True)
        if self.conv_shortcut is not None:  # 1x1 shortcut rides in conv2's K loop (ur_igemm_desc.t0)
            w2, c2 = one(pk, R.fold_tap, self, dt)
            return ops.conv3x3(h, w2, c2, tail=(x, None))
        w2, c2 = one(pk, R.conv3x3_tap, self.conv2, dt)
        return ops.conv3x3(h, w2, c2, res=x)


class _Attention(nn.Module):
    """diffusers ``Attention(heads=1, dim_head=C, bias=True, residual_connection=True, norm_num_groups=32, eps=1e-6)``
    of ``UNetMidBlock2D``: GN -> q, k, v (Linear + bias) -> softmax(q k^T / sqrt(C)) v -> to_out -> + input."""

    def __init__(self, c, groups, eps=1e-6):
        super().__init__()
        self.c, self.groups, self.eps = c, groups, eps
        self.group_norm = GroupNorm(groups, c, eps=eps)
        self.to_q, self.to_k, self.to_v = Linear(c, c), Linear(c, c), Linear(c, c)
        self.to_out = nn.ModuleList([Linear(c, c), nn.Dropout(0.0)])
        self._pk = PackCache()

    def forward(self, x):
        dt, pk, C = x.dtype, self._pk, self.c
        B, H, W, _ = x.shape
        T = H * W
        Tp = (T + 63) // 64 * 64
        g, b = one(pk, R.affine, self.group_norm, dt)
        wqk, bqk = one(pk, R.linear_rows, (self.to_q, self.to_k), dt)
        wv, bv = one(pk, R.linear, self.to_v, dt)
        wo, bo = one(pk, R.linear, self.to_out[0], dt)
        xn = ops.groupnorm(x, g, b, self.eps, groups=self.groups, silu=False).view(B, T, C)
        qk = ops.linear(xn, wqk, bqk)                      # [B, T, 2C] = q | k
        vt = ops.vt_proj(xn, wv)                           # [B, C, Tp] = (x Wv^T)^T without the bias (added below)
        # scores: one GEMM per sample (z = B), q rows x k rows, scaled in the epilogue; rows padded to Tp columns
        P = torch.empty(B, T, Tp, dtype=dt, device=x.device)
        ops.igemm(x0=qk, w=qk[..., C:], out=P, M=T, N=T, K=C, c0=C, ldx0=2 * C, ldw=2 * C, ldc=Tp, n_store=Tp,
                  out_scale=C ** -0.5, zbatch=B, zx=T * 2 * C, zw=T * 2 * C, zout=T * Tp)
        check(_lib.load().ur_softmax_rows(P.data_ptr(), Tp, B * T, T, ops.DT[dt], ops._stream()), "ur_softmax_rows")
        # o = P v: rows of P sum to one, so the value bias is a plain column bias of this GEMM
        o = torch.empty(B, T, C, dtype=dt, device=x.device)
        ops.igemm(x0=P, w=vt, out=o, M=T, N=C, K=Tp, c0=Tp, ldx0=Tp, ldw=vt.stride(1), ldc=C, bias=bv, zbatch=B,
                  zx=T * Tp, zw=vt.stride(0), zout=T * C)
        return ops.linear(o, wo, bo, res=x.view(B, T, C)).view(B, H, W, C)


class _Mid(nn.Module):
    def __init__(self, c, groups):
        super().__init__()
        self.resnets = nn.ModuleList([_Resnet(c, c, groups), _Resnet(c, c, groups)])
        self.attentions = nn.ModuleList([_Attention(c, groups)])

    def forward(self, x):
        return self.resnets[1](self.attentions[0](self.resnets[0](x)))


class _Down(nn.Module):
    """encoder Downsample2D: F.pad(x, (0, 1, 0, 1)) + conv3x3 stride 2 padding 0 = ``ur_igemm`` with ``pad = 0``."""

    def __init__(self, c):
        super().__init__()
        self.conv = Conv2d(c, c, 3, stride=2, padding=0)
        self._pk = PackCache()

    def forward(self, x):
        dt = x.dtype
        w, b = one(self._pk, R.conv3x3_tap, self.conv, dt)
        return ops.conv3x3(x, w, b, stride=2, pad=0)


class _Up(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.conv = Conv2d(c, c, 3, padding=1)
        self._pk = PackCache()

    def forward(self, x):
        dt = x.dtype
        w, b = one(self._pk, R.conv3x3_tap, self.conv, dt)
        return ops.conv3x3(x, w, b, ups=True)  # nearest-2x fused into the gather


class _Level(nn.Module):
    def __init__(self, cin, cout, n, groups, down=False, up=False):
        super().__init__()
        self.resnets = nn.ModuleList([_Resnet(cin if i == 0 else cout, cout, groups) for i in range(n)])
        self.downsamplers = nn.ModuleList([_Down(cout)]) if down else None
        self.upsamplers = nn.ModuleList([_Up(cout)]) if up else None

    def forward(self, x):
        for r in self.resnets:
            x = r(x)
        if self.downsamplers is not None:
            x = self.downsamplers[0](x)
        if self.upsamplers is not None:
            x = self.upsamplers[0](x)
        return x


class Encoder(nn.Module):
    def __init__(self, in_channels, latent_channels, boc, layers, groups):
        super().__init__()
        self.conv_in = Conv2d(in_channels, boc[0], 3, padding=1)
        self.down_blocks = nn.ModuleList()
        c = boc[0]
        for i, co in enumerate(boc):
            self.down_blocks.append(_Level(c, co, layers, groups, down=i != len(boc) - 1))
            c = co
        self.mid_block = _Mid(c, groups)
        self.conv_norm_out = GroupNorm(groups, c, eps=1e-6)
        self.conv_out = Conv2d(c, 2 * latent_channels, 3, padding=1)


class Decoder(nn.Module):
    def __init__(self, out_channels, latent_channels, boc, layers, groups):
        super().__init__()
        rev = list(reversed(boc))
        self.conv_in = Conv2d(latent_channels, rev[0], 3, padding=1)
        self.mid_block = _Mid(rev[0], groups)
        self.up_blocks = nn.ModuleList()
        c = rev[0]
        for i, co in enumerate(rev):
            self.up_blocks.append(_Level(c, co, layers + 1, groups, up=i != len(boc) - 1))
            c = co
        self.conv_norm_out = GroupNorm(groups, c, eps=1e-6)
        self.conv_out = Conv2d(c, out_channels, 3, padding=1)


class DiagonalGaussianDistribution:
    """diffusers' posterior object: ``parameters`` [B, 2C, h, w] = mean | logvar (clamped to [-30, 20])."""

    def __init__(self, parameters: torch.Tensor):
        self.parameters = parameters
        self.mean, logvar = torch.chunk(parameters, 2, dim=1)
        self.logvar = torch.clamp(logvar, -30.0, 20.0)
        self.std = torch.exp(0.5 * self.logvar)
        self.var = torch.exp(self.logvar)

    def sample(self, generator: Optional[torch.Generator] = None) -> torch.Tensor:
        noise = torch.randn(self.mean.shape, generator=generator, device=self.mean.device, dtype=self.mean.dtype)
        return self.mean + self.std * noise

    def mode(self) -> torch.Tensor:
        return self.mean


@dataclass
class AutoencoderKLOutput:
    latent_dist: DiagonalGaussianDistribution


@dataclass
class DecoderOutput:
    sample: torch.Tensor


class AutoencoderKL(ConfigModelMixin, nn.Module):
    @register_to_config
    def __init__(self, in_channels: int = 3, out_channels: int = 3,
                 down_block_types: Tuple[str, ...] = ("DownEncoderBlock2D",) * 4,
                 up_block_types: Tuple[str, ...] = ("UpDecoderBlock2D",) * 4,
                 block_out_channels: Tuple[int, ...] = (128, 256, 512, 512), layers_per_block: int = 2, act_fn: str = "silu",
                 latent_channels: int = 4, norm_num_groups: int = 32, sample_size: int = 512,
                 scaling_factor: float = 0.18215, force_upcast: bool = True):
        super().__init__()
        boc = tuple(block_out_channels)
        if (act_fn != "silu" or any(t != "DownEncoderBlock2D" for t in down_block_types[:len(boc)])
                or any(t != "UpDecoderBlock2D" for t in up_block_types[:len(boc)])):
            raise NotImplementedError("AutoencoderKL: only the SD-1.x encoder / decoder block types are implemented")
        if any(c % 64 for c in boc):
            raise NotImplementedError("AutoencoderKL: block_out_channels must be multiples of 64 (ur_igemm K granularity)")
        self.encoder = Encoder(in_channels, latent_channels, boc, layers_per_block, norm_num_groups)
        self.decoder = Decoder(out_channels, latent_channels, boc, layers_per_block, norm_num_groups)
        self.quant_conv = Conv2d(2 * latent_channels, 2 * latent_channels, 1)
        self.post_quant_conv = Conv2d(latent_channels, latent_channels, 1)
        self.compute_dtype: Optional[torch.dtype] = None
        self._pk = PackCache()
        # diffusers' tiling / slicing state, with its definitions (AutoencoderKL.__init__)
        self.use_slicing = False
        self.use_tiling = False
        self.tile_sample_min_size = sample_size[0] if isinstance(sample_size, (list, tuple)) else sample_size
        self.tile_latent_min_size = int(self.tile_sample_min_size / (2 ** (len(boc) - 1)))
        self.tile_overlap_factor = 0.25

    _DEPRECATED_ATTN = {"query": "to_q", "key": "to_k", "value": "to_v", "proj_attn": "to_out.0"}

    @classmethod
    def _convert_state_dict(cls, sd):
        """The ``vae/`` folders of SD 1.4 (the base the reference trains from), 1.5 and 2.x store the mid-block
        attention under the deprecated names ``query / key / value / proj_attn``; diffusers renames them while loading
        (``ModelMixin._convert_deprecated_attention_blocks``).  Same conversion here, plus the 1x1-conv weight shape
        ``[C, C, 1, 1]`` of still older exports."""
        out = {}
        for k, v in sd.items():
            parts = k.split(".")
            if len(parts) >= 4 and parts[-2] in cls._DEPRECATED_ATTN and "attentions" in parts:
                k = ".".join(parts[:-2] + [cls._DEPRECATED_ATTN[parts[-2]], parts[-1]])
                if parts[-1] == "weight" and v.dim() == 4 and v.shape[2:] == (1, 1):
                    v = v[:, :, 0, 0].contiguous()
            out[k] = v
        return out

    def _dt(self):
        dt = self.compute_dtype or self.dtype
        if dt not in (torch.float16, torch.bfloat16):
            if torch.is_autocast_enabled():
                return torch.get_autocast_dtype("cuda")
            raise RuntimeError("the MI355X path computes in fp16/bf16: cast the VAE (.to(torch.float16)), run under "
                               "torch.autocast, or set vae.compute_dtype")
        return dt

    @staticmethod
    def _io_dtype(t: torch.Tensor) -> torch.dtype:
        return t.dtype if t.dtype in (torch.float16, torch.bfloat16, torch.float32) else torch.float32

    # ---- tiling and slicing (diffusers AutoencoderKL.enable_tiling / enable_slicing; pipeline.py:185-215) -----------
    def enable_tiling(self, use_tiling: bool = True):
        """Inputs larger than ``tile_sample_min_size`` (``encode``) / ``tile_latent_min_size`` (``decode``) are processed
        as overlapping tiles stitched by one ``ur_blend_tiles`` launch.  The result differs from the plain path the way
        diffusers' does: every tile has its own GroupNorm statistics and mid-block attention.  Not supported:
        ``tile_overlap_factor`` above 1/3 (``NotImplementedError``), graph capture and autograd of the tiled paths, and
        ``blend_v`` / ``blend_h`` as methods.  Tiles of one shape run as one batch, so peak memory is that of the plain
        path (profiles/vae_tiling_ab.txt)."""
        self.use_tiling = use_tiling

    def disable_tiling(self):
        self.enable_tiling(False)

    def enable_slicing(self):
        """Batches are encoded / decoded one sample at a time and concatenated."""
        self.use_slicing = True

    def disable_slicing(self):
        self.use_slicing = False

    def _latent_len(self, n: int) -> int:
        """Latent length of ``n`` pixels: one (0, 1)-padded stride-2 3x3 conv per encoder level but the last."""
        for _ in range(len(self.config.block_out_channels) - 1):
            n = (n - 2) // 2 + 1
        return n

    def _tile_axes(self, height: int, width: int, decode: bool):
        scale = 2 ** (len(self.config.block_out_channels) - 1)
        if decode:
            tin, tout, out_len = self.tile_latent_min_size, self.tile_sample_min_size, lambda n: n * scale
        else:
            tin, tout, out_len = self.tile_sample_min_size, self.tile_latent_min_size, self._latent_len
        return tuple(tile_axis(n, tin, tout, self.tile_overlap_factor, out_len) for n in (height, width))

    def _tiled(self, x: torch.Tensor, decode: bool) -> torch.Tensor:
        """The network over the tiles of NCHW ``x`` and the stitch: one ``ur_blend_tiles`` launch."""
        tiles, blend, limit = self._network_tiles(x, decode)
        return ops.blend_tiles(tiles, blend, limit, self._io_dtype(x))

    def _network_tiles(self, x: torch.Tensor, decode: bool):
        """``(tiles, blend, limit)``: the NHWC network outputs ``tiles[i][j]`` of the tile grid over NCHW ``x``.  Tiles of one
        shape run as ONE batch, tile-major, the way ``num_images_per_prompt`` folds repeats (a 1024 x 1024 decode: four
        network calls for 4 + 2 + 2 + 1 tiles), so a tile is a slice along the batch of its group's output."""
        net = self._decode_nhwc if decode else self._encode_nhwc
        B = x.shape[0]
        ay, ax = self._tile_axes(x.shape[2], x.shape[3], decode)
        groups = {}
        for i, (py, ly) in enumerate(zip(ay.positions, ay.lengths)):
            for j, (px, lx) in enumerate(zip(ax.positions, ax.lengths)):
                groups.setdefault((ly, lx), []).append((i, j, py, px))
        tiles = [[None] * len(ax.positions) for _ in ay.positions]
        for (ly, lx), members in groups.items():
            views = [x[:, :, py:py + ly, px:px + lx] for _, _, py, px in members]
            y = net(views[0] if len(views) == 1 else torch.cat(views, 0))
            for k, (i, j, _, _) in enumerate(members):
                tiles[i][j] = y[k * B:(k + 1) * B]
        return tiles, ay.blend, ay.limit

    @torch.no_grad()
    def tiled_encode(self, x: torch.Tensor, return_dict: bool = True):
        """diffusers 0.24 ``tiled_encode``: tiles of ``tile_sample_min_size`` pixels stepping by ``int(tile_sample_min_size *
        (1 - tile_overlap_factor))``, their 8-channel moments blended over ``int(tile_latent_min_size * tile_overlap_factor)``
        latents; the posterior is built from the blended moments."""
        post = DiagonalGaussianDistribution(self._tiled(x, False))
        return AutoencoderKLOutput(latent_dist=post) if return_dict else (post,)

    @torch.no_grad()
    def tiled_decode(self, z: torch.Tensor, return_dict: bool = True):
        """diffusers 0.24 ``tiled_decode``: tiles of ``tile_latent_min_size`` latents stepping by ``int(tile_latent_min_size *
        (1 - tile_overlap_factor))``, the decoded images blended over ``int(tile_sample_min_size * tile_overlap_factor)``
        pixels."""
        img = self._tiled(z, True)
        return DecoderOutput(sample=img) if return_dict else (img,)

    # ---- encode (train.py:1266-1304; pipeline.py:2533-2538) ---------------------------------------------------------
    @torch.no_grad()
    def encode(self, x: torch.Tensor, return_dict: bool = True):
        if self.use_tiling and (x.shape[-1] > self.tile_sample_min_size or x.shape[-2] > self.tile_sample_min_size):
            return self.tiled_encode(x, return_dict=return_dict)
        dt = self._io_dtype(x)
        if self.use_slicing and x.shape[0] > 1:
            moments = torch.cat([ops.to_nchw(self._encode_nhwc(s), dt) for s in x.split(1)])
        else:
            moments = ops.to_nchw(self._encode_nhwc(x), dt)
        post = DiagonalGaussianDistribution(moments)
        return AutoencoderKLOutput(latent_dist=post) if return_dict else (post,)

    def _encode_nhwc(self, x: torch.Tensor) -> torch.Tensor:
        """The posterior moments of NCHW ``x`` as the network leaves them: NHWC ``[B, h, w, 2 * latent_channels]``."""
        dt, pk, e = self._dt(), self._pk, self.encoder
        w, b = one(pk, _CONV_IN, e.conv_in, dt)
        h = ops.conv3x3(ops.to_nhwc(x, dt, CIN_PAD), w, b)
        for lvl in e.down_blocks:
            h = lvl(h)
        h = e.mid_block(h)
        g, gb = one(pk, R.affine, e.conv_norm_out, dt)
        h = ops.groupnorm(h, g, gb, e.conv_norm_out.eps, groups=e.conv_norm_out.num_groups, silu=True)
        # quant_conv (1x1, per pixel) composed with conv_out on the host in fp32 (packs.vae_moments)
        q = self.quant_conv
        wc, bc = one(pk, R.vae_moments, self, dt)
        return ops.conv3x3(h, wc, bc, n_out=q.weight.shape[0])

    # ---- decode (pipeline.py:2755-2769) -----------------------------------------------------------------------------
    @torch.no_grad()
    def decode(self, z: torch.Tensor, return_dict: bool = True, generator=None):
        if self.use_slicing and z.shape[0] > 1:
            img = torch.cat([self._decode(s) for s in z.split(1)])
        else:
            img = self._decode(z)
        return DecoderOutput(sample=img) if return_dict else (img,)

    def _decode(self, z: torch.Tensor) -> torch.Tensor:
        if self.use_tiling and (z.shape[-1] > self.tile_latent_min_size or z.shape[-2] > self.tile_latent_min_size):
            return self.tiled_decode(z, return_dict=False)[0]
        return ops.to_nchw(self._decode_nhwc(z), self._io_dtype(z))

    def _decode_nhwc(self, z: torch.Tensor) -> torch.Tensor:
        """The image of NCHW latents ``z`` as the network leaves it: NHWC ``[B, H, W, out_channels]``."""
        dt, pk, d = self._dt(), self._pk, self.decoder
        pq = self.post_quant_conv
        B, Cz, H, W = z.shape
        # post_quant_conv: 1x1 over the (zero padded to 64) latent channels, output again 64 wide for conv_in
        wp, bp = one(pk, _POST_QUANT, pq, dt)
        zin = ops.to_nhwc(z, dt, CIN_PAD)
        zq = torch.empty(B, H, W, CIN_PAD, dtype=dt, device=z.device)
        ops.igemm(x0=zin, w=wp, out=zq, M=B * H * W, N=pq.weight.shape[0], K=CIN_PAD, c0=CIN_PAD, ldx0=CIN_PAD, ldw=CIN_PAD,
                  ldc=CIN_PAD, n_store=CIN_PAD, bias=bp)
        w, b = one(pk, _CONV_IN, d.conv_in, dt)
        h = d.mid_block(ops.conv3x3(zq, w, b))
        for lvl in d.up_blocks:
            h = lvl(h)
        g, gb = one(pk, R.affine, d.conv_norm_out, dt)
        h = ops.groupnorm(h, g, gb, d.conv_norm_out.eps, groups=d.conv_norm_out.num_groups, silu=True)
        wo, bo = one(pk, R.conv3x3_tap, d.conv_out, dt)
        return ops.conv3x3(h, wo, bo, n_out=d.conv_out.weight.shape[0])

    def forward(self, sample: torch.Tensor, sample_posterior: bool = False, return_dict: bool = True, generator=None):
        post = self.encode(sample).latent_dist
        z = post.sample(generator) if sample_posterior else post.mode()
        return self.decode(z, return_dict=return_dict)
