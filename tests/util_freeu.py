"""FreeU oracle for the tests (Si et al., arXiv 2309.11497; diffusers 0.24 ``apply_freeu`` / ``fourier_filter`` semantics,
restated -- diffusers is not a dependency):

  * ``fourier_filter_fft``     the literal fftn -> fftshift -> box * s -> ifftshift -> ifftn -> real, float64;
  * ``fourier_filter_closed``  the rank-7 closed form the HIP kernel evaluates (the box is the frequencies {-1, 0}^2);
  * ``apply_freeu_``           one apply_freeu call with the reference's in-place backbone scale;
  * ``oracle_freeu``           context manager: the oracle UNet's up blocks run FreeU with those semantics (their ``forward``
                               is replaced on the instance for the duration; ``oracle/`` itself is untouched).
"""
import contextlib
import math
import types

import torch

SD14 = dict(s1=0.9, s2=0.2, b1=1.2, b2=1.4)  # the SD-1.4 values of the FreeU repository


def fourier_filter_fft(x: torch.Tensor, scale: float, threshold: int = 1) -> torch.Tensor:
    """x [..., H, W] -> float64, the literal form."""
    x = x.double()
    H, W = x.shape[-2:]
    f = torch.fft.fftshift(torch.fft.fftn(x, dim=(-2, -1)), dim=(-2, -1))
    mask = torch.ones(x.shape, dtype=torch.float64)
    cr, cc = H // 2, W // 2
    mask[..., cr - threshold:cr + threshold, cc - threshold:cc + threshold] = scale
    f = f * mask
    return torch.fft.ifftn(torch.fft.ifftshift(f, dim=(-2, -1)), dim=(-2, -1)).real


def fourier_filter_closed(x: torch.Tensor, scale: float, dtype=torch.float64) -> torch.Tensor:
    """x [..., H, W]: x + (s - 1) / (H W) [a0 + a1 cos t + a2 sin t + a3 cos p + a4 sin p + a5 cos(t + p) + a6 sin(t + p)],
    a_k = sum over the map of x times the same basis function; evaluated in ``dtype``."""
    x = x.to(dtype)
    H, W = x.shape[-2:]
    t = (2 * math.pi * torch.arange(H, dtype=torch.float64) / H)[:, None].expand(H, W)
    p = (2 * math.pi * torch.arange(W, dtype=torch.float64) / W)[None, :].expand(H, W)
    basis = torch.stack([torch.ones(H, W, dtype=torch.float64), t.cos(), t.sin(), p.cos(), p.sin(), (t + p).cos(),
                         (t + p).sin()]).to(dtype)  # [7, H, W]
    a = (x[..., None, :, :] * basis).sum(dim=(-2, -1))  # [..., 7]
    corr = (a[..., :, None, None] * basis).sum(dim=-3)
    return x + corr * ((scale - 1.0) / (H * W))


def plane_wave(ky: int, kx: int, H: int, W: int) -> torch.Tensor:
    """cos(2 pi (ky y / H + kx x / W)) on an H x W map, float64."""
    y = torch.arange(H, dtype=torch.float64)[:, None]
    x = torch.arange(W, dtype=torch.float64)[None, :]
    return torch.cos(2 * math.pi * (ky * y / H + kx * x / W))


# (ky, kx) -> gain as a function of s (H, W >= 5).  (1, -1) is what separates the reference's box {-1, 0}^2 from a symmetric
# low-pass, which would give (1 + s) / 2 there
PLANE_WAVES = [((0, 0), lambda s: s), ((1, 0), lambda s: (1 + s) / 2), ((0, 1), lambda s: (1 + s) / 2),
               ((1, 1), lambda s: (1 + s) / 2), ((1, -1), lambda s: 1.0), ((2, 0), lambda s: 1.0), ((0, 2), lambda s: 1.0)]


def apply_freeu_(resolution_idx: int, hidden: torch.Tensor, skip: torch.Tensor, s1, s2, b1, b2):
    """NCHW.  Scales ``hidden[:, : C // 2]`` IN PLACE (the reference's setitem) and returns (hidden, new filtered skip) for
    resolution_idx 0 (b1, s1) and 1 (b2, s2); other blocks pass through."""
    if resolution_idx not in (0, 1):
        return hidden, skip
    b, s = (b1, s1) if resolution_idx == 0 else (b2, s2)
    half = hidden.shape[1] // 2
    hidden[:, :half] = hidden[:, :half] * b
    return hidden, fourier_filter_fft(skip, s).to(skip.dtype)


@contextlib.contextmanager
def oracle_freeu(unet_o, s1, s2, b1, b2):
    """Within the block, up block i of the oracle UNet applies FreeU with resolution_idx = i in front of every concat, as
    the reference's blocks do (FreeU on only when all four factors are truthy)."""
    on = bool(s1 and s2 and b1 and b2)

    def make(idx):
        def forward(self, x, skips, temb, context=None, upsample_size=None, extra=None):
            outs = ()
            attns = self.attentions if getattr(self, "has_cross_attention", False) else [None] * len(self.resnets)
            for k, (r, a) in enumerate(zip(self.resnets, attns)):
                s = skips[-1]
                skips = skips[:-1]
                if on:
                    x, s = apply_freeu_(idx, x, s, s1, s2, b1, b2)
                x = r(torch.cat([x, s], dim=1), temb)
                if a is not None:
                    x = a(x, context)
                if extra is not None:
                    x = x + extra[k]
                outs += (x,)
            if self.upsamplers is not None:
                x = self.upsamplers[0](x, upsample_size)
            return x, outs

        return forward

    for i, blk in enumerate(unet_o.up_blocks):
        blk.forward = types.MethodType(make(i), blk)
    try:
        yield unet_o
    finally:
        for blk in unet_o.up_blocks:
            del blk.forward


@torch.no_grad()
def oracle_step(unet_o, enc_o, dec_o, x_t, cond, ehs, t_img, t_attr, freeu=None, exchange=True, run_decoder=True):
    """The oracle's dual-stream step (or the UNet alone, ``exchange=False``) with FreeU ``freeu`` (a dict s1 s2 b1 b2) or off."""
    from util_models import O

    ctx = oracle_freeu(unet_o, **freeu) if freeu else contextlib.nullcontext()
    with ctx:
        if exchange:
            return O.dual_stream_step(unet_o, enc_o, dec_o, x_t, cond, ehs, t_img, t_attr, run_decoder=run_decoder)
        img, raw, raw_mid, ups = unet_o(x_t, t_img, ehs)
        return dict(img_pred=img, raw_unet=raw, raw_mid_unet=raw_mid, up_res=ups, attr_pred=None)
