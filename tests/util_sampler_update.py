"""The rig of the per-element tests of the sampler update kernels (``ur_ddim_update`` / ``ur_unipc_update`` /
``ur_sde_update``, csrc/sampler.hip): poisoned guard buffers, one launch configuration on them, the guidance combine."""
import numpy as np
import torch

POISON = 768.0  # exact in fp16 / bf16 / fp32
GUARD = 64
SHAPES = [(B, C, hw) for B in (1, 2) for C in (4, 24) for hw in ((8, 8), (5, 7))]  # 35 pixels: groups straddle planes, tail group
HALF_ULP = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8, torch.float32: 0.0}  # storage rounding, relative (normal range)


def guarded(shape, dtype, dev, fill=None):
    """A tensor of ``shape`` inside a poisoned flat buffer: (buffer, view)."""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), POISON, dtype=dtype, device=dev)
    view = buf[GUARD:GUARD + n].view(shape)
    if fill is not None:
        view.copy_(fill)
    return buf, view


def guards_intact(buf):
    return bool((buf[:GUARD] == POISON).all()) and bool((buf[-GUARD:] == POISON).all())


def combine(pred, cfg, guidance, cfg_channels, B, C):
    """m of the update: the guidance arithmetic in the prediction's dtype (one rounding per operation), channels 4 .. 4 + C."""
    p = pred[..., 4:4 + C]
    if not cfg:
        return p.permute(0, 3, 1, 2)
    pc, pu = p[:B], p[B:]
    g = pu + (pc - pu) * guidance
    return torch.cat([g[..., :cfg_channels], pc[..., cfg_channels:]], dim=-1).permute(0, 3, 1, 2)


class Case:
    """One launch configuration on guarded buffers: lat is channels 4 .. 4 + C of a 28-channel tensor (batch stride 28 HW),
    pred has 28 channels with the prediction at 4 .. 4 + C.  ``master`` holds the initial sample ``x0``; ``hist`` is zero:
    [B, C, H, W], or [2, B, C, H, W] with ``ring`` (UniPC's two previous predictions), which also adds ``last`` = ``x0``."""

    def __init__(self, dev, dtype, B, C, hw, cfg, nsteps, gen, integer, ring=False):
        self.B, self.C, self.hw, self.cfg, self.n = B, C, hw, cfg, nsteps
        H, W = hw
        Bt = 2 * B if cfg else B
        draw = (lambda *s: torch.randint(-2, 3, s, generator=gen).float()) if integer else (lambda *s: torch.randn(*s, generator=gen))
        self.lat_buf, self.lat_full = guarded((Bt, 28, H, W), dtype, dev)
        self.lat = self.lat_full[:, 4:4 + C]
        self.x0 = draw(B, C, H, W).to(dtype).float() if integer else draw(B, C, H, W)
        self.m_buf, self.master = guarded((B, C, H, W), torch.float32, dev, self.x0)
        hshape = ((2,) if ring else ()) + (B, C, H, W)
        self.h_buf, self.hist = guarded(hshape, torch.float32, dev, torch.zeros(hshape))
        self.bufs = [self.lat_buf, self.m_buf, self.h_buf]
        if ring:
            self.l_buf, self.last = guarded((B, C, H, W), torch.float32, dev, self.x0)
            self.bufs.append(self.l_buf)
        self.preds = [draw(Bt, H, W, 28).to(dtype).to(dev) for _ in range(nsteps)]
        self.step = torch.zeros(1, dtype=torch.int32, device=dev)
        self.seed = torch.tensor([0x1234_5678_9ABC], dtype=torch.int64, device=dev)

    def intact(self):
        ok = all(guards_intact(b) for b in self.bufs)
        outside = torch.cat([self.lat_full[:, :4].reshape(-1), self.lat_full[:, 4 + self.C:].reshape(-1)])
        return ok and bool((outside == POISON).all())
