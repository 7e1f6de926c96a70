"""Helpers of the LoRA tests: a float64 reference merge with the per-element error bound of ur_lora_merge_multi, guarded
output buffers, a seeded adapter builder for a model that covers the three key formats, and the oracle holding
float64-merged weights."""
import copy

import torch

from util_models import O  # noqa: F401  (re-exported for the tests)

DTYPES = [torch.float16, torch.bfloat16, torch.float32]
MANT = {torch.float16: 10, torch.bfloat16: 7, torch.float32: 23}         # stored significand bits
MIN_EXP = {torch.float16: -24, torch.bfloat16: -133, torch.float32: -149}  # log2 of the subnormal spacing
CANARY = {2: 0x5B5B, 4: 0x5B5B5B5B}
INT_VIEW = {2: torch.int16, 4: torch.int32}


# ---------------------------------------------------------------------------------------------------------------------
# reference and bound
# ---------------------------------------------------------------------------------------------------------------------
def ref_merge(base, up, down, rscale, scale):
    """float64: base + scale * sum_r rscale[r] * up[:, r] * down[r, :]  and the sum of the terms' magnitudes."""
    b = base.double().reshape(base.shape[0], -1)
    if up is None or up.shape[1] == 0:
        return b.clone(), torch.zeros_like(b)
    rs = torch.ones(up.shape[1], dtype=torch.float64) if rscale is None else rscale.double().cpu()
    u = up.double().cpu() * rs[None]
    d = down.double().cpu()
    return b + scale * (u @ d), abs(scale) * (u.abs() @ d.abs())


def ulp(x64, dtype):
    """Spacing of ``dtype`` at |x| (float64 in, float64 out); the subnormal spacing at and near zero."""
    _, e = torch.frexp(x64.abs())  # |x| = m * 2^e, m in [0.5, 1): floor(log2 |x|) = e - 1
    ex = (e.double() - 1 - MANT[dtype]).clamp_min(MIN_EXP[dtype])
    ex = torch.where(x64 == 0, torch.full_like(ex, MIN_EXP[dtype]), ex)
    return torch.pow(torch.tensor(2.0, dtype=torch.float64), ex)


def bound(base, up, down, rscale, scale, got, dtype):
    """(R + 2) 2^-24 (|base| + |scale| sum_r |rscale up down|) + ulp_dtype(got) / 2.
    Each term passes one rounding of rscale * up, at most R roundings of the ascending fma chain and the rounding of the
    final fma(scale, acc, base) -- the fp32 chain bound, first order -- and the result is rounded once to the dtype."""
    R = 0 if up is None else up.shape[1]
    _, mag = ref_merge(base, up, down, rscale, scale)
    b = base.double().reshape(base.shape[0], -1).abs()
    return (R + 2) * 2.0 ** -24 * (b + mag) + 0.5 * ulp(got.double().reshape(b.shape), dtype)


def representable(x64, dtype):
    return bool(torch.equal(x64.to(dtype).double(), x64))


# ---------------------------------------------------------------------------------------------------------------------
# problems and launches
# ---------------------------------------------------------------------------------------------------------------------
def int_problem(N, K, R, dtype, seed, scale):
    """Small-integer data whose merge is exact in every dtype: base in [-8, 8], up / down in {-1, 0, 1} with about 8 non-zero
    products per element however large R is, rscale in {1, 2}."""
    g = torch.Generator().manual_seed(seed)
    base = torch.randint(-8, 9, (N, K), generator=g).to(dtype)
    if R == 0:
        return base, None, None, None, scale
    up = torch.randint(-1, 2, (N, R), generator=g).float()
    keep = (torch.rand(R, K, generator=g) < min(1.0, 12.0 / R)).float()
    down = torch.randint(-1, 2, (R, K), generator=g).float() * keep
    rscale = torch.randint(1, 3, (R,), generator=g).float()
    return base, up, down, rscale, scale


def rand_problem(N, K, R, dtype, seed, scale):
    g = torch.Generator().manual_seed(seed)
    base = torch.randn(N, K, generator=g).to(dtype)
    up = torch.randn(N, R, generator=g)
    down = torch.randn(R, K, generator=g) * 0.1
    rscale = torch.rand(R, generator=g) * 2 - 0.5
    return base, up, down, rscale, scale


class Guarded:
    """Outputs of many items inside ONE buffer of canaries: ``reserve(numel, offset)`` books a span that starts
    ``guard + offset`` elements behind the previous one, ``allocate()`` makes the buffer, ``view(i, shape)`` hands out span
    ``i``; ``check()`` asserts that every element outside the spans still holds the canary."""

    def __init__(self, dtype, dev, guard=64):
        self.dtype, self.dev, self.guard = dtype, dev, guard
        self.spans, self.end, self.buf = [], guard, None

    def reserve(self, numel, offset=0):
        start = self.end + offset
        self.spans.append((start, numel))
        self.end = start + numel + self.guard
        return len(self.spans) - 1

    def allocate(self):
        size = self.dtype.itemsize
        self.buf = torch.full((self.end,), CANARY[size], dtype=INT_VIEW[size], device=self.dev).view(self.dtype)

    def view(self, i, shape):
        s, n = self.spans[i]
        return self.buf[s:s + n].view(shape)

    def check(self):
        size = self.dtype.itemsize
        bits = self.buf.view(INT_VIEW[size]).cpu()
        mask = torch.ones(bits.numel(), dtype=torch.bool)
        for s, n in self.spans:
            mask[s:s + n] = False
        bad = (bits[mask] != CANARY[size]).nonzero()
        assert bad.numel() == 0, f"{bad.numel()} canaries overwritten, first at masked index {int(bad[0])}"


def launch(problems, dtype, dev, outs=None):
    """One ``merge_items`` call (one launch per lora.multi_max() items) over ``problems`` = (base, up, down, rscale, scale)
    on the CPU; returns the device outputs and the device ``base`` tensors."""
    from uni_renderer_amd import lora

    rows, ws, bases, keep = [], [], [], []
    for i, (base, up, down, rscale, scale) in enumerate(problems):
        b = base.to(dev).contiguous()
        w = outs[i] if outs is not None else torch.empty_like(b)
        dv = [None if t is None else t.to(dev).contiguous() for t in (up, down, rscale)]
        keep.append(dv)
        rows.append((b, w, dv[0], dv[1], dv[2], float(scale)))
        ws.append(w)
        bases.append(b)
    lora.merge_items(rows, dtype)
    torch.cuda.synchronize()
    return ws, bases


# ---------------------------------------------------------------------------------------------------------------------
# adapters for a model
# ---------------------------------------------------------------------------------------------------------------------
KINDS = ("attn1.to_q", "attn1.to_k", "attn1.to_v", "attn1.to_out.0", "attn2.to_q", "attn2.to_k", "attn2.to_v", "attn2.to_out.0",
         "ff.net.0.proj", "ff.net.2", "proj_in", "proj_out", "conv1", "conv2", "conv_shortcut", "time_emb_proj",
         "downsamplers.0.conv", "upsamplers.0.conv")


def targets(model):
    """Every Linear / Conv2d of ``model`` whose name ends in one of KINDS, by kind."""
    out = {}
    for n, m in model.named_modules():
        if isinstance(m, (torch.nn.Linear, torch.nn.Conv2d)):
            for kind in KINDS:
                if n.endswith("." + kind):
                    out.setdefault(kind, []).append(n)
    return out


def make_adapter(model, seed, rank=4, mag=0.5, zero_up=False, prefix=""):
    """``(state_dict, network_alphas, spec)``: an adapter on every module of every kind of KINDS.  Attention projections of
    ``attn1`` use the legacy attention-processor keys, those of ``attn2`` the PEFT spelling, everything else the current
    diffusers one.  Every third module gets an alpha (= 2 * rank).  ``up`` is scaled so that the update's Frobenius norm
    is ``mag`` times the weight's.  ``spec`` = {module name: (down, up, alpha / rank or 1)} with the factors in their
    module's shape conventions ([R][Ci][kh][kw] / [Co][R][1][1] for convs)."""
    g = torch.Generator().manual_seed(seed)
    sd, alphas, spec = {}, {}, {}
    count = 0
    for kind, names in targets(model).items():
        for n in names:
            w = model.get_submodule(n).weight.detach().float().cpu()
            r = rank + (count % 2)  # two ranks, so that items differ
            down = torch.randn((r,) + tuple(w.shape[1:]), generator=g)
            up = torch.randn((w.shape[0], r) + (1,) * (w.dim() - 2), generator=g)
            factor = 1.0
            if count % 3 == 0:
                alphas[prefix + n] = 2.0 * r
                factor = 2.0
            delta = factor * (up.reshape(w.shape[0], r) @ down.reshape(r, -1))
            up = up * (mag * w.norm() / delta.norm().clamp_min(1e-12))
            if zero_up:
                up = torch.zeros_like(up)
            if kind.startswith("attn1."):
                attn, proj = n.rsplit(".to_", 1)
                stem = f"{attn}.processor.to_{proj.split('.')[0]}_lora"
                kd, ku = stem + ".down.weight", stem + ".up.weight"
            elif kind.startswith("attn2."):
                kd, ku = n + ".lora_A.weight", n + ".lora_B.weight"
            else:
                kd, ku = n + ".lora.down.weight", n + ".lora.up.weight"
            sd[prefix + kd], sd[prefix + ku] = down, up
            spec[n] = (down, up, factor)
            count += 1
    return sd, alphas, spec


def merged_weights(model, specs_and_weights, scale):
    """{parameter name: float64 merged weight} of ``model`` for a list of (spec, adapter weight)."""
    out = {}
    for spec, weight in specs_and_weights:
        for n, (down, up, factor) in spec.items():
            w = model.get_submodule(n).weight
            cur = out.get(n + ".weight", w.detach().double().cpu())
            delta = (up.double().reshape(w.shape[0], -1) @ down.double().reshape(down.shape[0], -1)).reshape(w.shape)
            out[n + ".weight"] = cur + scale * weight * factor * delta
    return out


def oracle_with_merged(unet_o, spec, scale):
    """A copy of the oracle UNet holding the float64-merged weights (stored in the oracle's fp32)."""
    m = copy.deepcopy(unet_o)
    sd = m.state_dict()
    with torch.no_grad():
        for k, v in merged_weights(unet_o, [(spec, 1.0)], scale).items():
            sd[k].copy_(v.to(sd[k].dtype))
    return m


def step_with_scale(unet, enc, dec, x_t, cond, ehs, t_img, t_attr, kw):
    """util_models.product_step with ``cross_attention_kwargs=kw`` handed to all three networks, as the reference's
    pipeline does."""
    res, mid, raw_enc, raw_mid_enc = enc(x_t, t_attr, encoder_hidden_states=ehs, controlnet_cond=cond, return_dict=False,
                                         cross_attention_kwargs=kw)
    img_pred, raw_unet, raw_mid_unet, _ = unet(x_t, t_img, encoder_hidden_states=ehs, down_block_additional_residuals=res,
                                               mid_block_additional_residual=mid, return_dict=False, cross_attention_kwargs=kw)
    attr_pred = dec(sample=raw_mid_enc, down_block_res_samples=raw_enc, timestep=t_attr, encoder_hidden_states=ehs,
                    down_block_additional_residuals=raw_unet, mid_block_additional_residual=raw_mid_unet, return_dict=False,
                    cross_attention_kwargs=kw)
    return dict(img_pred=img_pred, attr_pred=attr_pred)
