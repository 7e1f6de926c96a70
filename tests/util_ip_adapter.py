"""IP-Adapter (Ye et al., arXiv 2308.06721; diffusers 0.24 ``IPAdapterAttnProcessor2_0`` / ``ImageProjection`` semantics, restated
-- diffusers is not a dependency) for the tests:

  * ``ip_reference`` / ``ip_bound``   the kernel's function ``o + scale * softmax2(q k_ip^T) v_ip`` in float64 and the
                                      element-wise error bound of ``ur_ip_attention_add`` against it (derivation below);
  * ``ip_emulate_fp32``               the kernel's arithmetic, operation by operation, in numpy float32;
  * ``ImageProjection``, ``IPAttention``, ``oracle_ip_adapter``   the float restatement of the adapter on the oracle's UNet
                                      (its cross-attentions' ``forward`` is replaced on the instance for the duration;
                                      ``oracle/`` itself is untouched);
  * ``ip_state_dict`` / ``attn_processor_ids``   random adapters in the original key layout, and diffusers' processor order.

The bound.  Inputs are the SAME rounded fp16 / bf16 values on both sides, u = 2^-24 (fp32), u_s = 2^-11 / 2^-8 (storage),
gamma(n) = n u / (1 - n u).  Per (sample, token, head), s_j = q . k_j exactly, A_j = sum_i |q_i k_ij|, p = softmax2(s).

  1. scores.  The products are exact in fp32 (two 11-bit / 8-bit significands).  A term passes through at most
     L = 8 + log2 G + (R - 1) additions (8 fmas in a lane, the butterfly over G lanes, R - 1 adds of the group sums;
     d / 8 = G R with G a power of two and R in {1, 5}):                         |s^_j - s_j| <= gamma(L) A_j.
  2. max subtraction, one rounding: t_j = (s^_j - m^)(1 + e), |e| <= u, and |s^_j - m^| <= (max s - s_j) + 2 gamma(L) max_j A_j.
     Softmax does not depend on the constant subtracted, so take E_j = 2^(s_j - m^) as the exact weights:
         tau_j = t_j - (s_j - m^),   |tau_j| <= gamma(L) A_j + u ((max s - s_j) + 2 gamma(L) max A).
  3. exp2 (v_exp_f32: 1 ulp, relative 2^-23):   e_j = E_j (1 + rho_j),   1 + rho_j <= 2^|tau_j| (1 + 2^-23).  A weight below
     2^-126 may be flushed to zero: an absolute 2^-126 per weight against a sum l >= 1 -- the term FTZ below.
  4. l^ = e_0 + e_1 + ... left to right: each e_j passes through at most N - 1 additions; acc = fma(e_j, v_j, acc) from 0: at most
     N roundings per term.  With kn_j = (1 + rho_j)(1 + gamma(N)) - 1 and kd_j = (1 + rho_j)(1 + gamma(N - 1)) - 1:
         |acc_c - sum_j E_j v_jc| <= sum_j E_j |v_jc| kn_j,     |l^ / l - 1| <= sum_j p_j kd_j =: D
         |acc_c / l^ - ip_c| <= (sum_j p_j |v_jc| kn_j + D |ip_c|) / (1 - D) =: Q_c
  5. w = fl(scale * fl(1 / l^)): two roundings, om = 2 u + u^2:   |w acc_c - scale ip_c| <= |scale| (Q_c (1 + om) + om |ip_c|) =: E_c
  6. fma(acc, w, o) rounds once in fp32, the store once in the storage type (plus half a subnormal spacing, TINY):
         |got - ref| <= E_c + (|ref| + E_c) ((1 + u)(1 + u_s) - 1) + TINY.
"""
import contextlib
import math
import types

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

U32 = 2.0 ** -24
U_EXP2 = 2.0 ** -23
FTZ = 2.0 ** -126
U_ = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}
TINY = {torch.float16: 2.0 ** -25, torch.bfloat16: 2.0 ** -134}
LOG2E = 1.4426950408889634


def gamma(n):
    return n * U32 / (1.0 - n * U32)


def tree(d):
    """(G, R, L) of head width d: butterfly width, group sums, roundings a product passes through."""
    vpd = d // 8
    g = vpd & -vpd
    r = vpd // g
    assert vpd * 8 == d and r in (1, 5), d
    return g, r, 8 + int(math.log2(g)) + (r - 1)


def _heads(t, H):
    return t.reshape(t.shape[0], t.shape[1], H, -1)


def ip_reference(o, q, k, v, scale, H):
    """float64: o [B, T, C] + scale * per-head softmax2(q k^T) v over the N rows of k / v [B, N, C]; q [B, T, C] in log2 units."""
    o, q, k, v = (t.double() for t in (o, q, k, v))
    s = torch.einsum("bthd,bjhd->bthj", _heads(q, H), _heads(k, H))
    p = torch.softmax(s * math.log(2.0), dim=-1)
    ip = torch.einsum("bthj,bjhd->bthd", p, _heads(v, H)).reshape(o.shape)
    return o + scale * ip


def ip_bound(o, q, k, v, scale, H, dtype):
    """The element-wise bound of the module docstring, [B, T, C] float64."""
    o, q, k, v = (t.double() for t in (o, q, k, v))
    B, T, C = o.shape
    N, d = k.shape[1], C // H
    _, _, L = tree(d)
    qh, kh, vh = _heads(q, H), _heads(k, H), _heads(v, H)
    s = torch.einsum("bthd,bjhd->bthj", qh, kh)
    A = torch.einsum("bthd,bjhd->bthj", qh.abs(), kh.abs())
    p = torch.softmax(s * math.log(2.0), dim=-1)
    gap = s.amax(-1, keepdim=True) - s
    tau = gamma(L) * A + U32 * (gap + 2 * gamma(L) * A.amax(-1, keepdim=True))
    rho1 = torch.exp2(tau) * (1 + U_EXP2)            # 1 + rho_j
    kn = rho1 * (1 + gamma(N)) - 1
    kd = rho1 * (1 + gamma(N - 1)) - 1
    D = (p * kd).sum(-1, keepdim=True)               # [B, T, H, 1]
    ip = torch.einsum("bthj,bjhd->bthd", p, vh)
    num = torch.einsum("bthj,bjhd->bthd", p * kn, vh.abs())
    Q = (num + D * ip.abs()) / (1 - D)
    om = 2 * U32 + U32 * U32
    ftz = 2 * N * FTZ * vh.abs().amax(1)[:, None]     # [B, 1, H, d]
    E = (abs(scale) * (Q * (1 + om) + om * ip.abs() + ftz)).reshape(B, T, C)
    ref = o + scale * ip.reshape(B, T, C)
    return E + (ref.abs() + E) * ((1 + U32) * (1 + U_[dtype]) - 1) + TINY[dtype]


def _fma32(a, b, c):
    """fl32(a * b + c) for float32 arrays: the product of two float32 is exact in float64; the sum rounds to float64 and then
    to float32 (a double rounding that can differ from a true fma in the last place in rare ties -- an emulation, not the bits)."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def ip_emulate_fp32(o, q, k, v, scale, H, dtype, drop_token=None, wrong_head=False, scale_twice=False):
    """The kernel's arithmetic in numpy float32, in its order (csrc/ipadapter.hip): returns the result rounded to ``dtype`` as a
    float64 tensor.  The keyword switches plant the errors the bound must catch."""
    B, T, C = o.shape
    N, d = k.shape[1], C // H
    G, R, _ = tree(d)
    f32 = lambda t: _heads(t.float(), H).numpy()
    qh, kh, vh, oh = f32(q), f32(k), f32(v), f32(o)
    if wrong_head:
        kh, vh = np.roll(kh, 1, axis=2), np.roll(vh, 1, axis=2)
    sc = np.zeros((B, T, H, N), np.float32)
    for j in range(N):
        pv = np.zeros((B, T, H, d // 8), np.float32)
        for e in range(8):
            pv = _fma32(qh.reshape(B, T, H, -1, 8)[..., e], kh[:, j].reshape(B, 1, H, -1, 8)[..., e], pv)  # lane i: elements 8 i + e
        m = 1
        while m < G:  # the butterfly: what the first lane of every group of 2 m holds
            pv = pv.copy()
            pv[..., 0::2 * m] = pv[..., 0::2 * m] + pv[..., m::2 * m]
            m *= 2
        s = pv[..., 0]
        for i in range(1, R):
            s = s + pv[..., i * G]
        sc[..., j] = s
    mx = sc.max(-1, keepdims=True)
    e_ = np.exp2((sc - mx).astype(np.float32)).astype(np.float32)
    if drop_token is not None:
        e_[..., drop_token] = 0
    l = np.zeros((B, T, H), np.float32)
    for j in range(N):
        l = l + e_[..., j]
    w = (np.float32(scale) * (np.float32(1.0) / l)).astype(np.float32)
    if scale_twice:
        w = (w * np.float32(scale)).astype(np.float32)
    acc = np.zeros((B, T, H, d), np.float32)
    for j in range(N):
        acc = _fma32(e_[..., j:j + 1], vh[:, j][:, None], acc)
    res = _fma32(acc, w[..., None], oh).reshape(B, T, C)
    return torch.from_numpy(res).to(dtype).double()


# ---------------------------------------------------------------------------------------------------------------------------
# the adapter on the oracle's networks
# ---------------------------------------------------------------------------------------------------------------------------
class ImageProjection(nn.Module):
    """diffusers' ``ImageProjection``: Linear(clip_dim -> N * cross_attention_dim), reshape to [B, N, cross], LayerNorm."""

    def __init__(self, image_embed_dim, cross_attention_dim, num_image_text_embeds=4):
        super().__init__()
        self.num_image_text_embeds = num_image_text_embeds
        self.image_embeds = nn.Linear(image_embed_dim, num_image_text_embeds * cross_attention_dim)
        self.norm = nn.LayerNorm(cross_attention_dim)

    def forward(self, image_embeds):
        b = image_embeds.shape[0]
        return self.norm(self.image_embeds(image_embeds).reshape(b, self.num_image_text_embeds, -1))


def ip_attention(attn, x, context, ip_tokens, to_k_ip, to_v_ip, scale):
    """One cross-attention of ``IPAdapterAttnProcessor2_0`` on the oracle's ``Attention`` ``attn``: the prompt's SDPA, plus
    ``scale`` times the SDPA over the image tokens with the weights ``to_k_ip`` / ``to_v_ip`` [inner, cross], then to_out."""
    b, t, _ = x.shape
    h = attn.heads
    split = lambda y: y.view(b, -1, h, y.shape[-1] // h).transpose(1, 2)
    q = split(attn.to_q(x))
    hid = F.scaled_dot_product_attention(q, split(attn.to_k(context)), split(attn.to_v(context)))
    ip = F.scaled_dot_product_attention(q, split(ip_tokens @ to_k_ip.t()), split(ip_tokens @ to_v_ip.t()))
    hid = hid + scale * ip
    return attn.to_out[0](hid.transpose(1, 2).reshape(b, t, -1))


def attn_processor_ids(unet):
    """{id: module path of the attention} in diffusers' ``attn_processors`` order for a UNet with ``down_blocks``, ``up_blocks``,
    ``mid_block`` (registered in that order): per transformer block attn1 then attn2.  Works on the oracle's and the product's UNet."""
    ids, n = {}, 0
    for top in ("down_blocks", "up_blocks", "mid_block"):
        mod = getattr(unet, top)
        for name, m in mod.named_modules():
            if name.endswith("attn1") or name.endswith("attn2"):
                ids[n] = f"{top}.{name}"
                n += 1
    return ids


def ip_state_dict(unet, clip_dim, n_tokens=4, std=0.05, seed=7, cross_dim=None):
    """A random adapter for ``unet`` in the original IP-Adapter layout: ``image_proj.{proj,norm}.{weight,bias}`` and
    ``ip_adapter.{id}.to_{k,v}_ip.weight`` for the cross-attention ids."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    mods = dict(unet.named_modules())
    for i, path in attn_processor_ids(unet).items():
        if path.endswith("attn2"):
            a = mods[path]
            inner, cross = a.to_k.weight.shape
            cross_dim = cross
            sd[f"ip_adapter.{i}.to_k_ip.weight"] = torch.randn(inner, cross, generator=g) * std
            sd[f"ip_adapter.{i}.to_v_ip.weight"] = torch.randn(inner, cross, generator=g) * std
    sd["image_proj.proj.weight"] = torch.randn(n_tokens * cross_dim, clip_dim, generator=g) * clip_dim ** -0.5
    sd["image_proj.proj.bias"] = torch.randn(n_tokens * cross_dim, generator=g) * 0.1
    sd["image_proj.norm.weight"] = 1 + 0.1 * torch.randn(cross_dim, generator=g)
    sd["image_proj.norm.bias"] = 0.1 * torch.randn(cross_dim, generator=g)
    return sd


@contextlib.contextmanager
def oracle_ip_adapter(unet_o, sd, image_embeds, scale=1.0):
    """Within the block the oracle UNet's cross-attentions run the decoupled attention with the adapter ``sd`` (float32 of
    whatever it holds) on ``image_embeds`` [B, clip_dim]."""
    sd = {k: v.float() for k, v in sd.items()}
    cross = sd["image_proj.norm.weight"].shape[0]
    n = sd["image_proj.proj.weight"].shape[0] // cross
    proj = ImageProjection(sd["image_proj.proj.weight"].shape[1], cross, n)
    proj.image_embeds.weight.data, proj.image_embeds.bias.data = sd["image_proj.proj.weight"], sd["image_proj.proj.bias"]
    proj.norm.weight.data, proj.norm.bias.data = sd["image_proj.norm.weight"], sd["image_proj.norm.bias"]
    with torch.no_grad():
        tokens = proj(image_embeds.float())
    mods = dict(unet_o.named_modules())
    patched = []
    for i, path in attn_processor_ids(unet_o).items():
        if not path.endswith("attn2"):
            continue
        a = mods[path]
        wk, wv = sd[f"ip_adapter.{i}.to_k_ip.weight"], sd[f"ip_adapter.{i}.to_v_ip.weight"]
        a.forward = types.MethodType(lambda self, x, context=None, wk=wk, wv=wv: ip_attention(self, x, context, tokens, wk, wv, scale), a)
        patched.append(a)
    try:
        yield unet_o
    finally:
        for a in patched:
            del a.forward


@torch.no_grad()
def oracle_step(unet_o, enc_o, dec_o, x_t, cond, ehs, t_img, t_attr, adapter=None, image_embeds=None, scale=1.0, exchange=True,
                run_decoder=True):
    """The oracle's dual-stream step (or the UNet alone) with the adapter ``adapter`` on the UNet, or without one."""
    from util_models import O

    ctx = oracle_ip_adapter(unet_o, adapter, image_embeds, scale) if adapter is not None else contextlib.nullcontext()
    with ctx:
        if exchange:
            return O.dual_stream_step(unet_o, enc_o, dec_o, x_t, cond, ehs, t_img, t_attr, run_decoder=run_decoder)
        img, raw, raw_mid, ups = unet_o(x_t, t_img, ehs)
        return dict(img_pred=img, raw_unet=raw, raw_mid_unet=raw_mid, up_res=ups, attr_pred=None)
