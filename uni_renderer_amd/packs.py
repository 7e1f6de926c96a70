"""Packed operands of every layer, described once for every executor.

A ``Recipe`` says, for one kind of module, which tensors a packed operand is made of (``params``) and how (``build``, from the
layout primitives of layers.py and tchain.py).  ``one`` caches it for the module path (layers.py, controlnet.py, vae.py),
``stacked`` caches it stacked over the streams for the grouped path (fused.py, hoist.py).  A cached value is valid for the
``(data_ptr, _version, device)`` of exactly the tensors ``params`` names; tests/test_packs_cpu.py checks per recipe that those
are the tensors ``build`` reads.  The training path keeps its own differentiable copies (param_stage.py, autograd_ops.py).
"""
from __future__ import annotations

import math
from collections import namedtuple

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops, tchain


class PackCache:
    """Packed tensors under a key of (name, extra key parts, module ids, dtype); an entry is valid for the (data_ptr, _version,
    device) of the parameters it was built from.  ``build(*args)`` runs without autograd."""

    def __init__(self):
        self._store = {}

    def get(self, key, params, build, *args):
        ver = [(p.data_ptr(), p._version, p.device) for p in params]
        hit = self._store.get(key)
        if hit is not None and hit[0] == ver:
            return hit[1]
        with torch.no_grad():
            val = build(*args)
        self._store[key] = (ver, val)
        return val


# ``params(m)``: the tensors ``build(m, dtype, *args)`` reads; ``build`` returns a tensor or a tuple of tensors.  ``m`` is a module,
# or a sequence of modules for the recipes made by ``rows``.
Recipe = namedtuple("Recipe", "name params build args", defaults=((),))

_ids = lambda m: id(m) if isinstance(m, nn.Module) else tuple([id(x) for x in m])
_stk = lambda ts: torch.stack(ts, 0).contiguous()
_cat = lambda ts: torch.cat(ts, 0).contiguous()
# ``fn`` over a list of built values, element by element where they are tuples
_each = lambda fn, vals: tuple(fn([v[i] for v in vals]) for i in range(len(vals[0]))) if isinstance(vals[0], tuple) else fn(vals)


def one(cache: PackCache, recipe: Recipe, m, dt):
    """``recipe`` of ``m`` in ``dt`` (the module path)."""
    return cache.get((recipe.name, recipe.args, _ids(m), dt), recipe.params(m), recipe.build, m, dt, *recipe.args)


def stacked(cache: PackCache, recipe, mods, dt):
    """``recipe`` of every stream's module, stacked stream-major (tuples element by element): the grouped path's [S, ...]
    operands.  ``recipe`` may be a list with one recipe per stream (the exchange pair scales only its first stream)."""
    rs = [recipe] * len(mods) if isinstance(recipe, Recipe) else recipe

    build = lambda: _each(_stk, [r.build(m, dt, *r.args) for r, m in zip(rs, mods)])
    key = ("stacked", tuple([(r.name, r.args) for r in rs]), tuple([_ids(m) for m in mods]), dt)
    return cache.get(key, [p for r, m in zip(rs, mods) for p in r.params(m)], build)


def rows(recipe: Recipe) -> Recipe:
    """The row-concatenation of ``recipe`` over a list of modules (tuples element by element) -- every ``time_emb_proj`` of a
    network, the prompt ``Wk`` / ``Wv`` / ``[Wk; Wv]`` of a phase, the ``q | k (| v)`` of an attention -- itself stackable."""
    return Recipe("rows." + recipe.name, lambda ms: [p for m in ms for p in recipe.params(m)],
                  lambda ms, dt, *args: _each(_cat, [recipe.build(m, dt, *args) for m in ms]), recipe.args)


# ---------------------------------------------------------------------------------------------------- the recipes
from .layers import LOG2E, f32, geglu_perm, pack_cond_conv3x3, pack_cond_conv3x3_rot, pack_conv3x3, pack_matrix  # noqa: E402 -- layers imports the cache above

_wb = lambda m: (m.weight, m.bias)
_scaled = lambda t, scale: (t * scale).contiguous() if scale != 1.0 else t
_pad_rows = lambda t, n: t if t.shape[0] == n else torch.cat([t, t.new_zeros((n - t.shape[0],) + tuple(t.shape[1:]))], 0)
_cs = lambda t: t.transformer_blocks[0].attn1.dim_head ** -0.5 * LOG2E  # softmax scale in log2 units (layers.Attention)


def _conv3x3(m, dt, cin_pad, cblock):
    w = m.weight
    return pack_conv3x3(w, dt, cin_pad, cblock=ops.conv_cblock(w.shape[1]) if cblock else 0), f32(m.bias)


def _fold(r, dt, cblock):
    w2, c2 = _conv3x3(r.conv2, dt, None, cblock)
    return torch.cat([w2, pack_matrix(r.conv_shortcut.weight, dt)], 1).contiguous(), c2 + f32(r.conv_shortcut.bias)


def _geglu(m, dt):
    perm = geglu_perm(m.weight.shape[0] // 2, m.weight.device)
    return pack_matrix(m.weight, dt)[perm].contiguous(), f32(m.bias)[perm].contiguous()


# GroupNorm / LayerNorm (gamma, beta) in fp32
affine = Recipe("affine", _wb, lambda m, dt: (f32(m.weight), f32(m.bias)))
# Linear [N, K] or 1x1 conv [N, K, 1, 1]: the [N, K] matrix alone (the bias-free q / k / v), or with its fp32 bias
matrix = Recipe("matrix", lambda m: (m.weight,), lambda m, dt: pack_matrix(m.weight, dt))
linear = Recipe("linear", _wb, lambda m, dt: (pack_matrix(m.weight, dt), f32(m.bias)))
matrix_rows, linear_rows = rows(matrix), rows(linear)
# 3x3 conv (weight [Co, 9 Ci], fp32 bias): in the block-outer K order of ``ops.conv_cblock`` (the UNet's convs, whose launches
# pass the same cblock) or tap-outer (the VAE, the heads)
conv3x3 = Recipe("conv3x3", _wb, _conv3x3, (None, True))
conv3x3_tap = Recipe("conv3x3", _wb, _conv3x3, (None, False))
# ResnetBlock2D with a conv_shortcut: [conv2 | conv_shortcut] along K (the shortcut is conv2's 1x1 tail) and the summed bias
_fold_params = lambda r: (r.conv2.weight, r.conv2.bias, r.conv_shortcut.weight, r.conv_shortcut.bias)
fold = Recipe("fold", _fold_params, _fold, (True,))
fold_tap = Recipe("fold", _fold_params, _fold, (False,))
# FeedForward ``net.0.proj``: weight and bias rows in the order the GEGLU epilogue pairs value and gate (layers.geglu_perm)
geglu = Recipe("geglu", _wb, _geglu)


def scaled_linear(scale: float) -> Recipe:
    """``linear`` times ``scale`` (an exchange conv with its ``conditioning_scale``), scaled after the cast."""
    return Recipe("scaled_linear", _wb, lambda m, dt, s: (_scaled(pack_matrix(m.weight, dt), s), _scaled(f32(m.bias), s)), (scale,))


def conv3x3_padded(cin_pad: int) -> Recipe:
    """``conv3x3_tap`` with the input channels zero padded to ``cin_pad`` (conv_in: one K chunk)."""
    return Recipe("conv3x3", _wb, _conv3x3, (cin_pad, False))


def conv_out(n_out: int) -> Recipe:
    """``conv3x3_tap`` with the output rows zero padded to ``n_out``, the widest head of a grouped launch."""
    return Recipe("conv_out", _wb, lambda m, dt, n: tuple(_pad_rows(t, n) for t in _conv3x3(m, dt, None, False)), (n_out,))


def linear_padded(k_pad: int) -> Recipe:
    """``linear`` with K zero padded to ``k_pad`` (the VAE's post_quant_conv reads the padded latent)."""
    return Recipe("linear_padded", _wb, lambda m, dt, k: (
        F.pad(pack_matrix(m.weight, dt), (0, k - m.weight.shape[1])).contiguous(), f32(m.bias)), (k_pad,))


def cond_conv3x3(image: bool, bgr: bool) -> Recipe:
    """A conv of the ControlNet conditioning embedding in the weight image ``ops.cond_conv3x3`` reads."""
    return Recipe("cond_conv3x3", _wb, lambda m, dt, img, flip: (
        pack_cond_conv3x3(m.weight, dt, m.stride[0], image=img, bgr=flip), f32(m.bias)), (image, bgr and image))


# The same conv's rotated, channel-transposed weights in the image ``ops.cond_conv3x3_dgrad`` reads (the weight alone: the input
# gradient has no bias)
cond_conv3x3_rot = Recipe("cond_conv3x3_rot", lambda m: (m.weight,), lambda m, dt: pack_cond_conv3x3_rot(m.weight, dt))


# The three chain launches of a one-block 320-channel Transformer2DModel ``t`` (tchain.py): (weight stream, fp32 constants).
# The q / k scale d^-1/2 log2(e) is folded into the projection weights before their cast (layers.Attention has the why).
def _chain_pre_params(t):
    b = t.transformer_blocks[0]
    return (t.proj_in.weight, t.proj_in.bias, b.norm1.weight, b.norm1.bias, b.attn1.to_q.weight, b.attn1.to_k.weight,
            b.attn1.to_v.weight)


def _chain_q_params(t):
    b = t.transformer_blocks[0]
    return b.attn1.to_out[0].weight, b.attn1.to_out[0].bias, b.norm2.weight, b.norm2.bias, b.attn2.to_q.weight


def _chain_ff_params(t):
    b = t.transformer_blocks[0]
    return (b.attn2.to_out[0].weight, b.attn2.to_out[0].bias, b.norm3.weight, b.norm3.bias, b.ff.net[0].proj.weight,
            b.ff.net[0].proj.bias, b.ff.net[2].weight, b.ff.net[2].bias, t.proj_out.weight, t.proj_out.bias)


chain_pre = Recipe("chain_pre", _chain_pre_params,
                   lambda t, dt: tchain.pack_chain_pre(*_chain_pre_params(t), math.sqrt(_cs(t)), dt))
chain_q = Recipe("chain_q", _chain_q_params, lambda t, dt: tchain.pack_chain_q(*_chain_q_params(t), _cs(t), dt))
chain_ff = Recipe("chain_ff", _chain_ff_params, lambda t, dt: tchain.pack_chain_ff(*_chain_ff_params(t), dt))


# AutoencoderKL ``v``: the 1x1 quant_conv composed with the encoder's conv_out on the host in fp32,
# quant(conv(h)) = (Wq Wc) * h + (Wq bc + bq)
def _vae_moments(v, dt):
    q, c = v.quant_conv, v.encoder.conv_out
    wq = q.weight.detach().float().reshape(q.weight.shape[0], -1)
    wc = torch.einsum("oi,icyx->ocyx", wq, c.weight.detach().float())
    bc = wq @ c.bias.detach().float() + q.bias.detach().float()
    return pack_conv3x3(wc, dt), bc.contiguous()


vae_moments = Recipe("vae_moments", lambda v: _wb(v.encoder.conv_out) + _wb(v.quant_conv), _vae_moments)
