"""What one network forward under autograd (autograd_net.py) prepares of its parameters up front, in one place.

Entering ``Stage(net, dtype)`` issues the four barrier nodes of ``autograd_ops`` in this order -- ``LoraMerge`` (the merged
matrices of a trainable LoRA adapter), ``CastParams`` (the other Linear / 1x1-conv weights in the compute dtype, one packed
buffer), ``ParamBarrier`` (the fp32 biases and norm parameters, whose gradients may then be deferred with the weights') and
``PackConvWeights`` (the 3x3 conv weights in the kernels' layout) -- and keeps their outputs; leaving it, by an exception too,
drops them all at once.  While it is ``active`` the layer code finds them through ``wc`` / ``w2`` / ``lora_merged`` here and
``linear`` / ``conv3x3`` / ``group_norm`` / ``layer_norm_skip`` / ``pack_conv_weight`` of ``autograd_ops``.  With no active
stage each of these falls back to the unstaged form (a plain cast, a ``PackConvWeight`` node, the parameter itself): the
recompute of a gradient-checkpointed resnet runs in the backward, after the stage is gone, and relies on that.
Which parameters are staged, and in which order, is the network's ``plan``: computed once and dropped with the network.
"""
from __future__ import annotations

import weakref
from typing import NamedTuple, Optional

import torch

from . import _experiments as X, backward as B
from .controlnet import CIN_PAD
from .layers import BasicTransformerBlock, ResnetBlock2D


BATCH_CASTS = X.flag("batch_casts", True)
active: Optional["Stage"] = None  # the stage of the network forward that is running (the networks run one after the other)


class Plan(NamedTuple):
    matrices: list  # fp32 Linear / 1x1-conv weights, in the memory order of their packed compute-dtype copies
    vectors: list   # fp32 biases of the Linear / 1x1 / 3x3 layers, then gamma / beta of the norm layers
    convs: list     # (fp32 3x3 conv weight, cin_pad or None)


_plans: "weakref.WeakKeyDictionary[torch.nn.Module, Plan]" = weakref.WeakKeyDictionary()


def _cross_kv(net) -> list:
    """to_k / to_v weights of the cross-attentions, in the order ``autograd_net._context_projections`` concatenates them"""
    return [w for m in net.modules() if isinstance(m, BasicTransformerBlock) and getattr(m, "attn2", None) is not None
            for w in (m.attn2.to_k.weight, m.attn2.to_v.weight)]


def plan(net) -> Plan:
    hit = _plans.get(net)
    if hit is not None:
        return hit
    ws = [m.weight for m in net.modules()
          if isinstance(m, torch.nn.Linear) or (isinstance(m, torch.nn.Conv2d) and m.kernel_size == (1, 1))]
    # order = memory order of the packed copies (CastParams): the weights the forward concatenates into one GEMM operand come
    # first and in the order of their use, so the "concatenation" is a view (A.cat_adjacent): all time_emb_proj, then the
    # to_k / to_v pairs of the cross-attentions; q | k | v of a self-attention are neighbours in module order already
    temb = [m.time_emb_proj.weight for m in net.modules() if isinstance(m, ResnetBlock2D) and m.time_emb_proj is not None]
    first = temb + _cross_kv(net)
    seen = {id(w) for w in first}
    ws = first + [w for w in ws if id(w) not in seen]
    # the seven narrow convs of a ControlNet's conditioning embedding take no part: autograd_ops.CondConv3x3 reads the
    # parameters themselves and returns their gradients in the parameters' own layout (no cast, no pack, no barrier)
    emb = getattr(net, "controlnet_cond_embedding", None)
    narrow = {id(m) for m in ([emb.conv_in] + list(emb.blocks))} if emb is not None else set()
    bs = [m.bias for m in net.modules()
          if (isinstance(m, torch.nn.Linear) or (isinstance(m, torch.nn.Conv2d) and m.kernel_size in ((1, 1), (3, 3))))
          and m.bias is not None and m.bias.dtype == torch.float32 and id(m) not in narrow]
    # gamma / beta of the norm layers too: their gradients are summed in one launch at the barrier (backward.NormSums)
    bs += [p_ for m in net.modules() if isinstance(m, (torch.nn.GroupNorm, torch.nn.LayerNorm)) and m.weight is not None
           for p_ in (m.weight, m.bias) if p_ is not None and p_.dtype == torch.float32]
    conv_in = getattr(net, "conv_in", None)
    c3 = [(m.weight, CIN_PAD if m is conv_in else None) for m in net.modules()
          if isinstance(m, torch.nn.Conv2d) and m.kernel_size == (3, 3) and m.weight.dtype == torch.float32
          and id(m) not in narrow]
    hit = _plans[net] = Plan([w for w in ws if w.dtype == torch.float32], bs, c3)
    return hit


class Stage:
    """The staged parameters of ``net`` for the duration of one forward in the compute dtype ``dt``; ``lora``: the
    ``(rows, scale)`` of ``lora.UNetLoraMixin._lora_train_plan`` when the network carries a trainable adapter."""

    def __init__(self, net, dt, lora=None):
        self.net, self.dt, self.lora = net, dt, lora
        self.weights = {}    # id(fp32 weight) -> its compute-dtype copy (CastParams) or merged W' (LoraMerge)
        self.merged = set()  # the ids among them that are LoRA-merged: those exist only while this stage does
        self.vectors = {}    # id(fp32 bias / gamma / beta) -> its ParamBarrier output
        self.packed = {}     # (id(fp32 3x3 conv weight), cin_pad) -> its PackConvWeights output

    def _merge_lora(self, A):
        """ONE node writes the merged matrices W' of all adapted weights into one packed buffer: to_k / to_v of the cross-attentions
        first, then module order, as for the casts, so q | k | v and k | v stay neighbours when all are adapted (A.cat_adjacent)."""
        rows, s = self.lora
        first = {id(w): i for i, w in enumerate(_cross_kv(self.net))}
        rows = sorted(rows, key=lambda r: first.get(id(r[0]), len(first)))  # stable: the others keep their module order
        outs = A.LoraMerge.apply(self.dt, s, [(r[1], r[4]) for r in rows], *[f for r in rows for f in (r[2], r[3])])
        for r, o in zip(rows, outs):
            self.weights[id(r[0])] = o
            self.merged.add(id(r[0]))

    def __enter__(self):
        from . import autograd_ops as A  # the nodes; autograd_ops imports this module for its look-ups

        global active
        if active is not None:
            raise RuntimeError("param_stage.Stage: a network forward inside another one's stage")
        if self.lora is not None and torch.is_grad_enabled():
            self._merge_lora(A)
        if BATCH_CASTS and torch.is_grad_enabled():
            p = plan(self.net)
            ws = [w for w in p.matrices if w.requires_grad]
            if ws:
                self.weights.update((id(w), c) for w, c in zip(ws, A.CastParams.apply(self.dt, *ws)))
            # the vectors of the same layers behind one barrier node: their gradients may then be deferred with the weights'
            bs = [b for b in p.vectors if b.requires_grad] if (ws and B.WGRAD_DEFER and B.WGRAD) else []
            if bs:
                self.vectors.update((id(b), o) for b, o in zip(bs, A.ParamBarrier.apply(*bs)))
            # ... and the 3x3 conv weights packed up front by one node, same reason
            c3 = [(w, cp) for w, cp in p.convs if w.requires_grad and w.is_cuda] if (B.WGRAD_DEFER and B.WGRAD) else []
            if c3:
                outs = A.PackConvWeights.apply(self.dt, tuple(cp for _, cp in c3), *[w for w, _ in c3])
                self.packed.update(((id(w), cp), o) for (w, cp), o in zip(c3, outs))
        active = self  # last: a node that raised above leaves nothing behind
        return self

    def __exit__(self, *exc):
        global active
        active = None


def wc(w, dt):
    """compute-dtype copy of the weight ``w``: the staged one, else a plain differentiable cast"""
    c = active.weights.get(id(w)) if active is not None else None
    return c if c is not None and c.dtype == dt else w.to(dt)


def w2(conv_or_lin, dt):
    """[N, K] compute-dtype view of a Linear / 1x1-conv weight (differentiable)."""
    w = wc(conv_or_lin.weight, dt)
    return w.reshape(w.shape[0], -1)


def lora_merged(w) -> bool:
    return active is not None and id(w) in active.merged
