"""IP-Adapter image prompts on the UNet (Ye et al., arXiv 2308.06721; the reference's pipeline derives from diffusers 0.24's
``IPAdapterMixin``, models/pipeline.py:11,125, and its UNet has the ``encoder_hid_dim_type == "ip_image_proj"`` branch,
models/controlnet.py:1009-1016).

``UNetIPAdapterMixin._load_ip_adapter_weights`` reads the original IP-Adapter layout

    image_proj.proj.{weight,bias}      Linear(clip_dim -> N * cross_attention_dim)
    image_proj.norm.{weight,bias}      LayerNorm(cross_attention_dim) over the N tokens
    ip_adapter.{id}.to_k_ip.weight     [inner, cross_attention_dim], bias-free, one pair per cross-attention
    ip_adapter.{id}.to_v_ip.weight

where ``id`` counts the attention processors in diffusers' ``attn_processors`` order (``attn_processor_ids``).  Per forward the
projection, its LayerNorm and ONE GEMM over the stacked ``[to_k_ip ; to_v_ip]`` of all cross-attentions run on the existing
``ops.linear`` / ``ops.layernorm`` (``ip_context``); every UNet cross-attention then adds
``scale * softmax(q k_ip^T) v_ip`` to its prompt attention with one ``ops.ip_attention_add`` launch.  Inference only.

The image embeddings enter through a STATIC device buffer per batch size (``set_ip_adapter_image_embeds``): the step executors
(``fused.GroupedDualStreamStep``, ``hoist.HoistedSamplingStep``) and their captured graphs read it, so new embeddings are a
device copy, never a re-capture.  What a capture bakes in -- the adapter's identity, its scale, the buffer -- is
``ip_adapter_state``, part of the pipeline's graph key.
"""
from __future__ import annotations

import itertools
import math
import os
from collections import OrderedDict
from typing import Dict, Optional

import torch

from . import ops

IP_MAX_TOKENS = ops.IPA_MAX_TOKENS
IP_AUTOGRAD_MSG = ("an IP-Adapter is loaded on this network, but the differentiable path has no backward for its decoupled "
                   "cross-attention: image prompts are a sampling-time switch -- call unload_ip_adapter() for training, or run "
                   "the forward under torch.no_grad()")
IP_WEIGHT_NAME = "ip_adapter.safetensors"
_serial = itertools.count(1)


def attn_processor_ids(unet) -> "OrderedDict[int, str]":
    """``{id: module path}`` of every attention of ``unet`` in diffusers' ``attn_processors`` order: ``down_blocks``, then
    ``up_blocks``, then ``mid_block`` (the order the reference registers them in, controlnet.py:393-394,465), and per transformer
    block ``attn1`` then ``attn2``.  For the SD-1.x UNet the 16 cross-attentions are the odd ids 1, 3, ..., 31 (down 1..11,
    up 13..29, mid 31)."""
    ids, n = OrderedDict(), 0
    for top in ("down_blocks", "up_blocks", "mid_block"):
        for name, m in getattr(unet, top).named_modules():
            if name.endswith((".attn1", ".attn2")):
                ids[n] = f"{top}.{name}"
                n += 1
    return ids


def read_ip_adapter_file(path_or_dict, subfolder: Optional[str] = None, weight_name: Optional[str] = None) -> Dict[str, torch.Tensor]:
    """A state dict as given (flat keys, or diffusers' nested ``{"image_proj": {...}, "ip_adapter": {...}}``), or a local
    ``.safetensors`` / ``.bin`` file -- the path itself, or ``weight_name`` under ``path[/subfolder]``.  Nothing is downloaded."""
    if isinstance(path_or_dict, dict):
        sd = path_or_dict
    else:
        path = os.fspath(path_or_dict)
        if os.path.isdir(path):
            path = os.path.join(*(p for p in (path, subfolder, weight_name or IP_WEIGHT_NAME) if p))
        if not os.path.isfile(path):
            raise FileNotFoundError(f"{path}: no such IP-Adapter file (local files only; nothing is loaded from a hub)")
        if path.endswith(".safetensors"):
            from safetensors.torch import load_file

            sd = load_file(path)
        else:
            sd = torch.load(path, map_location="cpu", weights_only=True)
    flat = {}
    for k, v in sd.items():
        if isinstance(v, dict) and k in ("image_proj", "ip_adapter"):
            flat.update({f"{k}.{kk}": vv for kk, vv in v.items()})
        else:
            flat[k] = v
    return flat


class ImageProjection:
    """diffusers' ``ImageProjection`` as the UNet's ``encoder_hid_proj``: ``image_embeds`` [B, clip_dim] -> N tokens
    [B, N, cross_attention_dim] = LayerNorm(Linear(image_embeds).reshape(B, N, -1)).  A holder of the adapter's tensors (not an
    ``nn.Module``: they stay out of the UNet's ``state_dict``); calling it runs ``ops.linear`` + ``ops.layernorm``."""

    def __init__(self, state: "_IpAdapterState"):
        self._st = state
        self.num_image_text_embeds = state.n_tokens

    def __call__(self, image_embeds: torch.Tensor, dtype=None) -> torch.Tensor:
        st = self._st
        dt = dtype or image_embeds.dtype
        e = torch.zeros(image_embeds.shape[0], st.clip_pad, dtype=dt, device=image_embeds.device)
        e[:, : st.clip_dim] = image_embeds
        return st.tokens(e)


class _IpAdapterState:
    """What a UNet with an adapter keeps: the adapter's tensors by their original keys, the scale, the column slice of every
    cross-attention in the stacked image K | V projection, the packed copies and the static embedding buffers."""

    eps = 1e-5  # nn.LayerNorm's default, what ImageProjection constructs

    def __init__(self, tensors, clip_dim, n_tokens, cross_dim, slices, total):
        self.tensors: Dict[str, torch.Tensor] = tensors
        self.clip_dim, self.n_tokens, self.cross_dim = clip_dim, n_tokens, cross_dim
        self.clip_pad = (clip_dim + 63) // 64 * 64  # the GEMM's K granularity; the pad columns of the weight are zero
        self.slices: Dict[int, tuple] = slices     # id(Attention) -> (lo, hi) of the stacked inner dimensions
        self.ids: "OrderedDict[int, str]" = OrderedDict()
        self.total = total
        self.scale = 1.0
        self.serial = next(_serial)
        self.saved_config: Dict[str, object] = {}
        self._packed = {}
        self._embeds: Dict[tuple, torch.Tensor] = {}

    def packed(self, dt, device):
        key = (dt, str(device))
        hit = self._packed.get(key)
        if hit is None:
            t = self.tensors
            f32 = lambda x: x.detach().to(device=device, dtype=torch.float32).contiguous()
            wp = torch.zeros(t["image_proj.proj.weight"].shape[0], self.clip_pad, dtype=dt, device=device)
            wp[:, : self.clip_dim] = t["image_proj.proj.weight"].to(device=device, dtype=dt)
            order = sorted(self.ids)  # ids in ascending order = the order of ``slices``
            wkv = torch.cat([t[f"ip_adapter.{i}.to_k_ip.weight"] for i in order]
                            + [t[f"ip_adapter.{i}.to_v_ip.weight"] for i in order], 0).to(device=device, dtype=dt).contiguous()
            hit = (wp, f32(t["image_proj.proj.bias"]), f32(t["image_proj.norm.weight"]), f32(t["image_proj.norm.bias"]), wkv)
            self._packed[key] = hit
        return hit

    def buffer(self, B, dt, device, create=False) -> Optional[torch.Tensor]:
        key = (B, dt, str(device))
        buf = self._embeds.get(key)
        if buf is None and create:
            buf = self._embeds[key] = torch.zeros(B, self.clip_pad, dtype=dt, device=device)
        return buf

    def tokens(self, embeds_padded: torch.Tensor) -> torch.Tensor:
        """[B, clip_pad] -> [B, N, cross]: the projection and its LayerNorm."""
        dt, dev = embeds_padded.dtype, embeds_padded.device
        wp, bp, g, b, _ = self.packed(dt, dev)
        B = embeds_padded.shape[0]
        y = ops.linear(embeds_padded, wp, bp)                                   # [B, N * cross]
        return ops.layernorm(y.view(B * self.n_tokens, self.cross_dim), g, b, self.eps).view(B, self.n_tokens, self.cross_dim)

    def kv(self, embeds_padded: torch.Tensor) -> torch.Tensor:
        """[B, N, 2 * total]: to_k_ip of every cross-attention in columns [0, total), to_v_ip in [total, 2 total) -- one GEMM
        of B * N rows over the stacked weights."""
        tok = self.tokens(embeds_padded)
        return ops.linear(tok, self.packed(tok.dtype, tok.device)[4])


class IpContext:
    """The image K | V of one forward: what the executors hand to ``ops.ip_attention_add``."""

    __slots__ = ("kv", "scale", "slices", "total")

    def __init__(self, kv, scale, slices, total):
        self.kv, self.scale, self.slices, self.total = kv, scale, slices, total

    def of(self, attn):
        """(k_ip, v_ip) [B, N, inner] column slices for the cross-attention ``attn``, or None (not adapted, or scale 0)."""
        sl = self.slices.get(id(attn))
        if sl is None or self.scale == 0:
            return None
        lo, hi = sl
        return self.kv[:, :, lo:hi], self.kv[:, :, self.total + lo: self.total + hi]


class UNetIPAdapterMixin:
    """``_load_ip_adapter_weights`` / ``set_ip_adapter_scale`` / ``unload_ip_adapter`` of ``UNet2DConditionModel``.  The adapter's
    tensors live under the ONE container attribute ``_ip`` (an ``_IpAdapterState``, no ``nn.Module``), outside ``parameters()``,
    ``state_dict()`` and ``save_pretrained()`` -- those keep the network's own keys and configuration, as with the LoRA
    factors; ``.to()`` does not move them either (they are cast and placed per forward, cached)."""

    _ip: Optional[_IpAdapterState] = None
    encoder_hid_proj = None

    def _load_ip_adapter_weights(self, state_dict):
        """Attach the adapter ``state_dict`` (original IP-Adapter layout, see the module docstring): sets ``encoder_hid_proj``,
        ``config["encoder_hid_dim_type"] = "ip_image_proj"`` and ``config["encoder_hid_dim"]``; every cross-attention of the
        UNet gets its ``to_k_ip`` / ``to_v_ip``.  One adapter at a time; ``N = proj.weight.shape[0] // cross_attention_dim``
        image tokens, at most 16 (the "plus" / FaceID Resampler projections are not supported)."""
        if self._ip is not None:
            raise ValueError("an IP-Adapter is already loaded (several adapters at once are not supported); unload_ip_adapter() first")
        sd = read_ip_adapter_file(state_dict)
        need = lambda k: sd[k] if k in sd else (_ for _ in ()).throw(KeyError(f"IP-Adapter state dict has no {k!r}"))
        for k in sd:
            if k.startswith("image_proj.") and k not in ("image_proj.proj.weight", "image_proj.proj.bias", "image_proj.norm.weight",
                                                         "image_proj.norm.bias"):
                raise NotImplementedError(f"IP-Adapter key {k!r}: only the ImageProjection of the original IP-Adapter is supported "
                                          "(no Resampler / FaceID projections)")
        pw, pb, nw, nb = (need(f"image_proj.{k}") for k in ("proj.weight", "proj.bias", "norm.weight", "norm.bias"))
        ids = attn_processor_ids(self)
        mods = dict(self.named_modules())
        cross_ids = [i for i, p in ids.items() if p.endswith(".attn2")]
        if not cross_ids:
            raise ValueError("this UNet has no cross-attention to adapt")
        cross = mods[ids[cross_ids[0]]].to_k.weight.shape[1]
        if nw.dim() != 1 or nw.shape[0] != cross or tuple(nb.shape) != tuple(nw.shape):
            raise ValueError(f"IP-Adapter key 'image_proj.norm.weight': shape {tuple(nw.shape)} (bias {tuple(nb.shape)}) does not fit "
                             f"cross_attention_dim {cross}")
        if pw.dim() != 2 or pw.shape[0] % cross or pw.shape[0] == 0 or tuple(pb.shape) != (pw.shape[0],):
            raise ValueError(f"IP-Adapter key 'image_proj.proj.weight': shape {tuple(pw.shape)} (bias {tuple(pb.shape)}) is no "
                             f"Linear(clip_dim -> N * {cross})")
        n_tokens = pw.shape[0] // cross
        if n_tokens > IP_MAX_TOKENS:
            raise NotImplementedError(f"IP-Adapter key 'image_proj.proj.weight': {n_tokens} image tokens; at most {IP_MAX_TOKENS} are "
                                      "supported")
        tensors = {f"image_proj.{k}": v.detach().clone() for k, v in
                   (("proj.weight", pw), ("proj.bias", pb), ("norm.weight", nw), ("norm.bias", nb))}
        slices, off = {}, 0
        for i in cross_ids:
            a = mods[ids[i]]
            for nm in ("to_k_ip", "to_v_ip"):
                key = f"ip_adapter.{i}.{nm}.weight"
                w = need(key)
                if tuple(w.shape) != (a.inner, a.to_k.weight.shape[1]):
                    raise ValueError(f"IP-Adapter key {key!r}: shape {tuple(w.shape)} does not fit {ids[i]} "
                                     f"({a.to_k.weight.shape[1]} -> {a.inner})")
                tensors[key] = w.detach().clone()
            slices[id(a)] = (off, off + a.inner)
            off += a.inner
        extra = [k for k in sd if k.startswith("ip_adapter.") and k not in tensors]
        if extra:
            raise ValueError(f"IP-Adapter key {extra[0]!r} matches no cross-attention of this UNet (its cross-attention ids are "
                             f"{cross_ids})")
        st = _IpAdapterState(tensors, pw.shape[1], n_tokens, cross, slices, off)
        st.ids = OrderedDict((i, ids[i]) for i in cross_ids)
        st.saved_config = {k: self.config.get(k) for k in ("encoder_hid_dim_type", "encoder_hid_dim")}
        self._ip = st
        self.encoder_hid_proj = ImageProjection(st)
        self.config["encoder_hid_dim_type"] = "ip_image_proj"
        self.config["encoder_hid_dim"] = st.clip_dim

    def set_ip_adapter_scale(self, scale: float):
        """The weight of the image prompt in every cross-attention (``hidden + scale * ip``).  0 launches nothing.  A kernel
        argument of a captured step: part of ``ip_adapter_state``."""
        if self._ip is None:
            raise ValueError("set_ip_adapter_scale: no IP-Adapter is loaded")
        scale = float(scale)
        if not math.isfinite(scale):
            raise ValueError("set_ip_adapter_scale: the scale is not finite")
        self._ip.scale = scale

    def unload_ip_adapter(self):
        """Drop the adapter: configuration, ``encoder_hid_proj`` and behaviour exactly as before the load."""
        st = self._ip
        if st is None:
            return
        for k, v in st.saved_config.items():
            self.config[k] = v
        self._ip = None
        self.encoder_hid_proj = None

    def save_pretrained(self, save_directory: str, **kwargs):
        """The network's own configuration and keys: a loaded adapter is not part of the checkpoint."""
        st = self._ip
        if st is None:
            return super().save_pretrained(save_directory, **kwargs)
        now = {k: self.config[k] for k in st.saved_config}
        try:
            for k, v in st.saved_config.items():
                self.config[k] = v
            return super().save_pretrained(save_directory, **kwargs)
        finally:
            for k, v in now.items():
                self.config[k] = v

    # ------------------------------------------------------------------ per forward
    def set_ip_adapter_image_embeds(self, image_embeds: torch.Tensor, dtype=None):
        """Copy ``image_embeds`` [B, clip_dim] into the static device buffer for batch B that the executors (and the graphs
        captured from them) read.  Returns the buffer."""
        st = self._ip
        if st is None:
            raise ValueError("image_embeds were passed but no IP-Adapter is loaded (load_ip_adapter first)")
        if image_embeds.dim() != 2 or image_embeds.shape[1] != st.clip_dim:
            raise ValueError(f"image_embeds must be [batch, {st.clip_dim}], got {tuple(image_embeds.shape)}")
        from .controlnet import _compute_dtype

        dt = dtype or _compute_dtype(self.dtype, self.compute_dtype)
        buf = st.buffer(image_embeds.shape[0], dt, self.device, create=True)
        if image_embeds.data_ptr() != buf.data_ptr():  # (the buffer's own view: ``ip_added_cond_kwargs``)
            buf[:, : st.clip_dim].copy_(image_embeds)
        return buf

    def ip_added_cond_kwargs(self, B: int):
        """``added_cond_kwargs`` that hand ``forward`` the embeddings already in the static buffer for batch B (None without
        an adapter): what a step executor that goes through ``forward`` passes."""
        st = self._ip
        if st is None:
            return None
        from .controlnet import _compute_dtype

        buf = st.buffer(B, _compute_dtype(self.dtype, self.compute_dtype), self.device)
        if buf is None:
            raise ValueError(image_embeds_msg(type(self)))
        return {"image_embeds": buf[:, : st.clip_dim]}

    def ip_context(self, B: int, dt) -> Optional[IpContext]:
        """The image K | V of a forward over B samples from the static buffer (None without an adapter or at scale 0)."""
        st = self._ip
        if st is None or st.scale == 0:
            return None
        buf = st.buffer(B, dt, self.device)
        if buf is None:
            raise ValueError(image_embeds_msg(type(self)))
        return IpContext(st.kv(buf), st.scale, st.slices, st.total)

    def ip_adapter_state(self):
        """What a captured graph of this network bakes in of the adapter: its identity, token count and scale (None: no adapter).
        The static embedding buffers live as long as the adapter, so their addresses follow from the identity."""
        st = self._ip
        return None if st is None else (st.serial, st.n_tokens, st.scale)


def image_embeds_msg(cls) -> str:
    """The reference's message (models/controlnet.py:1010-1013)."""
    return (f"{cls} has the config param `encoder_hid_dim_type` set to 'ip_image_proj' which requires the keyword argument "
            "`image_embeds` to be passed in  `added_conditions`")
