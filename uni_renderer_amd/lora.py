"""LoRA adapters for ``UNet2DConditionModel``, merged into the weights (the counterpart of the reference's
``UNet2DConditionLoadersMixin.load_attn_procs`` / ``fuse_lora`` and of ``cross_attention_kwargs={"scale": s}``).

An adapter never becomes a second pair of GEMMs here: ``W + s * sum_adapters (alpha / rank) * weight * up @ down`` is
written IN PLACE into the parameter by one grouped HIP launch per ``multi_max()`` (48) matrices (``ur_lora_merge_multi``,
csrc/lora.hip) and the parameter's version counter is bumped, so every packed copy (one cache class, ``packs.PackCache``,
valid for the versions of exactly the parameters its recipe reads: module forwards, grouped / hoisted step, VAE) and every captured
graph (``graph.py``, ``pipeline._weights_signature``) is rebuilt on its next use.  The
step keeps its launch count and its graph.

The model keeps, per adapted parameter, one untouched copy (``base``, taken at the first merge), the fp32 factors on the
parameter's device and the scale currently merged.  ``state_dict()`` of a model with a merged adapter therefore returns
the MERGED weights (what diffusers returns after ``fuse_lora``); ``unload_lora()`` puts ``base`` back bit for bit.

Key formats of ``load_attn_procs`` (an optional leading ``unet.`` on all of them):
  ``<module>.lora.down.weight`` / ``<module>.lora.up.weight``                       current diffusers
  ``<module>.lora_A.weight`` / ``<module>.lora_B.weight``                           PEFT (A = down, B = up)
  ``<attention>.processor.to_{q,k,v,out}_lora.{down,up}.weight``                    legacy attention processors
where ``<module>`` is any ``Linear`` / ``Conv2d`` of the UNet under its ``state_dict`` name.  kohya ``lora_unet_*`` names,
keys that match no module and factors whose shapes do not fit raise a ``ValueError`` naming the key.

Training an adapter.  ``add_adapter`` (fresh factors: ``down`` ~ N(0, (1/rank)^2), ``up`` = 0) and
``load_attn_procs(..., trainable=True)`` (resuming) register the fp32 factors as ``nn.Parameter``s under ONE container
attribute of the UNet, ``lora_factors``: ``unet.parameters()`` yields them (optimizers, clipping, ``GradientBuckets`` and the
graph signatures see them), ``state_dict()`` / ``load_state_dict()`` / ``save_pretrained()`` do not -- the network's checkpoint
keeps its keys; ``save_attn_procs`` writes the file ``load_attn_procs`` reads.  The adapted weights are frozen by these calls.
Under autograd the step still runs on merged weights: one autograd node per network forward (``autograd_ops.LoraMerge``)
writes ``W' = base + s * (alpha / rank) * up @ down`` for all adapted matrices into one compute-dtype buffer with one grouped
launch per 48 matrices (``ur_lora_merge_cast_multi``: fp32 ``base`` in, ONE rounding), the network runs forward and backward
on ``W'`` exactly as on cast weights -- deferred, grouped ``ur_wgrad_group`` included -- and the node's backward projects the
weight gradients ``dW'`` onto the factors, again one grouped launch per 48 matrices (``ur_lora_grad_multi``):
``d_up = s (alpha / rank) dW' down^T``, ``d_down = s (alpha / rank) up^T dW'``.  The parameters and ``base`` are never written
by the differentiable forward; the inference path re-merges when the scale OR any factor's ``(data_ptr, _version)`` differs
from what the last merge read, so a ``no_grad`` forward after optimizer steps sees the updated factors.
The alternative that was not built: projecting without ever forming ``dW'`` (``dy^T (x down^T)``) needs fewer FLOPs but four
skinny GEMMs per layer and a grouped kernel family of its own.  Out of scope: trainable adapters on 3x3 convs (the
differentiable path keeps those weights in the packed ``[N][(ky, kx, c)]`` layout, which is not the matrix the factors multiply),
on the encoder / decoder networks and on the text encoder, kohya files, several trainable adapters at once, dropout in the LoRA
branch, optimizer-state resume through ``checkpointing.py`` and multi-GPU runs.
"""
from __future__ import annotations

import os
import re
from collections import OrderedDict
from typing import Dict, List, Optional

import torch
import torch.nn as nn

from . import _lib

LORA_WEIGHT_NAME = "pytorch_lora_weights.safetensors"
ITEM_WORDS = 9  # int64_t words per item of ur_lora_merge_multi's table: base, w, up, down, rscale, N, K, R, scale bits
GRAD_ITEM_WORDS = 10  # ... of ur_lora_grad_multi's: dw, up, down, rscale, d_up, d_down, N, K, R, scale bits
FACTORS_ATTR = "lora_factors"  # the container attribute of a UNet with a trainable adapter
_DT = {torch.float16: _lib.ABI.UR_DT_F16, torch.bfloat16: _lib.ABI.UR_DT_BF16, torch.float32: _lib.ABI.UR_DT_F32}

_PATTERNS = (
    (re.compile(r"(.+)\.processor\.to_(q|k|v|out)_lora\.(down|up)\.weight"), "legacy"),
    (re.compile(r"(.+)\.lora\.(down|up)\.weight"), "diffusers"),
    (re.compile(r"(.+)\.lora_(A|B)\.weight"), "peft"),
)


def scale_of(cross_attention_kwargs) -> Optional[float]:
    """The LoRA scale of a ``cross_attention_kwargs`` dict (``None`` when absent).  ``scale`` is the only key the reference's
    SD-1.x attention processors read; any other key raises ``NotImplementedError``."""
    if cross_attention_kwargs is None:
        return None
    other = [k for k in cross_attention_kwargs if k != "scale"]
    if other:
        raise NotImplementedError(f"cross_attention_kwargs[{other[0]!r}] is not supported on the MI355X hot path "
                                  "(only 'scale', the LoRA scale, is)")
    s = cross_attention_kwargs.get("scale")
    return None if s is None else float(s)


def _strip(key: str) -> str:
    return key[len("unet."):] if key.startswith("unet.") else key


def _split_key(key: str):
    """``(module name, 'down' | 'up')`` of a factor key, or ``None`` when it has none of the three spellings."""
    k = _strip(key)
    for pat, kind in _PATTERNS:
        m = pat.fullmatch(k)
        if not m:
            continue
        if kind == "legacy":
            proj = m.group(2)
            return f"{m.group(1)}.{'to_out.0' if proj == 'out' else 'to_' + proj}", m.group(3)
        if kind == "peft":
            return m.group(1), "down" if m.group(2) == "A" else "up"
        return m.group(1), m.group(2)
    return None


def parse_adapter(model: nn.Module, state_dict: Dict[str, torch.Tensor], network_alphas: Optional[Dict[str, float]] = None):
    """``{module name: (down fp32 [R][K], up fp32 [N][R], alpha / R)}`` of one adapter file for ``model``, the factors of a
    conv flattened as diffusers' ``_fuse_lora`` multiplies them.  Keys ending in ``.alpha`` are alphas (as
    ``network_alphas``).  Raises ``ValueError`` naming the first key it cannot place."""
    modules = {n: m for n, m in model.named_modules() if isinstance(m, (nn.Linear, nn.Conv2d))}
    alphas = {}
    for src in (network_alphas or {}), {k: v for k, v in state_dict.items() if k.endswith(".alpha")}:
        for k, v in src.items():
            name = _strip(k)
            name = name[:-len(".alpha")] if name.endswith(".alpha") else name
            for suffix in (".lora", ".processor"):
                name = name[:-len(suffix)] if name.endswith(suffix) else name
            if name not in modules:
                raise ValueError(f"LoRA alpha {k!r} names no Linear / Conv2d of {type(model).__name__}")
            alphas[name] = float(v)
    found: Dict[str, Dict[str, tuple]] = OrderedDict()
    for key, t in state_dict.items():
        if key.endswith(".alpha"):
            continue
        if _strip(key).startswith("lora_unet_") or key.startswith("lora_te_"):
            raise ValueError(f"LoRA key {key!r} is in the kohya format, which is not supported: convert the file to the "
                             "diffusers key layout first")
        hit = _split_key(key)
        if hit is None or hit[0] not in modules:
            raise ValueError(f"LoRA key {key!r} matches no Linear / Conv2d of {type(model).__name__}")
        if hit[1] in found.setdefault(hit[0], {}):
            raise ValueError(f"LoRA key {key!r} repeats the {hit[1]} factor of {hit[0]}")
        found[hit[0]][hit[1]] = (key, t)
    out = OrderedDict()
    for name, parts in found.items():
        if len(parts) != 2:
            key = next(iter(parts.values()))[0]
            raise ValueError(f"LoRA key {key!r} has no {'up' if 'down' in parts else 'down'} factor beside it")
        (kd, down), (ku, up) = parts["down"], parts["up"]
        w = modules[name].weight
        N, K = w.shape[0], w[0].numel()
        if w.dim() == 4 and down.dim() == 4 and tuple(down.shape[2:]) != tuple(w.shape[2:]):
            raise ValueError(f"LoRA key {kd!r}: kernel size {tuple(down.shape[2:])} differs from the module's {tuple(w.shape[2:])}")
        if down.dim() not in (2, 4) or down.dim() > w.dim() or down[0].numel() != K:
            raise ValueError(f"LoRA key {kd!r}: shape {tuple(down.shape)} does not fit {name} with weight {tuple(w.shape)}")
        R = down.shape[0]
        if up.dim() not in (2, 4) or up.dim() > w.dim() or up.shape[0] != N or up[0].numel() != R or R < 1:
            raise ValueError(f"LoRA key {ku!r}: shape {tuple(up.shape)} does not fit {name} with weight {tuple(w.shape)} "
                             f"and rank {R}")
        f = lambda t: t.detach().to(device=w.device, dtype=torch.float32).reshape(t.shape[0], -1).contiguous()
        out[name] = (f(down), f(up), alphas[name] / R if name in alphas else 1.0)
    if not out:
        raise ValueError("the LoRA state dict holds no factor")
    return out


def alpha_modules(state_dict, network_alphas=None) -> set:
    """The module names an adapter file (``.alpha`` keys) or ``network_alphas`` give an alpha for."""
    out = set()
    for src in (network_alphas or {}), [k for k in state_dict if k.endswith(".alpha")]:
        for k in src:
            name = _strip(k)
            name = name[:-len(".alpha")] if name.endswith(".alpha") else name
            for suffix in (".lora", ".processor"):
                name = name[:-len(suffix)] if name.endswith(suffix) else name
            out.add(name)
    return out


def read_lora_file(path_or_dict, weight_name: Optional[str] = None) -> Dict[str, torch.Tensor]:
    """A state dict as given, a ``.safetensors`` file, or a directory holding ``weight_name``.  Local files only."""
    if isinstance(path_or_dict, dict):
        return dict(path_or_dict)
    path = os.fspath(path_or_dict)
    if os.path.isdir(path):
        path = os.path.join(path, weight_name or LORA_WEIGHT_NAME)
    if not os.path.isfile(path):
        raise FileNotFoundError(f"{path}: no such LoRA file (local files only; nothing is downloaded)")
    from safetensors.torch import load_file

    return load_file(path)


class LoraFactors(nn.Module):
    """The container of a trainable adapter's factors: ``nn.Parameter``s that ``parameters()`` of the model yields and its
    ``state_dict()`` / ``load_state_dict()`` do not see.  ``names[i]`` is the module of the pair ``down_i`` / ``up_i``."""

    def __init__(self):
        super().__init__()
        self.names: List[str] = []

    def add(self, name: str, down: torch.Tensor, up: torch.Tensor):
        i = len(self.names)
        self.names.append(name)
        self.register_parameter(f"down_{i}", nn.Parameter(down, requires_grad=True))
        self.register_parameter(f"up_{i}", nn.Parameter(up, requires_grad=True))
        return getattr(self, f"down_{i}"), getattr(self, f"up_{i}")

    def state_dict(self, *args, destination=None, prefix="", keep_vars=False):
        return destination if destination is not None else OrderedDict()

    def _save_to_state_dict(self, destination, prefix, keep_vars):
        return

    def _load_from_state_dict(self, *args, **kwargs):
        return


class _LoraState:
    """What a model with adapters keeps: the adapters, the active ones with their weights, the ``base`` copies and the
    merged / pinned scale."""

    def __init__(self):
        self.trainable: Optional[str] = None       # the adapter whose factors are Parameters (LoraFactors), if any
        self.alphas: Dict[str, Dict[str, float]] = {}  # adapter -> {module: lora_alpha} where one was given (lora_state_dict)
        self.thawed: List[str] = []                # modules whose weight required a gradient before the trainable adapter froze it
        self.factor_sig: Optional[tuple] = None    # (data_ptr, _version) of every active factor as the last merge read them
        self.adapters: "OrderedDict[str, dict]" = OrderedDict()
        self.active: List[str] = []
        self.weights: Dict[str, float] = {}
        self.base: Dict[str, torch.Tensor] = {}
        self.written: Dict[str, tuple] = {}        # (data_ptr, _version) of each adapted parameter as the last merge left it
        self.merged_scale: Optional[float] = None  # None: the parameters hold `base` (nothing merged yet)
        self.fused_scale: Optional[float] = None   # not None: fuse_lora() pinned the merge, per-call scales are ignored
        self._assembled = None

    def modules(self) -> List[str]:
        seen = OrderedDict()
        for a in self.adapters.values():
            for name in a:
                seen[name] = True
        return list(seen)

    def assembled(self):
        """``{module name: (up [N][R], down [R][K], rscale [R]) or None}`` over the ACTIVE adapters, concatenated along r in
        the order of ``active``; ``None`` for a module no active adapter touches (it is restored from ``base``)."""
        if self._assembled is None:
            out = OrderedDict()
            for name in self.modules():
                ups, downs, rs = [], [], []
                for a in self.active:
                    if name in self.adapters[a]:
                        down, up, factor = self.adapters[a][name]
                        ups.append(up)
                        downs.append(down)
                        rs.append(torch.full((down.shape[0],), factor * self.weights[a], dtype=torch.float32, device=down.device))
                if not ups:
                    out[name] = None
                    continue
                R = sum(d.shape[0] for d in downs)
                cap = max_rank()
                if R > cap:
                    raise ValueError(f"{name}: the active adapters have {R} ranks in all, more than the {cap} one "
                                     "merge supports")
                out[name] = (torch.cat(ups, 1).contiguous(), torch.cat(downs, 0).contiguous(), torch.cat(rs).contiguous())
            self._assembled = out
        return self._assembled


def factor_signature(st: _LoraState) -> tuple:
    """``(data_ptr, _version)`` of every factor of the active adapters."""
    return tuple((t.data_ptr(), t._version) for a in st.active for down, up, _ in st.adapters[a].values() for t in (down, up))


def multi_max() -> int:
    """Items per launch of ``ur_lora_merge_multi`` (the library's ``ur_lora_multi_max``)."""
    return int(_lib.load().ur_lora_multi_max())


def max_rank() -> int:
    """Ranks per item, all active adapters together (the library's ``ur_lora_max_rank``)."""
    return int(_lib.load().ur_lora_max_rank())


def item_tables(rows, nmax: int) -> list:
    """The item tables of ``ur_lora_merge_multi`` over ``rows`` of (base, w, up, down, rscale, scale) -- tensors, ``up`` /
    ``down`` / ``rscale`` ``None`` for the copy path (R = 0) or for ones: one ctypes ``int64_t [k][9]`` array and its k per
    ``nmax`` rows."""
    import ctypes
    import struct

    def words(row):
        base, w, up, down, rscale, scale = row
        ptr = lambda t: 0 if t is None else t.data_ptr()
        return (base.data_ptr(), w.data_ptr(), ptr(up), ptr(down), ptr(rscale), w.shape[0], w[0].numel(),
                0 if up is None else up.shape[1], struct.unpack("<I", struct.pack("<f", scale))[0])

    tables = []
    for i in range(0, len(rows), nmax):
        part = rows[i:i + nmax]
        tables.append(((ctypes.c_int64 * (ITEM_WORDS * len(part)))(*(int(x) for row in part for x in words(row))), len(part)))
    return tables


def merge_items(rows, dtype: torch.dtype) -> None:
    """One ``ur_lora_merge_multi`` launch per ``multi_max()`` rows (``item_tables``) of one dtype."""
    from .ops import _stream

    lib = _lib.load()
    if lib.ur_lora_item_words() != ITEM_WORDS:
        raise _lib.UrLibraryError(f"ur_lora_merge_multi takes {lib.ur_lora_item_words()} words per item, this package writes {ITEM_WORDS}")
    for table, k in item_tables(rows, multi_max()):
        _lib.check(lib.ur_lora_merge_multi(table, k, _DT[dtype], _stream()), "ur_lora_merge_multi")


def grad_item_tables(rows, nmax: int) -> list:
    """The item tables of ``ur_lora_grad_multi`` over ``rows`` of (dw, up, down, rscale or None, d_up, d_down, scale): one
    ctypes ``int64_t [k][10]`` array and its k per ``nmax`` rows."""
    import ctypes
    import struct

    def words(row):
        dw, up, down, rscale, d_up, d_down, scale = row
        return (dw.data_ptr(), up.data_ptr(), down.data_ptr(), 0 if rscale is None else rscale.data_ptr(), d_up.data_ptr(),
                d_down.data_ptr(), up.shape[0], down.shape[1], up.shape[1], struct.unpack("<I", struct.pack("<f", scale))[0])

    tables = []
    for i in range(0, len(rows), nmax):
        part = rows[i:i + nmax]
        tables.append(((ctypes.c_int64 * (GRAD_ITEM_WORDS * len(part)))(*(int(x) for row in part for x in words(row))), len(part)))
    return tables


def launch_merge_cast(tables, base_dtype: torch.dtype, out_dtype: torch.dtype) -> None:
    """``ur_lora_merge_cast_multi`` over ready ``item_tables``."""
    from .ops import _stream

    lib = _lib.load()
    for table, k in tables:
        _lib.check(lib.ur_lora_merge_cast_multi(table, k, _DT[base_dtype], _DT[out_dtype], _stream()), "ur_lora_merge_cast_multi")


def merge_cast_items(rows, base_dtype: torch.dtype, out_dtype: torch.dtype) -> None:
    """``merge_items`` with ``base`` read in ``base_dtype`` and ``w`` written in ``out_dtype``."""
    launch_merge_cast(item_tables(rows, multi_max()), base_dtype, out_dtype)


def launch_grad(tables, dw_dtype: torch.dtype) -> None:
    """``ur_lora_grad_multi`` over ready ``grad_item_tables``."""
    from .ops import _stream

    lib = _lib.load()
    if lib.ur_lora_grad_item_words() != GRAD_ITEM_WORDS:
        raise _lib.UrLibraryError(f"ur_lora_grad_multi takes {lib.ur_lora_grad_item_words()} words per item, this package writes {GRAD_ITEM_WORDS}")
    for table, k in tables:
        _lib.check(lib.ur_lora_grad_multi(table, k, _DT[dw_dtype], _stream()), "ur_lora_grad_multi")


def grad_items(rows, dw_dtype: torch.dtype) -> None:
    """One ``ur_lora_grad_multi`` launch per ``multi_max()`` rows (``grad_item_tables``) of one ``dw`` dtype."""
    launch_grad(grad_item_tables(rows, multi_max()), dw_dtype)


DEFAULT_TARGETS = ("to_q", "to_k", "to_v", "to_out.0")


class UNetLoraMixin:
    """``load_attn_procs`` / ``fuse_lora`` / ``unfuse_lora`` / ``unload_lora`` / ``set_adapters`` / ``lora_scale`` of
    ``UNet2DConditionModel`` (the encoder / decoder networks have no loader, as in the reference)."""

    _lora: Optional[_LoraState] = None

    @property
    def lora_scale(self) -> Optional[float]:
        """The scale currently merged into the weights (``None``: no adapter is merged)."""
        return None if self._lora is None else self._lora.merged_scale

    def load_attn_procs(self, pretrained_model_name_or_path_or_dict, weight_name: Optional[str] = None,
                        network_alphas: Optional[Dict[str, float]] = None, adapter_name: str = "default",
                        trainable: bool = False, **ignored_hub_kwargs):
        """Adds the adapter ``adapter_name`` (a state dict, a ``.safetensors`` file or a directory holding ``weight_name``;
        local files only) and makes it active beside those already loaded.  On the GPU the weights are merged at once at
        the pinned scale, or at 1.0 -- what a ``forward`` without ``cross_attention_kwargs`` uses.
        ``trainable=True`` (resuming a run): the loaded factors become parameters as those of ``add_adapter`` do."""
        sd = read_lora_file(pretrained_model_name_or_path_or_dict, weight_name)
        st = self._lora if self._lora is not None else _LoraState()
        if adapter_name in st.adapters:
            raise ValueError(f"adapter name {adapter_name!r} is already in use; unload_lora() first or pick another name")
        parsed = parse_adapter(self, sd, network_alphas)
        if trainable:
            parsed = self._lora_register(st, adapter_name, parsed,
                                         {n: f * parsed[n][0].shape[0] for n, (_, _, f) in parsed.items()
                                          if n in alpha_modules(sd, network_alphas)})
        st.adapters[adapter_name] = parsed
        st.active.append(adapter_name)
        st.weights[adapter_name] = 1.0
        st._assembled = None
        self._lora = st
        self._lora_remerge()

    def add_adapter(self, rank: int = 4, lora_alpha: Optional[float] = None, target_modules=DEFAULT_TARGETS,
                    adapter_name: str = "default", generator: Optional[torch.Generator] = None):
        """A fresh TRAINABLE adapter (diffusers' PEFT-era name for what the 0.24 training script does with
        ``LoRAAttnProcessor``s) on every ``nn.Linear`` / 1x1 ``nn.Conv2d`` whose name ends in one of ``target_modules``:
        ``down`` [rank][K] ~ N(0, (1 / rank)^2), ``up`` [N][rank] = 0 (``LoRALinearLayer``'s init), both fp32 parameters on
        the weight's device; the update is scaled by ``lora_alpha / rank`` (1 without ``lora_alpha``).  The adapter becomes
        loaded and active like one from ``load_attn_procs``; the adapted weights are frozen.  A target that resolves to a
        3x3 conv raises a ``ValueError`` naming the module (module docstring)."""
        rank = int(rank)
        if rank < 1 or rank > max_rank():
            raise ValueError(f"rank {rank}: 1 .. {max_rank()}")
        st = self._lora if self._lora is not None else _LoraState()
        if adapter_name in st.adapters:
            raise ValueError(f"adapter name {adapter_name!r} is already in use; unload_lora() first or pick another name")
        if st.trainable is not None:
            raise ValueError(f"adapter {st.trainable!r} is trainable already: several trainable adapters at once are not supported")
        targets = [target_modules] if isinstance(target_modules, str) else list(target_modules)
        parsed = OrderedDict()
        for name, m in self.named_modules():
            if name == FACTORS_ATTR or not any(name == t or name.endswith("." + t) for t in targets):
                continue
            if not isinstance(m, (nn.Linear, nn.Conv2d)):
                continue
            w = m.weight
            if isinstance(m, nn.Conv2d) and tuple(m.kernel_size) != (1, 1):
                raise ValueError(f"{name}: a trainable LoRA adapter on a {m.kernel_size[0]}x{m.kernel_size[1]} conv is not supported "
                                 "(Linear and 1x1 Conv2d are)")
            K = w[0].numel()
            down = torch.empty(rank, K, dtype=torch.float32)
            down.normal_(0.0, 1.0 / rank, generator=generator)
            parsed[name] = (down.to(w.device).contiguous(), torch.zeros(w.shape[0], rank, dtype=torch.float32, device=w.device),
                            1.0 if lora_alpha is None else float(lora_alpha) / rank)
        if not parsed:
            raise ValueError(f"target_modules {tuple(targets)} name no Linear / Conv2d of {type(self).__name__}")
        alphas = {} if lora_alpha is None else {n: float(lora_alpha) for n in parsed}
        st.adapters[adapter_name] = self._lora_register(st, adapter_name, parsed, alphas)
        st.active.append(adapter_name)
        st.weights[adapter_name] = 1.0
        st._assembled = None
        self._lora = st
        self._lora_remerge()

    def lora_parameters(self, adapter_name: Optional[str] = None) -> List[nn.Parameter]:
        """The factor parameters of the trainable adapter (down, up per module, in module order)."""
        st = self._lora_trainable(adapter_name)
        return [p for down, up, _ in st.adapters[st.trainable].values() for p in (down, up)]

    def lora_state_dict(self, adapter_name: Optional[str] = None) -> Dict[str, torch.Tensor]:
        """``{<module>.lora.down.weight, <module>.lora.up.weight, <module>.alpha}`` of the trainable adapter (alpha only where
        ``lora_alpha`` was given), conv factors 4-D as diffusers stores them: what ``load_attn_procs`` reads."""
        st = self._lora_trainable(adapter_name)
        out = OrderedDict()
        for name, (down, up, _) in st.adapters[st.trainable].items():
            conv = self.get_submodule(name).weight.dim() == 4
            d, u = down.detach().clone(), up.detach().clone()
            out[name + ".lora.down.weight"] = d.reshape(d.shape[0], -1, 1, 1) if conv else d
            out[name + ".lora.up.weight"] = u.reshape(u.shape[0], -1, 1, 1) if conv else u
            if name in st.alphas.get(st.trainable, {}):
                out[name + ".alpha"] = torch.tensor(st.alphas[st.trainable][name], dtype=torch.float32)
        return out

    def save_attn_procs(self, save_directory, weight_name: Optional[str] = None, safe_serialization: bool = True,
                        adapter_name: Optional[str] = None):
        """Writes ``lora_state_dict()`` to ``save_directory / pytorch_lora_weights.safetensors`` (or ``weight_name``)."""
        if not safe_serialization:
            raise NotImplementedError("save_attn_procs writes safetensors files only")
        from safetensors.torch import save_file

        os.makedirs(save_directory, exist_ok=True)
        sd = {k: v.contiguous().cpu() for k, v in self.lora_state_dict(adapter_name).items()}
        save_file(sd, os.path.join(os.fspath(save_directory), weight_name or LORA_WEIGHT_NAME))

    def set_adapters(self, adapter_names, adapter_weights=None):
        """Which loaded adapters are active, and their weights (default 1.0 each)."""
        st = self._lora_required()
        names = [adapter_names] if isinstance(adapter_names, str) else list(adapter_names)
        if adapter_weights is None:
            adapter_weights = [1.0] * len(names)
        elif not isinstance(adapter_weights, (list, tuple)):
            adapter_weights = [adapter_weights] * len(names)
        if len(adapter_weights) != len(names) or len(set(names)) != len(names):
            raise ValueError(f"{len(names)} adapter names (each once) need as many weights, got {len(adapter_weights)}")
        for n in names:
            if n not in st.adapters:
                raise ValueError(f"adapter {n!r} is not loaded (loaded: {list(st.adapters)})")
        st.active = names
        st.weights.update({n: float(w) for n, w in zip(names, adapter_weights)})
        st._assembled = None
        self._lora_remerge()

    def fuse_lora(self, lora_scale: float = 1.0):
        """Pins the merge at ``lora_scale``: per-call scales are ignored from now on, as in diffusers, where a fused layer
        has no LoRA branch left."""
        st = self._lora_required()
        st.fused_scale = float(lora_scale)
        self._lora_remerge()

    def unfuse_lora(self):
        """Back to per-call scaling (1.0 until a call asks for another scale)."""
        st = self._lora_required()
        st.fused_scale = None
        self._lora_remerge()

    def unload_lora(self, keep_weights: bool = False):
        """Restores every adapted parameter from its untouched copy, bit for bit, then frees the factors and the copies.
        ``keep_weights=True`` frees them without restoring: the parameters stay as they are (merged, or written since)."""
        st = self._lora
        if st is None:
            return
        if st.merged_scale is not None and not keep_weights:
            self._lora_check_params(st)
            by_dtype: Dict[torch.dtype, list] = {}
            for name, base in st.base.items():
                w = self.get_submodule(name).weight
                by_dtype.setdefault(w.dtype, []).append((name, (base, w.detach(), None, None, None, 0.0)))
            self._lora_launch(by_dtype)
        self._lora = None
        if FACTORS_ATTR in self._modules:
            del self._modules[FACTORS_ATTR]
        for name in st.thawed:
            self.get_submodule(name).weight.requires_grad_(True)

    # ---- internals ------------------------------------------------------------------------------------
    def _lora_register(self, st: _LoraState, adapter_name: str, parsed, alphas: Dict[str, float]):
        """Makes the factors of ``parsed`` parameters of the container and freezes the adapted weights; returns ``parsed``
        holding the parameters."""
        if st.trainable is not None:
            raise ValueError(f"adapter {st.trainable!r} is trainable already: several trainable adapters at once are not supported")
        for name in parsed:
            m = self.get_submodule(name)
            if isinstance(m, nn.Conv2d) and tuple(m.kernel_size) != (1, 1):
                raise ValueError(f"{name}: a trainable LoRA adapter on a {m.kernel_size[0]}x{m.kernel_size[1]} conv is not supported "
                                 "(Linear and 1x1 Conv2d are)")
        box = LoraFactors()
        out = OrderedDict()
        for name, (down, up, factor) in parsed.items():
            d, u = box.add(name, down.contiguous(), up.contiguous())
            out[name] = (d, u, factor)
            w = self.get_submodule(name).weight
            if w.requires_grad:
                st.thawed.append(name)  # unload_lora() gives the flag back
                w.requires_grad_(False)
        self.add_module(FACTORS_ATTR, box)
        st.trainable = adapter_name
        st.alphas[adapter_name] = dict(alphas)
        return out

    def _lora_trainable(self, adapter_name: Optional[str] = None) -> _LoraState:
        st = self._lora_required()
        if st.trainable is None or (adapter_name is not None and adapter_name != st.trainable):
            raise ValueError(f"adapter {adapter_name!r} is not trainable" if adapter_name is not None else
                             "no trainable LoRA adapter (add_adapter / load_attn_procs(..., trainable=True))")
        return st

    def _lora_train_plan(self, scale: Optional[float]):
        """What the differentiable forward needs (autograd_ops.LoraMerge): ``(rows, s)`` with rows of (weight parameter,
        source matrix, down, up, alpha / rank x adapter weight) per adapted module -- the source is ``base`` once something was
        merged into the parameter, else the parameter -- and ``s`` the scale in force.  Raises when the set-up cannot train."""
        st = self._lora
        if st.trainable is None:
            from .autograd_net import LORA_AUTOGRAD_MSG

            raise NotImplementedError(LORA_AUTOGRAD_MSG)
        if st.active != [st.trainable]:
            raise ValueError(f"training needs the trainable adapter {st.trainable!r} to be the only active one (active: "
                             f"{st.active}); set_adapters({st.trainable!r}) first")
        s = st.fused_scale if st.fused_scale is not None else (1.0 if scale is None else float(scale))
        rows = []
        for name, (down, up, factor) in st.adapters[st.trainable].items():
            w = self.get_submodule(name).weight
            if w.requires_grad:
                raise ValueError(f"{name}.weight requires a gradient beside its trainable LoRA adapter: freeze it "
                                 "(requires_grad_(False)); the factors carry its training")
            if down.device != w.device or up.device != w.device:
                raise RuntimeError(f"the LoRA factors of {name} are not on the weight's device")
            src = st.base[name] if (st.merged_scale is not None and name in st.base) else w
            rows.append((w, src.detach(), down, up, factor * st.weights[st.trainable]))
        return rows, s

    def _lora_required(self) -> _LoraState:
        if self._lora is None:
            raise ValueError("no LoRA adapter is loaded")
        return self._lora

    def _lora_apply(self, scale: Optional[float]) -> None:
        """Makes the weights those of ``scale`` (``None``: 1.0) unless the merge is pinned; a no-op without an adapter, and
        whenever the wanted scale is the merged one."""
        st = self._lora
        if st is None:
            return
        wanted = st.fused_scale if st.fused_scale is not None else (1.0 if scale is None else float(scale))
        stale = st.trainable is not None and st.factor_sig != factor_signature(st)  # an optimizer step wrote the factors
        if stale:
            st._assembled = None
        if st.merged_scale is None or wanted != st.merged_scale or stale:
            self._lora_merge(wanted)

    def _lora_remerge(self) -> None:
        """After a change of adapters / weights / pinning: merge again where the kernel can run (a model still on the CPU
        merges on its first call on the GPU)."""
        st = self._lora
        if next(self.parameters()).is_cuda:
            self._lora_merge(st.fused_scale if st.fused_scale is not None else 1.0)
        elif st.merged_scale is not None:
            raise RuntimeError("the model left the GPU with a LoRA adapter merged; unload_lora() before moving it")

    def _lora_check_params(self, st: _LoraState) -> None:
        for name, base in st.base.items():
            w = self.get_submodule(name).weight
            if w.device != base.device or w.dtype != base.dtype or w.shape != base.shape:
                raise RuntimeError(f"{name}.weight changed device, dtype or shape while a LoRA adapter was merged "
                                   "(move / cast the model before load_attn_procs, or unload_lora() first)")
            if name in st.written and (w.data_ptr(), w._version) != st.written[name]:
                # load_state_dict, an optimizer step, ...: merging again or restoring `base` would silently undo that write
                raise RuntimeError(f"{name}.weight was written from outside while a LoRA adapter was merged into it; the kept "
                                   "copy no longer is its base.  unload_lora(keep_weights=True) drops the adapter and keeps "
                                   "the parameters as they are; load weights before load_attn_procs")

    def _lora_merge(self, scale: float) -> None:
        st = self._lora
        if not next(self.parameters()).is_cuda:
            raise RuntimeError("merging a LoRA adapter needs the model on an MI355X (no CPU fallback)")
        self._lora_check_params(st)
        by_dtype: Dict[torch.dtype, list] = {}
        with torch.no_grad():
            for name, fac in st.assembled().items():
                w = self.get_submodule(name).weight
                if not w.is_contiguous():
                    raise RuntimeError(f"{name}.weight is not contiguous")
                if name not in st.base:
                    st.base[name] = w.detach().clone()
                if fac is not None and fac[0].device != w.device:  # loaded while the model was on the CPU
                    st._assembled[name] = fac = tuple(t.to(w.device) for t in fac)
                up, down, rscale = fac if fac is not None else (None, None, None)
                by_dtype.setdefault(w.dtype, []).append((name, (st.base[name], w.detach(), up, down, rscale, float(scale))))
        self._lora_launch(by_dtype)
        st.merged_scale = float(scale)
        st.factor_sig = factor_signature(st)

    def _lora_launch(self, by_dtype) -> None:
        """``by_dtype``: dtype -> [(module name, merge_items row)]."""
        for dtype, named in by_dtype.items():
            if dtype not in _DT:
                raise RuntimeError(f"LoRA merge into {dtype} weights is not supported")
            merge_items([row for _, row in named], dtype)
            for name, row in named:
                # every packed copy and captured graph is keyed by (data_ptr, _version) and so rebuilt on its next use;
                # detach() shares the parameter's version counter
                torch.autograd.graph.increment_version(row[1])
                self._lora.written[name] = (row[1].data_ptr(), row[1]._version)
