"""AdamW for the training loop on one HIP kernel (``ur_adamw_multi``, csrc/backward.hip).

The reference builds ``torch.optim.AdamW`` (or bitsandbytes' 8-bit variant) over the parameters of the three networks in
ONE parameter group (train/train.py:1082-1100: lr, betas, weight_decay, eps from the command line) and calls
``optimizer.step()`` once per batch (1425).  This class is that optimizer with the update of up to 64 parameter tensors
per launch (descriptors as kernel arguments: ~12 launches for the 700 tensors of enc + unet + dec instead of ~95
multi-tensor launches), fp32 state, the arithmetic of torch's fused AdamW kernel.

Interchangeable with ``torch.optim.AdamW``: same constructor arguments, ``param_groups`` and ``state_dict()`` layout
(``step`` / ``exp_avg`` / ``exp_avg_sq`` per parameter, so ``optimizer.bin`` of checkpointing.py loads in either), the
``grad_scale`` / ``found_inf`` attributes of torch's AMP-aware fused optimizers (train_step.py folds gradient clipping
into the update through ``grad_scale``), and no host synchronisation in ``step()`` (the step counter is a device
scalar): the whole training step still captures into one HIP graph.

``AdamW8bit`` (below) is the reference's other choice, ``--use_8bit_adam`` (train/train.py:1101-1128): the same optimizer with
block-wise 8-bit moments on ``ur_adamw8_multi`` (csrc/adamw8.hip).
"""
from __future__ import annotations

from typing import Iterable, Tuple

import torch

from . import _lib
from ._lib import ABI, check
from .ops import _stream

MAX_TENSORS = ABI.UR_ADAMW_MAX_TENSORS
_Tensor = _lib.STRUCTS["ur_adamw_tensor"]
BLOCK_8BIT = 256  # elements per absmax of the 8-bit state (csrc/adamw8.hip)


def adamw8_tables(rows) -> list:
    """The item tables of ``ur_adamw8_multi`` over ``rows`` of (p, g, m, v, absmax_m, absmax_v, n) -- six device addresses and
    the element count: one ctypes ``int64_t [k][7]`` array and its k per ``MAX_TENSORS`` rows."""
    import ctypes

    tables = []
    for i in range(0, len(rows), MAX_TENSORS):
        part = rows[i:i + MAX_TENSORS]
        tables.append(((ctypes.c_int64 * (7 * len(part)))(*(int(w) for row in part for w in row)), len(part)))
    return tables


class FusedAdamW(torch.optim.Optimizer):
    _step_supports_amp_scaling = True

    def __init__(self, params: Iterable, lr: float = 1e-3, betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 1e-2, fused: bool = True, capturable: bool = True):
        if lr < 0 or eps < 0 or weight_decay < 0 or not (0 <= betas[0] < 1) or not (0 <= betas[1] < 1):
            raise ValueError("invalid AdamW hyper-parameters")
        # ``fused`` / ``capturable`` are accepted (and recorded) so that code written for torch.optim.AdamW(fused=True,
        # capturable=True) constructs this class unchanged; this implementation is always both
        defaults = dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, fused=True, capturable=True,
                        amsgrad=False, maximize=False, foreach=None, differentiable=False)
        super().__init__(params, defaults)
        # bumped whenever the addresses a captured update may hold could have changed (load_state_dict that had to replace
        # state tensors, add_param_group): train_step.GraphedTrainStep compares it and captures again
        self.generation = 0

    def sync_hyper(self):
        """Copy every group's lr / weight_decay into its device scalar pair (created on first use).  The kernel reads them
        from there, so an ``lr_scheduler`` (train.py --lr_scheduler / --lr_warmup_steps) changes what a CAPTURED update
        does without a re-capture: ``step()`` calls this itself when it runs eagerly; around a graph replay the owner of
        the graph calls it before ``replay()`` (train_step.GraphedTrainStep.step)."""
        for group in self.param_groups:
            lr = group["lr"]
            if isinstance(lr, torch.Tensor):
                raise NotImplementedError("FusedAdamW: tensor learning rates are not supported")
            want = (float(lr), float(group["weight_decay"]))
            hy = group.get("_ur_hyper")
            if hy is None:
                dev = next((p.device for p in group["params"]), None)
                if dev is None or dev.type != "cuda":
                    continue
                hy = group["_ur_hyper"] = [torch.empty(2, dtype=torch.float32, device=dev), None]
            if hy[1] != want:
                # staged through a pinned pair: an lr_scheduler changes lr on every step, and a blocking copy from pageable
                # memory would host-synchronise the stream each time.  The staging buffer is rewritten only after the
                # previous copy out of it has completed (event), so back-to-back changes never race.
                if len(hy) < 4:
                    hy += [torch.empty(2, dtype=torch.float32).pin_memory(), torch.cuda.Event()]
                    hy[3].record()
                hy[3].synchronize()
                hy[2][0], hy[2][1] = want
                hy[0].copy_(hy[2], non_blocking=True)
                hy[3].record()
                hy[1] = want

    def _init_state(self, p):
        st = self.state[p]
        if not st:
            st["step"] = torch.zeros((), dtype=torch.float32, device=p.device)
            st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        return st

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        lib = _lib.load()
        grad_scale = getattr(self, "grad_scale", None)
        found_inf = getattr(self, "found_inf", None)
        if not torch.cuda.is_current_stream_capturing():
            self.sync_hyper()  # inside a capture the device pair must already exist (and is refreshed outside the graph)
        for group in self.param_groups:
            if group.get("amsgrad") or group.get("maximize"):
                raise NotImplementedError("FusedAdamW: amsgrad / maximize are not used by the reference (train.py:1093-1100)")
            ps = [p for p in group["params"] if p.grad is not None]
            if not ps:
                continue
            gptrs = tuple(p.grad.data_ptr() for p in ps)
            cached = group.get("_ur_launches")
            if cached is not None and cached[0] == gptrs and cached[1] == tuple(p.data_ptr() for p in ps):
                # same tensors as last step (gradient views of flat buckets, or a captured graph's addresses): the
                # descriptor arrays are reused -- building them is ~6 ms of host time per step for 700 tensors
                step_t = cached[3]
                step_t += 1
                self._launch(lib, group, cached[2], step_t, grad_scale, found_inf)
                torch.autograd.graph.increment_version(ps)
                continue
            for p in ps:
                if p.dtype != torch.float32 or p.grad.dtype != torch.float32 or not p.is_cuda:
                    raise RuntimeError("FusedAdamW updates fp32 master parameters on the GPU (train.py:1082-1089)")
                if not p.is_contiguous() or not p.grad.is_contiguous():
                    raise RuntimeError("FusedAdamW needs contiguous parameters and gradients")
            states = [self._init_state(p) for p in ps]
            # one device step counter per group: the per-parameter ``step`` entries all alias it after the first call
            step_t = states[0]["step"]
            for st in states[1:]:
                if st["step"] is not step_t:
                    st["step"] = step_t
            step_t += 1

            def fill(d, p, i):
                d.p, d.g, d.n = p.data_ptr(), p.grad.data_ptr(), p.numel()
                d.m, d.v = states[i]["exp_avg"].data_ptr(), states[i]["exp_avg_sq"].data_ptr()

            arrays = _lib.desc_arrays(_Tensor, ps, MAX_TENSORS, fill)
            # the cache holds raw addresses: keep what they point into alive next to it (states live in self.state)
            group["_ur_launches"] = (gptrs, tuple(p.data_ptr() for p in ps), arrays, step_t)
            self._launch(lib, group, arrays, step_t, grad_scale, found_inf)
            # the kernel wrote the parameters through their addresses: bump their version counters, as an in-place torch op
            # would, so that everything keyed by (data_ptr, _version) -- packed copies, captured inference graphs, a merged
            # LoRA adapter's factor signature -- notices the update
            torch.autograd.graph.increment_version(ps)
        return loss

    @staticmethod
    def _launch(lib, group, arrays, step_t, grad_scale, found_inf):
        beta1, beta2 = group["betas"]
        lr = group["lr"]
        if isinstance(lr, torch.Tensor):
            raise NotImplementedError("FusedAdamW: tensor learning rates are not supported")
        s_ = _stream()
        hy = group.get("_ur_hyper")
        if hy is None:
            raise RuntimeError("FusedAdamW.step() inside a graph capture before any eager step: call sync_hyper() first")
        for arr in arrays:
            check(lib.ur_adamw_multi(arr, len(arr), float(lr), float(beta1), float(beta2), float(group["eps"]),
                                     float(group["weight_decay"]), step_t.data_ptr(),
                                     grad_scale.data_ptr() if grad_scale is not None else None,
                                     found_inf.data_ptr() if found_inf is not None else None, hy[0].data_ptr(), s_), "ur_adamw_multi")
        if found_inf is not None:
            # the kernel leaves parameters and moments alone when found_inf != 0; like torch's fused AdamW, a skipped
            # step must not advance the bias correction either (a device op: no host synchronisation, capturable)
            step_t -= found_inf.to(step_t.dtype).reshape(())

    def __getstate__(self):
        state = super().__getstate__()
        state["param_groups"] = [{k: v for k, v in g.items() if k not in ("_ur_launches", "_ur_hyper")} for g in state["param_groups"]]
        return state  # the launch cache holds raw device addresses in ctypes arrays: never pickled, rebuilt on the next step

    def state_dict(self):
        """torch.optim.AdamW's layout.  The per-parameter ``step`` entries alias one device scalar inside this object;
        a state dict hands out independent copies (torch's optimizers increment every entry on their own)."""
        sd = super().state_dict()
        for grp in sd["param_groups"]:
            grp.pop("_ur_launches", None)  # host-side launch cache, not optimizer state
            grp.pop("_ur_hyper", None)     # device copy of (lr, weight_decay), rebuilt from the group's values
        # torch hands out the LIVE per-parameter dicts: build copies, never assign into them (replacing the live
        # ``step`` entry would cut its alias to the device counter the cached launches keep incrementing)
        sd["state"] = {k: ({**st, "step": st["step"].clone()} if "step" in st else dict(st)) for k, st in sd["state"].items()}
        return sd

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        self.generation = getattr(self, "generation", 0) + 1

    def load_state_dict(self, state_dict):
        """Loads IN PLACE where it can: existing ``exp_avg`` / ``exp_avg_sq`` / step-counter tensors and the device (lr,
        weight_decay) pair keep their addresses and receive the loaded values, so a captured ``ur_adamw_multi`` (HIP-graph
        replays of the training step) keeps reading live memory after ``resume_from_checkpoint`` (train.py:1191-1218).
        Only state that did not exist yet, or changed shape, is adopted as new tensors -- ``generation`` is bumped then, and
        GraphedTrainStep captures again."""
        old_hyper = [g.get("_ur_hyper") for g in self.param_groups]
        old_launch = [g.get("_ur_launches") for g in self.param_groups]
        old_state = {p: dict(self.state[p]) for g in self.param_groups for p in g["params"] if self.state.get(p)}
        super().load_state_dict(state_dict)
        replaced = False
        for gi, group in enumerate(self.param_groups):
            group.pop("_ur_launches", None)
            group.pop("_ur_hyper", None)
            hy = old_hyper[gi] if gi < len(old_hyper) else None
            if hy is not None:
                hy[1] = None  # same device pair, value re-sent by the next sync_hyper()
                group["_ur_hyper"] = hy
            step_t = None
            for p in group["params"]:
                st = self.state.get(p)
                prev = old_state.get(p)
                if prev is not None and not (st and all(k in st for k in ("exp_avg", "exp_avg_sq", "step"))):
                    # live state that the loaded dict lacks (a checkpoint from before the first step, a partial state):
                    # torch dropped the old moments, so the cached descriptor arrays / a captured ur_adamw_multi would
                    # keep the addresses of freed tensors -- rebuild them
                    replaced = True
                if not st:
                    continue
                for k in ("exp_avg", "exp_avg_sq"):
                    if k in st and prev is not None and k in prev and prev[k].shape == st[k].shape and prev[k].dtype == torch.float32:
                        prev[k].copy_(st[k])
                        st[k] = prev[k]
                    elif k in st:
                        replaced = True
                if "step" in st:
                    new = torch.as_tensor(st["step"], dtype=torch.float32).to(p.device).reshape(())
                    if prev is not None and "step" in prev:
                        if step_t is None or prev["step"] is not step_t:
                            prev["step"].copy_(new)
                        st["step"] = step_t = prev["step"]  # the group's one device counter keeps its address
                    else:
                        st["step"] = new.clone()  # private fp32 device scalar (torch may hand back the caller's tensor uncopied)
                        replaced = True
            if not replaced and gi < len(old_launch) and old_launch[gi] is not None:
                group["_ur_launches"] = old_launch[gi]  # same addresses: the descriptor arrays are still right
        if replaced:
            self.generation = getattr(self, "generation", 0) + 1


# ---------------------------------------------------------------------------------------------
# block-wise 8-bit state (ur_adamw8_multi, csrc/adamw8.hip)
# ---------------------------------------------------------------------------------------------
_MOMENTS = (("exp_avg", "exp_avg_absmax", 1), ("exp_avg_sq", "exp_avg_sq_absmax", 0))  # codes, block maxima, signed book?


def codebook(signed: bool) -> torch.Tensor:
    """The library's 256-entry fp32 code book (``ur_adam8_codebook``): ``signed`` for exp_avg, unsigned for exp_avg_sq."""
    import ctypes

    out = (ctypes.c_float * 256)()
    check(_lib.load().ur_adam8_codebook(int(bool(signed)), out), "ur_adam8_codebook")
    return torch.tensor(list(out), dtype=torch.float32)


def quantize_blockwise(x: torch.Tensor, signed: bool, codes: torch.Tensor = None, absmax: torch.Tensor = None):
    """``(codes, absmax)`` of the fp32 GPU tensor ``x`` (``ur_adam8_quantize``): uint8 of x's shape and fp32 [ceil(n / 256)],
    written into ``codes`` / ``absmax`` when given."""
    if not x.is_cuda or x.dtype != torch.float32 or not x.is_contiguous() or x.numel() == 0:
        raise RuntimeError("quantize_blockwise needs a non-empty contiguous fp32 tensor on the GPU")
    n = x.numel()
    if codes is None:
        codes = torch.empty(x.shape, dtype=torch.uint8, device=x.device)
    if absmax is None:
        absmax = torch.empty(-(-n // BLOCK_8BIT), dtype=torch.float32, device=x.device)
    check(_lib.load().ur_adam8_quantize(x.data_ptr(), codes.data_ptr(), absmax.data_ptr(), n, int(bool(signed)), _stream()),
          "ur_adam8_quantize")
    return codes, absmax


def dequantize_blockwise(codes: torch.Tensor, absmax: torch.Tensor, signed: bool) -> torch.Tensor:
    """fp32 ``book[codes] * absmax`` of the GPU tensors ``codes`` (uint8) / ``absmax`` (``ur_adam8_dequantize``)."""
    n = codes.numel()
    if (not codes.is_cuda or codes.dtype != torch.uint8 or not codes.is_contiguous() or n == 0 or absmax.dtype != torch.float32
            or absmax.device != codes.device or not absmax.is_contiguous() or absmax.numel() != -(-n // BLOCK_8BIT)):
        raise RuntimeError("dequantize_blockwise needs contiguous uint8 codes and fp32 [ceil(n / 256)] block maxima on the GPU")
    x = torch.empty(codes.shape, dtype=torch.float32, device=codes.device)
    check(_lib.load().ur_adam8_dequantize(x.data_ptr(), codes.data_ptr(), absmax.data_ptr(), n, int(bool(signed)), _stream()),
          "ur_adam8_dequantize")
    return x


class AdamW8bit(FusedAdamW):
    """``FusedAdamW`` with block-wise dynamic 8-bit moments (Dettmers et al., arXiv 2110.02861): what the reference's
    ``--use_8bit_adam`` selects (``bnb.optim.AdamW8bit``, train/train.py:1101-1128).  Tensors of at least ``min_8bit_size``
    elements keep ``exp_avg`` / ``exp_avg_sq`` as one byte per element plus one fp32 block maximum per 256 elements and moment
    (2 n + 8 ceil(n / 256) bytes instead of 8 n) and are updated by ``ur_adamw8_multi``; smaller ones (biases, norm vectors)
    keep fp32 state and go through ``ur_adamw_multi`` bit-for-bit as in ``FusedAdamW``.  Everything else is ``FusedAdamW``:
    one device step counter per group, lr / weight decay in device memory, ``grad_scale`` / ``found_inf``, no host
    synchronisation in ``step()``, in-place ``load_state_dict``.

    The scheme is restated in include/ur_kernels.h, not taken from bitsandbytes: parity with bitsandbytes is unpinned, and a
    strictly positive ``exp_avg_sq`` never rounds to zero (code 1 instead), which the published scheme does not say.  8-bit
    state is not a numerical drop-in for fp32 AdamW (DESIGN.md has the measured distance).

    ``state_dict()``: per parameter ``step``, ``exp_avg`` / ``exp_avg_sq`` as uint8 tensors of the parameter's shape and
    ``exp_avg_absmax`` / ``exp_avg_sq_absmax`` as fp32 [ceil(n / 256)]; small tensors as in torch.  ``load_state_dict`` takes
    that or torch's fp32 layout (quantised on load); ``dequantized_state_dict()`` hands out torch's layout."""

    def __init__(self, params: Iterable, lr: float = 1e-3, betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 1e-2, min_8bit_size: int = 4096, amsgrad: bool = False, percentile_clipping: int = 100,
                 block_wise: bool = True):
        # the switches of bnb.optim.AdamW8bit that change the arithmetic: accepted at their defaults only
        if amsgrad or percentile_clipping != 100 or not block_wise:
            raise NotImplementedError("AdamW8bit: amsgrad, percentile_clipping != 100 and block_wise=False are not implemented")
        if min_8bit_size < 0:
            raise ValueError("invalid min_8bit_size")
        self.min_8bit_size = int(min_8bit_size)
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)

    def _is_8bit(self, p) -> bool:
        return p.numel() >= self.min_8bit_size and p.numel() > 0

    def _init_state(self, p):
        if not self._is_8bit(p):
            return super()._init_state(p)
        st = self.state[p]
        if not st:
            nblk = -(-p.numel() // BLOCK_8BIT)
            st["step"] = torch.zeros((), dtype=torch.float32, device=p.device)
            st["exp_avg"] = torch.full(p.shape, 127, dtype=torch.uint8, device=p.device)  # the signed book's zero
            st["exp_avg_sq"] = torch.zeros(p.shape, dtype=torch.uint8, device=p.device)
            st["exp_avg_absmax"] = torch.zeros(nblk, dtype=torch.float32, device=p.device)
            st["exp_avg_sq_absmax"] = torch.zeros(nblk, dtype=torch.float32, device=p.device)
        return st

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        lib = _lib.load()
        grad_scale = getattr(self, "grad_scale", None)
        found_inf = getattr(self, "found_inf", None)
        if not torch.cuda.is_current_stream_capturing():
            self.sync_hyper()
        for group in self.param_groups:
            if group.get("amsgrad") or group.get("maximize"):
                raise NotImplementedError("AdamW8bit: amsgrad / maximize are not used by the reference (train.py:1101-1128)")
            ps = [p for p in group["params"] if p.grad is not None]
            if not ps:
                continue
            gptrs = tuple(p.grad.data_ptr() for p in ps)
            cached = group.get("_ur_launches")
            if cached is None or cached[0] != gptrs or cached[1] != tuple(p.data_ptr() for p in ps):
                for p in ps:
                    if p.dtype != torch.float32 or p.grad.dtype != torch.float32 or not p.is_cuda:
                        raise RuntimeError("AdamW8bit updates fp32 master parameters on the GPU (train.py:1082-1089)")
                    if not p.is_contiguous() or not p.grad.is_contiguous():
                        raise RuntimeError("AdamW8bit needs contiguous parameters and gradients")
                states = {p: self._init_state(p) for p in ps}
                step_t = states[ps[0]]["step"]  # one device step counter per group, shared by both kinds of tensor
                for st in states.values():
                    if st["step"] is not step_t:
                        st["step"] = step_t
                big = [p for p in ps if self._is_8bit(p)]
                small = [p for p in ps if not self._is_8bit(p)]

                def row8(p):
                    st = states[p]
                    return (p.data_ptr(), p.grad.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(),
                            st["exp_avg_absmax"].data_ptr(), st["exp_avg_sq_absmax"].data_ptr(), p.numel())

                def fill(d, p, i):
                    d.p, d.g, d.n = p.data_ptr(), p.grad.data_ptr(), p.numel()
                    d.m, d.v = states[p]["exp_avg"].data_ptr(), states[p]["exp_avg_sq"].data_ptr()

                cached = group["_ur_launches"] = (gptrs, tuple(p.data_ptr() for p in ps), _lib.desc_arrays(_Tensor, small, MAX_TENSORS, fill),
                                                  step_t, adamw8_tables([row8(p) for p in big]))
            step_t = cached[3]
            step_t += 1
            beta1, beta2 = group["betas"]
            hy = group.get("_ur_hyper")
            if hy is None:
                raise RuntimeError("AdamW8bit.step() inside a graph capture before any eager step: call sync_hyper() first")
            for table, count in cached[4]:
                check(lib.ur_adamw8_multi(table, count, float(group["lr"]), float(beta1), float(beta2), float(group["eps"]),
                                          float(group["weight_decay"]), step_t.data_ptr(),
                                          grad_scale.data_ptr() if grad_scale is not None else None,
                                          found_inf.data_ptr() if found_inf is not None else None, hy[0].data_ptr(), _stream()),
                      "ur_adamw8_multi")
            # the fp32 tensors, and the step counter's correction after a skipped step, exactly as FusedAdamW
            self._launch(lib, group, cached[2], step_t, grad_scale, found_inf)
            torch.autograd.graph.increment_version(ps)  # as FusedAdamW.step
        return loss

    def dequantized_state_dict(self):
        """``state_dict()`` in torch.optim.AdamW's layout (fp32 ``exp_avg`` / ``exp_avg_sq``, no block maxima): loads into
        ``FusedAdamW`` or ``torch.optim.AdamW``."""
        sd = self.state_dict()
        for st in sd["state"].values():
            for key, amax, signed in _MOMENTS:
                if amax in st:
                    st[key] = dequantize_blockwise(st[key], st.pop(amax), signed)
        return sd

    def load_state_dict(self, state_dict):
        """As ``FusedAdamW.load_state_dict`` (in place wherever the live state has the loaded shapes, ``generation`` bumped
        otherwise), for this class's layout and for torch's: fp32 moments of an 8-bit tensor are quantised on the way in, and
        codes of a tensor that is below ``min_8bit_size`` here are decoded."""
        old_hyper = [g.get("_ur_hyper") for g in self.param_groups]
        old_launch = [g.get("_ur_launches") for g in self.param_groups]
        old_state = {p: dict(self.state[p]) for g in self.param_groups for p in g["params"] if self.state.get(p)}
        # torch casts every state tensor to the parameter's dtype (uint8 codes would come back as fp32, and fp32 moments of
        # the whole model would be resident at once): it gets the step counters only, the moments are placed below
        keys = {k for m in _MOMENTS for k in m[:2]}
        moments = {pid: {k: v for k, v in st.items() if k in keys} for pid, st in state_dict["state"].items()}
        torch.optim.Optimizer.load_state_dict(self, {
            "state": {pid: {k: v for k, v in st.items() if k not in keys} for pid, st in state_dict["state"].items()},
            "param_groups": state_dict["param_groups"]})
        replaced = False
        for gi, (group, saved) in enumerate(zip(self.param_groups, state_dict["param_groups"])):
            group.pop("_ur_launches", None)
            group.pop("_ur_hyper", None)
            hy = old_hyper[gi] if gi < len(old_hyper) else None
            if hy is not None:
                hy[1] = None  # same device pair, value re-sent by the next sync_hyper()
                group["_ur_hyper"] = hy
            step_t = None
            for p, pid in zip(group["params"], saved["params"]):
                st, prev, mom = self.state.get(p), old_state.get(p), moments.get(pid, {})
                want = [k for m in _MOMENTS for k in (m[:2] if self._is_8bit(p) else m[:1])]
                if prev is not None and not ("step" in (st or {}) and "exp_avg" in mom and "exp_avg_sq" in mom):
                    replaced = True  # live state that the loaded dict lacks: its addresses are gone (see FusedAdamW)
                if not st and not mom:
                    continue
                st = self.state[p]
                if "exp_avg" in mom and "exp_avg_sq" in mom:
                    new = self._convert(p, mom)
                    for k in want:
                        if prev is not None and k in prev and prev[k].shape == new[k].shape and prev[k].dtype == new[k].dtype:
                            prev[k].copy_(new[k])
                            st[k] = prev[k]
                        else:
                            st[k] = new[k] if new[k].device == p.device and new[k] is not mom.get(k) else new[k].to(p.device, copy=True)
                            replaced = True
                if "step" in st:
                    new = torch.as_tensor(st["step"], dtype=torch.float32).to(p.device).reshape(())
                    if prev is not None and "step" in prev:
                        if step_t is None or prev["step"] is not step_t:
                            prev["step"].copy_(new)
                        st["step"] = step_t = prev["step"]  # the group's one device counter keeps its address
                    else:
                        st["step"] = new.clone()
                        replaced = True
            if not replaced and gi < len(old_launch) and old_launch[gi] is not None:
                group["_ur_launches"] = old_launch[gi]  # same addresses: the descriptor arrays are still right
        if replaced:
            self.generation = getattr(self, "generation", 0) + 1

    def _convert(self, p, mom):
        """The loaded moments ``mom`` of parameter ``p`` in the layout ``p`` has here: codes + block maxima (8-bit tensors) or
        fp32 (small ones).  Tensors already in that layout pass through untouched, on whatever device they are."""
        out = {}
        for key, amax, signed in _MOMENTS:
            t = mom[key]
            coded = amax in mom
            if coded and (t.dtype != torch.uint8 or mom[amax].numel() != -(-t.numel() // BLOCK_8BIT)):
                raise ValueError(f"AdamW8bit.load_state_dict: {key} has block maxima but is not a uint8 code tensor of their size")
            if t.shape != p.shape:
                raise ValueError(f"AdamW8bit.load_state_dict: {key} of shape {tuple(t.shape)} for a parameter of shape {tuple(p.shape)}")
            if self._is_8bit(p):
                if coded:
                    out[key], out[amax] = t, mom[amax].to(torch.float32)
                else:
                    out[key], out[amax] = quantize_blockwise(t.to(p.device, torch.float32).contiguous(), signed)
            elif coded:
                out[key] = dequantize_blockwise(t.to(p.device).contiguous(), mom[amax].to(p.device, torch.float32).contiguous(), signed)
            else:
                out[key] = t.to(torch.float32)
        return out
