"""``EMAModel``: the exponential moving average of the weights of ``diffusers.training_utils.EMAModel`` (diffusers 0.24; the
``--use_ema`` switch of its training scripts), on one multi-tensor HIP kernel (``ur_ema_multi``, csrc/ema.hip).

diffusers updates every parameter with ``s_param.sub_(one_minus_decay * (s_param - param))``: three torch launches and a
temporary per tensor, 20 B of memory traffic per element, and a decay schedule computed on the host -- so it cannot be part
of a captured training step.  Here ``step()`` is one ``ur_ema_advance`` (the step counter and ``get_decay`` in device
memory) plus one ``ur_ema_multi`` per 64 tensors (12 B per fp32 element), with the same three fp32 roundings per element, no
host synchronisation and no allocation: it captures into the training step's HIP graph (train_step.GraphedTrainStep(...,
ema=...)), and every replay advances the schedule by itself.

Differences from diffusers, all deliberate:

* shadows are fp32 whatever the parameter dtype (diffusers clones the parameter's dtype); the masters this package trains are
  fp32, where nothing differs.  16-bit / 8-bit shadows are not implemented: ``to(dtype=...)`` other than fp32 raises.
* ``optimization_step`` and ``cur_decay_value`` are properties that read device scalars: reading them synchronises.
* ``copy_to`` / ``restore`` write through ``Tensor.copy_`` (not ``.data.copy_``), so the parameters' ``_version`` counters move
  and packed weight copies and captured inference graphs notice; ``store`` keeps its copies on the parameters' device.
* ``state_dict()`` hands out copies of the shadows, ``load_state_dict`` loads IN PLACE (a captured step stays valid).
* no EMA of buffers, no sharding across ranks (every rank holds the full average, identical after the all-reduce).

Parity with diffusers is unpinned (it is not a dependency); ``get_decay`` is restated in include/ur_kernels.h.
"""
from __future__ import annotations

import ctypes as C
from typing import Any, Dict, Iterable, List, Optional

import torch

from . import _lib
from ._lib import ABI, check

_SCALAR_KEYS = ("decay", "min_decay", "optimization_step", "update_after_step", "use_ema_warmup", "inv_gamma", "power")
_COPY = 0x100  # flag bit of an item of ur_ema_multi (include/ur_kernels.h)
_DTYPES = {torch.float32: ABI.UR_DT_F32, torch.float16: ABI.UR_DT_F16, torch.bfloat16: ABI.UR_DT_BF16}


def _listed(parameters) -> List[torch.Tensor]:
    if isinstance(parameters, torch.nn.Module):
        parameters = parameters.parameters()
    return list(parameters)


class EMAModel:
    """Exponential moving average of ``parameters`` (an iterable of tensors, or a module).  Constructor, methods and
    ``state_dict()`` keys are diffusers'; ``foreach`` is accepted and ignored (there is one kernel)."""

    def __init__(self, parameters: Iterable[torch.nn.Parameter], decay: float = 0.9999, min_decay: float = 0.0,
                 update_after_step: int = 0, use_ema_warmup: bool = False, inv_gamma: float = 1.0, power: float = 2 / 3,
                 model_cls: Optional[Any] = None, model_config: Optional[Dict[str, Any]] = None, foreach: bool = False):
        parameters = _listed(parameters)
        self._set_schedule(decay, min_decay, update_after_step, use_ema_warmup, inv_gamma, power)
        devices = {p.device for p in parameters}
        if len(devices) > 1:
            raise ValueError(f"EMAModel: parameters on several devices ({sorted(map(str, devices))}); build one EMAModel per device")
        dev = devices.pop() if devices else torch.device("cpu")
        with torch.no_grad():
            self.shadow_params = [p.detach().to(torch.float32, copy=True).contiguous() for p in parameters]
        self.temp_stored_params = None
        # created here, never in step(): a step() inside a graph capture allocates nothing
        self._step = torch.zeros((), dtype=torch.int64, device=dev)
        self._cur_decay = torch.zeros((), dtype=torch.float64, device=dev)
        self._one_minus_decay = torch.ones((), dtype=torch.float32, device=dev)
        self.model_cls, self.model_config = model_cls, model_config
        self.foreach = bool(foreach)
        # bumped whenever the addresses a captured step() holds were replaced (to(device)): GraphedTrainStep captures again
        self.generation = 0
        self._cache = None        # (key, item tables, the tensors whose addresses the tables hold)

    def _set_schedule(self, decay, min_decay, update_after_step, use_ema_warmup, inv_gamma, power):
        decay, min_decay, inv_gamma, power = float(decay), float(min_decay), float(inv_gamma), float(power)
        if not (0.0 <= decay <= 1.0) or not (0.0 <= min_decay <= 1.0) or not inv_gamma > 0.0 or power != power:
            raise ValueError("EMAModel: decay and min_decay must lie in [0, 1], inv_gamma must be positive")
        self.decay, self.min_decay, self.inv_gamma, self.power = decay, min_decay, inv_gamma, power
        self.update_after_step, self.use_ema_warmup = int(update_after_step), bool(use_ema_warmup)

    # -- the schedule ------------------------------------------------------------------------------------------------------
    def get_decay(self, optimization_step: int) -> float:
        """The decay factor of step ``optimization_step`` (host, Python floats): diffusers 0.24's schedule, which
        ``ur_ema_advance`` evaluates on the device."""
        step = max(0, int(optimization_step) - self.update_after_step - 1)
        if step <= 0:
            return 0.0
        if self.use_ema_warmup:
            cur = 1 - (1 + step / self.inv_gamma) ** -self.power
        else:
            cur = (1 + step) / (10 + step)
        return max(min(cur, self.decay), self.min_decay)

    @property
    def optimization_step(self) -> int:
        """The number of ``step()`` calls so far, read from the device counter: SYNCHRONISES."""
        return int(self._step.item())

    @optimization_step.setter
    def optimization_step(self, value: int):
        self._step.fill_(int(value))  # in place: the counter keeps its address

    @property
    def cur_decay_value(self) -> Optional[float]:
        """The decay the last ``step()`` used (None before the first), read from the device: SYNCHRONISES."""
        return float(self._cur_decay.item()) if self.optimization_step > 0 else None

    # -- the update --------------------------------------------------------------------------------------------------------
    def _checked(self, parameters, what: str) -> List[torch.Tensor]:
        parameters = _listed(parameters)
        if len(parameters) != len(self.shadow_params):
            raise ValueError(f"EMAModel.{what}: {len(parameters)} parameters for {len(self.shadow_params)} shadows")
        for i, (s, p) in enumerate(zip(self.shadow_params, parameters)):
            if p.shape != s.shape:
                raise ValueError(f"EMAModel.{what}: parameter {i} has shape {tuple(p.shape)}, its shadow {tuple(s.shape)}")
        return parameters

    @torch.no_grad()
    def step(self, parameters: Iterable[torch.nn.Parameter]) -> None:
        """One update of the average towards ``parameters`` (the tensors of the constructor, in its order).  Parameters with
        ``requires_grad=False`` are copied, not averaged, as in diffusers.  There is no ``found_inf``: like the diffusers
        scripts, a step the GradScaler skipped still advances the average, towards the unchanged parameters.
        On the GPU: ``ur_ema_advance`` + ceil(n / 64) ``ur_ema_multi``, no host synchronisation, capturable."""
        parameters = self._checked(parameters, "step")
        if self._step.is_cuda:
            self._step_gpu(parameters)
            return
        # the CPU path: the same three roundings in torch (s - p, d * t, s - u, each an fp32 tensor operation)
        self._step += 1
        cur = self.get_decay(int(self._step))
        self._cur_decay.fill_(cur)
        self._one_minus_decay.fill_(1.0 - cur)  # rounded to fp32 once, as the device scalar is
        for s, p in zip(self.shadow_params, parameters):
            if p.requires_grad:
                t = s - p.to(device=s.device, dtype=torch.float32)
                t.mul_(self._one_minus_decay)
                s.sub_(t)
            else:
                s.copy_(p)

    def _tables(self, parameters):
        key = (tuple(p.data_ptr() for p in parameters), tuple(p.requires_grad for p in parameters))
        if self._cache is not None and self._cache[0] == key:
            return self._cache[1]  # same tensors as last step: building the tables is host time per step, as in FusedAdamW
        lib = _lib.load()
        words, nmax = lib.ur_ema_item_words(), lib.ur_ema_multi_max()
        rows = []
        for i, (s, p) in enumerate(zip(self.shadow_params, parameters)):
            if p.device != s.device or p.dtype not in _DTYPES or not p.is_contiguous():
                raise RuntimeError(f"EMAModel.step: parameter {i} must be a contiguous fp32 / fp16 / bf16 tensor on {s.device}")
            if p.numel():
                rows.append((s.data_ptr(), p.data_ptr(), p.numel(), _DTYPES[p.dtype] | (0 if p.requires_grad else _COPY)))
        tables = []
        for i in range(0, len(rows), nmax):
            part = rows[i:i + nmax]
            tables.append(((C.c_int64 * (words * len(part)))(*(int(w) for row in part for w in row)), len(part)))
        # the tables hold raw addresses: keep what they point into alive next to them
        self._cache = (key, tables, list(parameters))
        return tables

    def _step_gpu(self, parameters):
        from .ops import _stream

        lib = _lib.load()
        tables = self._tables(parameters)
        stream = _stream()
        schedule = (C.c_double * 4)(self.inv_gamma, self.power, self.min_decay, self.decay)
        omd = self._one_minus_decay.data_ptr()
        check(lib.ur_ema_advance(C.cast(self._step.data_ptr(), C.POINTER(C.c_int64)), self.update_after_step, int(self.use_ema_warmup),
                                 schedule, self._cur_decay.data_ptr(), omd, stream), "ur_ema_advance")
        for table, count in tables:
            check(lib.ur_ema_multi(table, count, omd, stream), "ur_ema_multi")
        # the kernel wrote the shadows through their addresses: bump their version counters, as an in-place torch op would
        torch.autograd.graph.increment_version(self.shadow_params)

    # -- moving the average in and out of a model --------------------------------------------------------------------------
    @torch.no_grad()
    def copy_to(self, parameters: Iterable[torch.nn.Parameter]) -> None:
        """Copy the averaged weights into ``parameters`` (rounded to their dtype).  Through ``copy_``: their ``_version`` moves,
        so everything keyed by it -- packed weight copies, captured inference graphs -- sees the new values."""
        for s, p in zip(self.shadow_params, self._checked(parameters, "copy_to")):
            p.copy_(s)

    @torch.no_grad()
    def store(self, parameters: Iterable[torch.nn.Parameter]) -> None:
        """Keep a copy of ``parameters`` (on their device) for ``restore``: ``store`` -> ``copy_to`` -> validate -> ``restore``."""
        self.temp_stored_params = [p.detach().clone() for p in _listed(parameters)]

    @torch.no_grad()
    def restore(self, parameters: Iterable[torch.nn.Parameter]) -> None:
        """Put back what ``store`` kept (through ``copy_``, as ``copy_to``) and drop the copies."""
        if self.temp_stored_params is None:
            raise RuntimeError("This ExponentialMovingAverage has no `store()`ed weights to `restore()`")
        parameters = _listed(parameters)
        if len(parameters) != len(self.temp_stored_params):
            raise ValueError(f"EMAModel.restore: {len(parameters)} parameters for {len(self.temp_stored_params)} stored tensors")
        for c, p in zip(self.temp_stored_params, parameters):
            p.copy_(c)
        self.temp_stored_params = None

    def to(self, device=None, dtype=None) -> None:
        """Move the shadows and the device scalars to ``device``.  ``dtype``: fp32 only (16-bit shadows are out of scope).
        A move replaces the tensors: ``generation`` is bumped and a captured training step is captured again."""
        if dtype is not None and dtype != torch.float32:
            raise NotImplementedError("EMAModel keeps fp32 shadows; 16-bit / 8-bit shadows are not implemented")
        if device is None:
            return
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if device == self._step.device:
            return
        self.shadow_params = [s.to(device) for s in self.shadow_params]
        self._step, self._cur_decay, self._one_minus_decay = (t.to(device) for t in (self._step, self._cur_decay, self._one_minus_decay))
        self._cache = None
        self.generation += 1

    # -- state -------------------------------------------------------------------------------------------------------------
    def state_dict(self) -> dict:
        """diffusers' keys: ``decay, min_decay, optimization_step, update_after_step, use_ema_warmup, inv_gamma, power,
        shadow_params`` (copies of the shadows: a saved state does not follow later steps).  Synchronises."""
        return dict(decay=self.decay, min_decay=self.min_decay, optimization_step=self.optimization_step,
                    update_after_step=self.update_after_step, use_ema_warmup=self.use_ema_warmup, inv_gamma=self.inv_gamma,
                    power=self.power, shadow_params=[s.clone() for s in self.shadow_params])

    @torch.no_grad()
    def load_state_dict(self, state_dict: dict) -> None:
        """Loads IN PLACE: the shadows, the step counter and the decay scalars keep their addresses and receive the loaded
        values, so a captured ``step()`` (HIP-graph replays of the training step) stays valid after a resume.  Compare
        ``FusedAdamW.load_state_dict``.  Keys that are absent keep their current value, as in diffusers."""
        sd = dict(state_dict)
        step = sd.get("optimization_step", None)
        for key, kind in (("decay", float), ("min_decay", float), ("inv_gamma", (float, int)), ("power", (float, int))):
            if key in sd and (not isinstance(sd[key], kind) or isinstance(sd[key], bool)):
                raise ValueError(f"Invalid {key}")
        for key in ("optimization_step", "update_after_step"):
            if key in sd and (not isinstance(sd[key], int) or isinstance(sd[key], bool)):
                raise ValueError(f"Invalid {key}")
        if "use_ema_warmup" in sd and not isinstance(sd["use_ema_warmup"], bool):
            raise ValueError("Invalid use_ema_warmup")
        shadows = sd.get("shadow_params", None)
        if shadows is not None:
            if not isinstance(shadows, (list, tuple)) or not all(isinstance(t, torch.Tensor) for t in shadows):
                raise ValueError("shadow_params must be a list of tensors")
            if len(shadows) != len(self.shadow_params) or any(a.shape != b.shape for a, b in zip(shadows, self.shadow_params)):
                raise ValueError("shadow_params do not match this EMAModel's parameters in number or shape")
        self._set_schedule(*(sd.get(k, getattr(self, k)) for k in ("decay", "min_decay", "update_after_step", "use_ema_warmup",
                                                                    "inv_gamma", "power")))
        if step is not None:
            self.optimization_step = step
            cur = self.get_decay(step)
            self._cur_decay.fill_(cur)
            self._one_minus_decay.fill_(1.0 - cur)
        if shadows is not None:
            for mine, theirs in zip(self.shadow_params, shadows):
                mine.copy_(theirs)

    def save_pretrained(self, path: str) -> None:
        """The averaged weights as a model in the diffusers on-disk layout: ``model_cls.from_config(model_config)`` holding the
        shadows, with the seven EMA scalars registered into its ``config.json``."""
        if self.model_cls is None:
            raise ValueError("`save_pretrained` can only be used if `model_cls` was defined at __init__.")
        if self.model_config is None:
            raise ValueError("`save_pretrained` can only be used if `model_config` was defined at __init__.")
        model = self.model_cls.from_config(self.model_config)
        state = self.state_dict()
        state.pop("shadow_params")
        model.register_to_config(**state)
        self.copy_to(model.parameters())
        model.save_pretrained(path)

    @classmethod
    def from_pretrained(cls, path: str, model_cls, foreach: bool = False) -> "EMAModel":
        """An ``EMAModel`` over the weights ``save_pretrained`` wrote to ``path``, its scalars read back out of ``config.json``."""
        _, ema_kwargs = model_cls.load_config(path, return_unused_kwargs=True)
        model = model_cls.from_pretrained(path)
        ema = cls(model.parameters(), model_cls=model_cls, model_config=model.config, foreach=foreach)
        ema.load_state_dict({k: v for k, v in ema_kwargs.items() if k in _SCALAR_KEYS})
        return ema
