"""Restatements the EMA tests compare against: the decay schedule of diffusers 0.24's EMAModel in float64, the update
``s' = s - d (s - p)`` in float64 (the definition), and the same update as the three fp32 roundings the kernel and torch's
``s.sub_(d * (s - p))`` perform (numpy float32 arrays round after every operation)."""
import numpy as np
import torch


def get_decay(step, decay=0.9999, min_decay=0.0, update_after_step=0, use_ema_warmup=False, inv_gamma=1.0, power=2 / 3):
    """float64 (Python floats) decay of optimisation step ``step`` (the value AFTER the counter was advanced)."""
    k = max(0, int(step) - int(update_after_step) - 1)
    if k <= 0:
        return 0.0
    cur = 1.0 - (1.0 + k / inv_gamma) ** -power if use_ema_warmup else (1.0 + k) / (10.0 + k)
    return max(min(cur, decay), min_decay)


def one_minus_decay32(step, **kw) -> np.float32:
    """The fp32 scalar the update multiplies by: 1 - decay in float64, rounded once."""
    return np.float32(1.0 - get_decay(step, **kw))


def definition64(s, p, d):
    """s - d (s - p) in float64 from fp32 / 16-bit inputs (widened exactly) and the fp32 scalar d."""
    s, p = np.asarray(s, dtype=np.float64), np.asarray(p, dtype=np.float64)
    return s - float(d) * (s - p)


def emulate32(s, p, d):
    """The three separately rounded fp32 operations t = s - p, u = d * t, s' = s - u."""
    s, p, d = np.asarray(s, dtype=np.float32), np.asarray(p, dtype=np.float32), np.float32(d)
    t = s - p
    u = d * t
    assert t.dtype == u.dtype == np.float32
    return s - u


def contracted32(s, p, d):
    """What a contraction of the last two operations into one fma would give: s - d * t rounded ONCE (for the tests that show
    the data would see it)."""
    s, p = np.asarray(s, dtype=np.float32), np.asarray(p, dtype=np.float32)
    t = (s - p).astype(np.float64)
    return (s.astype(np.float64) - float(np.float32(d)) * t).astype(np.float32)  # the fp64 product of two fp32 is exact


def bound64(s, p, d):
    """Per-element bound on |fp32 result - definition64|: with u = 2^-24, the rounding of t = s - p contributes u |s - p| d,
    that of d t another u d |s - p| (1 + u), the final subtraction u |s'| (1 + ...): 2^-24 (2 d |s - p| + |s'|), times
    (1 + 2^-22) for the second-order terms."""
    s64, p64 = np.asarray(s, dtype=np.float64), np.asarray(p, dtype=np.float64)
    return 2.0 ** -24 * (2.0 * float(d) * np.abs(s64 - p64) + np.abs(definition64(s, p, d))) * (1.0 + 2.0 ** -22)


def widen(t: torch.Tensor) -> np.ndarray:
    """A torch tensor (fp32 / fp16 / bf16, any device) as a flat fp32 numpy array of its own (never a view of a CPU tensor that
    a later step rewrites): exact."""
    return t.detach().float().cpu().numpy().reshape(-1).copy()


def replay(shadows, params, step, requires_grad=None, **kw):
    """One EMAModel.step of the emulation: the new fp32 shadows (flat numpy arrays) from the old ones and the parameters, at
    optimisation step ``step`` (after the advance)."""
    d = one_minus_decay32(step, **kw)
    out = []
    for i, (s, p) in enumerate(zip(shadows, params)):
        if requires_grad is not None and not requires_grad[i]:
            out.append(np.asarray(p, dtype=np.float32).copy())
        else:
            out.append(emulate32(s, p, d))
    return out
