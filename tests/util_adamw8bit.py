"""The block-wise 8-bit AdamW state of include/ur_kernels.h (ABI 17), restated in float64 numpy: what csrc/adamw8.hip and
optim.AdamW8bit are tested against.  Nothing here calls the library.

Blocks of 256 consecutive elements, one absmax per block and moment; a moment is stored as the index of the code-book entry
nearest to value / absmax (ties: the lower index) and read back as book[code] * absmax.  A block of absmax 0 stores the zero
code without dividing; a strictly positive exp_avg_sq never takes code 0 but code 1.
"""
import numpy as np

BLOCK = 256


def book(signed: bool) -> np.ndarray:
    """The 256 ascending code-book entries: the formula in float64, rounded to fp32 (the library's constants), as float64."""
    vals = [0.0, 1.0]
    for i in range(7):
        n = 2 ** i if signed else 2 ** (i + 1)
        pts = np.linspace(0.1, 1.0, n + 1)
        mid = (pts[:-1] + pts[1:]) / 2 * 10.0 ** (i - 6)
        vals += list(mid) + (list(-mid) if signed else [])
    return np.sort(np.asarray(vals, dtype=np.float64)).astype(np.float32).astype(np.float64)


BOOKS = {True: book(True), False: book(False)}
ZERO_CODE = {True: 127, False: 0}


def nblocks(n: int) -> int:
    return -(-n // BLOCK)


def block_absmax(x: np.ndarray) -> np.ndarray:
    x = np.abs(np.asarray(x, dtype=np.float64).reshape(-1))
    pad = np.zeros(nblocks(x.size) * BLOCK)
    pad[:x.size] = x
    return pad.reshape(-1, BLOCK).max(axis=1)


def normalised(x: np.ndarray, absmax: np.ndarray) -> np.ndarray:
    """x / absmax of x's block; 0 where the block's absmax is 0 (no division)."""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    am = np.repeat(absmax, BLOCK)[:x.size]
    return np.divide(x, am, out=np.zeros_like(x), where=am > 0)


def nearest(r: np.ndarray, signed: bool, positive=None) -> np.ndarray:
    """Index of the book entry nearest to each r.  ``positive`` (unsigned book only): mask of strictly positive values, which
    never take code 0."""
    b = BOOKS[signed]
    code = np.searchsorted((b[:-1] + b[1:]) / 2, r, side="left")  # a tie goes to the lower entry
    if not signed and positive is not None:
        code = np.where(positive & (code == 0), 1, code)
    return code.astype(np.uint8)


def encode(x: np.ndarray, signed: bool):
    """(codes uint8 [n], absmax float64 [ceil(n / 256)]) of the flat float64 x."""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    am = block_absmax(x)
    return nearest(normalised(x, am), signed, positive=None if signed else x > 0), am


def decode(codes: np.ndarray, absmax: np.ndarray, signed: bool) -> np.ndarray:
    codes = np.asarray(codes).reshape(-1)
    return BOOKS[signed][codes] * np.repeat(np.asarray(absmax, dtype=np.float64), BLOCK)[:codes.size]


def adamw8_step(p, g, cm, am, cv, av, step, lr, beta1, beta2, eps, wd, grad_scale=1.0):
    """One update of a flat tensor from its stored state.  Returns dict(p, m, v: fresh float64; cm, am, cv, av: the state
    stored afterwards; g: the unscaled gradient).  The parameter is updated from the fresh moments, before re-quantisation."""
    p, g = np.asarray(p, dtype=np.float64).reshape(-1), np.asarray(g, dtype=np.float64).reshape(-1) / grad_scale
    m, v = decode(cm, am, True), decode(cv, av, False)
    bc1, bc2 = 1.0 - beta1 ** step, 1.0 - beta2 ** step
    p = p * (1.0 - lr * wd)
    m = m + (1.0 - beta1) * (g - m)
    v = beta2 * v + (1.0 - beta2) * g * g
    upd = (lr / bc1) * m / (np.sqrt(v) / np.sqrt(bc2) + eps)
    cm2, am2 = encode(m, True)
    cv2, av2 = encode(v, False)
    return dict(p=p - upd, update=upd, m=m, v=v, g=g, cm=cm2, am=am2, cv=cv2, av=av2)


def fresh_state(n: int):
    """cm, am, cv, av of a tensor that has not been updated yet."""
    return (np.full(n, 127, np.uint8), np.zeros(nblocks(n)), np.zeros(n, np.uint8), np.zeros(nblocks(n)))


def adamw_fp64(p, grads, lr, beta1, beta2, eps, wd):
    """Plain AdamW (float64 state) over the list of gradients: the parameter after each step."""
    p = np.asarray(p, dtype=np.float64).copy()
    m, v, out = np.zeros_like(p), np.zeros_like(p), []
    for t, g in enumerate(grads, 1):
        p = p * (1.0 - lr * wd)
        m = m + (1.0 - beta1) * (g - m)
        v = beta2 * v + (1.0 - beta2) * g * g
        p = p - (lr / (1.0 - beta1 ** t)) * m / (np.sqrt(v) / np.sqrt(1.0 - beta2 ** t) + eps)
        out.append(p.copy())
    return out


def adamw8_trajectory(p, grads, lr, beta1, beta2, eps, wd, code1_rule=True):
    """The 8-bit optimizer over the list of gradients from fresh state: the parameter after each step.  ``code1_rule=False`` is
    plain nearest rounding of exp_avg_sq (the published scheme), kept to show what the rule is for."""
    p = np.asarray(p, dtype=np.float64).copy()
    cm, am, cv, av = fresh_state(p.size)
    out = []
    for t, g in enumerate(grads, 1):
        r = adamw8_step(p, g, cm, am, cv, av, t, lr, beta1, beta2, eps, wd)
        p, cm, am, cv, av = r["p"], r["cm"], r["am"], r["cv"], r["av"]
        if not code1_rule:
            cv = nearest(normalised(r["v"], av), False)
        out.append(p.copy())
    return out


def trajectory_data(seed: int, n: int = 65536, steps: int = 20, spread: float = 0.5):
    """p0 = 0.02 N; g = (N + 0.3) s per step, s = exp(2 N) per block times exp(spread N) per element (fixed over the steps)."""
    rng = np.random.default_rng(seed)
    p0 = 0.02 * rng.standard_normal(n)
    s = np.repeat(np.exp(2.0 * rng.standard_normal(nblocks(n))), BLOCK)[:n] * np.exp(spread * rng.standard_normal(n))
    grads = [((rng.standard_normal(n) + 0.3) * s).astype(np.float32).astype(np.float64) for _ in range(steps)]
    return p0.astype(np.float32).astype(np.float64), grads


def rel_l2(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))
