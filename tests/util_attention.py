"""Attention forward / backward against float64, per (batch, head, row): data families, references with their bound
terms, rounding emulations and the per-row checks shared by test_attention_range_gpu.py (the kernels) and
test_attention_bounds_cpu.py (the proof that the bounds fit correct arithmetic and reject the errors they are for).

Everything is in LOG2 units: the kernels evaluate P = exp2(S2 - reference) with S2 = (q . k) * c, c = scale * log2(e)
(``scale`` > 0) or c = 1 (``scale`` = 0: the q projection already folded d**-0.5 * log2(e) in, and the STORED q is what
the kernel multiplies).  The reference is evaluated on exactly the stored (fp16 / bf16 rounded) operands; for the
pre-scaled mode S2 = q_stored . k_stored, which is the softmax of (q_stored / (d**-0.5 log2 e)) at scale d**-0.5 that
test_attention_prescaled_log2_scores writes, without the division and re-multiplication.

Notation: u = 2^-11 (fp16) / 2^-8 (bf16); P the exact softmax row; A[q, c] = sum_k P[q, k] |v[k, c]|.

Forward bounds (csrc/attention.hip)
  |o - ref| <= 3 u A, element by element.  The kernel rounds each exp2(S2 - reference) ONCE to the storage type before it
  enters the P.V MFMA and (through the row of ones in V^T, or the fp32 sum of the SAME values for the other head dims)
  the denominator.  The reference sits at most 2^8 below the row maximum (RESCALE_THR), so the rounded values are <= 2^8
  and every one that matters is a normal number: relative error <= u each, in numerator and denominator alike, which moves
  o by <= 2 u A.  The stored output costs u |o| <= u A.  fp32 accumulation over <= 2^13 keys and v_exp_f32 add O(1e-6) A.
  The emulation (``emulate_forward``: reference 0 / 3.3 / 7.9 below the row maximum, the reference itself rounded to the
  storage type as the slot kernel keeps it) stays below HALF of it on every family (test_attention_bounds_cpu.py).
  Per-row rel-L2 < TOL * 1.5 (the per-tensor tolerance of test_ops_gpu.py, now per row): three roundings give <= 3 u
  unless the row cancels (|o| << A).  The emulated roundings stay within a quarter of it on every family (flat rows over
  many keys cancel a little, by ~sqrt(Tk), but so do their rounding errors), so no forward family is exempt.
  lse: |lse - ref| <= 2 u + 2^-22 |ref|.  The row sum of rounded P has relative error <= u, i.e. <= 1.44 u in log2;
  v_log_f32 and the fp32 reference term (|ref| up to ~300 -> 2^-24 |ref| per operation) are the rest.

Backward bounds (csrc/attention_bwd.hip; S = scale, W[q] = sum_c |dO[q, c]| |o[q, c]|, exact P, dP = dO v^T,
D = rowsum(dO o), dS = P (dP - D))
  The kernels recompute P = exp2(S2 - lse) (lse: 1.44 u from the forward), round P and dS to the storage type before
  the MFMA, take D from the STORED o (u |o| per element -> |D - ref| <= u W) and round the outputs.
    |dv - ref|[k, c] <= 4 u sum_q P[q, k] |dO[q, c]|         (P: 1.44 u + u, output u, < 4)
    |dq - ref|[q, c] <= S sum_k (5 u |dS[q, k]| + 2 u P[q, k] W[q]) |k[k, c]|
    |dk - ref|[k, c] <= S sum_q (5 u |dS[q, k]| + 2 u P[q, k] W[q]) |q[q, c]|
  (dS: P's 2.44 u, its own rounding u, output u -> 4.44 u |dS| < 5 u |dS|; the D term P u W, doubled for the rounding
  of the product.)  Rows whose reference gradient is below 1e-6 of the tensor's largest row norm get the max-abs bound
  only (a sink leaves most dk rows nearly zero).  ``emulate_backward`` applies exactly these roundings in float64 and
  the CPU test asserts it stays within half of the dq / dk bounds (reached: 0.29) and of the per-row rel-L2 tolerance
  TOL_BWD * 2 wherever REL_OK applies it.  The dv bound does NOT leave a factor 2: see EMU_FRAC.

Materialised-P fallback (``attention_backward`` without ``o``; Tq % 64 != 0): it stores the scaled scores, P, dP and dS
  as storage-type tensors between its GEMMs.  A stored score of magnitude |S2| (log2 units) costs P a relative
  r = u |S2| ln 2 before the normalisation and r + sum_j P_j r_j after it; stored P and dP add u each; D = rowsum(dP P)
  inherits them; dS carries u P (|dP| + |D|).  With EP = P (r + sum_j P_j r_j + u):
    dv:  + EP^T |dO|
    dS:  + EP |dP - D| + P sum_j (EP_j |dP_j| + u P_j |dP_j|) + u P (|dP| + |D|),  then S (.) |k| / |q| as above.
  Only the flat, peaky and sink families: a shift of +-60 makes r = 60 u ln 2 (bf16: 16 % per P) and offset V makes dP
  ~30 with cancelling D -- outside what stored intermediates can resolve; that is a property of the fallback, not a
  defect to test for (emulated per-row rel-L2 over half the tolerance: dv 2.3 .. 3.1 times at a shift of +-60, dk 7 .. 15
  times with offset V; the emulated max-abs error stays below 0.26 of these bounds on the three families kept).

Layout contract not tested as a violation: ``vt`` columns >= Tk are zero (ops.vt_proj / transpose2d_many pad64 write
zeros there); the kernels multiply them by P = 0 and a NaN there would propagate by design.  The backward wrapper takes
UNPADDED k / v [B, Tk, C] and returns unpadded dk / dv: rows >= Tk are never exposed, so there is no masked-row case.
"""
import math

import torch

U = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}
TOL_FWD = {torch.float16: 2e-3 * 1.5, torch.bfloat16: 1.2e-2 * 1.5}   # tests/test_ops_gpu.py: TOL * 1.5
TOL_BWD = {torch.float16: 3e-3 * 2, torch.bfloat16: 2e-2 * 2}         # tests/test_backward_gpu.py: TOL * 2
OLD_LSE = {torch.float16: 2e-3, torch.bfloat16: 1.5e-2}               # the old test_attention_forward_lse figure
LOG2E = 1.4426950408889634
DTYPES = [torch.float16, torch.bfloat16]

FAMILIES = ["flat", "peaky", "sink_first", "sink_last", "ramp_7.5", "ramp_8.5", "ramp_down", "mixed_one_jumps",
            "mixed_31_jump", "shift_-300", "shift_-60", "shift_0", "shift_60", "shift_300", "offset_v"]
BWD_FAMILIES = ["flat", "peaky", "sink_first", "sink_last", "ramp_8.5", "shift_-60", "shift_60", "offset_v"]
MAT_FAMILIES = ["flat", "peaky", "sink_first", "sink_last"]
# Per-row rel-L2 is asserted only where the emulated roundings of a CORRECT kernel stay within half of the tolerance
# (test_attention_bounds_cpu.py asserts exactly these entries; every other (tensor, family) keeps the element-wise bound).
# Forward: every family.  Backward: a query row with one dominant key has dP - D ~ 0 on that key, so dS and with it the dq
# row (and the dk rows of the other keys) is a small difference of terms that each carry u: peaky / sink rows of dq sit
# 30 .. 280 times over half the tolerance in the emulation, dk 1 .. 2.5 times.  A constant score shift is a constant
# column of k (k0 ~ 33) whose dq column is S k0 sum_k dS = 0 exactly, so the rounding of dS shows undivided (1.1 .. 1.6).
# Offset V: dP ~ 30 sum|dO| cancelled by D (dq 3 .. 7, dk 7 .. 19 times).  The rising ramp leaves dk rows of the early
# tiles with P ~ 2^-8.5 per tile (0.75).  dv never cancels (<= 0.2).  Materialised path: the stored scores add u |S2| ln 2
# per P, which a sink's 12 log2 units carry into dv (0.4 .. 0.6).
REL_OK = {
    "flash": {"dq": {"flat", "ramp_8.5"}, "dk": {"flat", "shift_-60", "shift_60"},
              "dv": {"flat", "peaky", "sink_first", "sink_last", "ramp_8.5", "shift_-60", "shift_60", "offset_v"}},
    "materialised": {"dq": {"flat"}, "dk": {"flat"}, "dv": {"flat", "peaky"}},
}
# dv: the three terms of its bound can align on a key that one query dominates (P ~ 1: lse 1.44 u + rounding of P u +
# output u = 3.44 u of the 4 u), so the emulation, which perturbs EVERY lse by the full 1.44 u, is held to 3.44 / 4 there
# instead of 1 / 2 (it reaches 0.55); dq / dk and the forward are held to 1 / 2.
EMU_FRAC = {"dq": 0.5, "dk": 0.5, "dv": 3.44 / 4}
# lse: one dominant key with a mantissa just above a power of two gives the full 1.44 u of the 2 u
EMU_FRAC_LSE = 0.75


def rnd(x, dtype):
    """float64 -> storage type -> float64 (round to nearest even, gradual underflow)."""
    return x.to(dtype).to(torch.float64)


def score_unit(d, prescaled):
    """c of S2 = (q . k) * c for the STORED operands, and the ``scale`` argument of ops.attention."""
    cs = d ** -0.5 * LOG2E
    return (1.0, 0.0, cs) if prescaled else (cs, None, cs)


def make_case(family, B, H, Tq, Tk, d, dtype, prescaled=False, seed=0):
    """-> dict(q [B, H, Tq, d], k, v [B, H, Tk, d], do [B, H, Tq, d]: float64 holding the STORED values; c; scale).
    Families are built in the logical (unscaled) q so that both scale modes see the same scores; channel 0 of q is a
    constant 8 and channel 0 of k carries a per-key score offset f(key) / (8 cs) (log2 units), channel 1 the per-query
    switch of the mixed-row families; the remaining channels are N(0, 1)."""
    g = torch.Generator().manual_seed(1000 * seed + 7 * Tq + 13 * Tk + d)
    c, _, cs = score_unit(d, prescaled)
    q = torch.randn(B, H, Tq, d, generator=g, dtype=torch.float64)
    k = torch.randn(B, H, Tk, d, generator=g, dtype=torch.float64)
    v = torch.randn(B, H, Tk, d, generator=g, dtype=torch.float64)
    do = torch.randn(B, H, Tq, d, generator=g, dtype=torch.float64)
    key = torch.arange(Tk, dtype=torch.float64)
    qi = torch.arange(Tq)
    f = None
    if family == "peaky":       # query i < min(Tq, Tk) has its dominant key at (i * st + 1) % Tk, scattered along the keys
        n = min(Tq, Tk)
        st = next(s for s in (37, 31, 29, 23, 19, 17, 13, 11, 7, 5, 3, 1) if math.gcd(s, Tk) == 1)
        j = (torch.arange(n) * st + 1) % Tk
        k[:, :, j] += (10.0 / (cs * d)) * q[:, :, :n]           # + ~10 log2 units (chi-square spread: 5 .. 16)
    elif family.startswith("sink"):
        f = torch.zeros(Tk, dtype=torch.float64)
        f[0 if family == "sink_first" else Tk - 1] = 12.0
    elif family.startswith("ramp"):
        step = -8.5 if family == "ramp_down" else float(family.split("_")[1])
        f = step * torch.floor(key / 64)
        q *= 0.5                                                  # score noise 0.7: the per-tile step decides the crossing
    elif family.startswith("mixed"):
        one = (qi % 32) == 5
        on = one if family == "mixed_one_jumps" else ~one
        q[..., 1] = torch.where(on, 8.0, 0.0).to(torch.float64)
        k[..., 1] = 0.0
        k[:, :, max(Tk - 3, 0), 1] = 40.0 / (8.0 * cs)
        f = torch.zeros(Tk, dtype=torch.float64)
    elif family.startswith("shift"):
        f = torch.full((Tk,), float(family.split("_")[1]), dtype=torch.float64)
    elif family == "offset_v":
        sign = torch.where(torch.rand(d, generator=g) < 0.5, -1.0, 1.0).to(torch.float64)
        v = v + 30.0 * sign
        v[..., 3] *= 50.0
    elif family != "flat":
        raise ValueError(family)
    if f is not None:
        q[..., 0] = 8.0
        k[..., 0] = f / (8.0 * cs)
    q = rnd(q * cs, dtype) if prescaled else rnd(q, dtype)
    return dict(q=q, k=rnd(k, dtype), v=rnd(v, dtype), do=rnd(do, dtype), c=c, scale=d ** -0.5, family=family,
                prescaled=prescaled, dtype=dtype)


# ---------------------------------------------------------------------------------------------------------------
# float64 references
def _head_scores(q, k, c):
    S2 = (q @ k.transpose(-1, -2)) * c
    m = S2.amax(-1, keepdim=True)
    E = torch.exp2(S2 - m)
    l = E.sum(-1, keepdim=True)
    return S2, E / l, (m + torch.log2(l)).squeeze(-1)


def forward_ref(case):
    """-> o, A [B, H, Tq, d], lse [B, H, Tq] (log2 units); one head's score matrix at a time."""
    q, k, v, c = case["q"], case["k"], case["v"], case["c"]
    o, A, lse = torch.empty_like(q), torch.empty_like(q), torch.empty(q.shape[:3], dtype=torch.float64)
    for b in range(q.shape[0]):
        for h in range(q.shape[1]):
            _, P, lse[b, h] = _head_scores(q[b, h], k[b, h], c)
            o[b, h], A[b, h] = P @ v[b, h], P @ v[b, h].abs()
    return o, A, lse


def backward_ref(case, materialised=False):
    """Closed-form float64 gradients of sum(o * do) for scale d**-0.5 on the stored operands (scale > 0 mode)
    -> dict(dq, dk, dv and their element-wise bounds bq, bk, bv in units of u; materialised: with that path's terms)."""
    q, k, v, do, c, S = case["q"], case["k"], case["v"], case["do"], case["c"], case["scale"]
    out = {n: torch.empty_like(t) for n, t in (("dq", q), ("bq", q), ("dk", k), ("bk", k), ("dv", v), ("bv", v))}
    for b in range(q.shape[0]):
        for h in range(q.shape[1]):
            S2, P, _ = _head_scores(q[b, h], k[b, h], c)
            o = P @ v[b, h]
            dP = do[b, h] @ v[b, h].T
            D = (do[b, h] * o).sum(-1, keepdim=True)
            W = (do[b, h].abs() * o.abs()).sum(-1, keepdim=True)
            dS = P * (dP - D)
            out["dv"][b, h] = P.T @ do[b, h]
            out["dq"][b, h] = S * (dS @ k[b, h])
            out["dk"][b, h] = S * (dS.T @ q[b, h])
            bv = 4 * (P.T @ do[b, h].abs())
            e = 5 * dS.abs() + 2 * P * W
            if materialised:
                r = S2.abs() * math.log(2.0)
                EP = P * (r + (P * r).sum(-1, keepdim=True) + 1.0)
                bv = bv + EP.T @ do[b, h].abs()
                e = e + EP * (dP - D).abs() + P * ((EP + P) * dP.abs()).sum(-1, keepdim=True) + P * (dP.abs() + D.abs())
            out["bv"][b, h] = bv
            out["bq"][b, h] = S * (e @ k[b, h].abs())
            out["bk"][b, h] = S * (e.T @ q[b, h].abs())
    return out


# ---------------------------------------------------------------------------------------------------------------
# emulations: float64 arithmetic with exactly the documented roundings of a CORRECT kernel
def emulate_forward(case, below=0.0, round_ref=False):
    """P rounded once relative to a reference ``below`` log2 units under the row maximum (rounded to the storage type
    itself when ``round_ref``: the slot kernel), numerator and denominator from the same rounded P, output rounded."""
    q, k, v, c, dt = case["q"], case["k"], case["v"], case["c"], case["dtype"]
    o, lse = torch.empty_like(q), torch.empty(q.shape[:3], dtype=torch.float64)
    for b in range(q.shape[0]):
        for h in range(q.shape[1]):
            S2 = (q[b, h] @ k[b, h].T) * c
            ref = S2.amax(-1, keepdim=True) - below
            if round_ref:
                ref = rnd(ref, dt)
            Pr = rnd(torch.exp2(S2 - ref), dt)
            l = Pr.sum(-1, keepdim=True)
            o[b, h] = rnd((Pr @ v[b, h]) / l, dt)
            lse[b, h] = (ref + torch.log2(l)).squeeze(-1)
    return o, lse


def emulate_backward(case, materialised=False, seed=0):
    """flash: lse off by +-1.44 u per row, P and dS rounded, D from the rounded o, outputs rounded.
    materialised: the scaled scores, P, dP and dS rounded as stored tensors, D = rowsum(dP P), outputs rounded."""
    q, k, v, do, c, S, dt = case["q"], case["k"], case["v"], case["do"], case["c"], case["scale"], case["dtype"]
    g = torch.Generator().manual_seed(seed)
    out = {n: torch.empty_like(t) for n, t in (("dq", q), ("dk", k), ("dv", v))}
    for b in range(q.shape[0]):
        for h in range(q.shape[1]):
            if materialised:
                s_nat = rnd((q[b, h] @ k[b, h].T) * S, dt)
                P = rnd(torch.softmax(s_nat, -1), dt)
                dP = rnd(do[b, h] @ v[b, h].T, dt)
                D = (dP * P).sum(-1, keepdim=True)
                Pm, dS = P, rnd(P * (dP - D) * S, dt)
                sc = 1.0
            else:
                S2, Px, lse = _head_scores(q[b, h], k[b, h], c)
                sign = torch.where(torch.rand(lse.shape, generator=g) < 0.5, -1.0, 1.0).to(torch.float64)
                P = torch.exp2(S2 - (lse + 1.44 * U[dt] * sign).unsqueeze(-1))
                o_st = rnd(Px @ v[b, h], dt)
                D = (do[b, h] * o_st).sum(-1, keepdim=True)
                Pm, dS = rnd(P, dt), rnd(P * (do[b, h] @ v[b, h].T - D), dt)
                sc = S
            out["dv"][b, h] = rnd(Pm.T @ do[b, h], dt)
            out["dq"][b, h] = rnd(sc * (dS @ k[b, h]), dt)
            out["dk"][b, h] = rnd(sc * (dS.T @ q[b, h]), dt)
    return out


# ---------------------------------------------------------------------------------------------------------------
# per-row checks.  Every tensor is [B, H, T, d] (lse [B, H, T]); ``heads`` turns a [B, T, H*d] result into that.
def heads(t, H):
    B, T, C = t.shape
    return t.detach().to("cpu", torch.float64).view(B, T, H, C // H).permute(0, 2, 1, 3)


def row_figures(got, ref, bound):
    """-> (rel-L2 per row, worst |err| / bound per row); a zero bound with a zero error counts as 0."""
    e = (got - ref).abs()
    rel = e.norm(dim=-1) / ref.norm(dim=-1).clamp_min(1e-300)
    ratio = torch.where(e <= bound, e / bound.clamp_min(1e-300), torch.full_like(e, float("inf")))
    ratio = torch.where(e == 0, torch.zeros_like(e), ratio)
    return rel, ratio.amax(-1)


def check_rows(got, ref, bound, tol, what, rel=True, floor=None, frac=1.0, frac_rel=None):
    """finite; |got - ref| <= frac * bound element by element; per-row rel-L2 < frac * tol (rows whose reference norm is
    below ``floor`` of the largest row norm: max-abs only; ``frac_rel`` if it differs from ``frac``).  Returns (worst rel-L2, worst |err| / bound)."""
    assert torch.isfinite(got).all(), f"{what}: non-finite output"
    frac_rel = frac if frac_rel is None else frac_rel
    e = (got - ref).abs()
    rel_l2, _ = row_figures(got, ref, bound)
    worst = (e / bound.clamp_min(1e-300)).masked_fill(e == 0, 0.0)
    over = worst > frac
    rn = ref.norm(dim=-1)
    use = torch.ones_like(rn, dtype=torch.bool) if floor is None else rn >= floor * rn.max()
    rel_w = rel_l2[use].max().item() if (rel and use.any()) else 0.0
    msg = (f"{what}: worst |err| / bound {worst.max().item():.3g} (allowed {frac:g}), elements over: {int(over.sum())} / "
           f"{over.numel()}, rows over: {int(over.any(-1).sum())} / {over.any(-1).numel()}; worst row rel-L2 {rel_w:.3e} "
           f"(allowed {frac_rel * tol:.2e})")
    assert not over.any() and rel_w < frac_rel * tol, msg
    return rel_w, worst.max().item()


def check_forward(o, ref, A, dtype, what, rel=True, frac=1.0):
    """o, ref, A: [B, H, Tq, d] float64."""
    return check_rows(o, ref, 3 * U[dtype] * A, TOL_FWD[dtype], what, rel=rel, frac=frac)


def lse_bound(ref, dtype):
    return 2 * U[dtype] + 2.0 ** -22 * ref.abs()


def check_lse(lse, ref, dtype, what, frac=1.0):
    assert torch.isfinite(lse).all(), f"{what}: non-finite lse"
    r = ((lse - ref).abs() / lse_bound(ref, dtype)).max().item()
    assert r <= frac, f"{what}: worst |lse - ref| / (2 u + 2^-22 |ref|) = {r:.3g} (allowed {frac:g})"
    return r


def check_backward(got, ref, dtype, what, family, path="flash", frac=None):
    """got: dict dq / dk / dv [B, H, T, d]; ref: backward_ref(...); frac: dict per tensor (the emulation test's)."""
    figs = {}
    for n, bn in (("dq", "bq"), ("dk", "bk"), ("dv", "bv")):
        f = 1.0 if frac is None else frac[n]
        figs[n] = check_rows(got[n], ref[n], U[dtype] * ref[bn], TOL_BWD[dtype], f"{what} {n}",
                             rel=family in REL_OK[path][n], floor=1e-6, frac=f, frac_rel=1.0 if frac is None else 0.5)
    return figs


def old_rel_l2(a, b):
    """conftest.rel_l2 on float64 stand-ins: the whole-tensor figure the earlier tests asserted."""
    return float((a - b).norm() / b.norm().clamp_min(1e-20))
