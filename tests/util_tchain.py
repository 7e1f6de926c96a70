"""ur_tchain (csrc/tchain.hip, host side uni_renderer_amd/tchain.py) per ELEMENT against float64: problems, references with
their bound terms, an fp32 emulation, checkers and a guarded launcher shared by test_tchain_range_gpu.py (the kernel) and
test_tchain_bounds_cpu.py (the proof that the reference is the operation, that the exact family is exact, that the bounds
fit correct arithmetic and that the checkers reject the errors they are for).  The checkers, the guard / sentinel buffers
and the constants u, LO_REL, TINY* are util_igemm's.

A problem is built by ``make_problem(spec)`` from a small dict (DEFAULTS below): mode "q" | "pre" | "ff", S = streams, M
rows per stream (= B * T when the spec names samples), different weights and constants per stream.  The weight streams
and const blocks come from the product's packers (tchain.pack_chain_q / _pre / _ff); the float64 reference runs over the
STORED operands, r(.) = round to the storage type:

    stored weights: r(w);  r(wq * scale) with the scale multiplied in fp32;  w2s = r(0.5 * w2)
    y    = a0 W0^T + b0 (+ res + res_lo)                     y_out = (hi, lo), hi = r(y), lo = lo_encode(y - hi)
    xn   = r(LN(y; gamma, beta, eps))                        (LayerNorm over the unrounded y)
    Q:   q = r(xn Wq^T)         PRE:  q, k, V^T[sample][channel][token] = r(xn W^T)
    FF:  hcat = xn W1^T + b1;  h2 = r(2 value gelu_erf(gate))   (the kernel forms 2 value gelu; the host halves w2)
         y3 = y + b2 + h2 w2s^T;  out = r(y3) Wpo^T + bpo + blk + blk_lo, stored as (hi, lo)
    head-major q / k: the same values at [sample][head][token][40].

Exact family ("gamma0")
  The LayerNorm stores fmaf((x - mean) * rstd, gamma, beta): with gamma = 0 the operand is beta, whatever the row holds.
  a0 in [-3, 3], b0 / b2 / bpo in [-4, 4], res / blk in [-8, 8] are integers, beta in {-1, 0, 1}; every weight is 0 / +-1:
  W0, Wq, Wk, Wv density 1/8, W1 value rows 1/64 with value bias in [-1, 1], W1 gate rows exactly one +-1 with gate bias
  9 (gates in [8, 10] by construction), W2 1/320 (stored +-0.5), Wpo exactly one +-1 per row; q_scale = qk_scale = 1.
  fp16 problems with low parts carry res_lo, blk_lo = +-0.25 (e5m2-exact), bf16 ones 0.  Every gate is an integer >= 7,
  where the program's erf is exactly 1 in fp32
  (p t exp2(-zc^2) < 2^-25: test_tchain_bounds_cpu.py runs the formula for gates 7 .. 16), so h2 = 2 gate value.  Every
  product and partial sum, in any order, is a multiple of 1/4 below 2^22 and exact in fp32.  ``make_problem`` asserts on the
  float64 reference, without re-drawing, that xn, h2, r(y3) and every output are representable in the problem's storage
  type and at most 256.5 in magnitude (integers <= 256 -- which fp16 AND bf16 hold -- plus, in fp16 problems only, the
  quarter offsets of the low parts; 256.5 has 11 significant bits).  The outputs must then be torch.equal to the reference
  and the low parts zero.  y and, through y3, the FF out differ from row to row: every row, wave and tile position of the
  first and last GEMM and every column of every streamed matrix is pinned.  All rows share one xn: this family cannot see
  a row mix-up in q, k or V^T -- the toleranced family's job.

Toleranced family ("gauss": the data of test_tchain_gpu.py)
  Notation: u = 2^-11 / 2^-8; c(K) = (K + 8) 2^-23; |.| element-wise; v the reference.
  * GEMM sums (util_igemm's derivation): products of two fp16 / bf16 numbers are exact in fp32; a sum of K of them plus a
    few more terms, in any order, is off by at most (K + 1) 2^-24 sum|terms| to first order (Higham 4.2).  CHARGED, not
    derived: 2^-23 per term instead of 2^-24 (the MFMA's internal alignment is not documented) and "+ 8" for the bias,
    residual and low-part additions.  fp = c(320) A, A = |a| |W|^T + |bias| + |res| + |res_lo|; y3 sums 1280 + 2 more terms
    on top of y: c(1280) (|y| + |b2| + |h2| |w2s|^T) + fp_y.
  * pair outputs (y_out, FF out): hi within u |v| + fp + TINY, hi + lo within LO_REL u |v| + fp + TINY_LO (util_igemm).
  * rounded operands.  The reference rounds its own float64 value x; the kernel rounds x' with |x' - x| <= delta.
    Rounding is monotone, so both operands lie in [r(x - delta), r(x + delta)]: the operand is "susceptible" when these
    two differ, and then the difference is at most ch = r(x + delta) - r(x - delta) (one ulp while delta < ulp).  Computed
    from the reference alone and charged to the next GEMM as D[m][n] = sum_k ch[m][k] |w[n][k]|; the next GEMM's A uses
    max(|r(x - delta)|, |r(x + delta)|).  Bound of q, k, V^T, FF out: u |v| + fp + D (pair: LO_REL u |v| + fp + D).  In FF
    the deltas propagate xn -> h2 -> r(y3), each including the D of the layer before.
  * delta of the LayerNorm in fp32 (two passes, per row; dy = fp_y):
      mean: sum of 320 terms and one multiplication: E_mean = mean(dy) + c(320) mean|y|  (factor 2 charged as above);
      c_i = y_i - mean: dc_i = dy_i + E_mean + 2^-24 |c_i|;  rho = rms(dc);
      var = mean(c^2): dvar = 2 sqrt(var) rho + rho^2 (Cauchy-Schwarz, second order kept: it matters when var ~ eps)
                              + c(320) var + 2^-23 (var + eps)  (the fma sum, the 1/320 and the + eps);
      rstd = (var + eps)^-1/2: relative change (1 - X)^-1/2 - 1 with X = dvar / (var + eps) (asserted < 1/2), plus 2^-22
        for rsqrtf, CHARGED at 4 ulp;
      xhat = c rstd: dxhat = (rstd dc + |xhat| rel)(1 + rel) + 2^-23 |xhat|;
      xn = fma(xhat, gamma, beta): dxn = |gamma| dxhat + 2^-23 (|gamma xhat| + |beta|)   (one rounding, charged twice).
  * delta of the GEGLU program (tools/gen_tchain_asm.py: g + |g| erf(|g| / sqrt 2) with Abramowitz-Stegun 7.1.26, v_rcp_f32
    for 1 / (1 + p z), v_exp_f32 for exp2(-zc^2)):  |erf error| <= 1.5e-7 (the formula) + 2^-22 CHARGED for its fp32
    evaluation (v_rcp and v_exp at one ulp each, the rounded exponent argument, whose effect a e^-a <= 0.37 bounds, five
    FMAs on values <= 1.5), two more roundings for |g| erf and the sum: 2 c_gelu(gate) with util_igemm's c_gelu.  With
    dv, dg the deltas of value and gate (fp + D of hcat) and max |gelu'| <= 1.13:
      dh2 = 2 (|gelu(gate)| dv + 1.13 |value| dg + 1.13 dv dg + |value| c_gelu(gate)) + 2^-23 |h2|.
  * per row: rel-L2 < 1.5e-3 (fp16) / 1.2e-2 (bf16), the tolerances of test_tchain_gpu.py, for every output and pair;
    for V^T also per (sample, channel) row over the tokens.
  What is NOT derived (charged): the factor 2 on every summation term, "+ 8", the 4 ulp of rsqrtf, the 2^-22 evaluation
  allowance of the erf polynomial.  It is held on the CPU: test_tchain_bounds_cpu.py keeps an fp32 emulation of a correct
  kernel (``emulate``: torch float32, 64-wide k chunks forwards and backwards, two-pass LayerNorm, the program's formula
  with the constants read from tchain_asm.inc, ops.lo_encode) within HALF of fp + D before the storage rounding and
  within the whole bound after it.
  How tight the bounds are.  D is a worst-case (same-sign) sum over the susceptible operands.  For q / k / V^T it is one
  layer deep (figures below).  In FF it passes through three layers, and with the dense N(0, 1/320) matrices of this
  family nearly every h2 and r(y3)
  operand is susceptible: the element bound of the FF out is then far wider than u |v| (figures below) and the per-row
  rel-L2 is the assertion that binds there.  The case "ff_po1" (Wpo with one N(0, 1) entry per row, residuals ~ 16) keeps
  D_out to one term, so that the pair bound of the FF out resolves the low part.
  Worst figures, row rel-L2 / |err| / bound (pairs: of hi + lo), forwards and backwards k order:
    CPU fp32 emulation (printed by test_tchain_bounds_cpu.py); "fp32" = the unrounded value's error over fp + D (held < 0.5);
    susceptible share of xn: 1.00 (fp16), 0.70 - 0.81 (bf16; 0.25 with residuals ~ 16); of h2 and r(y3): 1.00
      fp16  y 2.4e-4 / 0.75 (res 16: 0.88)   y pair 1.3e-5 / 0.17 (0.26)   q k v 2.6e-4 / 0.05 (flat rows 3.4e-4; res 16: 0.11)
            V^T rows 2.7e-4   FF out 2.7e-4 / 5e-5 (res 16: 1.5e-3; po1: 0.81)   FF out pair 1.8e-4 / 2e-5 (3e-4; po1: 0.19)
            fp32: y 0.005, q k v 0.017, FF out 3e-4 (po1: 0.02)
            median bound / (u |v|): y 2, q 113 - 155, FF out 9e4 (po1: 140)
      bf16  y 2.0e-3 / 0.98   y pair 3.2e-6 / 0.11   q k v 1.9e-3 / 0.22 (res 16: 0.55)   V^T rows 2.1e-3
            FF out 2.0e-3 / 5e-4 (res 16: 0.016; po1: 0.95)   FF out pair 8.2e-4 / 8e-5 (1.5e-3; po1: 0.077)
            fp32: y 0.004, q k v 0.07 (res 16: 0.17), FF out 1.5e-3 (po1: 0.077)
            median bound / (u |v|): y 1.1, q 15 - 20, FF out 1e4 (po1: 18)
    MI355X (printed by test_tchain_range_gpu.py::test_c_gauss / test_d_gauss_large_residuals):
      fp16  y 2.4e-4 / 0.75 (res 16: 0.88)   y pair 1.3e-5 / 0.17 (0.26)   q k v 2.4e-4 / 0.05 (flat rows 3.4e-4; res 16: 0.11)
            V^T rows 2.7e-4   FF out 2.7e-4 / 5e-5 (res 16: 1.5e-3; po1: 0.81)   FF out pair 1.6e-4 / 2e-5 (3e-4; po1: 0.19)
      bf16  y 2.0e-3 / 0.98   y pair 3.2e-6 / 0.11   q k v 1.9e-3 / 0.22 (res 16: 0.55)   V^T rows 2.1e-3
            FF out 2.4e-3 / 5e-4 (res 16: 0.016; po1: 0.95)   FF out pair 1.7e-3 / 1.4e-4 (3e-3; po1: 0.077)
      i.e. the CPU emulation's figures to the digits shown, except the dense FF out in bf16 (row rel-L2 2.4e-3 against
      2.0e-3, its pair 1.7e-3 against 8e-4: another summation order flips other operands).  The exact family passed
      bit for bit in every case, the guards held, two runs gave identical bits.
  What the figures say: the y bound and the y pair bound are tight (the stored y uses 0.75 - 0.98 of its bound, which is the
  rounding term).  The q / k / V^T bound is 15 - 20 u |v| in bf16 and > 100 u |v| in fp16, where the worst-case fp32 error
  of y alone (c(320) A ~ 7e-4) reaches an ulp of xn: an error of a few ulp in ONE fp16 element of q is below what it
  resolves (test_tchain_bounds_cpu.py::test_sensitivity_5 prints it); the exact family and the per-row rel-L2 cover fp16.
  The element bound of the dense FF out is vacuous (1e4 u |v|); "ff_po1" is the FF case with a bound that bites.

Guards
  ``launch`` calls tchain._launch with buffers of its own: a0, res, res_lo, blk, blk_lo embedded in NaN with GUARD_ROWS
  rows in front and behind (row stride 320: the kernel's), the const block with NaN behind each stream's floats (z_consts >
  the block for S = 2), the weight stream between two NaN pads; y, y.lo, q, k, out, out.lo in sentinel buffers with
  GUARD_ROWS on both sides; V^T a sentinel tensor [samples + 2][320][ld_vt] with one guard sample on each side and ld_vt =
  Tpad + 8 (136 for T = 96): token columns T .. ld_vt must keep the sentinel bit for bit.  Nothing outside the named regions
  may change.  ``hilo=False`` problems pass every *_lo as NULL.
"""
import math
import os
import re

import torch

import util_igemm as ug
from util_igemm import LO_REL, TINY, TINY_LO, U, rnd

C = 320
FF = 4 * C
HEADS, HEAD_DIM = 8, 40
TOL = {torch.float16: 1.5e-3, torch.bfloat16: 1.2e-2}          # tests/test_tchain_gpu.py, here per row
OLD_PAIR_TOL = {torch.float16: 2e-4, torch.bfloat16: 2e-3}     # its whole-tensor tolerance for the pair y
C320, C1280 = (C + 8) * 2.0 ** -23, (FF + 8) * 2.0 ** -23
GUARD_ROWS = ug.GUARD_ROWS
PAD = 64  # NaN floats behind each const block / NaN elements around the weight stream (128 bytes: keeps 16-byte alignment)
f64 = torch.float64

DEFAULTS = dict(mode="q", family="gamma0", dtype=torch.float16, seed=0, S=1, M=0, B=0, T=0, eps=1e-5, hilo=True,
                res_std=1.5,     # gauss: standard deviation of res / blk (1.5: test_tchain_gpu.py; 16: coarse-ulp residuals)
                flat=False,      # gauss: every 5th row has a0 = 0 and res = 0.5 + {-1, 0, 1} ulp (near-zero variance); b0 = 0
                po1=False)       # gauss ff: Wpo with one N(0, 1) entry per row instead of N(0, 1/320) everywhere


def gelu2_64(g):
    """g + |g| erf(|g| / sqrt 2) = 2 gelu_erf(g)."""
    return g + g.abs() * torch.erf(g.abs() * 0.7071067811865476)


def _span(x, d, dtype):
    """Monotone rounding: an operand computed within d of x rounds into [lo, hi].  -> (r(x), hi - lo, max(|lo|, |hi|))."""
    lo, hi = rnd(x - d, dtype), rnd(x + d, dtype)
    return rnd(x, dtype), hi - lo, torch.maximum(lo.abs(), hi.abs())


def ln_delta(y, dy, gamma, beta, eps):
    """-> (xn float64, dxn): the LayerNorm of the docstring and the bound on what a two-pass fp32 evaluation over inputs
    within dy of y can differ from it."""
    mean = y.mean(-1, keepdim=True)
    c = y - mean
    var = (c * c).mean(-1, keepdim=True)
    rstd = (var + eps) ** -0.5
    xhat = c * rstd
    xn = xhat * gamma + beta
    e_mean = dy.mean(-1, keepdim=True) + C320 * y.abs().mean(-1, keepdim=True)
    dc = dy + e_mean + 2.0 ** -24 * c.abs()
    rho = (dc * dc).mean(-1, keepdim=True).sqrt()
    dvar = 2 * var.sqrt() * rho + rho * rho + C320 * var + 2.0 ** -23 * (var + eps)
    X = dvar / (var + eps)
    assert float(X.max()) < 0.5, f"LayerNorm bound: relative variance error {float(X.max())} is not small"
    rel = (1 - X) ** -0.5 - 1 + 2.0 ** -22
    dxhat = (rstd * dc + xhat.abs() * rel) * (1 + rel) + 2.0 ** -23 * xhat.abs()
    return xn, gamma.abs() * dxhat + 2.0 ** -23 * ((gamma * xhat).abs() + beta.abs())


def _draw(p, g):
    """Raw parameters and inputs of one problem: dict of float64 tensors (weights / consts per stream stacked on dim 0)."""
    dt, S, M, fam, mode = p["dtype"], p["S"], p["M"], p["family"], p["mode"]
    ints = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g).to(f64)
    normal = lambda *s: torch.randn(*s, generator=g, dtype=f64)
    sign = lambda *s: 2 * ints(0, 1, *s) - 1
    sparse = lambda dens, *s: torch.where(torch.rand(*s, generator=g) < dens, 1.0, 0.0).to(f64) * sign(*s)
    d = {}
    if fam == "gamma0":
        quarter = (lambda *s: 0.25 * sign(*s)) if dt == torch.float16 else (lambda *s: torch.zeros(*s, dtype=f64))
        d.update(a0=ints(-3, 3, S, M, C), w0=sparse(1 / 8, S, C, C), b0=ints(-4, 4, S, C), gamma=torch.zeros(S, C, dtype=f64),
                 beta=ints(-1, 1, S, C), scale=1.0)
        if mode != "pre":
            d.update(res=ints(-8, 8, S, M, C), res_lo=quarter(S, M, C))
        if mode in ("q", "pre"):
            d.update(wq=sparse(1 / 8, S, C, C))
        if mode == "pre":
            d.update(wk=sparse(1 / 8, S, C, C), wv=sparse(1 / 8, S, C, C))
        if mode == "ff":
            one_per_row = lambda n: torch.zeros(S, n, C, dtype=f64).scatter_(2, torch.randint(0, C, (S, n, 1), generator=g), sign(S, n, 1))
            w1 = torch.cat([sparse(1 / 64, S, FF, C), one_per_row(FF)], 1)
            b1 = torch.cat([ints(-1, 1, S, FF), torch.full((S, FF), 9.0, dtype=f64)], 1)
            wpo = one_per_row(C)
            d.update(w1=w1, b1=b1, w2=sparse(1 / 320, S, C, FF), b2=ints(-4, 4, S, C), wpo=wpo, bpo=ints(-4, 4, S, C),
                     blk=ints(-8, 8, S, M, C), blk_lo=quarter(S, M, C))
    else:
        assert fam == "gauss", fam
        r32 = lambda t: t.float().double()  # fp32 parameters, as a checkpoint holds them
        pair = lambda v: ug._lo_pair(v, dt)
        d.update(a0=rnd(normal(S, M, C) * 1.5, dt), w0=rnd(normal(S, C, C) * C ** -0.5, dt), b0=r32(normal(S, C) * 0.1),
                 gamma=r32(1 + normal(S, C) * 0.1), beta=r32(normal(S, C) * 0.1))
        sc = HEAD_DIM ** -0.5 * 1.4426950408889634
        d["scale"] = sc if mode == "q" else math.sqrt(sc)
        if mode != "pre":
            d["res"], d["res_lo"] = pair(normal(S, M, C) * p["res_std"])
        if p["flat"]:
            assert mode != "pre"
            rows = torch.arange(0, M, 5)
            ulp = 2 * U[dt] * 0.5  # spacing of the storage type in [0.5, 1)
            d["b0"] = torch.zeros(S, C, dtype=f64)
            d["a0"][:, rows] = 0.0
            d["res"][:, rows] = 0.5 + ulp * ints(-1, 1, S, len(rows), C)
            d["res_lo"][:, rows] = 0.0
            d["flat_rows"] = rows
        if mode in ("q", "pre"):
            d.update(wq_raw=r32(normal(S, C, C) * C ** -0.5))
        if mode == "pre":
            d.update(wk_raw=r32(normal(S, C, C) * C ** -0.5), wv=rnd(normal(S, C, C) * C ** -0.5, dt))
        if mode == "ff":
            if p["po1"]:
                wpo = torch.zeros(S, C, C, dtype=f64)
                wpo.scatter_(2, torch.randint(0, C, (S, C, 1), generator=g), normal(S, C, 1))
            else:
                wpo = normal(S, C, C) * C ** -0.5
            d.update(w1=rnd(normal(S, 2 * FF, C) * C ** -0.5, dt), b1=r32(normal(S, 2 * FF) * 0.1),
                     w2_raw=r32(normal(S, C, FF) * FF ** -0.5), b2=r32(normal(S, C) * 0.1), wpo=rnd(wpo, dt),
                     bpo=r32(normal(S, C) * 0.1))
            d["blk"], d["blk_lo"] = pair(normal(S, M, C) * p["res_std"])
    if not p["hilo"]:
        for k in ("res_lo", "blk_lo"):
            d.pop(k, None)
    return d


def _scaled(w_raw, scale, dt):
    """What the packers store for a scaled matrix: the fp32 product, rounded."""
    return rnd((w_raw.float() * scale).double(), dt)


def make_problem(spec):
    """-> dict: the spec's entries plus the stored operands (float64; weights and consts [S, ...], rows [S, M, 320]), the
    raw matrices the packers take (wq_raw, wk_raw, w2_raw), ``ref`` = {name: float64 reference before the storage
    rounding} for y, q, k, v (token-major; ``vt`` is its transpose per sample) and out, ``fp`` / ``D`` = the fp32 part of
    each bound and its operand-rounding part, ``sus`` = share of susceptible elements per rounded operand."""
    p = dict(DEFAULTS)
    unknown = set(spec) - set(p)
    assert not unknown, unknown
    p.update(spec)
    if p["B"]:
        p["M"] = p["B"] * p["T"]
    dt, S, M, fam, mode = p["dtype"], p["S"], p["M"], p["family"], p["mode"]
    g = torch.Generator().manual_seed(1000003 * p["seed"] + 7 * M + 13 * S + {"q": 1, "pre": 2, "ff": 3}[mode])
    d = _draw(p, g)
    p.update(d)
    if fam == "gauss":  # the stored forms of the matrices the packers scale
        if "wq_raw" in p:
            p["wq"] = _scaled(p["wq_raw"], p["scale"], dt)
        if "wk_raw" in p:
            p["wk"] = _scaled(p["wk_raw"], p["scale"], dt)
    else:
        for k in ("wq", "wk"):
            if k in p:
                p[k + "_raw"] = p[k]
    if mode == "ff":
        if fam == "gamma0":
            p["w2_raw"] = p["w2"]
        p["w2s"] = _scaled(p["w2_raw"], 0.5, dt)
    zero = torch.zeros(S, M, C, dtype=f64)
    bc = lambda v: v[:, None, :]                                    # [S, C] -> [S, 1, C]
    mm = lambda a, w: torch.einsum("smk,snk->smn", a, w)
    res, res_lo = p.get("res", zero), p.get("res_lo", zero)
    ref, fp, D, sus = {}, {}, {}, {}
    y = mm(p["a0"], p["w0"]) + bc(p["b0"]) + res + res_lo
    dy = C320 * (mm(p["a0"].abs(), p["w0"].abs()) + bc(p["b0"]).abs() + res.abs() + res_lo.abs())
    ref["y"], fp["y"], D["y"] = y, dy, torch.zeros_like(y)
    xn, dxn = ln_delta(y, dy, bc(p["gamma"]), bc(p["beta"]), p["eps"])
    xn_op, ch, xmax = _span(xn, dxn, dt)
    sus["xn"] = float((ch > 0).double().mean())
    p["xn"] = xn_op
    inter = {"xn": xn_op}
    for name in ("q", "k", "v"):
        w = p.get("w" + name)
        if w is not None:
            ref[name], fp[name], D[name] = mm(xn_op, w), C320 * mm(xmax, w.abs()), mm(ch, w.abs())
    if mode == "ff":
        hc = mm(xn_op, p["w1"]) + bc(p["b1"])
        dh = C320 * (mm(xmax, p["w1"].abs()) + bc(p["b1"]).abs()) + mm(ch, p["w1"].abs())
        val, gate, dv, dg = hc[..., :FF], hc[..., FF:], dh[..., :FF], dh[..., FF:]
        h2 = val * gelu2_64(gate)
        dh2 = (gelu2_64(gate).abs() * dv + 2 * ug.L_GELU * (val.abs() * dg + dv * dg) + 2 * val.abs() * ug.c_gelu(gate)
               + 2.0 ** -23 * h2.abs())
        h2_op, ch_h, hmax = _span(h2, dh2, dt)
        y3 = y + bc(p["b2"]) + mm(h2_op, p["w2s"])
        d3 = dy + C1280 * (y.abs() + bc(p["b2"]).abs() + mm(hmax, p["w2s"].abs())) + mm(ch_h, p["w2s"].abs())
        y3_op, ch_3, y3max = _span(y3, d3, dt)
        blk, blk_lo = p["blk"], p.get("blk_lo", zero)
        ref["out"] = mm(y3_op, p["wpo"]) + bc(p["bpo"]) + blk + blk_lo
        fp["out"] = C320 * (mm(y3max, p["wpo"].abs()) + bc(p["bpo"]).abs() + blk.abs() + blk_lo.abs())
        D["out"] = mm(ch_3, p["wpo"].abs())
        sus.update(h2=float((ch_h > 0).double().mean()), y3=float((ch_3 > 0).double().mean()))
        inter.update(h2=h2_op, y3=y3_op)
        p.update(gate=gate, value=val, h2=h2_op, y3=y3_op)
    if fam == "gamma0":
        what = f"exact family ({ {k: v for k, v in spec.items() if k != 'dtype'} }, {dt})"
        assert torch.equal(xn, bc(p["beta"]).expand_as(xn)), f"{what}: xn is not beta"
        if mode == "ff":
            assert torch.equal(gate, gate.round()) and float(gate.min()) >= 7, f"{what}: gates reach {float(gate.min())} < 7"
            assert float((h2 - 2 * gate * val).abs().max()) < 1e-6, f"{what}: erf(gate) is not 1 to rounding"
            assert torch.equal(h2_op, 2 * gate * val), f"{what}: h2 is not 2 gate value"
            inter["y3_unrounded"] = y3
        for k, v in list(inter.items()) + [("ref " + k, v) for k, v in ref.items()]:
            worst = float(v.abs().max())
            assert worst <= 256.5, f"{what}: max |{k}| = {worst} > 256.5"
            assert torch.equal(rnd(v, dt), v), f"{what}: {k} is not representable in {dt}"
        p["ranges"] = {k: float(v.abs().max()) for k, v in list(inter.items()) + list(ref.items())}
        if mode == "ff":
            p["ranges"]["gate"] = (float(gate.min()), float(gate.max()))
    p.update(ref=ref, fp=fp, D=D, sus=sus)
    return p


def vt_of(p, v):
    """token-major [S, M, 320] -> V^T [S, B, 320, T]."""
    return v.reshape(p["S"], p["B"], p["T"], C).transpose(2, 3).contiguous()


def head_major(p, t):
    """token matrix [S, M, 320] -> the [sample][head][token][40] image, as [S, M, 320] storage."""
    S, B, T = p["S"], p["B"], p["T"]
    return t.reshape(S * B, T, HEADS, HEAD_DIM).permute(0, 2, 1, 3).reshape(S, B * T, C)


def bounds(p, name):
    """-> dict(hi = bound on |stored - ref|, pair = bound on |hi + lo - ref|, fp = the part of both that is not a storage
    rounding: fp32 sums and functions + D)."""
    dt, v = p["dtype"], p["ref"][name].abs()
    f = p["fp"][name] + p["D"][name]
    return dict(hi=U[dt] * (v + f) + f + TINY[dt], pair=LO_REL[dt] * U[dt] * (v + f) + f + TINY_LO[dt], fp=f)


def expected_pair(p, name):
    """(hi, lo) float64 of the pair that stores the reference (exact family: what the kernel must produce bit for bit)."""
    return ug._lo_pair(p["ref"][name], p["dtype"])


OUTPUTS = {"q": ("y", "q"), "pre": ("y", "q", "k", "v"), "ff": ("out",)}
PAIRS = {"q": ("y",), "pre": ("y",), "ff": ("out",)}


# ---------------------------------------------------------------------------------------------------------------
# packing (the product's packers) and the guarded launch
def pack(p):
    """-> (wstream [S, L] storage type, consts [S, NC] fp32) from tchain.pack_chain_*."""
    from uni_renderer_amd import tchain
    dt, mode = p["dtype"], p["mode"]
    f = lambda k, s: p[k][s].float()
    ws, cs = [], []
    for s in range(p["S"]):
        if mode == "q":
            w, c = tchain.pack_chain_q(f("w0", s), f("b0", s), f("gamma", s), f("beta", s), f("wq_raw", s), p["scale"], dt)
        elif mode == "pre":
            w, c = tchain.pack_chain_pre(f("w0", s).view(C, C, 1, 1), f("b0", s), f("gamma", s), f("beta", s), f("wq_raw", s),
                                         f("wk_raw", s), f("wv", s), p["scale"], dt)
        else:
            w, c = tchain.pack_chain_ff(f("w0", s), f("b0", s), f("gamma", s), f("beta", s), f("w1", s), f("b1", s),
                                        f("w2_raw", s), f("b2", s), f("wpo", s), f("bpo", s), dt)
        ws.append(w)
        cs.append(c)
    return torch.stack(ws), torch.stack(cs)


def ld_vt_of(T):
    return ug.roundup(T, 64) + 8


def launch(p, dev, head_major_qk=False):
    """Run problem ``p`` through tchain._launch with every operand embedded in NaN and every output in a sentinel buffer;
    asserts that nothing outside the named regions changed and returns float64 CPU tensors {y, y_lo, q, k, vt, out,
    out_lo} ([S, M, 320]; vt [S, B, 320, T]; the *_lo only for hilo problems), q / k as stored (head-major images when
    asked)."""
    from uni_renderer_amd import ops, tchain
    dt, S, M, mode, hilo = p["dtype"], p["S"], p["M"], p["mode"], p["hilo"]
    lo_dt = ops.lo_dtype(dt)
    rows = S * M
    G = GUARD_ROWS

    def stream_in(name):
        if name not in p:
            return None
        t = ug.embed(p[name].reshape(rows, C), C, 0, G, G, dt, dev)
        if hilo:
            t.lo = ug.embed(ug.lo_bytes(p[name + "_lo"].reshape(rows, C), dt), C, 0, G, G, lo_dt, dev)
        return t

    a0 = ug.embed(p["a0"].reshape(rows, C), C, 0, G, G, dt, dev)
    res, blk = stream_in("res"), stream_in("blk")
    ws, cs = pack(p)
    nc, L = cs.shape[1], ws.shape[1]
    cbuf = torch.full((S, nc + PAD), float("nan"), dtype=torch.float32)
    cbuf[:, :nc] = cs
    cbuf = cbuf.to(dev)
    consts = cbuf[:, :nc] if S > 1 else cbuf[0, :nc]
    wbuf = torch.full((2 * PAD + S * L,), float("nan"), dtype=dt)
    wbuf[PAD:PAD + S * L] = ws.reshape(-1)
    wbuf = wbuf.to(dev)
    wstream = wbuf[PAD:PAD + S * L].view(S, L) if S > 1 else wbuf[PAD:PAD + L]
    checks = {}

    def out_buf(name, pair):
        _, view, chk = ug.sentinel_out(rows, C, C, dt, dev)
        checks[name] = chk
        if pair and hilo:
            _, lo, chk_lo = ug.sentinel_out(rows, C, C, lo_dt, dev)
            view.lo = lo
            checks[name + "_lo"] = chk_lo
        return view

    kw = dict(streams=S)
    vt = None
    if mode == "ff":
        kw.update(blk=blk, out=out_buf("out", True))
    else:
        kw.update(y_out=out_buf("y", True), out=out_buf("q", False))
        if head_major_qk:
            kw.update(rows_per_b=p["T"], qk_heads=HEADS)
    if mode == "pre":
        B, T = p["B"], p["T"]
        vt = ug.sentinel((S * B + 2, C, ld_vt_of(T)), dt, dev)
        kw.update(out2=out_buf("k", False), out3=vt[1:-1], rows_per_b=T)
    tchain._launch({"q": tchain.MODE_Q, "pre": tchain.MODE_PRE, "ff": tchain.MODE_FF}[mode], a0, res, wstream, consts,
                   p["eps"], **kw)
    torch.cuda.synchronize()
    what = f"tchain {mode} {p['family']} {dt} S {S} M {M} hilo {hilo} head-major {head_major_qk}"
    got = {}
    for name, chk in checks.items():
        t = chk(f"{what}: {name}")
        if name.endswith("_lo"):
            t = ops.lo_float(t)
        got[name] = t.double().view(S, M, C)
    if vt is not None:
        named = torch.zeros(vt.shape, dtype=torch.bool)
        named[1:-1, :, :p["T"]] = True
        ug.assert_untouched(vt, named, f"{what}: V^T (token columns T .. ld_vt, guard samples)")
        got["vt"] = vt.cpu()[1:-1, :, :p["T"]].double().view(S, p["B"], C, p["T"])
    return got


# ---------------------------------------------------------------------------------------------------------------
# fp32 emulation of a correct kernel (torch float32 on the CPU)
def gelu_constants():
    """(KS[3], KV[5]) as the kernel has them: the TC_GELU_KS / TC_GELU_KV lines of csrc/tchain_asm.inc."""
    import uni_renderer_amd
    path = os.path.join(os.path.dirname(os.path.abspath(uni_renderer_amd.__file__)), "csrc", "tchain_asm.inc")
    text = open(path).read()
    out = []
    for name in ("TC_GELU_KS", "TC_GELU_KV"):
        body = re.search(r"#define " + name + r" \{([^}]*)\}", text).group(1)
        out.append([float(x.strip().rstrip("f")) for x in body.split(",")])
    assert len(out[0]) == 3 and len(out[1]) == 5
    return out


def geglu_program_f32(pv, bv, pg, bg):
    """The VALU program of tools/gen_tchain_asm.py::geglu_program, operation by operation in torch float32 (v_rcp_f32 ->
    1 / t, v_exp_f32 -> exp2; separate multiply and add where the program has an FMA) -> 2 value gelu(gate) before packing."""
    ks, kv = gelu_constants()
    c = lambda x: torch.tensor(x, dtype=torch.float32)
    g = pg + bg
    e = g.abs() * c(ks[0])
    t = e * c(ks[1]) + 1.0
    t = 1.0 / t
    e = torch.exp2(-e * e)
    pl = t * c(ks[2]) + c(kv[4])
    pl = pl * t + c(kv[3])
    pl = pl * t + c(kv[2])
    pl = pl * t + c(kv[1])
    pl = pl * t
    pl = -pl * e + 1.0
    pl = g.abs() * pl
    g = g + pl
    return (pv + bv) * g


def emulate(p, order="fwd"):
    """-> {name: (value32 as float64 [S, M, 320] before the storage rounding, hi, lo)} for the outputs of the mode; lo is
    None for q / k / v.  Every GEMM sums its k in 64-wide chunks, ``order`` fwd | rev; accumulators start as the kernel's
    do (residual + bias first; the FF hidden units from 0 with the bias added by the program)."""
    from uni_renderer_amd import ops
    f32 = torch.float32
    dt, S, mode = p["dtype"], p["S"], p["mode"]
    t32 = lambda k, s: p[k][s].to(f32)

    def gemm(acc, a, w):
        ch = list(range(a.shape[1] // 64))
        if order == "rev":
            ch.reverse()
        for c in ch:
            acc = acc + a[:, 64 * c:64 * c + 64] @ w[:, 64 * c:64 * c + 64].T
        return acc

    def stored(v32, pair):
        hi = v32.to(dt)
        lo = ops.lo_float(ops.lo_encode(v32 - hi.float(), dt)).double() if pair else None
        return v32.double(), hi.double(), lo

    res = {k: [] for k in OUTPUTS[mode]}
    for s in range(S):
        acc = torch.zeros(p["M"], C, dtype=f32)
        if "res" in p:
            acc = acc + t32("res", s)
            if "res_lo" in p:
                acc = acc + t32("res_lo", s)
        y = gemm(acc + t32("b0", s), t32("a0", s), t32("w0", s))
        mean = y.sum(-1, keepdim=True) * f32_const(1.0 / C)
        dd = y - mean
        rstd = torch.rsqrt((dd * dd).sum(-1, keepdim=True) * f32_const(1.0 / C) + f32_const(p["eps"]))
        xn = ((dd * rstd) * t32("gamma", s) + t32("beta", s)).to(dt).to(f32)
        if mode != "ff":
            res["y"].append(stored(y, p["hilo"]))
            for name in OUTPUTS[mode][1:]:
                res[name].append(stored(gemm(torch.zeros_like(y), xn, t32("w" + name, s)), False))
            continue
        hc = gemm(torch.zeros(p["M"], 2 * FF, dtype=f32), xn, t32("w1", s))
        b1 = t32("b1", s)
        h2 = geglu_program_f32(hc[:, :FF], b1[:FF], hc[:, FF:], b1[FF:]).to(dt).to(f32)
        y3 = gemm(y + t32("b2", s), h2, t32("w2s", s)).to(dt).to(f32)
        out = gemm(torch.zeros_like(y), y3, t32("wpo", s)) + t32("bpo", s) + t32("blk", s)
        if "blk_lo" in p:
            out = out + t32("blk_lo", s)
        res["out"].append(stored(out, p["hilo"]))
    return {k: tuple(torch.stack([r[i] for r in v]) if v[0][i] is not None else None for i in range(3)) for k, v in res.items()}


def f32_const(x):
    return torch.tensor(x, dtype=torch.float32)


# ---------------------------------------------------------------------------------------------------------------
# checkers over a whole set of outputs
def check_exact_outputs(p, got, head_major_qk=False):
    """Exact family: every output torch.equal to the reference (ug.check_exact names rows and columns), low parts as the
    reference's pair has them (zero)."""
    what = f"{p['mode']} {p['dtype']} S {p['S']} M {p['M']} hilo {p['hilo']}"
    for name in OUTPUTS[p["mode"]]:
        exp = p["ref"][name]
        if name in PAIRS[p["mode"]]:
            hi, lo = expected_pair(p, name)
            ug.check_exact(got[name], hi, f"{what}: {name}")
            if p["hilo"]:
                ug.check_exact(got[name + "_lo"], lo, f"{what}: {name}.lo")
        elif name == "v":
            ug.check_exact(got["vt"], vt_of(p, exp), f"{what}: V^T")
        else:
            ug.check_exact(got[name], head_major(p, exp) if head_major_qk else exp, f"{what}: {name}")


def check_toleranced_outputs(p, got):
    """Toleranced family: every output within its element bound and per-row rel-L2 < TOL (V^T also per (sample, channel)
    row over the tokens); pairs within the pair bound.  -> {name: (worst row rel-L2, worst |err| / bound)}."""
    dt = p["dtype"]
    what = f"{p['mode']} {dt} S {p['S']} M {p['M']} hilo {p['hilo']}"
    figs = {}
    for name in OUTPUTS[p["mode"]]:
        ref, b = p["ref"][name], bounds(p, name)
        if name == "v":
            tok = got["vt"].transpose(2, 3).reshape(ref.shape)
            figs["v"] = ug.check_elem(tok, ref, b["hi"], TOL[dt], f"{what}: v per token")
            figs["vt"] = ug.check_elem(got["vt"], vt_of(p, ref), vt_of(p, b["hi"]), TOL[dt], f"{what}: V^T per channel row")
            continue
        figs[name] = ug.check_elem(got[name], ref, b["hi"], TOL[dt], f"{what}: {name}")
        if name in PAIRS[p["mode"]] and p["hilo"]:
            figs[name + "_pair"] = ug.check_elem(got[name] + got[name + "_lo"], ref, b["pair"], TOL[dt], f"{what}: {name} pair")
    return figs


def standin(p):
    """The rounded reference in the layout ``launch`` returns: what a kernel without any fp32 error would store."""
    got = {}
    for name in OUTPUTS[p["mode"]]:
        if name in PAIRS[p["mode"]]:
            hi, lo = expected_pair(p, name)
            got[name] = hi
            if p["hilo"]:
                got[name + "_lo"] = lo
        elif name == "v":
            got["vt"] = vt_of(p, rnd(p["ref"]["v"], p["dtype"]))
        else:
            got[name] = rnd(p["ref"][name], p["dtype"])
    return got


# ---------------------------------------------------------------------------------------------------------------
# the problems of test_tchain_range_gpu.py (built once and shared; test_tchain_bounds_cpu.py builds every gamma0 one)
_cache = {}


def problem(**spec):
    key = tuple(sorted(spec.items()))
    if key not in _cache:
        _cache[key] = make_problem(spec)
    return _cache[key]


def specs_a(dtype):
    """(a) exact: M = 200 (the last tile has 72 rows: the third wave 8, the fourth none; with S = 2 a ragged tile overhangs
    the other stream's rows), M = 5, M = 129; PRE -- whose rows are whole samples of a multiple of 32 tokens, so that M =
    200 / 5 / 129 are descriptors it refuses -- at (B, T) = (3, 96) (Tpad 128 != T) and (5, 32) padded to 64: sample
    boundaries inside tiles.  hilo and non-hilo runs."""
    out = []
    for mode in ("q", "ff"):
        for S, M, hilo in ((1, 200, True), (2, 200, True), (2, 200, False), (1, 5, True), (1, 129, False)):
            out.append((f"{mode}_S{S}_M{M}_{'hilo' if hilo else 'plain'}", dict(mode=mode, dtype=dtype, S=S, M=M, hilo=hilo)))
    for S, B, T, hilo in ((1, 3, 96, True), (2, 3, 96, False), (2, 5, 32, True), (1, 2, 64, True)):
        out.append((f"pre_S{S}_B{B}_T{T}_{'hilo' if hilo else 'plain'}", dict(mode="pre", dtype=dtype, S=S, B=B, T=T, hilo=hilo)))
    return out


def specs_b(dtype):
    """(b) exact, head-major q / k at (3, 96)."""
    return [("pre_hm", dict(mode="pre", dtype=dtype, S=2, B=3, T=96)), ("q_hm", dict(mode="q", dtype=dtype, S=2, B=3, T=96))]


def specs_c(dtype):
    """(c) gauss: M = 200, S = 2 in the modes without samples, PRE at (3, 96); eps 1e-5; one Q case with eps 1e-6 and rows of
    near-zero variance."""
    g = dict(family="gauss", dtype=dtype, S=2)
    return [("q", dict(g, mode="q", M=200)), ("ff", dict(g, mode="ff", M=200)), ("pre", dict(g, mode="pre", B=3, T=96)),
            ("q_plain", dict(g, mode="q", M=200, hilo=False, seed=1)),
            ("q_flat_eps1e-6", dict(g, mode="q", M=200, eps=1e-6, flat=True))]


def specs_d(dtype):
    """(d) gauss with residuals ~ N(0, 16^2): coarse ulps, the low part carries what the pair bound tests; "ff_po1": one
    entry per Wpo row, so that D_out is one term and the FF out's pair bound resolves its low part."""
    g = dict(family="gauss", dtype=dtype, S=2, M=200, res_std=16.0)
    return [("q_res16", dict(g, mode="q")), ("ff_res16", dict(g, mode="ff")), ("ff_po1_res16", dict(g, mode="ff", po1=True))]


def gamma0_problems(dtype):
    """Builds every exact-family problem of the GPU file (each asserts its exactness conditions) -> their ranges."""
    return {name: problem(**spec)["ranges"] for name, spec in specs_a(dtype) + specs_b(dtype)}
