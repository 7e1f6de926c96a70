"""ur_igemm (csrc/igemm.hip, igemm_epi.h, igemm_pp.hip) per ELEMENT against float64: problems, references with their
bound terms, fp32 emulations, checkers and the guard / sentinel buffers shared by test_igemm_range_gpu.py (the kernels)
and test_igemm_bounds_cpu.py (the proof that the reference is the operation, that the exact family is exact, that the
bounds fit correct arithmetic with room and that the checkers reject the errors they are for).

A problem is built by ``make_problem(spec)`` from a small dict (DEFAULTS below).  It holds the STORED operands as float64
tensors (fp16 / bf16-rounded activations and weights, fp32 bias), one leading dimension S = streams (the z batch of a
grouped launch), the weight matrix in the K order the kernel is told to walk (tap-outer, ``cblock``-outer, 1x1 tail
appended: layers.pack_conv3x3, the packer of the product), and the float64 reference of

    out[m][n] = out_scale * ( act( sum_k X[m][k] W[n][k] + bias[n] + rowadd[m / rows_per_b][n] ) + res[m][n] + res_lo[m][n] )

evaluated from an explicit im2col (``im2col``: stride 1 | 2, nearest-2x in front, pad 1 | 0, two sources, taps in
k = tap * Cin + c order) that test_igemm_bounds_cpu.py holds against F.conv2d in float64 for every gather mode.

Exact family ("int")
  x in [-3, 3], res in [-8, 8], rowadd and bias in [-4, 4] are integers, w is +-1 with density 1/8 (1/32 for K > 4000)
  and 0 elsewhere, out_scale is 1 or 0.5.  Every product and every partial sum, in ANY order and under any split of K,
  is an integer below 2^24 and therefore exact in fp32; the result is an integer or half-integer that fp16 AND bf16
  hold exactly while |value before out_scale| <= 256 (n / 2 with |n| <= 256 has at most 8 significant bits).
  ``make_problem`` asserts that condition on the float64 reference and fails loudly (no re-draw).  The kernel output must
  then be torch.equal to the reference: no tolerance, on every tile, with or without split-K.  With the (hi, lo) pair the
  expected low part is exactly zero; the fp16 problems carry res_lo = +-0.25 (e5m2-exact; |v| <= 256 plus a quarter fits
  fp16's 11 bits, halved by out_scale still does), bf16 res_lo = 0.

Toleranced families ("gauss": N(0, 1) operands, w ~ N(0, 1/K), the data of test_ops_gpu.py; "act": x = SiLU(N(0, 1)),
w ~ N(0.02, 1/K): post-activation statistics, sums that do not cancel, A ~ |y|; pre-activation magnitude <= 30 asserted)
  Notation: u = 2^-11 (fp16) / 2^-8 (bf16); s = sum_k x w; A[m, n] = sum_k |x w| + |bias| + |rowadd| (>= |pre|, the
  pre-activation value); f = act(pre); R = |res| + |res_lo|; v the reference.
  * fp32 accumulation.  Products of two fp16 / bf16 numbers are exact in fp32.  A sum of K terms in any order, with the
    bias and rowadd added in two more operations, has |error| <= (K + 1) 2^-24 sum|terms| to first order whatever the
    order (Higham, Accuracy and Stability, 4.2).  The MFMA's internal alignment / rounding of its 4- or 8-term dot
    products is not documented, so every term is charged 2^-23 instead of 2^-24: delta_pre <= (K + 8) 2^-23 A.  The "+ 8"
    covers the epilogue's own fp32 roundings (bias, rowadd, the activation's result, res, res_lo, out_scale), each
    relative to a partial result that A' below dominates.
  * activation.  |act(pre + d) - act(pre)| <= L |d| with L = 1 (none), 1.1 (SiLU: max |silu'| = 1.0998) and, for GEGLU
    out = value * gelu(gate), delta <= |gelu(gate)| d_value + 1.13 |value| d_gate (max |gelu'| = 1.1290).  So
        A' = |out_scale| (L A + R)            resp.  |out_scale| (A_value |gelu(gate)| + 1.13 |value| A_gate).
  * c_act, the error of the activation's own fp32 formula (csrc/ur_common.h):
      silu_f(x) = x / (1 + __expf(-x)).  __expf(-x) = v_exp_f32(-x log2 e): the rounded argument costs the exponential
        |x| 2^-24 relative, v_exp_f32 one ulp (2^-23); charged (|x| + 2) 2^-23, it moves silu by
        |x| s (1 - s) (|x| + 2) 2^-23 (s = sigmoid(x)); the add and the division are charged 4 ulp: 2^-22 |silu(x)|.
      gelu_erf_f(x) = 0.5 x + 0.5 |x| erf_abs, erf by Abramowitz-Stegun 7.1.26: |erf error| <= 1.5e-7 absolute, plus
        2^-22 for its fp32 evaluation (v_rcp and v_exp at one ulp each, the rounded exponent argument -- whose effect
        a e^-a <= 0.37 bounds -- and five FMAs on values <= 1.5), and 2^-23 |x| for the last two operations:
        c_gelu(x) = |x| (0.5 (1.5e-7 + 2^-22) + 2^-23).  For gates in [-12, -6] the two halves cancel to ~1e-9 .. 1e-32
        and c_gelu IS the error; GEGLU's c_act = |value| c_gelu(gate).
  * stored output: u |y| <= u (|v| + everything above), plus half the subnormal spacing of the format (fp16: 2^-25).
        |y - v| <= u |v| + (K + 8) 2^-23 A' + |out_scale| c_act            (``bounds(p)["hi"]``; the u term also covers
                                                                             u times the fp32 part, a second-order term)
  * (hi, lo) pair: lo = lo_from_f(y - hi) rounds a remainder |r| <= u |y| to 3 significant bits (e5m2, fp16 streams) or
    8 (bf16): |hi + lo - v| <= 2^-3 u |v| / 2^-8 u |v| + the same fp32 part.  e5m2 shares fp16's exponent range, so a
    remainder below 2^-14 (|y| < 1/8) is rounded on the subnormal grid of spacing 2^-16: + 2^-17 absolute for fp16
    streams (a property of the format, not a tolerance: the N(0, 1) outputs of these tests do reach |y| < 1/8).
  * per-row rel-L2 < TOL of test_ops_gpu.py (2e-3 / 1.2e-2) for the stored output, and for the pair.
  What is NOT derived: the factor 2 on the summation term (MFMA internals), the 4-ulp division and the 2^-22 evaluation
  allowance of the erf polynomial.  test_igemm_bounds_cpu.py therefore holds fp32 emulations of a correct kernel
  (``emulate``: torch float32, 64-wide chunks forwards, backwards, and 3 / 7 split-K slabs summed in slab order, the
  ur_common.h formulas, ops.lo_encode) to HALF of the fp32 part -- the value BEFORE the storage rounding, because the
  storage rounding itself is exact arithmetic: round-to-nearest reaches u |v| (0.5 ulp just above a power of two), so no
  factor 2 exists for the u term -- and the rounded results to the whole bound.
  Worst GPU figures (MI355X, all REP tiles; row rel-L2 / |err| / bound), as printed by test_g_toleranced:
      fp16  SiLU 2.6e-4 / 0.90   GEGLU 3.0e-4 / 0.85   hilo: hi 2.3e-4 / 0.77, pair 1.2e-5 / 0.15   K = 5760 conv 2.8e-4 / 0.24
      bf16  SiLU 2.0e-3 / 0.98   GEGLU 2.4e-3 / 0.97   hilo: hi 1.9e-3 / 0.96, pair 3.0e-6 / 0.05   K = 5760 conv 2.2e-3 / 0.71
  identical with and without split-K and, to the digits shown, on every tile: the u |v| term (a rounding of nearly half an
  ulp just above a power of two) is what the stored outputs use; with it taken off (``fp_part_used``) no output needs
  more than 0.001 of the fp32 part (GEGLU; 0.000 everywhere else), and the CPU emulations use at most 0.008 of it.

Guards
  ``embed`` puts an operand inside a larger NaN-filled buffer (columns off .. off + c of rows of ld elements, whole
  guard rows before and after -- for an image: lines of W + 2 pixels) and returns the view the descriptor names: a gather
  that reads pixel -1 of the buffer, the channel behind the last, or a row past M turns the output into NaN instead of
  a plausible number.  ``sentinel_out`` allocates an output with guard rows and guard columns filled with the bit pattern
  of -1234 (0x5B for e5m2 bytes; ``sentinel`` for other shapes, e.g. V^T) and its checker (``assert_untouched``) requires
  every element outside the region the descriptor names to hold it still, bit for bit.
"""
import math

import torch

U = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}
TOL = {torch.float16: 2e-3, torch.bfloat16: 1.2e-2}            # tests/test_ops_gpu.py, here per row
LO_REL = {torch.float16: 2.0 ** -3, torch.bfloat16: 2.0 ** -8}  # significant bits of a low part: e5m2 / bf16
TINY = {torch.float16: 2.0 ** -25, torch.bfloat16: 2.0 ** -134}     # half the subnormal spacing of the storage type
TINY_LO = {torch.float16: 2.0 ** -17, torch.bfloat16: 2.0 ** -134}  # ... of the low part's format (e5m2: 2^-16 / 2)
DTYPES = [torch.float16, torch.bfloat16]
L_SILU, L_GELU = 1.1, 1.13
SENTINEL = -1234.0
SENTINEL_LO = 0x5B

PP_TILES = list(range(49, 56))
ALL_TILES = [t for t in range(1, 47) if t != 39] + PP_TILES + list(range(56, 62))  # the list of tests/test_ops_gpu.py
REP = [3, 2, 9, 11, 13, 17, 26, 31, 44, 61, 49, 54]  # one per loader, MFMA shape and BN; 49 / 54 when built (make PP=1)

DEFAULTS = dict(
    mode="gemm", family="int", dtype=torch.float16, seed=0, streams=1,
    M=0, N=0, c0=0, c1=0,                                  # gemm: M rows per stream; K = c0 + c1
    B=0, H=0, W=0, stride=1, ups=False, pad=1, cblock=0, ct0=0, ct1=0,  # conv: B samples per stream, H x W input
    bias=True, rowadd=False, rows_per_b=0,                 # rows_per_b: gemm only (conv: Hout * Wout)
    res=False, res_lo=False, out_scale=1.0, act="none",    # act: none | silu | geglu (N packed columns -> N / 2 outputs)
    gate_shift=0.0,                                        # geglu: bias of every 7th gate column moved by this
)


def rnd(x, dtype):
    """float64 -> storage type -> float64 (round to nearest even, gradual underflow)."""
    return x.to(dtype).to(torch.float64)


def roundup(a, b):
    return (a + b - 1) // b * b


def out_hw(H, W, stride=1, ups=False, pad=1):
    if ups:
        return 2 * H, 2 * W
    if pad == 0:  # F.pad(x, (0, 1, 0, 1)) + conv(stride 2, padding 0): the VAE encoder's Downsample2D
        return (H + 1 - 3) // stride + 1, (W + 1 - 3) // stride + 1
    return (H + 2 - 3) // stride + 1, (W + 2 - 3) // stride + 1


def im2col(x, stride=1, ups=False, pad=1):
    """x [B, H, W, C] -> [B * Hout * Wout, 9, C]: row (b, oy, ox), tap = ky * 3 + kx reads pixel
    (oy * stride - pad + ky, ox * stride - pad + kx) of the (nearest-2x upsampled, if ``ups``) image, zero outside it."""
    B, H, W, C = x.shape
    Ho, Wo = out_hw(H, W, stride, ups, pad)
    Hu, Wu = (2 * H, 2 * W) if ups else (H, W)
    cols = torch.zeros(B, Ho, Wo, 9, C, dtype=x.dtype)
    for ky in range(3):
        for kx in range(3):
            for oy in range(Ho):
                iy = oy * stride - pad + ky
                if not 0 <= iy < Hu:
                    continue
                for ox in range(Wo):
                    ix = ox * stride - pad + kx
                    if 0 <= ix < Wu:
                        cols[:, oy, ox, ky * 3 + kx] = x[:, iy // 2 if ups else iy, ix // 2 if ups else ix]
    return cols.view(B * Ho * Wo, 9, C)


def silu64(x):
    return x * torch.sigmoid(x)


def gelu64(x):
    return 0.5 * x * (1.0 + torch.erf(x * 0.7071067811865476))


def c_silu(x):
    s = torch.sigmoid(x)
    return x.abs() * s * (1 - s) * (x.abs() + 2) * 2.0 ** -23 + 2.0 ** -22 * silu64(x).abs()


def c_gelu(x):
    return x.abs() * (0.5 * (1.5e-7 + 2.0 ** -22) + 2.0 ** -23)


def geglu_perm(n_half):
    from uni_renderer_amd.layers import geglu_perm as gp
    return gp(n_half, "cpu")


def _lo_pair(v, dtype):
    """fp64 values -> (hi, lo) float64 of the (hi, lo) pair that stores them (ops.lo_encode)."""
    from uni_renderer_amd import ops
    hi = v.to(dtype)
    lo = ops.lo_float(ops.lo_encode((v - hi.double()).float(), dtype))
    return hi.double(), lo.double()


def make_problem(spec):
    """-> dict: the spec's entries plus
      x0, x1 [S, R, c] (R = M, or B * H * W input pixels), t0, t1 [S, M, ct] (1x1 tail sources), w [S, N, K] in the
      kernel's K order, bias [S, N], rowadd [S, nb, N], res, res_lo [S, M, n_out]  (None when absent)   -- stored values
      ref [S, M, n_out], pre (pre-activation, [S, M, N]), A (same shape as pre), fp (the fp32 part of the bound), K, M,
      n_out, rows_per_b, conv = (B, H, W, Hout, Wout)."""
    from uni_renderer_amd.layers import pack_conv3x3
    p = dict(DEFAULTS)
    unknown = set(spec) - set(p)
    assert not unknown, unknown
    p.update(spec)
    dt, fam, S, N = p["dtype"], p["family"], p["streams"], p["N"]
    conv = p["mode"] == "conv"
    C = p["c0"] + p["c1"]
    ct = p["ct0"] + p["ct1"]
    if conv:
        Ho, Wo = out_hw(p["H"], p["W"], p["stride"], p["ups"], p["pad"])
        M, R, K = p["B"] * Ho * Wo, p["B"] * p["H"] * p["W"], 9 * C + ct
        p["rows_per_b"], p["conv"] = Ho * Wo, (p["B"], p["H"], p["W"], Ho, Wo)
    else:
        M, R, K = p["M"], p["M"], C
        p["conv"] = None
    geglu = p["act"] == "geglu"
    n_out = N // 2 if geglu else N
    p.update(M=M, K=K, n_out=n_out)
    g = torch.Generator().manual_seed(1000003 * p["seed"] + 7 * M + 13 * N + K)
    f64 = torch.float64

    def ints(lo, hi, *shape):
        return torch.randint(lo, hi + 1, shape, generator=g).to(f64)

    def normal(*shape):
        return torch.randn(*shape, generator=g, dtype=f64)

    if fam == "int":
        assert p["act"] == "none" and p["out_scale"] in (1.0, 0.5)
        dens = 1 / 32 if K > 4000 else 1 / 8
        xs = lambda *s: ints(-3, 3, *s)
        ws = lambda *s: torch.where(torch.rand(*s, generator=g) < dens, 1.0, 0.0).to(f64) * (2 * ints(0, 1, *s) - 1)
        bs = lambda *s: ints(-4, 4, *s)
        rs = lambda *s: ints(-4, 4, *s)
    else:
        assert fam in ("gauss", "act"), fam
        xs = (lambda *s: rnd(normal(*s), dt)) if fam == "gauss" else (lambda *s: rnd(silu64(normal(*s)), dt))
        mean = 0.0 if fam == "gauss" else 0.02
        ws = lambda *s: rnd(mean + normal(*s) / math.sqrt(K), dt)
        bs = lambda *s: normal(*s).float().double()
        rs = lambda *s: rnd(normal(*s), dt)
    x0 = xs(S, R, p["c0"])
    x1 = xs(S, R, p["c1"]) if p["c1"] else None
    t0 = xs(S, M, p["ct0"]) if p["ct0"] else None
    t1 = xs(S, M, p["ct1"]) if p["ct1"] else None
    if conv:
        w4 = ws(S, N, C, 3, 3)                                                                   # OIHW, stored values
        wt = ws(S, N, ct) if ct else None
        wref = torch.stack([pack_conv3x3(w4[s], f64) for s in range(S)])                         # tap-outer: the reference's order
        wk = torch.stack([pack_conv3x3(w4[s], f64, cblock=p["cblock"]) for s in range(S)])       # what the kernel walks
        if ct:
            wref, wk = torch.cat([wref, wt], -1), torch.cat([wk, wt], -1)
        p["w4"], p["wt"] = w4, wt
    else:
        wref = wk = ws(S, N, K)
    bias = bs(S, N) if p["bias"] else None
    if geglu and p["gate_shift"]:  # packed column q is a gate when q % 8 >= 4
        q = torch.arange(N)
        bias[:, ((q % 8) >= 4) & ((q // 8) % 7 == 3)] += p["gate_shift"]
        bias = bias.float().double()
    nb = -(-M // p["rows_per_b"]) if p["rowadd"] else 0
    rowadd = rs(S, nb, N) if p["rowadd"] else None
    res = res_lo = None
    if p["res"]:
        if fam == "int":
            res = ints(-8, 8, S, M, n_out)
            if p["res_lo"]:
                res_lo = (0.25 * (2 * ints(0, 1, S, M, n_out) - 1)) if dt == torch.float16 else torch.zeros(S, M, n_out, dtype=f64)
        elif p["res_lo"]:
            res, res_lo = _lo_pair(normal(S, M, n_out) * 2 + 0.3, dt)
        else:
            res = rnd(normal(S, M, n_out), dt)
    # ---- float64 reference over the stored values
    xc = x0 if x1 is None else torch.cat([x0, x1], -1)
    pre, A = torch.empty(S, M, N, dtype=f64), torch.empty(S, M, N, dtype=f64)
    for s in range(S):
        if conv:
            cols = im2col(xc[s].view(p["B"], p["H"], p["W"], C), p["stride"], p["ups"], p["pad"]).reshape(M, 9 * C)
            if ct:
                cols = torch.cat([cols, t0[s]] + ([t1[s]] if t1 is not None else []), -1)
        else:
            cols = xc[s]
        pre[s], A[s] = cols @ wref[s].T, cols.abs() @ wref[s].abs().T
        if bias is not None:
            pre[s] += bias[s]
            A[s] += bias[s].abs()
        if rowadd is not None:
            ra = rowadd[s][torch.arange(M) // p["rows_per_b"]]
            pre[s] += ra
            A[s] += ra.abs()
    sc = abs(p["out_scale"])
    eps = (K + 8) * 2.0 ** -23
    if geglu:
        assert res is None
        perm = geglu_perm(n_out)  # packed column q holds logical column perm[q] (value j | gate n_out + j)
        lg, la = torch.empty_like(pre), torch.empty_like(A)
        lg[..., perm], la[..., perm] = pre, A
        val, gate, Av, Ag = lg[..., :n_out], lg[..., n_out:], la[..., :n_out], la[..., n_out:]
        f = val * gelu64(gate)
        fp = sc * (eps * (Av * gelu64(gate).abs() + L_GELU * val.abs() * Ag) + val.abs() * c_gelu(gate))
        p["gate"] = gate
    elif p["act"] == "silu":
        f = silu64(pre)
        fp = sc * (eps * L_SILU * A + c_silu(pre))
    else:
        assert p["act"] == "none", p["act"]
        f, fp = pre, sc * eps * A
    before_scale = f if res is None else f + res + (res_lo if res_lo is not None else 0.0)
    if res is not None:
        fp = fp + sc * eps * (res.abs() + (res_lo.abs() if res_lo is not None else 0.0))
    ref = before_scale * p["out_scale"]
    if fam == "int":
        worst = float(before_scale.abs().max())
        assert worst <= 256.0, f"exact family: max |value before out_scale| = {worst} > 256 ({spec}): not exact in bf16"
        assert torch.equal(rnd(ref, dt), ref), f"exact family: the reference is not representable in {dt} ({spec})"
    elif fam == "act":
        assert float(pre.abs().max()) <= 30.0, f"act family: |pre-activation| reaches {float(pre.abs().max())} > 30"
    p.update(x0=x0, x1=x1, t0=t0, t1=t1, w=wk, wref=wref, bias=bias, rowadd=rowadd, res=res, res_lo=res_lo, ref=ref,
             pre=pre, A=A, fp=fp)
    return p


def bounds(p):
    """-> dict(hi = bound on |out - ref|, pair = bound on |out + out_lo - ref|, fp = their fp32 part)."""
    dt, v, fp = p["dtype"], p["ref"].abs(), p["fp"]
    return dict(hi=U[dt] * (v + fp) + fp + TINY[dt], pair=LO_REL[dt] * U[dt] * (v + fp) + fp + TINY_LO[dt], fp=fp)


# ---------------------------------------------------------------------------------------------------------------
# fp32 emulation of a correct kernel (torch float32 on the CPU)
def silu_f32(x):
    return x / (1.0 + torch.exp(-x))


def gelu_erf_f32(x):
    """csrc/ur_common.h gelu_erf_f, operation by operation in float32."""
    z = x.abs() * 0.70710678118654752
    t = 1.0 / (0.3275911 * z + 1.0)
    pl = 1.061405429 * t + -1.453152027
    pl = pl * t + 1.421413741
    pl = pl * t + -0.284496736
    pl = pl * t + 0.254829592
    e = torch.exp2(-1.44269504088896341 * z * z)
    erf_abs = (-pl * t) * e + 1.0
    return 0.5 * x + 0.5 * x.abs() * erf_abs


def emulate(p, order="fwd", slabs=1):
    """-> (y32 [S, M, n_out] fp32 value before the storage rounding, hi, lo as float64; lo is None without res_lo).
    K is summed in 64-wide chunks: ``order`` fwd | rev inside a slab, ``slabs`` slices of ceil(chunks / slabs) chunks each
    (the kernel's split), slab sums added in slab order; then the epilogue of csrc/igemm_epi.h in float32."""
    from uni_renderer_amd import ops
    f32 = torch.float32
    S, M, N, K, dt = p["streams"], p["M"], p["N"], p["K"], p["dtype"]
    xc = p["x0"] if p["x1"] is None else torch.cat([p["x0"], p["x1"]], -1)
    out = []
    for s in range(S):
        if p["conv"] is not None:
            B, H, W, _, _ = p["conv"]
            cols = im2col(xc[s].view(B, H, W, -1), p["stride"], p["ups"], p["pad"]).reshape(M, -1)
            if p["t0"] is not None:
                cols = torch.cat([cols, p["t0"][s]] + ([p["t1"][s]] if p["t1"] is not None else []), -1)
        else:
            cols = xc[s]
        cols, w = cols.to(f32), p["wref"][s].to(f32)
        nchunk = K // 64
        per = -(-nchunk // slabs)
        acc = torch.zeros(M, N, dtype=f32)
        for z in range(slabs):
            ch = list(range(z * per, min(nchunk, (z + 1) * per)))
            if order == "rev":
                ch.reverse()
            part = torch.zeros(M, N, dtype=f32)
            for c in ch:
                part = part + cols[:, c * 64:(c + 1) * 64] @ w[:, c * 64:(c + 1) * 64].T
            acc = acc + part
        if p["bias"] is not None:
            acc = acc + p["bias"][s].to(f32)
        if p["rowadd"] is not None:
            acc = acc + p["rowadd"][s][torch.arange(M) // p["rows_per_b"]].to(f32)
        if p["act"] == "geglu":
            q = torch.arange(p["n_out"])
            vcol = (q // 4) * 8 + q % 4
            acc = acc[:, vcol] * gelu_erf_f32(acc[:, vcol + 4])
        elif p["act"] == "silu":
            acc = silu_f32(acc)
        if p["res"] is not None:
            acc = acc + p["res"][s].to(f32)
            if p["res_lo"] is not None:
                acc = acc + p["res_lo"][s].to(f32)
        out.append(acc * torch.tensor(p["out_scale"], dtype=f32))
    y32 = torch.stack(out)
    hi = y32.to(dt)
    lo = ops.lo_float(ops.lo_encode(y32 - hi.float(), dt)).double() if p["res_lo"] is not None else None
    return y32.double(), hi.double(), lo


# ---------------------------------------------------------------------------------------------------------------
# checkers
def check_exact(got, exp, what):
    """torch.equal, with the rows and columns of the mismatches in the message."""
    assert got.shape == exp.shape, f"{what}: shape {tuple(got.shape)} vs {tuple(exp.shape)}"
    bad = (got != exp) | torch.isnan(got)
    if bad.any():
        idx = bad.nonzero()
        rows, cols = sorted(set(idx[:, -2].tolist())), sorted(set(idx[:, -1].tolist()))
        first = [(tuple(i.tolist()), float(got[tuple(i)]), float(exp[tuple(i)])) for i in idx[:6]]
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ ({int(torch.isnan(got).sum())} NaN); "
                             f"{len(rows)} rows {rows[:12]}{'...' if len(rows) > 12 else ''}, {len(cols)} columns "
                             f"{cols[:12]}{'...' if len(cols) > 12 else ''}; first (index, got, expected): {first}")


def check_elem(got, ref, bound, tol, what, frac=1.0, rel=True):
    """finite; |got - ref| <= frac * bound element by element; per-row rel-L2 < tol.  -> (worst row rel-L2, worst |err| / bound)."""
    assert got.shape == ref.shape, f"{what}: shape {tuple(got.shape)} vs {tuple(ref.shape)}"
    assert torch.isfinite(got).all(), f"{what}: {int((~torch.isfinite(got)).sum())} non-finite outputs"
    e = (got - ref).abs()
    ratio = (e / bound.clamp_min(1e-300)).masked_fill(e == 0, 0.0)
    over = ratio > frac
    rel_w = float((e.norm(dim=-1) / ref.norm(dim=-1).clamp_min(1e-300)).max()) if rel else 0.0
    if over.any() or not rel_w < tol:
        idx = over.nonzero()
        first = [(tuple(i.tolist()), float(got[tuple(i)]), float(ref[tuple(i)]), float(bound[tuple(i)])) for i in idx[:4]]
        raise AssertionError(f"{what}: worst |err| / bound {float(ratio.max()):.3g} (allowed {frac:g}), {int(over.sum())} of "
                             f"{over.numel()} elements over in {int(over.any(-1).sum())} rows; worst row rel-L2 {rel_w:.3e} "
                             f"(allowed {tol:.2e}); first (index, got, ref, bound): {first}")
    return rel_w, float(ratio.max())


def fp_part_used(got, p):
    """Largest share of the fp32 part of the bound an output needs once the storage rounding u |v| is taken off (0: the
    rounding term alone explains every error)."""
    dt = p["dtype"]
    e = (got - p["ref"]).abs() - U[dt] * p["ref"].abs() - TINY[dt]
    return float((e.clamp_min(0) / p["fp"].clamp_min(1e-300)).max())


def old_rel_l2(a, b):
    """conftest.rel_l2 on float64 stand-ins: the whole-tensor figure tests/test_ops_gpu.py asserts."""
    return float((a - b).norm() / b.norm().clamp_min(1e-20))


# ---------------------------------------------------------------------------------------------------------------
# guards
def _nan_like(dtype):
    return 0x7F if dtype == torch.uint8 else float("nan")  # 0x7F: the e5m2 byte of a NaN


def embed(t, ld, off, rows_before, rows_after, dtype, dev):
    """t [rows, c] (float64 values; uint8 bytes for e5m2 low parts) -> the [rows, c] view at columns off .. off + c of
    rows rows_before .. of a [rows_before + rows + rows_after, ld] buffer of ``dtype`` on ``dev`` that holds NaN everywhere
    else.  The view keeps the buffer alive; its stride(0) is ld."""
    rows, c = t.shape
    assert ld >= off + c
    buf = torch.full((rows_before + rows + rows_after, ld), _nan_like(dtype), dtype=dtype)
    buf[rows_before:rows_before + rows, off:off + c] = t.to(dtype)
    return buf.to(dev)[rows_before:rows_before + rows, off:off + c]


def lo_bytes(lo, dtype):
    """float64 low parts -> their storage (e5m2 bytes for fp16 streams, bf16)."""
    from uni_renderer_amd import ops
    return ops.lo_encode(lo.float(), dtype)


def sentinel(shape, dtype, dev):
    """Output buffer filled with the sentinel: -1234 rounded to ``dtype``, or the byte 0x5B for e5m2 low parts."""
    return torch.full(tuple(shape), SENTINEL_LO if dtype == torch.uint8 else SENTINEL, dtype=dtype, device=dev)


def assert_untouched(buf, written, what):
    """Every element of ``buf`` (any device) outside the boolean mask ``written`` still holds the sentinel, bit for bit."""
    b = buf.detach().cpu()
    bits = b if b.dtype == torch.uint8 else b.view(torch.int16)
    s = sentinel((1,), b.dtype, "cpu")
    sbits = int((s if s.dtype == torch.uint8 else s.view(torch.int16))[0])
    bad = (bits != sbits) & ~written
    if bad.any():
        idx = bad.nonzero()
        raise AssertionError(f"{what}: {int(bad.sum())} elements outside the region the descriptor names were overwritten; "
                             f"first (index): {[tuple(i.tolist()) for i in idx[:8]]}")


def region2d(shape, r0, rows, cols):
    m = torch.zeros(tuple(shape), dtype=torch.bool)
    m[r0:r0 + rows, :cols] = True
    return m


GUARD_ROWS = 8  # rows of sentinel in front of and behind every output (8 rows keep any ldc 16-byte aligned)


def sentinel_out(rows, ldc, n_store, dtype, dev):
    """An output of ``rows`` rows of ``ldc`` elements with GUARD_ROWS sentinel rows in front and behind, columns
    n_store .. ldc being guard columns.  -> (buffer, the [rows, ldc] view the descriptor names, check(what) that asserts
    everything outside [rows][n_store] is untouched and returns the named region as a CPU tensor)."""
    buf = sentinel((rows + 2 * GUARD_ROWS, ldc), dtype, dev)

    def check(what):
        assert_untouched(buf, region2d(buf.shape, GUARD_ROWS, rows, n_store), what)
        return buf.cpu()[GUARD_ROWS:GUARD_ROWS + rows, :n_store]

    return buf, buf[GUARD_ROWS:GUARD_ROWS + rows], check


def launch(p, dev, tile, splitk=1, hilo=False, n_store=0, ldc=None, guard=True):
    """Run problem ``p`` through ops.igemm with every operand embedded in NaN (``guard``) and the outputs in sentinel
    buffers; asserts that nothing outside [S * M][n_store] was written and returns (out, out_lo) as float64 CPU tensors
    [S, M, n_store] (out_lo None without ``hilo``)."""
    from uni_renderer_amd import ops
    dt, S, M, N, K = p["dtype"], p["streams"], p["M"], p["N"], p["K"]
    n_out = p["n_out"]
    ns = n_store or n_out
    ldc = ldc if ldc is not None else (roundup(ns, 8) + 8 if guard else ns)
    conv = p["conv"]
    gl = (conv[2] + 2) if conv is not None else 3  # whole guard lines of W + 2 pixels around the image

    def emb(t, pad_c, off, rows, dtype=dt):
        """[S, R, c] -> one guarded matrix of S * R rows; returns (view, per-stream element stride)."""
        if t is None:
            return None, 0
        s_, r, c = t.shape
        flat = t.reshape(s_ * r, c)
        if not guard:
            return flat.to(dtype).to(dev).contiguous(), r * c
        v = embed(flat, roundup(c, 8) + pad_c, off, rows, rows, dtype, dev)
        return v, r * v.stride(0)

    x0, zx = emb(p["x0"], 24, 8, gl)
    x1, zx1 = emb(p["x1"], 8, 8, gl)
    t0, zt0 = emb(p["t0"], 16, 8, gl)
    t1, zt1 = emb(p["t1"], 8, 0, gl)
    w, zw = emb(p["w"], 16, 8, 2)
    bias, zbias = emb(p["bias"][:, None, :] if p["bias"] is not None else None, 8, 4, 1, torch.float32)
    rowadd, zrow = emb(p["rowadd"], 16, 8, 1)
    res, zres = emb(p["res"], 8, 0, 2)
    res_lo = None
    if p["res_lo"] is not None:
        ld_t = lo_bytes(p["res_lo"], dt)
        res_lo, _ = emb(ld_t, 8, 0, 2, ld_t.dtype)
        assert res_lo.stride(0) == res.stride(0)
    rows = S * M
    _, out, check_out = sentinel_out(rows, ldc, ns, dt, dev)
    _, out_lo, check_lo = sentinel_out(rows, ldc, ns, ops.lo_dtype(dt), dev) if hilo else (None, None, None)
    kw = {}
    if conv is not None:
        kw = dict(taps=9, conv=conv, stride=p["stride"], ups=int(p["ups"]), pad=p["pad"], cblock=p["cblock"])
        if t0 is not None:
            kw.update(t0=t0, t1=t1, ldt0=t0.stride(0), ldt1=(t1.stride(0) if t1 is not None else 0), zt0=zt0, zt1=zt1,
                      ct0=p["ct0"], ct1=p["ct1"])
    if S > 1:
        kw.update(zbatch=S, zx=zx, zx1=zx1, zw=zw, zout=M * ldc, zbias=zbias, zrow=zrow, zres=zres)
    ops.igemm(x0=x0, x1=x1, w=w, out=out, M=M, N=N, K=K, c0=p["c0"], c1=p["c1"], ldx0=x0.stride(0),
              ldx1=(x1.stride(0) if x1 is not None else 0), ldw=w.stride(0), ldc=ldc, bias=bias,
              rowadd=rowadd, rows_per_b=p["rows_per_b"], res=res, ldres=(res.stride(0) if res is not None else 0),
              n_store=n_store, act={"none": ops.ACT_NONE, "silu": ops.ACT_SILU, "geglu": ops.ACT_GEGLU}[p["act"]],
              out_scale=p["out_scale"], tile=tile, splitk=splitk, res_lo=res_lo, out_lo=out_lo, **kw)
    torch.cuda.synchronize()
    what = f"tile {tile} splitk {splitk} {p['mode']} M {M} N {N} K {K} n_store {ns} ldc {ldc}"
    got = check_out(what + " out").double().view(S, M, ns)
    lo = ops.lo_float(check_lo(what + " out_lo")).double().view(S, M, ns) if hilo else None
    return got, lo


# ---------------------------------------------------------------------------------------------------------------
# the problems of test_igemm_range_gpu.py (built once per dtype and shared; test_igemm_bounds_cpu.py builds every "int"
# one to show that the exactness condition holds)
_cache = {}


def problem(**spec):
    key = tuple(sorted(spec.items()))
    if key not in _cache:
        _cache[key] = make_problem(spec)
    return _cache[key]


EPI = dict(bias=True, rowadd=True, res=True, out_scale=0.5)


def specs_a(dtype):
    """(a) every tile: M = 300 -> 5 / 3 / 2 row tiles (last: 44 rows), N = 328 -> >= 2 column tiles for every BN, the last
    ragged and no multiple of 16 (masked epilogue); 9 x 11 images, B = 3: samples end at m = 99, 198 inside tiles."""
    g = dict(mode="gemm", dtype=dtype, M=300, N=328, c0=128, c1=64, rows_per_b=100, **EPI)
    c = dict(mode="conv", dtype=dtype, B=3, H=9, W=11, N=328, c0=128, c1=64, **EPI)
    return ([("gemm_128|64", g)] + [(f"gemm_K{k}", dict(g, c0=k, c1=0)) for k in (64, 128, 192, 320)]
            + [("gemm_M5", dict(g, M=5, rows_per_b=2)), ("conv_s1", c), ("conv_s2_pad1", dict(c, stride=2)),
               ("conv_s2_pad0", dict(c, stride=2, pad=0)), ("conv_ups", dict(c, H=5, W=6, ups=True))])


def specs_b(dtype):
    """(b) split-K: (name, spec, split-K values).  K = 704: 11 chunks (uneven slices, one chunk per slice, the clamp at 16);
    the conv walks 2 channel blocks of 320 and a 64 | 64 tail (K = 5888 = 92 chunks: 7 starts slices inside a block, 46
    puts a slice's start inside the tail); M = 2970 reaches the second pass without the pipelined loads."""
    h = dict(res_lo=True)
    return [("gemm_K704", dict(mode="gemm", dtype=dtype, M=300, N=328, c0=704, rows_per_b=100, **EPI, **h), (2, 3, 4, 11, 16)),
            ("conv_cblock_tail", dict(mode="conv", dtype=dtype, B=3, H=9, W=11, N=72, c0=640, cblock=320, ct0=64, ct1=64, **EPI, **h),
             (1, 4, 7, 46)),
            ("conv_M2970", dict(mode="conv", dtype=dtype, B=30, H=9, W=11, N=328, c0=64, **EPI, **h), (3,))]


N_STORE = [(77, 128, 128), (150, 192, 200), (4, 64, 64), (28, 28, 28)]  # (N, n_store, ldc)


def specs_c(dtype):
    return [(f"N{n}_store{ns}_ldc{ldc}", dict(mode="gemm", dtype=dtype, M=300, N=n, c0=128, rows_per_b=100, **EPI), ns, ldc)
            for n, ns, ldc in N_STORE]


def spec_e_grouped(dtype):
    return dict(mode="conv", dtype=dtype, B=3, H=9, W=11, N=328, c0=64, streams=2, **EPI)


def _exact(before_scale, ref, dtype, what):
    worst = float(before_scale.abs().max())
    assert worst <= 256.0, f"{what}: max |value before out_scale| = {worst} > 256"
    assert torch.equal(rnd(ref, dtype), ref), f"{what}: the reference is not representable in {dtype}"
    return ref


def case_vt(dtype, S):
    """(d) q | k | v projection with the value columns leaving transposed: B = 3 samples of 77 tokens (sample boundaries
    inside every tile), C = 176: N = 528, vt_n0 = 352; the S streams share x (zx = 0).
    -> dict(p, qk [S, 231, 352] = out_scale * (x w^T + b)[:, :352], vt [S, 3, 176, 77] = (x w^T + b)[:, 352:] per sample, transposed)."""
    B, T, C = 3, 77, 176
    p = problem(mode="gemm", dtype=dtype, M=B * T, N=3 * C, c0=128, streams=S, bias=True, out_scale=0.5, seed=4)
    full = torch.stack([p["x0"][0] @ p["w"][s].T + p["bias"][s] for s in range(S)])
    _exact(full, full * 0.5, dtype, "case_vt")
    return dict(p=p, B=B, T=T, C=C, qk=full[..., :2 * C] * 0.5, vt=full[..., 2 * C:].reshape(S, B, T, C).transpose(2, 3).contiguous())


def case_qk(dtype):
    """(e) the VAE attention's scores: x0 and w alias ONE [B, T, 2C] matrix (q | k), ldx0 = ldw = 2C > K = C."""
    B, T, C = 3, 100, 128
    p = problem(mode="gemm", dtype=dtype, M=B * T, N=B * T, c0=C, bias=False, seed=5)  # x0 = q rows, w = k rows (sparse +-1)
    q, k = p["x0"][0].view(B, T, C), p["w"][0].view(B, T, C)
    s = torch.einsum("btc,bsc->bts", q, k)
    return dict(B=B, T=T, C=C, qk=torch.cat([q, k], -1), ref=_exact(s, s * 0.5, dtype, "case_qk"))


def case_zx_div(dtype):
    """(e) ops.vt_proj's descriptor: x0 = the stream's weight (shared by its B samples: zx_div = B), w = the sample's tokens."""
    S, B, T, Co, Ci = 2, 3, 77, 176, 128
    p = problem(mode="gemm", dtype=dtype, M=S * B * T, N=S * Co, c0=Ci, bias=False, seed=6)  # x0 = tokens, w = weights
    x, wv = p["x0"][0].view(S * B, T, Ci), p["w"][0].view(S, Co, Ci)
    ref = torch.stack([wv[z // B] @ x[z].T for z in range(S * B)])
    return dict(S=S, B=B, T=T, Co=Co, Ci=Ci, x=x, wv=wv, ref=_exact(ref, ref, dtype, "case_zx_div"))


def case_exchange(dtype):
    """(e) two streams whose residual is the OTHER stream's tensor: res points at the second half, zres < 0."""
    p = problem(mode="gemm", dtype=dtype, M=300, N=328, c0=128, streams=2, bias=True, res=True, seed=7)
    before = p["pre"] + p["res"].flip(0)
    return dict(p=p, ref=_exact(before, before, dtype, "case_exchange"))


def int_problems(dtype):
    """Builds every exact-family problem of the GPU file (each asserts its exactness condition)."""
    n = 0
    for _, s in specs_a(dtype):
        n += problem(**s) is not None
    for _, s, _ in specs_b(dtype):
        n += problem(**s) is not None
    for _, s, _, _ in specs_c(dtype):
        n += problem(**s) is not None
    n += problem(**spec_e_grouped(dtype)) is not None
    for c in (case_vt(dtype, 1), case_vt(dtype, 2), case_qk(dtype), case_zx_div(dtype), case_exchange(dtype)):
        n += c is not None
    return n


def specs_g(dtype, family):
    """(g) toleranced: (name, spec, hilo, split-K values)."""
    b = dict(mode="gemm", dtype=dtype, family=family, M=300, rows_per_b=100, bias=True, rowadd=True)
    return [("silu", dict(b, N=328, c0=192, act="silu", out_scale=0.5), False, (1,)),
            ("geglu", dict(b, N=336, c0=128, act="geglu", gate_shift=-9.0), False, (1,)),
            ("hilo", dict(b, N=328, c0=704, res=True, res_lo=True), True, (1, 4))]


def spec_g_long_conv(dtype):
    return dict(mode="conv", dtype=dtype, family="act", B=3, H=9, W=11, N=72, c0=640, cblock=320, act="silu", bias=True)


def spec_f(dtype):
    return dict(mode="conv", dtype=dtype, family="gauss", B=3, H=9, W=11, N=328, c0=128, c1=64, **EPI)
