"""ur_cond_conv3x3 (csrc/condconv.hip) per ELEMENT: problems with their float64 references and bound terms, the float64
emulation of a correct kernel, damaged outputs, the independent reader of the packed weight image and the guarded launch,
shared by test_condconv_cpu.py and test_condconv_gpu.py.  Checkers and guard buffers are those of util_igemm.py.

A problem holds the STORED operands as float64 tensors -- x (NHWC [B, H, W, Cin], or in image mode the caller's NCHW
[B, Cin, H, W] in its own dtype), w4 [Cout, Cin, 3, 3] and fp32 bias -- and the float64 reference
    ref = act( conv2d(round_dtype(x), w4, padding 1, stride) + bias ).

Exact family ("int"): x in {-2 .. 2}, w in {-1, 0, 1}, bias in {-8 .. 8}, no activation.  |sum| <= 9 * 256 * 2 + 8 < 2^24, so
the fp32 accumulation is exact in ANY order and only the final rounding to the storage type remains: the output must be
torch.equal to the integer result cast to that type.

Toleranced family ("gauss": x ~ N(0, 1) rounded to its dtype, w ~ N(0, 1 / K) rounded to the compute dtype, bias ~ N(0, 1)
fp32, SiLU).  The bound is util_igemm.bounds' with K = 9 Cin:
    A = conv2d(|x|, |w|) + |bias|  >= |pre|,     fp = (K + 8) 2^-23 * 1.1 * A + c_silu(pre)     (1.1 = max |silu'|)
    |y - ref| <= u (|ref| + fp) + fp + tiny(dtype)
-- every term charged 2^-23 (the MFMA's internal alignment is not documented), the epilogue's fp32 roundings inside the
"+ 8", c_silu the error of x / (1 + __expf(-x)) (util_igemm's derivation), u the unit roundoff of the storage type.  Nothing
in it comes from what the kernel produces.
"""
import math

import torch
import torch.nn.functional as F

from util_igemm import L_SILU, TINY, TOL, U, assert_untouched, c_silu, check_elem, check_exact, embed, rnd, sentinel, silu64, silu_f32

# (Cin, Cout, stride): the narrow layers of the default conditioning embedding, then two widths off that chain
CHAIN = [(16, 16, 1), (16, 32, 2), (32, 32, 1), (32, 96, 2), (96, 96, 1), (96, 256, 2)]
EXTRA = [(48, 80, 1), (80, 48, 2)]
IMAGE = [(1, torch.float32), (3, torch.float32), (3, torch.float16), (4, torch.float16)]  # first layer: channels, x dtype
MAPS = [(5, 7), (16, 16), (33, 19), (40, 72)]  # below a tile; one tile; odd, 3 x 2 tiles; 3 x 5 tiles
DTYPES = [torch.float16, torch.bfloat16]
_cache = {}


def out_hw(H, W, stride):
    return (H - 1) // stride + 1, (W - 1) // stride + 1


def conv64(x_nchw, w4, stride):
    return F.conv2d(x_nchw, w4, None, stride=stride, padding=1)


def problem(cin, cout, stride, H, W, dtype, family="int", B=2, image=False, x_dtype=None, seed=0):
    """-> dict (cached): x (float64, NHWC, or NCHW with ``image``), x_dtype, w4, bias, ref / pre / A / fp as NHWC
    [B, Ho, Wo, Cout] float64."""
    key = (cin, cout, stride, H, W, dtype, family, B, image, x_dtype, seed)
    if key in _cache:
        return _cache[key]
    x_dtype = x_dtype if image else dtype
    g = torch.Generator().manual_seed(7919 * seed + 31 * cin + 17 * cout + 5 * H + W + stride)
    f64 = torch.float64
    K = 9 * cin
    if family == "int":
        x = torch.randint(-2, 3, (B, cin, H, W), generator=g).to(f64)
        w4 = torch.randint(-1, 2, (cout, cin, 3, 3), generator=g).to(f64)
        bias = torch.randint(-8, 9, (cout,), generator=g).to(f64)
    else:
        x = rnd(torch.randn(B, cin, H, W, generator=g, dtype=f64), x_dtype)
        w4 = rnd(torch.randn(cout, cin, 3, 3, generator=g, dtype=f64) / math.sqrt(K), dtype)
        bias = torch.randn(cout, generator=g, dtype=f64).float().double()
    xr = rnd(x, dtype)  # image mode: the kernel rounds the caller's values to the compute dtype first
    pre = (conv64(xr, w4, stride) + bias[None, :, None, None]).permute(0, 2, 3, 1).contiguous()
    A = (conv64(xr.abs(), w4.abs(), stride) + bias.abs()[None, :, None, None]).permute(0, 2, 3, 1).contiguous()
    eps = (K + 8) * 2.0 ** -23
    if family == "int":
        assert torch.equal(pre, pre.round()) and float(A.max()) < 2 ** 24
        ref, fp, act = pre.to(torch.int64).to(dtype).double(), eps * A, "none"
    else:
        ref, fp, act = silu64(pre), eps * L_SILU * A + c_silu(pre), "silu"
    p = dict(cin=cin, cout=cout, stride=stride, H=H, W=W, B=B, dtype=dtype, family=family, image=image, x_dtype=x_dtype,
             x=x if image else x.permute(0, 2, 3, 1).contiguous(), x_nchw=x, w4=w4, bias=bias, pre=pre, A=A, fp=fp, ref=ref,
             act=act, K=K)
    _cache[key] = p
    return p


def bound(p):
    """Per-element bound on |out - ref| (util_igemm.bounds' ``hi``)."""
    dt = p["dtype"]
    return U[dt] * (p["ref"].abs() + p["fp"]) + p["fp"] + TINY[dt]


def finish32(pre64, p):
    """The fp32 value a correct kernel holds before it stores, for the exact pre-activation ``pre64``: the exact sum rounded
    to fp32 ONCE, SiLU in fp32 by the kernel's formula.  -> float64."""
    y = pre64.float()
    if p["act"] == "silu":
        y = silu_f32(y)
    return y.double()


def finish(pre64, p):
    """... and what it stores: one rounding to the storage type.  -> float64."""
    return finish32(pre64, p).to(p["dtype"]).double()


def emulate(p):
    return finish(p["pre"], p)


# ---- damaged outputs: what the bound has to reject
def damaged_corner_tap(p):
    """Output pixel (0, 0) of sample 0 without its tap (ky, kx) = (2, 2)."""
    xr = rnd(p["x_nchw"], p["dtype"])
    pre = p["pre"].clone()
    pre[0, 0, 0] -= p["w4"][:, :, 2, 2] @ xr[0, :, 1, 1]
    return finish(pre, p)


def damaged_neighbour_halo(p):
    """Stride 1: the halo row above sample b >= 1 is the last row of sample b - 1 (the samples read as one tall image)."""
    assert p["stride"] == 1 and p["B"] >= 2
    xr = rnd(p["x_nchw"], p["dtype"])
    B, C, H, W = xr.shape
    tall = xr.permute(1, 0, 2, 3).reshape(1, C, B * H, W)
    pre = (conv64(tall, p["w4"], 1) + p["bias"][None, :, None, None]).reshape(-1, B, H, W).permute(1, 2, 3, 0).contiguous()
    return finish(pre, p)


def damaged_last_odd_column(p):
    """Stride 2, odd W: the last output column gathered one input column to the left."""
    assert p["stride"] == 2 and p["W"] % 2 == 1
    xr = rnd(p["x_nchw"], p["dtype"])
    shifted = F.pad(xr, (1, 0))[..., :-1]
    pre = p["pre"].clone()
    pre[:, :, -1] = (conv64(shifted, p["w4"], 2) + p["bias"][None, :, None, None]).permute(0, 2, 3, 1)[:, :, -1]
    return finish(pre, p)


# ---- the packed weight image, read back by the formula of include/ur_kernels.h (independent of layers.pack_cond_conv3x3)
def unpack(packed, cin, cout, cc):
    """packed [Cout / 16][Cp / CC][STEPS][64][8] -> (w4 [Cout, Cp, 3, 3] float64, every padding entry is zero)."""
    cp = -(-cin // cc) * cc
    steps = -(-9 * cc // 32)
    img = packed.double().reshape(cout // 16, cp // cc, steps, 64, 8)
    w4 = torch.zeros(cout, cp, 3, 3, dtype=torch.float64)
    pad_zero = True
    for s in range(steps):
        for lane in range(64):
            for j in range(8):
                k = 32 * s + 8 * (lane // 16) + j
                tap, c = k // cc, k % cc
                v = img[:, :, s, lane, j]  # [block, chunk]
                if tap >= 9:
                    pad_zero &= bool((v == 0).all())
                    continue
                for q in range(cp // cc):
                    w4[lane % 16::16, q * cc + c, tap // 3, tap % 3] = v[:, q]
    pad_zero &= bool((w4[:, cin:] == 0).all())
    return w4, pad_zero


# ---- guarded launch
GUARD = 64  # sentinel elements in front of and behind the output


def launch(p, dev, bgr=False):
    """ops.cond_conv3x3 on problem ``p`` with x, the packed weights and the bias inside NaN-filled buffers and the output
    inside a sentinel buffer that must come back untouched outside [B, Ho, Wo, Cout].  -> float64 CPU [B, Ho, Wo, Cout]."""
    from uni_renderer_amd import ops
    from uni_renderer_amd.layers import pack_cond_conv3x3

    dt, B, H, W, cin, cout, s = p["dtype"], p["B"], p["H"], p["W"], p["cin"], p["cout"], p["stride"]
    Ho, Wo = out_hw(H, W, s)
    if p["image"]:
        x = embed(p["x"].reshape(-1, W), W, 0, 2, 2, p["x_dtype"], dev).view(B, cin, H, W)
    else:
        x = embed(p["x"].reshape(-1, cin), cin, 0, W + 2, W + 2, dt, dev).view(B, H, W, cin)
    wp = pack_cond_conv3x3(p["w4"], dt, s, image=p["image"], bgr=bgr)  # bgr: the image is launched as it lies
    w = embed(wp.double().reshape(-1, 8), 8, 0, 16, 16, dt, dev)
    bias = embed(p["bias"][None], cout, 0, 1, 1, torch.float32, dev)[0]
    n = B * Ho * Wo * cout
    buf = sentinel((n + 2 * GUARD,), dt, dev)
    out = buf[GUARD:GUARD + n].view(B, Ho, Wo, cout)
    ops.cond_conv3x3(x, w.reshape(wp.shape), bias, n_out=cout, stride=s, act=ops.ACT_SILU if p["act"] == "silu" else ops.ACT_NONE,
                     dtype=dt, image=p["image"], out=out)
    torch.cuda.synchronize()
    written = torch.zeros(n + 2 * GUARD, dtype=torch.bool)
    written[GUARD:GUARD + n] = True
    what = f"{cin}->{cout} s{s} {H}x{W} B{B} {dt} image={p['image']}"
    assert_untouched(buf, written, what)
    return buf.cpu()[GUARD:GUARD + n].view(B, Ho, Wo, cout).double(), what
