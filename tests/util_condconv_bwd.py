"""ur_cond_conv3x3_dgrad / ur_cond_conv3x3_wgrad (csrc/condconv_bwd.hip) per ELEMENT: problems with their float64 references and
bound terms, fp32 emulations of a correct kernel, damaged outputs, the independent reader of the ``w_rot`` image and the guarded
launches, shared by test_condconv_bwd_cpu.py and test_condconv_bwd_gpu.py.  Layers, maps and dtypes are util_condconv.py's.

A problem holds the STORED operands as float64 tensors -- x (NCHW; ``x_lay`` is what the kernel is handed: NHWC, or in image mode
the caller's NCHW in its own dtype), dy (NCHW; ``dy_lay`` NHWC) and w4 [Cout, Cin, 3, 3] -- and the float64 references
    dx = conv_transpose2d(dy, w4)    dw = sum over pixels of dy (x) patch(round_dtype(x))    db = sum over pixels of dy.

Exact family ("int"): dy in {-2 .. 2}, x and w in {-1, 0, 1}.  The helper asserts that every sum of absolute values is below
2^24, so fp32 accumulation is exact in ANY order and with ANY split: dx must be torch.equal to the integer result cast to the
storage type, dw and db to the integer result in fp32.

Toleranced family ("gauss"): dy, x ~ N(0, 1) rounded to their dtypes, w ~ N(0, 1 / (9 Cin)) rounded to the compute dtype.
  dgrad: util_condconv.bound's form with K = 9 Cout terms per output:
      A = conv_transpose2d(|dy|, |w|),  fp = (K + 8) 2^-23 A,  |dx - ref| <= u (|ref| + fp) + fp + tiny(dtype)
  wgrad (fp32 outputs, no storage rounding): |dw - ref| <= (P + 8) 2^-23 A + tiny with P = B Ho Wo the number of pixels that
      can contribute and A = sum |dy| |x| (for db: A = sum |dy|); every partial sum of at most P terms is charged 2^-23 per
      term, the "+ 8" covers the cross-wave and cross-split additions' own roundings at the scale of A.
Nothing in a bound comes from what the kernel produces.
"""
import torch
import torch.nn.functional as F

import util_condconv as CCV
from util_igemm import SENTINEL, TINY, U, assert_untouched, embed, rnd, sentinel

CHAIN, EXTRA, IMAGE, MAPS, DTYPES = CCV.CHAIN, CCV.EXTRA, CCV.IMAGE, CCV.MAPS, CCV.DTYPES
LAYERS = CHAIN + EXTRA
TINY32 = 2.0 ** -126
SPLITS = [0, 1, 2, 3, 7]
_cache = {}


def patches(x_nchw, stride, Ho, Wo):
    """[B, C, H, W] -> [3, 3, B, C, Ho, Wo]: the input value under tap (ky, kx) of every output pixel, zero outside the map."""
    xp = F.pad(x_nchw, (1, 1, 1, 1))
    return torch.stack([torch.stack([xp[:, :, ky:ky + (Ho - 1) * stride + 1:stride, kx:kx + (Wo - 1) * stride + 1:stride]
                                     for kx in range(3)]) for ky in range(3)])


def dgrad64(dy_nchw, w4, stride, H, W):
    Ho, Wo = dy_nchw.shape[2:]
    op = (H - ((Ho - 1) * stride + 1), W - ((Wo - 1) * stride + 1))
    return F.conv_transpose2d(dy_nchw, w4, None, stride=stride, padding=1, output_padding=op)


def wgrad64(dy_nchw, x_nchw, stride):
    Ho, Wo = dy_nchw.shape[2:]
    return torch.einsum("bnhw,yxbchw->ncyx", dy_nchw, patches(x_nchw, stride, Ho, Wo))


def problem(cin, cout, stride, H, W, dtype, family="int", B=2, image=False, x_dtype=None, seed=0):
    key = (cin, cout, stride, H, W, dtype, family, B, image, x_dtype, seed)
    if key in _cache:
        return _cache[key]
    x_dtype = x_dtype if image else dtype
    Ho, Wo = CCV.out_hw(H, W, stride)
    g = torch.Generator().manual_seed(104729 * seed + 31 * cin + 17 * cout + 5 * H + W + stride + 1000)
    f64 = torch.float64
    if family == "int":
        dy = torch.randint(-2, 3, (B, cout, Ho, Wo), generator=g).to(f64)
        x = torch.randint(-1, 2, (B, cin, H, W), generator=g).to(f64)
        w4 = torch.randint(-1, 2, (cout, cin, 3, 3), generator=g).to(f64)
    else:
        dy = rnd(torch.randn(B, cout, Ho, Wo, generator=g, dtype=f64), dtype)
        x = rnd(torch.randn(B, cin, H, W, generator=g, dtype=f64), x_dtype)
        w4 = rnd(torch.randn(cout, cin, 3, 3, generator=g, dtype=f64) / (9 * cin) ** 0.5, dtype)
    xr = rnd(x, dtype)  # image mode: the kernel rounds the caller's values to the compute dtype first
    nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous()
    dx, A_dx = nhwc(dgrad64(dy, w4, stride, H, W)), nhwc(dgrad64(dy.abs(), w4.abs(), stride, H, W))
    dw, A_dw = wgrad64(dy, xr, stride), wgrad64(dy.abs(), xr.abs(), stride)
    db, A_db = dy.sum((0, 2, 3)), dy.abs().sum((0, 2, 3))
    P = B * Ho * Wo
    if family == "int":
        assert max(float(A_dx.max()), float(A_dw.max()), float(A_db.max())) < 2 ** 24
        assert torch.equal(dx, dx.round()) and torch.equal(dw, dw.round())
        dx = dx.to(torch.int64).to(dtype).double()
    p = dict(cin=cin, cout=cout, stride=stride, H=H, W=W, Ho=Ho, Wo=Wo, B=B, dtype=dtype, family=family, image=image,
             x_dtype=x_dtype, x=x, xr=xr, x_lay=x if image else nhwc(x), dy=dy, dy_lay=nhwc(dy), w4=w4, dx=dx, A_dx=A_dx,
             fp_dx=(9 * cout + 8) * 2.0 ** -23 * A_dx, dw=dw, A_dw=A_dw, db=db, A_db=A_db, P=P)
    _cache[key] = p
    return p


def what(p):
    return f"{p['cin']}->{p['cout']} s{p['stride']} {p['H']}x{p['W']} B{p['B']} {p['dtype']} {p['family']} image={p['image']}"


def bound_dx(p):
    dt = p["dtype"]
    return U[dt] * (p["dx"].abs() + p["fp_dx"]) + p["fp_dx"] + TINY[dt]


def bound_dw(p):
    return (p["P"] + 8) * 2.0 ** -23 * p["A_dw"] + TINY32


def bound_db(p):
    return (p["P"] + 8) * 2.0 ** -23 * p["A_db"] + TINY32


def over(got, ref, bound):
    """Worst |got - ref| / bound."""
    e = (got - ref).abs()
    return float((e / bound.clamp_min(1e-300)).masked_fill(e == 0, 0.0).max())


# ---- fp32 emulations of a correct kernel: every product exact (16-bit operands), sums in fp32
def _tree(parts):
    while len(parts) > 1:
        parts = [parts[i] + parts[i + 1] if i + 1 < len(parts) else parts[i] for i in range(0, len(parts), 2)]
    return parts[0]


def _sum32(terms, n, order, groups=8):
    """fp32 sum of ``terms(i)``, i < n: sequential, or ``groups`` sequential runs combined as a binary tree."""
    g = 1 if order == "seq" else min(groups, n)
    parts = []
    for k in range(g):
        s = None
        for i in range(n * k // g, n * (k + 1) // g):
            t = terms(i)
            s = t if s is None else s + t
        parts.append(s)
    return _tree(parts)


def emulate_dx(p, order="seq"):
    """-> float64 [B, H, W, Cin]: the K = 9 Cout products summed in fp32 in ``order``, one rounding to the storage type."""
    B, H, W, s, cout = p["B"], p["H"], p["W"], p["stride"], p["cout"]
    w = p["w4"].float()
    # Z: dy zero-inserted and padded so that dx[y][x] = sum over (ky', kx') of Z[y + ky'][x + kx'] * w[2 - ky'][2 - kx']
    Z = torch.zeros(B, cout, H + 2, W + 2)
    Z[:, :, 1:1 + (p["Ho"] - 1) * s + 1:s, 1:1 + (p["Wo"] - 1) * s + 1:s] = p["dy"].float()

    def term(i):
        tap, n = divmod(i, cout)
        ky, kx = divmod(tap, 3)
        return Z[:, n, ky:ky + H, kx:kx + W, None] * w[n, :, 2 - ky, 2 - kx]

    return _sum32(term, 9 * cout, order).to(p["dtype"]).double()


def emulate_dw(p, order="seq"):
    """-> (dw, db) float64: the P pixel terms summed in fp32 in ``order``."""
    Ho, Wo = p["Ho"], p["Wo"]
    pt = patches(p["xr"], p["stride"], Ho, Wo).float().permute(2, 4, 5, 3, 0, 1).reshape(p["P"], p["cin"], 3, 3)
    dyp = p["dy"].float().permute(0, 2, 3, 1).reshape(p["P"], p["cout"])
    dw = _sum32(lambda i: dyp[i, :, None, None, None] * pt[i], p["P"], order)
    db = _sum32(lambda i: dyp[i], p["P"], order)
    return dw.double(), db.double()


# ---- damaged outputs: what the checks have to reject
def _store(dx64_nchw, p):
    return dx64_nchw.permute(0, 2, 3, 1).float().to(p["dtype"]).double()


def _dx_nchw(p, dy=None):
    return dgrad64(p["dy"] if dy is None else dy, p["w4"], p["stride"], p["H"], p["W"])


def damaged_dx_corner_tap(p):
    """Stride 1: pixel (0, 0) of sample 0 without the tap (ky, kx) = (0, 0), i.e. without output pixel (1, 1)."""
    assert p["stride"] == 1
    dx = _dx_nchw(p)
    dx[0, :, 0, 0] -= p["w4"][:, :, 0, 0].T @ p["dy"][0, :, 1, 1]
    return _store(dx, p)


def damaged_dx_neighbour_halo(p):
    """Stride 1: the halo rows of a sample are its neighbours' edge rows (the samples read as one tall map)."""
    assert p["stride"] == 1 and p["B"] >= 2
    B, N, Ho, Wo = p["dy"].shape
    tall = p["dy"].permute(1, 0, 2, 3).reshape(1, N, B * Ho, Wo)
    dx = dgrad64(tall, p["w4"], 1, B * p["H"], p["W"]).reshape(-1, B, p["H"], p["W"]).permute(1, 0, 2, 3)
    return _store(dx, p)


def damaged_dx_parity_swapped(p):
    """Stride 2: the even and odd rows of dx (1-tap and 2-tap parity classes along y) written to each other's place."""
    assert p["stride"] == 2
    dx = _dx_nchw(p)
    He = p["H"] // 2 * 2
    out = dx.clone()
    out[:, :, 0:He:2], out[:, :, 1:He:2] = dx[:, :, 1:He:2], dx[:, :, 0:He:2]
    return _store(out, p)


def damaged_dx_last_odd_column(p):
    """Stride 2, odd W: the last column of dx gathered from dy one column to the left."""
    assert p["stride"] == 2 and p["W"] % 2 == 1
    dx = _dx_nchw(p)
    dx[..., -1] = _dx_nchw(p, F.pad(p["dy"], (1, 0))[..., :-1])[..., -1]
    return _store(dx, p)


def damaged_dw_tail_chunk(p, splits=7):
    """The last of ``splits`` chunks of the pixels (b, oy, ox) never reaches the sums."""
    dy = p["dy"].permute(0, 2, 3, 1).reshape(p["P"], -1).clone()
    dy[p["P"] * (splits - 1) // splits:] = 0
    dy = dy.reshape(p["B"], p["Ho"], p["Wo"], -1).permute(0, 3, 1, 2)
    return wgrad64(dy, p["xr"], p["stride"]).float().double(), dy.sum((0, 2, 3)).float().double()


def damaged_dw_taps_transposed(p):
    return p["dw"].transpose(2, 3).float().double()


# ---- the w_rot image, read back by the formula of include/ur_kernels.h (independent of layers.pack_cond_conv3x3_rot)
def unpack_rot(packed, cin, cout, cc):
    """packed [Cin / 16][Cout / CC][STEPS][64][8] -> (w4 [Cout, Cin, 3, 3] float64, every padding entry is zero)."""
    steps = -(-9 * cc // 32)
    img = packed.double().reshape(cin // 16, cout // cc, steps, 64, 8)
    w4 = torch.zeros(cout, cin, 3, 3, dtype=torch.float64)
    pad_zero = True
    for s in range(steps):
        for lane in range(64):
            for j in range(8):
                k = 32 * s + 8 * (lane // 16) + j
                tap, n = k // cc, k % cc
                v = img[:, :, s, lane, j]  # [block of input channels, chunk of output channels]
                if tap >= 9:
                    pad_zero &= bool((v == 0).all())
                    continue
                for q in range(cout // cc):
                    w4[q * cc + n, lane % 16::16, 2 - tap // 3, 2 - tap % 3] = v[:, q]
    return w4, pad_zero


# ---- guarded launches
GUARD = 64


def _guarded(t64, last, dtype, dev):
    """A contiguous tensor of ``t64``'s shape inside a NaN-filled buffer, two rows of NaN in front of and behind it."""
    return embed(t64.reshape(-1, last), last, 0, 2, 2, dtype, dev).view(t64.shape)


def launch_dgrad(p, dev):
    """ops.cond_conv3x3_dgrad with dy and w_rot inside NaN-filled buffers and dx inside a sentinel buffer that must come back
    untouched outside [B, H, W, Cin].  -> float64 CPU [B, H, W, Cin]."""
    from uni_renderer_amd import ops
    from uni_renderer_amd.layers import pack_cond_conv3x3_rot

    dt, B, H, W, cin, cout = p["dtype"], p["B"], p["H"], p["W"], p["cin"], p["cout"]
    dy = _guarded(p["dy_lay"], cout, dt, dev)
    wp = pack_cond_conv3x3_rot(p["w4"], dt)
    w = _guarded(wp.double(), 8, dt, dev)
    n = B * H * W * cin
    buf = sentinel((n + 2 * GUARD,), dt, dev)
    out = buf[GUARD:GUARD + n].view(B, H, W, cin)
    ops.cond_conv3x3_dgrad(dy, w, in_hw=(H, W), n_in=cin, stride=p["stride"], out=out)
    torch.cuda.synchronize()
    written = torch.zeros(n + 2 * GUARD, dtype=torch.bool)
    written[GUARD:GUARD + n] = True
    assert_untouched(buf, written, what(p) + " dgrad")
    return buf.cpu()[GUARD:GUARD + n].view(B, H, W, cin).double()


def launch_wgrad(p, dev, splits=0, need_dw=True, need_bias=True):
    """ops.cond_conv3x3_wgrad with x and dy inside NaN-filled buffers and dw / db inside fp32 sentinel buffers that must come back
    untouched outside their extent (a result that is not asked for: untouched everywhere).  -> (dw | None, db | None) float64 CPU."""
    from uni_renderer_amd import ops

    dt, cin, cout = p["dtype"], p["cin"], p["cout"]
    x = _guarded(p["x_lay"], p["W"] if p["image"] else cin, p["x_dtype"] if p["image"] else dt, dev)
    dy = _guarded(p["dy_lay"], cout, dt, dev)
    nw = cout * cin * 9
    bw_, bb_ = sentinel((nw + 2 * GUARD,), torch.float32, dev), sentinel((cout + 2 * GUARD,), torch.float32, dev)
    dw, db = ops.cond_conv3x3_wgrad(x, dy, stride=p["stride"], image=p["image"], need_dw=need_dw, need_bias=need_bias, splits=splits,
                                    dw_out=bw_[GUARD:GUARD + nw].view(cout, cin, 3, 3) if need_dw else None,
                                    db_out=bb_[GUARD:GUARD + cout] if need_bias else None)
    torch.cuda.synchronize()
    for buf, n, used in ((bw_.cpu(), nw, need_dw), (bb_.cpu(), cout, need_bias)):
        keep = torch.ones(buf.numel(), dtype=torch.bool)
        if used:
            keep[GUARD:GUARD + n] = False
        assert bool((buf[keep] == SENTINEL).all()), what(p) + f" wgrad splits={splits}: written outside the output"
    return (bw_.cpu()[GUARD:GUARD + nw].view(cout, cin, 3, 3).double() if need_dw else None,
            bb_.cpu()[GUARD:GUARD + cout].double() if need_bias else None)
