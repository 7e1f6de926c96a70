"""Normalisation kernels on realistic value ranges, against a float64 reference, checked per (sample, group) / per row.

The other suites feed nearly zero-mean data (|mean| / std <= 0.25) and check one rel-L2 over the whole tensor.  Real
activations carry group-wide offsets (|mean| / std of 30 .. 1000 on the residual stream), outlier channels, constant
groups and ~1M-value groups at the VAE's sizes; and one bad (sample, group) out of 96 moves a whole-tensor rel-L2 by only
~1e-3.  Every case here builds x = m + s * N(0, 1) per (sample, group) with m / s in RATIOS (both signs), rounds it to the
storage dtype (plus a low part for the (hi, lo) inputs), evaluates F.group_norm / F.layer_norm (and autograd) in float64
on exactly those values, and asserts on every group:

  * rel-L2 < TOL (the suites' per-tensor tolerances, now per group), and
  * max |got - ref| <= 2 u M_g, u = 2^-11 (fp16) / 2^-8 (bf16) the unit roundoff of the output, M_g = max over the group of
    |xhat * gamma| + |beta| (>= |y| before the activation).  Derivation: the one storage rounding of y costs <= u |y|
    (SiLU's slope is <= 1.1); the fp32 arithmetic of a correct kernel -- statistics summed over <= 2^20 values, then
    (x - mean) * rstd * gamma + beta -- adds O(1e-5) M_g.  Their sum stays below 2 u M_g.  A statistic with a relative
    error d moves y by ~d |xhat gamma|, so the bound catches any d >~ u.
"""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

TOL = {torch.float16: 2e-3, torch.bfloat16: 1.2e-2}       # tests/test_ops_gpu.py
TOL_BWD = {torch.float16: 3e-3, torch.bfloat16: 2e-2}     # tests/test_backward_gpu.py (dx: 2x)
U = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}
DTYPES = [torch.float16, torch.bfloat16]
RATIOS = [0, 3, 30, 100, 300, 1000]
EPS = [1e-5, 1e-6]  # UNet, VAE


def _offset_data(B, rows, C, groups, ratio, dtype, seed, outliers=None):
    """float64 [B, rows, C]: per (sample, group) a mean of +-ratio * s and spread s in [0.5, 2] (|x| <= ~2.1e3);
    outliers: 'group' = one channel of every group scaled x30 .. x100, 'sparse' = 1 % of the channels."""
    g = torch.Generator().manual_seed(seed)
    cpg = C // groups
    s = 0.5 + 1.5 * torch.rand(B, 1, groups, 1, generator=g, dtype=torch.float64)
    sign = torch.where(torch.rand(B, 1, groups, 1, generator=g) < 0.5, -1.0, 1.0).to(torch.float64)
    z = torch.randn(B, rows, groups, cpg, generator=g, dtype=torch.float64)
    if outliers == "group":
        z[..., torch.randint(cpg, (1,), generator=g).item()] *= 30 + 70 * torch.rand(1, generator=g).item()
    elif outliers == "sparse":
        zc = z.view(B, rows, C)
        for c in torch.randperm(C, generator=g)[:max(1, C // 100)].tolist():
            zc[..., c] *= 30 + 70 * torch.rand(1, generator=g).item()
    return (sign * ratio * s + s * z).view(B, rows, C)


def _to_dev(v, dtype, dev, hilo=False):
    """-> (device tensor [B, rows, 1, C] carrying .lo when hilo, float64 value the kernel sees)."""
    from uni_renderer_amd import ops
    hi = v.to(dtype).contiguous()
    seen = hi.double()
    x = hi.unsqueeze(2).to(dev)
    if hilo:
        lo = ops.lo_encode((v - seen).float(), dtype)
        seen = seen + ops.lo_float(lo).double()
        x.lo = lo.unsqueeze(2).to(dev)
    return x, seen


def _affine(C, S, seed):
    g = torch.Generator().manual_seed(seed)
    return (1.0 + 0.5 * torch.randn(S * C, generator=g)), 0.5 * torch.randn(S * C, generator=g)


def _gn_ref(x, gam, beta, groups, eps, silu):
    """float64 GroupNorm of [B, rows, C] -> (y, M) with M = |xhat * gamma| + |beta| elementwise."""
    B, rows, C = x.shape
    xg = x.permute(0, 2, 1)
    y = F.group_norm(xg, groups, gam.double(), beta.double(), eps).permute(0, 2, 1)
    xhat = F.group_norm(xg, groups, None, None, eps).permute(0, 2, 1)
    M = (xhat * gam.double()).abs() + beta.double().abs()
    return (F.silu(y) if silu else y), M


def _per_group(t, groups):
    B, rows, C = t.shape
    return t.reshape(B, rows, groups, C // groups).permute(0, 2, 1, 3).reshape(B, groups, -1)


def _check(got, ref, M, groups, dtype, tol, what, extra=None):
    """Per-(sample, group) rel-L2 < tol and max-abs <= 2 u M_g (+ extra, [B, groups], where a case needs one)."""
    got = got.detach().double().cpu().reshape(ref.shape)
    e, r = _per_group(got - ref, groups), _per_group(ref, groups)
    rel = e.norm(dim=-1) / r.norm(dim=-1).clamp_min(1e-30)
    bound = 2 * U[dtype] * _per_group(M, groups).amax(-1)
    if extra is not None:
        bound = bound + extra
    worst = (e.abs().amax(-1) / bound).max().item()
    assert torch.isfinite(got).all(), what
    assert rel.max().item() < tol and worst <= 1.0, (
        f"{what}: worst group rel-L2 {rel.max().item():.3e} (tol {tol:.1e}), worst max-abs / bound {worst:.3g}, "
        f"groups over: {int((rel >= tol).sum())} / {rel.numel()}")


# (name, c0, c1, rows, streams, ops.groupnorm keywords): every forward GroupNorm path
PATHS = [
    ("stats_apply", 320, 0, 4096, 1, dict(fused=False)),
    ("one_launch", 640, 0, 256, 1, dict(fused=True, resident=False)),
    ("resident", 1280, 0, 256, 1, dict(fused=True, resident=True)),
    ("two_src_apply", 640, 320, 256, 1, dict(fused=False)),        # cpg 30: group 21 straddles the x0 | x1 boundary
    ("two_src_one_launch", 640, 320, 256, 1, dict(fused=True)),
    ("streams_apply", 320, 0, 1024, 2, dict(fused=False)),
    ("streams_resident", 640, 640, 64, 2, dict(fused=True, resident=True)),
    ("hilo_apply", 320, 0, 4096, 1, dict(fused=False, hilo=True)),
    ("hilo_one_launch", 640, 0, 256, 1, dict(fused=True, resident=False, hilo=True)),
    ("hilo_resident", 1280, 0, 256, 1, dict(fused=True, resident=True, hilo=True)),
    ("tiny_apply", 64, 0, 64, 1, dict(fused=False)),                 # cpg 2 < 8: the narrow-group statistics
    ("tiny_one_launch", 64, 0, 64, 1, dict(fused=True)),
]


def _run_gn(path, dtype, ratio, eps, silu, dev, outliers=None, data=None):
    from uni_renderer_amd import ops
    name, c0, c1, rows, S, kw = path
    kw = dict(kw)
    hilo = kw.pop("hilo", False)
    B, C, groups = 2 * S, c0 + c1, 32
    v = _offset_data(B, rows, C, groups, ratio, dtype, seed=ratio + 7 * c0 + rows, outliers=outliers) if data is None else data
    x0, s0 = _to_dev(v[..., :c0], dtype, dev, hilo)
    x1, s1 = _to_dev(v[..., c0:], dtype, dev) if c1 else (None, None)
    seen = torch.cat([s0, s1], -1) if c1 else s0
    gam, bet = _affine(C, S, seed=3)
    y = ops.groupnorm(x0, gam.to(dev), bet.to(dev), eps, x1=x1, groups=groups, silu=silu, streams=S, **kw)
    for s_ in range(S):
        sl = slice(s_ * 2, s_ * 2 + 2)
        ref, M = _gn_ref(seen[sl], gam[s_ * C:(s_ + 1) * C], bet[s_ * C:(s_ + 1) * C], groups, eps, silu)
        _check(y[sl], ref, M, groups, dtype, TOL[dtype], f"{name} ratio {ratio} eps {eps} stream {s_}")
    return y, seen


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("path", PATHS, ids=[p[0] for p in PATHS])
@pytest.mark.parametrize("ratio", RATIOS)
@pytest.mark.parametrize("eps", EPS)
def test_groupnorm_offsets(dev, dtype, path, ratio, eps):
    """Group-wide offsets m / s in 0 .. 1000 on every forward path (SiLU on: the UNet's norm -> SiLU)."""
    _run_gn(path, dtype, ratio, eps, True, dev)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("path", PATHS, ids=[p[0] for p in PATHS])
@pytest.mark.parametrize("outliers", ["group", "sparse"])
@pytest.mark.parametrize("ratio", [3, 100])
def test_groupnorm_outlier_channels(dev, dtype, path, outliers, ratio):
    """One channel per group, or 1 % of the channels, scaled x30 .. x100 on top of an offset."""
    _run_gn(path, dtype, ratio, 1e-6, False, dev, outliers=outliers)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("path", PATHS, ids=[p[0] for p in PATHS])
@pytest.mark.parametrize("silu", [False, True])
@pytest.mark.parametrize("eps", EPS)
def test_groupnorm_constant_and_zero_groups(dev, dtype, path, silu, eps):
    """Groups whose values are all equal (some large: 300.25, -1000, 0.1) or all zero: var = 0, so the output is beta (SiLU
    of beta) exactly up to its rounding -- an inexact mean times rsqrt(eps) (316 / 1000) would show at once."""
    from uni_renderer_amd import ops
    name, c0, c1, rows, S, kw = path
    B, C, groups = 2 * S, c0 + c1, 32
    v = _offset_data(B, rows, C, groups, 30, dtype, seed=11)
    vg = v.view(B, rows, groups, C // groups)
    for i, (b, g, val) in enumerate([(0, 0, 300.25), (0, 5, 0.0), (1, 31, -1000.0), (B - 1, 21, 0.1), (B - 1, 7, 0.0)]):
        vg[b, :, g, :] = val
    y, seen = _run_gn(path, dtype, 30, eps, silu, dev, data=v)
    gam, bet = _affine(C, S, seed=3)
    for b, g in [(0, 0), (0, 5), (1, 31), (B - 1, 21), (B - 1, 7)]:
        s_ = b // 2
        beta = bet[s_ * C:(s_ + 1) * C].view(groups, -1)[g].double()
        want = (F.silu(beta) if silu else beta).to(dtype).double()
        got = y[b].double().cpu().view(rows, groups, -1)[:, g]
        assert torch.isfinite(got).all()
        if silu:  # the kernel's SiLU is fp32 arithmetic: one output ulp
            assert ((got - want).abs() <= 2 * U[dtype] * want.abs() + 1e-7).all(), (name, b, g)
        else:
            assert torch.equal(got, want.expand_as(got)), (name, b, g, (got - want).abs().max().item())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("hw", [256, 512])
@pytest.mark.parametrize("ratio", [30, 300])
def test_groupnorm_vae_size_groups(dev, dtype, hw, ratio):
    """VAE-size strips: 128 channels at 256x256 / 512x512, 32 groups -> 0.26M / 1.05M values per group, 32 statistics
    chunks, the VAE's eps."""
    from uni_renderer_amd import ops
    B, C, groups, rows = 1, 128, 32, hw * hw
    v = _offset_data(B, rows, C, groups, ratio, dtype, seed=hw + ratio)
    x, seen = _to_dev(v, dtype, dev)
    gam, bet = _affine(C, 1, seed=3)
    y = ops.groupnorm(x, gam.to(dev), bet.to(dev), 1e-6, groups=groups, silu=True, nstat=32)
    ref, M = _gn_ref(seen, gam, bet, groups, 1e-6, True)
    _check(y, ref, M, groups, dtype, TOL[dtype], f"vae {hw}x{hw} ratio {ratio}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cfg", [(16, 640, 1280, 4, 2), (8, 1280, 1280, 8, 2), (16, 320, 640, 2, 1)])
@pytest.mark.parametrize("ratio", [0, 30, 300])
def test_conv_groupnorm_splitk_second_pass_offsets(dev, dtype, cfg, ratio, monkeypatch):
    """ur_igemm_splitk_gn with a large common bias per group (the conv output carries group-wide offsets), against float64
    group_norm of the conv output the unfused path stores.  The fused pass rounds its own fp32 sum of the same value, which
    may land one storage ulp away from the unfused one: that is <= ulp(max |h_g|) * rstd_g * max |gamma| more in max-abs."""
    from uni_renderer_amd import ops
    from uni_renderer_amd.layers import pack_conv3x3
    monkeypatch.setattr(ops, "SPLITK_GN", True)
    L, Ci, Co, sk, S = cfg
    B, groups, eps = 2, 32, 1e-5
    g = torch.Generator().manual_seed(ratio + Ci)
    x = torch.randn(S * B, L, L, Ci, generator=g).to(dtype).to(dev)
    wt = [torch.randn(Co, Ci, 3, 3, generator=g) * (9 * Ci) ** -0.5 for _ in range(S)]
    w = torch.stack([pack_conv3x3(t.to(dev), dtype) for t in wt])
    sign = torch.where(torch.rand(S, groups, 1, generator=g) < 0.5, -1.0, 1.0)
    bias = (sign * ratio * (1 + 0.01 * torch.randn(S, groups, Co // groups, generator=g))).view(S, Co).to(dev)
    gam = torch.stack([1.0 + 0.3 * torch.randn(Co, generator=g) for _ in range(S)]).to(dev)
    bet = torch.stack([0.2 * torch.randn(Co, generator=g) for _ in range(S)]).to(dev)
    if S == 1:
        w, bias, gam, bet = w[0], bias[0], gam[0], bet[0]
    kw = dict(streams=S, splitk=sk, tile=2)
    fused = ops.conv3x3(x, w, bias, gn=(gam, bet, eps, groups, True), **kw)
    h = ops.conv3x3(x, w, bias, **kw)
    for s_ in range(S):
        sl = slice(s_ * B, (s_ + 1) * B)
        hs = h[sl].double().cpu().reshape(B, L * L, Co)
        gs, bs = (gam[s_], bet[s_]) if S > 1 else (gam, bet)
        ref, M = _gn_ref(hs, gs.cpu(), bs.cpu(), groups, eps, True)
        hg = _per_group(hs, groups)
        ulp = torch.finfo(dtype).eps * 2.0 ** torch.floor(torch.log2(hg.abs().amax(-1)))
        rstd = (hg.var(-1, unbiased=False) + eps).rsqrt()
        _check(fused[sl], ref, M, groups, dtype, TOL[dtype], f"splitk_gn {cfg} ratio {ratio}",
               extra=1.1 * ulp * rstd * gs.abs().max().item())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(2, 32, 32, 640), (2, 16, 16, 960), (1, 64, 64, 320), (2, 8, 8, 64)])
@pytest.mark.parametrize("route", ["one_launch", "chunked", "chunked_fwd_stats"])
@pytest.mark.parametrize("ratio", RATIOS)
def test_groupnorm_backward_offsets(dev, dtype, shape, route, ratio, monkeypatch):
    """dx, dgamma, dbeta of GroupNorm + SiLU against float64 autograd: the one-launch backward (maps <= 1024 pixels), the
    chunked four-launch path recomputing the statistics, and the chunked path fed the forward's own partials."""
    from uni_renderer_amd import backward as bw
    from uni_renderer_amd import ops
    B, H, W, C = shape
    groups, eps = 32, 1e-5
    if route == "one_launch" and H * W > bw.GN_BWD_FUSED_MAX_ROWS:
        route = "chunked"  # the 64x64 map only has the chunked backward
    if route != "one_launch":
        monkeypatch.setattr(bw, "GN_BWD_FUSED_MAX_ROWS", 0)
    v = _offset_data(B, H * W, C, groups, ratio, dtype, seed=ratio + C)
    x, seen = _to_dev(v, dtype, dev)
    x = x.view(B, H, W, C)
    g = torch.Generator().manual_seed(5)
    dy = torch.randn(B, H, W, C, generator=g).to(dtype).to(dev)
    gam, bet = _affine(C, 1, seed=3)
    gam, bet = gam.to(dev), bet.to(dev)
    stats = None
    if route == "chunked_fwd_stats":
        _, stats = ops.groupnorm(x, gam, bet, eps, groups=groups, silu=True, fused=False, return_stats=True)
    dx, dg, db = bw.groupnorm_backward(x, dy, gam, bet, eps, groups=groups, silu=True, stats=stats)
    xr = seen.view(B, H, W, C).permute(0, 3, 1, 2).contiguous().requires_grad_()
    gr, br = gam.cpu().double().requires_grad_(), bet.cpu().double().requires_grad_()
    y = F.silu(F.group_norm(xr, groups, gr, br, eps))
    (y * dy.double().cpu().permute(0, 3, 1, 2)).sum().backward()
    rdx = xr.grad.permute(0, 2, 3, 1).reshape(B, H * W, C)
    e = _per_group(dx.double().cpu().reshape(B, H * W, C) - rdx, groups)
    rel = e.norm(dim=-1) / _per_group(rdx, groups).norm(dim=-1)
    assert rel.max().item() < 2 * TOL_BWD[dtype], f"dx {route} ratio {ratio}: worst group rel-L2 {rel.max().item():.3e}"
    for got, ref, nm in ((dg, gr.grad, "dgamma"), (db, br.grad, "dbeta")):
        eg = (got.double().cpu() - ref).view(groups, -1)
        relg = eg.norm(dim=-1) / ref.view(groups, -1).norm(dim=-1)
        assert relg.max().item() < TOL_BWD[dtype], f"{nm} {route} ratio {ratio}: worst group rel-L2 {relg.max().item():.3e}"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", [320, 640, 1280, 768])  # the three five-vector kernels and the generic one
@pytest.mark.parametrize("ratio", RATIOS)
@pytest.mark.parametrize("hilo", [False, True])
def test_layernorm_offsets(dev, dtype, C, ratio, hilo):
    """LayerNorm forward (exact two-pass variance) with a per-row offset, checked per row."""
    from uni_renderer_amd import ops
    rows = 333
    v = _offset_data(1, rows, C, 1, 0, dtype, seed=C + ratio)[0]
    g = torch.Generator().manual_seed(ratio)
    v = v + ratio * (0.5 + 1.5 * torch.rand(rows, 1, generator=g, dtype=torch.float64)) * torch.where(
        torch.rand(rows, 1, generator=g) < 0.5, -1.0, 1.0).double()
    x, seen = _to_dev(v.unsqueeze(1), dtype, dev, hilo)  # [rows, 1, 1, C]: one "group" per row in _check
    gam, bet = _affine(C, 1, seed=3)
    y = ops.layernorm(x, gam.to(dev), bet.to(dev), 1e-5)
    seen = seen.view(rows, 1, C)
    ref = F.layer_norm(seen, (C,), gam.double(), bet.double(), 1e-5)
    M = (F.layer_norm(seen, (C,), None, None, 1e-5) * gam.double()).abs() + bet.double().abs()
    _check(y, ref, M, 1, dtype, TOL[dtype], f"layernorm C {C} ratio {ratio}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", [320, 640, 1280])
@pytest.mark.parametrize("ratio", RATIOS)
def test_layernorm_backward_offsets(dev, dtype, C, ratio):
    from uni_renderer_amd import backward as bw
    rows = 222
    v = _offset_data(1, rows, C, 1, 0, dtype, seed=C + ratio)[0]
    v = v + ratio * torch.where(torch.arange(rows) % 2 == 0, 1.0, -1.0).double()[:, None]
    x, seen = _to_dev(v, dtype, dev)
    x = x.view(rows, C)
    dy = torch.randn(rows, C, generator=torch.Generator().manual_seed(2)).to(dtype).to(dev)
    gam, _ = _affine(C, 1, seed=3)
    dx, dg, db = bw.layernorm_backward(x, dy, gam.to(dev), 1e-5)
    xr = seen.view(rows, C).clone().requires_grad_()
    gr, br = gam.double().requires_grad_(), torch.zeros(C, dtype=torch.float64, requires_grad=True)
    (F.layer_norm(xr, (C,), gr, br, 1e-5) * dy.double().cpu()).sum().backward()
    rel = (dx.double().cpu() - xr.grad).norm(dim=-1) / xr.grad.norm(dim=-1)
    assert rel.max().item() < 2 * TOL_BWD[dtype], f"dx ratio {ratio}: worst row rel-L2 {rel.max().item():.3e}"
    for got, ref, nm in ((dg, gr.grad, "dgamma"), (db, br.grad, "dbeta")):
        r = ((got.double().cpu() - ref).norm() / ref.norm()).item()
        assert r < TOL_BWD[dtype], f"{nm} ratio {ratio}: rel-L2 {r:.3e}"
