"""FreeU (arXiv 2309.11497) on the MI355X: the ``ur_freeu`` kernel per element against float64, and the three executors
(module forward, grouped step, hoisted render loop) with FreeU on against the CPU oracle running the reference's
in-place semantics (util_freeu.py)."""
import functools
import json
import math

import pytest
import torch

import util_freeu as F
from conftest import rel_l2
from util_models import O, build_product_from_oracle, product_step

pytestmark = pytest.mark.gpu

KERNEL_SHAPES = [(8, 8, 1280, 1280), (16, 16, 1280, 640), (32, 32, 320, 320), (2, 2, 128, 128), (5, 7, 128, 64),
                 (12, 20, 64, 64), (64, 64, 64, 64)]  # (H, W, Ch, Cs)
BS = [(1.2, 0.9), (1.4, 0.2), (1.0, 1.7)]
U_ = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}  # one storage rounding
TINY = {torch.float16: 2.0 ** -25, torch.bfloat16: 2.0 ** -134}  # half the spacing of the subnormals


def _nhwc(t, dev):
    return t.permute(0, 2, 3, 1).contiguous().to(dev)


def _nchw64(t):
    return t.detach().cpu().permute(0, 3, 1, 2).double()


def _inputs(H, W, Ch, Cs, dtype, case, seed=0):
    """NCHW tensors already rounded to ``dtype``.  case "zero": zero-mean randn * 3; "offset": per-channel offsets of +-40 and
    one channel x50 (the ranges the norm tests use)."""
    g = torch.Generator().manual_seed(1000 * H + 10 * W + seed)
    hid = torch.randn(2, Ch, H, W, generator=g) * 3
    skip = torch.randn(2, Cs, H, W, generator=g) * 3
    if case == "offset":
        for t in (hid, skip):
            t += (torch.randint(0, 2, (1, t.shape[1], 1, 1), generator=g).float() * 2 - 1) * 40
            t[:, 3] *= 50
    return hid.to(dtype), skip.to(dtype)


def _filter_bound(ref, x64, s, dtype):
    """|got - ref| <= u |ref| + tiny + |s - 1| * 7 * (ceil(log2(H W)) + 8) * 2^-24 * max|x|: one storage rounding plus the
    pairwise-summation bound of the seven fp32 sums; max|x| is taken per (sample, channel) map, the set one sum runs over."""
    H, W = x64.shape[-2:]
    depth = math.ceil(math.log2(H * W)) + 8
    xmax = x64.abs().amax(dim=(-2, -1), keepdim=True)
    return U_[dtype] * ref.abs() + TINY[dtype] + abs(s - 1) * 7 * depth * 2.0 ** -24 * xmax


def _check_filter(got, x64, s, dtype, tag):
    ref = F.fourier_filter_fft(x64, s)
    err = (_nchw64(got) - ref).abs()
    ratio = float((err / _filter_bound(ref, x64, s, dtype)).max())
    print(json.dumps(dict(tag=tag, s=s, max_err=float(err.max()), worst_err_over_bound=round(ratio, 4))))
    assert ratio <= 1.0, (tag, s, ratio)  # every element


def _check_scale(got, h64, b, dtype, tag):
    """channels [0, Ch / 2) = round(h * b) (the fp32 product in between: 2^-24 relative more), the rest untouched"""
    half = h64.shape[1] // 2
    got64 = _nchw64(got)
    assert torch.equal(got64[:, half:], h64[:, half:]), tag
    ref = h64[:, :half] * b
    err = (got64[:, :half] - ref).abs()
    assert bool((err <= (U_[dtype] + 2.0 ** -24) * ref.abs() + TINY[dtype]).all()), (tag, float(err.max()))
    if b == 1.0:
        assert torch.equal(got64[:, :half], h64[:, :half])


@pytest.mark.parametrize("case", ["zero", "offset"])
@pytest.mark.parametrize("shape", KERNEL_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
def test_kernel_per_element_against_float64(dev, dtype, shape, case):
    """Both halves of one launch, every element, (b, s) in BS.  Also: in place == out of place, each half alone == the
    combined launch, and a second run, all bit for bit."""
    from uni_renderer_amd import ops

    H, W, Ch, Cs = shape
    hid, skip = _inputs(H, W, Ch, Cs, dtype, case)
    h64, s64 = hid.double(), skip.double()
    for b, s in BS:
        tag = f"{dtype}/{shape}/{case}/b{b}"
        hd, sd = _nhwc(hid, dev), _nhwc(skip, dev)
        out = ops.freeu(hd, sd, b, s)
        assert out.data_ptr() != sd.data_ptr() and torch.equal(sd.cpu(), _nhwc(skip, "cpu")) and ops.lo_of(out) is None
        _check_filter(out, s64, s, dtype, tag)
        _check_scale(hd, h64, b, dtype, tag)
        # second run
        hd2, sd2 = _nhwc(hid, dev), _nhwc(skip, dev)
        out2 = ops.freeu(hd2, sd2, b, s)
        assert torch.equal(out2, out) and torch.equal(hd2, hd)
        # in place
        same = ops.freeu(None, sd2, b, s, out=sd2)
        assert same is sd2 and torch.equal(sd2, out)
        # halves alone
        hd3 = _nhwc(hid, dev)
        assert ops.freeu(hd3, None, b, s) is None and torch.equal(hd3, hd)
        assert torch.equal(ops.freeu(None, _nhwc(skip, dev), b, s), out)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("hw", [(3, 1030), (1025, 2)], ids=lambda s: "x".join(map(str, s)))
def test_kernel_on_maps_beyond_the_twiddle_table(dev, dtype, hw):
    """H + W > 1024: the row / column twiddles no longer come from the workgroup's LDS table but are computed per pixel.  Same
    bound, every element; 24 channels = one full and one quarter-filled 32-channel slice."""
    from uni_renderer_amd import ops

    hid, skip = _inputs(*hw, 16, 24, dtype, "offset")
    for b, s in BS[:2]:
        hd, sd = _nhwc(hid, dev), _nhwc(skip, dev)
        out = ops.freeu(hd, sd, b, s)
        _check_filter(out, skip.double(), s, dtype, f"notable/{dtype}/{hw}")
        _check_scale(hd, hid.double(), b, dtype, f"notable/{dtype}/{hw}")
        assert torch.equal(ops.freeu(None, sd, b, s, out=sd), out)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("hw", [(5, 7), (8, 8), (12, 20)])
def test_kernel_plane_wave_known_answers(dev, dtype, hw):
    """cos(2 pi (ky y / H + kx x / W)) -> gain * itself; gain 1 for (1, -1) is what a symmetric low-pass gets wrong.  The
    stored wave is rounded (|delta| <= u), and the filter maps delta to at most (1 + 7 |s - 1|) |delta|."""
    from uni_renderer_amd import ops
    PLANE_WAVES, _plane = F.PLANE_WAVES, F.plane_wave

    H, W = hw
    waves = torch.stack([_plane(ky, kx, H, W) for (ky, kx), _ in PLANE_WAVES] + [torch.zeros(H, W, dtype=torch.float64)])[None]
    x = _nhwc(waves.to(dtype), dev)  # [1, H, W, 8]
    for s in (0.9, 0.2, 1.7):
        got = _nchw64(ops.freeu(None, x, 1.0, s))[0]
        u = U_[dtype]
        tol = u + u * (1 + 7 * abs(s - 1)) + abs(s - 1) * 7 * (math.ceil(math.log2(H * W)) + 8) * 2.0 ** -24
        for c, ((ky, kx), gain) in enumerate(PLANE_WAVES):
            err = float((got[c] - gain(s) * waves[0, c]).abs().max())
            assert err <= tol, (hw, ky, kx, s, err, tol)
        assert float(got[7].abs().max()) == 0.0


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("shape", [(8, 8, 128, 64), (16, 16, 64, 64), (5, 7, 64, 72), (40, 40, 32, 32)], ids=lambda s: "x".join(map(str, s)))
def test_kernel_hi_lo_pairs(dev, dtype, shape):
    """(hi, lo) operands: the value read is hi + lo (same bound against float64 of that value), the written pair is closer
    to float64 than its hi part alone, and in place over the pair == out of place."""
    from uni_renderer_amd import ops

    H, W, Ch, Cs = shape
    g = torch.Generator().manual_seed(7)
    b, s = 1.4, 0.2

    def pair(C):
        v = _nhwc(torch.randn(2, C, H, W, generator=g) * 3, dev)
        hi = v.to(dtype)
        hi.lo = ops.lo_encode(v - hi.float(), dtype)
        return hi, (hi.float() + ops.lo_float(hi.lo))

    hid, hval = pair(Ch)
    skip, sval = pair(Cs)
    skip_hi0, skip_lo0 = skip.clone(), skip.lo.clone()
    s64, h64 = _nchw64(sval), _nchw64(hval)
    out = ops.freeu(hid, skip, b, s)
    assert ops.lo_of(out) is not None and out.lo.dtype == ops.lo_dtype(dtype) and out.data_ptr() != skip.data_ptr()
    assert torch.equal(skip, skip_hi0) and torch.equal(skip.lo, skip_lo0)
    _check_filter(out, s64, s, dtype, f"hilo/{dtype}/{shape}")
    ref = F.fourier_filter_fft(s64, s)
    e_hi = (_nchw64(out) - ref).pow(2).mean().sqrt()
    e_pair = (_nchw64(out.float() + ops.lo_float(out.lo)) - ref).pow(2).mean().sqrt()
    half = Ch // 2
    href = h64[:, :half] * b
    eh_hi = (_nchw64(hid)[:, :half] - href).pow(2).mean().sqrt()
    eh_pair = (_nchw64(hid.float() + ops.lo_float(hid.lo))[:, :half] - href).pow(2).mean().sqrt()
    print(json.dumps(dict(dtype=str(dtype), shape=shape, skip_rms_hi=float(e_hi), skip_rms_pair=float(e_pair),
                          hidden_rms_hi=float(eh_hi), hidden_rms_pair=float(eh_pair))))
    assert e_pair < 0.5 * e_hi and eh_pair < 0.5 * eh_hi
    assert torch.equal(_nchw64(hid.float() + ops.lo_float(hid.lo))[:, half:], h64[:, half:])  # upper half: the pair is untouched
    # a skip without a low part gives an output without one; in place over the pair is the same bits
    inplace = ops.freeu(None, skip, b, s, out=skip)
    assert inplace is skip and torch.equal(skip, out) and torch.equal(skip.lo, out.lo)
    # rows: only samples [1, 2) of a two-sample pair
    hid2, _ = pair(Ch)
    skip2, _ = pair(Cs)
    h0, hl0, s0, sl0 = hid2.clone(), hid2.lo.clone(), skip2.clone(), skip2.lo.clone()
    full_h, full_s = hid2.clone(), skip2.clone()
    full_h.lo, full_s.lo = hl0.clone(), sl0.clone()
    full_out = ops.freeu(full_h, full_s, b, s)
    ops.freeu(hid2, skip2, b, s, out=skip2, rows=(1, 2))
    assert torch.equal(hid2[0], h0[0]) and torch.equal(hid2.lo[0], hl0[0]) and torch.equal(skip2[0], s0[0]) and torch.equal(skip2.lo[0], sl0[0])
    assert torch.equal(hid2[1], full_h[1]) and torch.equal(hid2.lo[1], full_h.lo[1])
    assert torch.equal(skip2[1], full_out[1]) and torch.equal(skip2.lo[1], full_out.lo[1])


def test_kernel_rejects_bad_shapes(dev):
    from uni_renderer_amd import ops

    z = lambda *shape: torch.zeros(*shape, dtype=torch.float16, device=dev)
    for hw in ((1, 8), (8, 1), (1, 1)):
        with pytest.raises(RuntimeError, match="UR_E_UNSUPPORTED"):
            ops.freeu(z(1, *hw, 16), z(1, *hw, 16), 1.2, 0.9)
    with pytest.raises(RuntimeError, match="UR_E_BADARG"):
        ops.freeu(z(1, 4, 4, 12), z(1, 4, 4, 16), 1.2, 0.9)
    with pytest.raises(RuntimeError, match="UR_E_BADARG"):
        ops.freeu(z(1, 4, 4, 16), z(1, 4, 4, 20), 1.2, 0.9)
    lib = ops._lib.load()  # both halves null: nothing to do is a bad call
    assert lib.ur_freeu(None, None, 0, 1.2, None, None, None, None, 0, 0.9, 1, 4, 4, 0, None) == -1001
    hid = torch.ones(1, 2, 2, 8, dtype=torch.float16, device=dev)  # channel counts whose half is not a vector: 8 -> 4 scaled
    ops.freeu(hid, None, 1.5, 1.0)
    assert torch.equal(hid[..., :4].cpu(), torch.full((1, 2, 2, 4), 1.5).half()) and torch.equal(hid[..., 4:].cpu(), torch.ones(1, 2, 2, 4).half())


# ---------------------------------------------------------------------------------------------------------------------------
# networks
# ---------------------------------------------------------------------------------------------------------------------------
LATENTS = [(32, 32), (20, 12)]  # FreeU on 4x4 / 8x8 maps; on 3x2 / 5x3 maps behind the upsample_size path
TOLS = [(torch.float16, 3e-3), (torch.bfloat16, 2.5e-2)]  # the tiny-config bounds of tests/test_model_gpu.py


@functools.lru_cache(maxsize=None)
def _oracle():
    return O.build_triplet(O.TINY_CONFIG, seed=1234)


@functools.lru_cache(maxsize=None)
def _case(hw):
    g = torch.Generator().manual_seed(99)
    x = torch.randn(2, 4, *hw, generator=g)
    c = torch.randn(2, 28, *hw, generator=g)
    ehs = torch.randn(2, 77, 64, generator=g) * 0.5
    return x, c, ehs, torch.tensor([500, 200]), torch.tensor([300, 700])


@functools.lru_cache(maxsize=None)
def _ref(hw, on, exchange, run_decoder=True, t_attr0=False):
    """The oracle's outputs, computed once per case and shared (never modified)."""
    x, c, ehs, ti, ta = _case(hw)
    if t_attr0:
        ta = torch.zeros_like(ta)
    return F.oracle_step(*_oracle(), x, c, ehs, ti, ta, freeu=F.SD14 if on else None, exchange=exchange, run_decoder=run_decoder)


@functools.lru_cache(maxsize=None)
def _product(dtype):
    return build_product_from_oracle(*_oracle(), dtype, torch.device("cuda:0"))


def _errs(out, ref, keys=("img_pred", "attr_pred", "raw_mid_unet"), lists=("raw_unet", "up_res")):
    e = {}
    for k in keys:
        if ref.get(k) is not None and out.get(k) is not None:
            e[k] = rel_l2(out[k], ref[k])
    for k in lists:
        if k in out and k in ref:
            assert len(out[k]) == len(ref[k])
            for i, (a, b) in enumerate(zip(out[k], ref[k])):
                e[f"{k}[{i}]"] = rel_l2(a, b)
    return e


def _assert_sees_feature(hw, exchange, tol, got_on):
    """The comparison can see FreeU: the oracle's img_pred moves by >= 10x the fp16 bound when it is switched on (0.073 at
    32x32, 0.087 at 20x12: 24x / 29x 3e-3; that is 2.9x / 3.5x the bf16 bound of 2.5e-2, so for bf16 the 10x does not hold
    and what is asserted is the consequence that matters: the product with FreeU on FAILS the bound against the FreeU-off
    oracle)."""
    on, off = _ref(hw, True, exchange), _ref(hw, False, exchange)
    sep = rel_l2(on["img_pred"], off["img_pred"])
    assert sep >= 10 * 3e-3, sep
    assert rel_l2(got_on, off["img_pred"]) > 2 * tol
    return sep


@pytest.mark.parametrize("exchange", [True, False], ids=["exchange", "unet_alone"])
@pytest.mark.parametrize("hw", LATENTS, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("dtype,tol", TOLS, ids=["f16", "bf16"])
def test_module_forward_vs_oracle(dev, dtype, tol, hw, exchange):
    """enc -> unet -> dec through the modules (or the UNet alone, without residuals), FreeU on with the SD-1.4 factors and off:
    img_pred / attr_pred within the tiny-config bound, raw_mid_unet, the 12 raw down samples and all 13 up_res (whose
    entries 0, 1, 2, 4, 5 -- and raw_mid without a mid residual -- come back scaled, as in the reference) within twice it.
    Measured on the MI355X, rel-L2 against the oracle, FreeU on / off (worst = the largest over all 27 / 26 tensors):
      fp16 32x32  exchange: img 1.16e-3 / 1.18e-3, attr 1.53e-3 / 1.53e-3, worst (up_res[1]) 1.57e-3 / 1.55e-3;  UNet alone: img 1.19e-3 / 1.17e-3, worst 1.58e-3 / 1.55e-3
      fp16 20x12  exchange: img 1.19e-3 / 1.16e-3, attr 1.55e-3 / 1.55e-3, worst (up_res[2]) 1.82e-3 / 1.79e-3;  UNet alone: img 1.17e-3 / 1.18e-3, worst 1.83e-3 / 1.77e-3
      bf16 32x32  exchange: img 9.62e-3 / 9.56e-3, attr 1.21e-2 / 1.21e-2, worst 1.25e-2 / 1.24e-2;              UNet alone: img 9.47e-3 / 9.34e-3, worst 1.24e-2 / 1.22e-2
      bf16 20x12  exchange: img 9.51e-3 / 9.65e-3, attr 1.28e-2 / 1.28e-2, worst 1.37e-2 / 1.35e-2;              UNet alone: img 9.87e-3 / 9.73e-3, worst 1.39e-2 / 1.36e-2
    FreeU adds nothing measurable to the error: on and off agree to 3 % everywhere."""
    unet, enc, dec = _product(dtype)
    x, c, ehs, ti, ta = [t.to(dev) for t in _case(hw)]
    res = {}
    for on in (True, False):
        unet.enable_freeu(**F.SD14) if on else unet.disable_freeu()
        try:
            with torch.no_grad():
                if exchange:
                    out = product_step(unet, enc, dec, x, c, ehs, ti, ta)
                else:
                    img, raw, raw_mid, ups = unet(x, ti, ehs, return_dict=False)
                    out = dict(img_pred=img, raw_unet=raw, raw_mid_unet=raw_mid, up_res=ups)
        finally:
            unet.disable_freeu()
        assert len(out["up_res"]) == 13 and len(out["raw_unet"]) == 12
        res[on] = (out, _errs(out, _ref(hw, on, exchange)))
    e_on, e_off = res[True][1], res[False][1]
    print(json.dumps(dict(executor="modules", dtype=str(dtype), hw=hw, exchange=exchange,
                          on={k: round(v, 6) for k, v in e_on.items()}, off={k: round(v, 6) for k, v in e_off.items()})))
    _assert_sees_feature(hw, exchange, tol, res[True][0]["img_pred"])
    for e in (e_on, e_off):
        assert e["img_pred"] < tol and e.get("attr_pred", 0.0) < tol, e
        assert max(e.values()) < 2 * tol, e
    # the aliasing itself: entry 0 is the tensor block 0 scaled, so it differs from the FreeU-off run by b1 on the first half of
    # its channels
    on_out, off_out = res[True][0], res[False][0]
    t_on, t_off = on_out["up_res"][0].float(), off_out["up_res"][0].float()  # the same tensor in both runs before the scale
    half = t_on.shape[1] // 2
    assert rel_l2(t_on[:, :half], t_off[:, :half] * 1.2) < 2 * U_[dtype] and torch.equal(t_on[:, half:], t_off[:, half:])
    if exchange:
        assert torch.equal(on_out["raw_mid_unet"], off_out["raw_mid_unet"])
    else:
        assert on_out["raw_mid_unet"].data_ptr() == on_out["up_res"][0].data_ptr()
    for a, b_ in zip(on_out["raw_unet"], off_out["raw_unet"]):
        assert torch.equal(a, b_)


@pytest.mark.parametrize("hw", LATENTS, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("dtype,tol", TOLS, ids=["f16", "bf16"])
def test_grouped_step_vs_oracle_and_its_graph(dev, dtype, tol, hw):
    """The grouped executor ([unet ; dec] rows in one launch: FreeU on the UNet's rows only), eager against the oracle and
    its captured graph against the eager run bit for bit.  Measured rel-L2 against the oracle, FreeU on / off: fp16 img 1.17e-3 /
    1.17e-3 (32x32), 1.20e-3 / 1.18e-3 (20x12), attr 1.53e-3 / 1.55e-3 (unchanged by FreeU, bit for bit); bf16 img 9.66e-3 / 9.42e-3,
    9.52e-3 / 9.54e-3, attr 1.21e-2 / 1.28e-2."""
    from uni_renderer_amd.fused import GroupedDualStreamStep
    from uni_renderer_amd.graph import GraphedDualStreamStep

    unet, enc, dec = _product(dtype)
    x, c, ehs, ti, ta = [t.to(dev) for t in _case(hw)]
    errs, outs = {}, {}
    try:
        for on in (True, False):
            unet.enable_freeu(**F.SD14) if on else unet.disable_freeu()
            with torch.no_grad():
                out = GroupedDualStreamStep(unet, enc, dec)(x, c, ehs, ti, ta)
            outs[on] = {k: v.clone() for k, v in out.items()}
            errs[on] = _errs(out, _ref(hw, on, True))
            if on:
                g = GraphedDualStreamStep(unet, enc, dec, 2, hw, 64, dtype=dtype, device=dev, mode="grouped")
                rep = g.step(x.to(dtype), c.to(dtype), ehs.to(dtype), ti, ta)
                for k in ("img_pred", "attr_pred"):
                    assert torch.equal(rep[k], outs[on][k]), k
    finally:
        unet.disable_freeu()
    print(json.dumps(dict(executor="grouped", dtype=str(dtype), hw=hw, on=errs[True], off=errs[False])))
    _assert_sees_feature(hw, True, tol, outs[True]["img_pred"])
    for e in errs.values():
        assert e["img_pred"] < tol and e["attr_pred"] < tol, e
    assert torch.equal(outs[True]["attr_pred"], outs[False]["attr_pred"])  # the decoder's rows are not touched


@pytest.mark.parametrize("hw", LATENTS, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("dtype,tol", TOLS, ids=["f16", "bf16"])
def test_hoisted_render_step_vs_oracle_and_its_graph(dev, dtype, tol, hw):
    """The hoisted rendering loop's step (encoder once, UNet per step; clean attributes: t_attr = 0) with FreeU on and off
    against the oracle, and its captured graphs against the eager run.  Measured rel-L2 against the oracle, FreeU on / off:
    fp16 1.18e-3 / 1.18e-3 (32x32), 1.22e-3 / 1.18e-3 (20x12); bf16 9.58e-3 / 9.50e-3, 9.73e-3 / 9.47e-3."""
    from uni_renderer_amd.graph import GraphedHoistedStep
    from uni_renderer_amd.hoist import HoistedSamplingStep

    unet, enc, dec = _product(dtype)
    x, c, ehs, ti, _ = [t.to(dev) for t in _case(hw)]
    t0 = torch.zeros(2, device=dev)
    errs, outs = {}, {}
    try:
        for on in (True, False):
            unet.enable_freeu(**F.SD14) if on else unet.disable_freeu()
            with torch.no_grad():
                h = HoistedSamplingStep(unet, enc, dec, "render")
                out = h.prologue(c, ehs, t0).step(x, ti.float())
            outs[on] = out["img_pred"].clone()
            ref = _ref(hw, on, True, run_decoder=False, t_attr0=True)
            errs[on] = rel_l2(out["img_pred"], ref["img_pred"])
            if on:
                g = GraphedHoistedStep(unet, enc, dec, 2, hw, 64, dtype=dtype, device=dev, run_decoder=False)
                rep = g.step(x.to(dtype), c.to(dtype), ehs.to(dtype), ti.float(), t0)
                assert torch.equal(rep["img_pred"], outs[on])
    finally:
        unet.disable_freeu()
    print(json.dumps(dict(executor="hoisted_render", dtype=str(dtype), hw=hw, on=errs[True], off=errs[False])))
    on_ref, off_ref = (_ref(hw, o, True, run_decoder=False, t_attr0=True)["img_pred"] for o in (True, False))
    assert rel_l2(on_ref, off_ref) >= 10 * 3e-3 and rel_l2(outs[True], off_ref) > 2 * tol
    assert errs[True] < tol and errs[False] < tol, errs


def test_module_graph_replay_equals_eager_with_freeu(dev):
    """serial and concurrent captures of the module path with FreeU on == the eager launches, bit for bit."""
    from uni_renderer_amd.graph import GraphedDualStreamStep, dual_stream_step

    unet, enc, dec = _product(torch.float16)
    x, c, ehs, ti, ta = [t.to(dev) for t in _case((20, 12))]
    x, c, ehs, ti, ta = x.half(), c.half(), ehs.half(), ti.float(), ta.float()
    unet.enable_freeu(**F.SD14)
    try:
        with torch.no_grad():
            ref = dual_stream_step(unet, enc, dec, x, c, ehs, ti, ta)
        for mode in ("serial", "concurrent"):
            o = GraphedDualStreamStep(unet, enc, dec, 2, (20, 12), 64, mode=mode).step(x, c, ehs, ti, ta)
            for k in ("img_pred", "attr_pred"):
                assert torch.equal(o[k], ref[k]), (mode, k)
    finally:
        unet.disable_freeu()


def _pipe(dev, seed=21):
    from uni_renderer_amd.pipeline import UniRendererPipeline

    models = O.build_triplet(O.TINY_CONFIG, seed=seed)
    unet, enc, dec = build_product_from_oracle(*models, torch.float16, dev)
    pipe = UniRendererPipeline(unet=unet, controlnet=enc, controldec=dec)
    pipe.set_progress_bar_config(disable=True)
    return pipe


@pytest.mark.parametrize("fused_sampler", [True, False], ids=["device_loop", "step_by_step"])
def test_pipeline_toggle_on_off_on(dev, fused_sampler):
    """Rendering loop through the pipeline: off after on == a pipeline that never enabled it, the second on == the first
    (no stale graph in either direction), and on != off.  The inverse loop never runs the UNet's up path: on == off."""
    g = torch.Generator().manual_seed(5)
    ehs = (torch.randn(1, 77, 64, generator=g) * 0.5).to(dev).half()
    noise = torch.randn(2, 4, 16, 16, generator=g)
    attr = torch.randn(2, 28, 16, 16, generator=g).to(dev)
    img, mask = torch.randn(2, 4, 16, 16, generator=g).to(dev), torch.randn(2, 4, 16, 16, generator=g).to(dev)
    kw = dict(prompt_embeds=ehs, attr_latents=attr, latents=noise, num_inference_steps=2, guidance_scale=0.0, output_type="latent")
    kwi = dict(prompt_embeds=ehs, image_latents=img, mask_latents=mask, latents=noise, num_inference_steps=2, guidance_scale=0.0,
               output_type="latent")
    never = _pipe(dev)
    never.use_fused_sampler = fused_sampler
    base = never.mask2image_3mod_albedo(**kw)
    base_inv = never.real_image2mask_3mod_albedo(**kwi)
    pipe = _pipe(dev)
    pipe.use_fused_sampler = fused_sampler
    off0 = pipe.mask2image_3mod_albedo(**kw)
    assert torch.equal(off0, base)
    pipe.enable_freeu(**F.SD14)
    on1 = pipe.mask2image_3mod_albedo(**kw)
    inv_on = pipe.real_image2mask_3mod_albedo(**kwi)
    pipe.disable_freeu()
    off1 = pipe.mask2image_3mod_albedo(**kw)
    pipe.enable_freeu(**F.SD14)
    on2 = pipe.mask2image_3mod_albedo(**kw)
    pipe.disable_freeu()
    assert torch.equal(off1, base) and torch.equal(on2, on1)
    assert rel_l2(on1, base) > 1e-2
    for a, b in zip(inv_on, base_inv):
        assert torch.equal(a, b)


def test_autograd_forward_with_freeu_raises(dev):
    unet, enc, dec = _product(torch.float16)
    x, c, ehs, ti, ta = [t.to(dev) for t in _case((32, 32))]
    unet.enable_freeu(**F.SD14)
    try:
        with pytest.raises(NotImplementedError, match="FreeU"):
            unet(x.half().requires_grad_(True), ti, ehs.half())
    finally:
        unet.disable_freeu()
