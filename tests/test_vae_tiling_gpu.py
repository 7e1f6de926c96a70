"""GPU tests of VAE tiling and slicing: ``ur_blend_tiles`` per element against the float64 restatement of diffusers' sequential
in-place stitch (exactly on integer data, within a bound derived from the kernel's stated arithmetic on random data, on
guarded buffers), and ``AutoencoderKL.tiled_decode`` / ``tiled_encode`` / slicing / the pipeline switches against the CPU
oracle VAE run per tile and stitched by the same restatement."""
import functools
import json

import pytest
import torch

import util_vae_tiling as T
from conftest import rel_l2
from util_models import O, build_product_from_oracle

from oracle import vae_oracle as V

pytestmark = pytest.mark.gpu

HALF = [torch.float16, torch.bfloat16]
# base shape: tiles of 16 px, blend 4, limit 12
HS, WS, BLEND, LIMIT = (16, 16, 16), (16, 16, 16), 4, 12


def _run(tiles, blend, limit, out_dtype, dev, batched=False, offset=0):
    """One ``ops.blend_tiles`` over NCHW CPU ``tiles``: the device tiles sit between NaN bands, the output between canaries
    that must survive.  Returns the output on the CPU."""
    from uni_renderer_amd import ops

    dt, keep = T.device_tiles(tiles, dev, batched=batched, offset=offset)
    B, C = tiles[0][0].shape[:2]
    shape = (B, C, sum(min(limit, r[0].shape[2]) for r in tiles), sum(min(limit, t.shape[3]) for t in tiles[0]))
    g = T.Guarded(out_dtype, dev)
    k = g.reserve(B * C * shape[2] * shape[3], offset=offset)
    g.allocate()
    out = g.view(k, shape)
    assert ops.blend_tiles(dt, blend, limit, out=out) is out
    torch.cuda.synchronize()
    g.check()
    return out.cpu()


def _check_bound(tiles, blend, limit, out_dtype, dev, **kw):
    got = _run(tiles, blend, limit, out_dtype, dev, **kw)
    ref, bnd = T.stitch(tiles, blend, limit), T.bound(tiles, blend, limit, out_dtype)
    assert got.shape == ref.shape
    assert not bool(torch.isnan(got).any()), "a read outside a tile"
    d = (got.double() - ref).abs()
    worst = float((d / bnd.clamp_min(1e-300)).max())
    assert bool((d <= bnd).all()), f"{int((d > bnd).sum())} elements over the bound, worst ratio {worst}"
    return worst


# ---------------------------------------------------------------------------------------------------------------------
# kernel level
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tdt", HALF)
def test_exact_on_integer_data(dev, tdt):
    """Integers in [-64, 64], extents 4 (16 px tiles) and 2 (the 2 px last tiles), fp32 output.  Every weight is k / 4 or k / 2,
    an fp32 number with at most two fractional bits, and so is 1 - w.  A product |t| <= 64 times such a weight is a multiple of
    1 / 4 below 2^7, a lerp of two of them the same; the corner nests three lerps, so every intermediate is a multiple of 2^-6
    of magnitude <= 64: 13 significant bits at most, far inside fp32's 24.  Every product, fma and sum is therefore exact and
    the result equals the float64 restatement bit for bit; with fp32 output there is no rounding at all."""
    tiles = T.make_tiles((16, 16, 2), (16, 16, 2), 2, 3, tdt, seed=3, integer=True)
    got = _run(tiles, BLEND, LIMIT, torch.float32, dev)
    ref = T.stitch(tiles, BLEND, LIMIT)
    assert got.shape == (2, 3, 26, 26)
    assert torch.equal(got.double(), ref)
    assert not torch.equal(ref, T.stitch_raw_neighbours(tiles, BLEND, LIMIT))


@pytest.mark.parametrize("odt", HALF + [torch.float32])
@pytest.mark.parametrize("tdt", HALF)
def test_random_data_within_the_derived_bound(dev, tdt, odt):
    """Blend 6 and last tiles of 3 px (e = 3): weights k / 6 and k / 3 are rounded fp32 quotients.  The bound (util_vae_tiling
    ``_lerp`` / ``bound``): per lerp u (|a| (w + 3 (1 - w)) + 2 |b| w) with u = 2^-24, propagated through the nest of the closed
    form, plus half an ulp of a 16-bit output dtype -- from the arithmetic ur_kernels.h states, not from what the kernel gives."""
    hs, ws, blend, limit = (16, 12, 3), (13, 16, 3), 6, 10
    tiles = T.make_tiles(hs, ws, 2, 3, tdt, seed=4)
    worst = _check_bound(tiles, blend, limit, odt, dev)
    print(json.dumps(dict(test="blend_tiles_bound", tiles=str(tdt), out=str(odt), worst_ratio=worst)))
    # the aliasing is what is tested: in the corners the blend against RAW neighbours is further from the restatement than
    # the bound allows, so a kernel that computed it would fail above
    ref, raw = T.stitch(tiles, blend, limit), T.stitch_raw_neighbours(tiles, blend, limit)
    corner = T.corner_mask(tiles, blend, limit)
    over = ((ref - raw).abs() > T.bound(tiles, blend, limit, odt))[..., corner]
    assert int(corner.sum()) == (6 + 3) * (6 + 3) and float(over.double().mean()) > 0.9, float(over.double().mean())


def test_one_tile_is_to_nchw(dev):
    from uni_renderer_amd import ops

    for C in (3, 8):
        x = torch.randn(2, 7, 5, C, generator=torch.Generator().manual_seed(5)).half().to(dev)
        for odt in (torch.float16, torch.bfloat16, torch.float32):
            assert torch.equal(ops.blend_tiles([[x]], 4, 12, odt), ops.to_nchw(x, odt))
        assert ops.blend_tiles([[x]], 0, 4).shape == (2, C, 4, 4)          # the crop alone
        assert torch.equal(ops.blend_tiles([[x]], 0, 4), ops.to_nchw(x)[:, :, :4, :4])


SHAPES = [((16,), (16, 16, 16)), ((16, 16, 16), (16,)), ((16, 16, 10), (16, 16, 10)), ((16, 16, 2), (16, 16, 2)),
          ((16, 16, 10), (16, 16, 2))]


@pytest.mark.parametrize("C,offset", [(3, 0), (3, 1), (8, 0), (8, 1)])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("hs,ws", SHAPES)
def test_grid_shapes_batches_and_channels(dev, hs, ws, B, C, offset):
    """1 x 3, 3 x 1 and 3 x 3 grids with last tiles longer and shorter than the blend; C = 8 tiles at 16-byte alignment take
    the one-load-per-pixel path, one element off it the element-wise one."""
    tiles = T.make_tiles(hs, ws, B, C, torch.float16, seed=6 + B + C)
    _check_bound(tiles, BLEND, LIMIT, torch.float16, dev, offset=offset)


@pytest.mark.parametrize("C", [3, 8])
def test_tiles_that_are_slices_of_a_batched_tensor(dev, C):
    tiles = T.make_tiles((16, 16, 10), (16, 16, 2), 3, C, torch.bfloat16, seed=9)
    dt, _ = T.device_tiles(tiles, dev, batched=True)
    assert dt[0][0].stride(0) == 2 * 16 * 16 * C
    _check_bound(tiles, BLEND, LIMIT, torch.float32, dev, batched=True)


@pytest.mark.parametrize("nrows,ncols", [(9, 8), (14, 5), (33, 2)])
def test_a_grid_larger_than_one_launch_runs_in_bands(dev, nrows, ncols):
    from uni_renderer_amd import ops

    assert nrows * ncols > ops.blend_tiles_max() >= 2 * ncols
    hs, ws = (8,) * (nrows - 1) + (5,), (8,) * (ncols - 1) + (3,)
    tiles = T.make_tiles(hs, ws, 2, 3, torch.float16, seed=10)
    _check_bound(tiles, 2, 6, torch.float16, dev)
    ints = T.make_tiles(hs, ws, 1, 3, torch.float16, seed=11, integer=True)
    assert torch.equal(_run(ints, 2, 6, torch.float32, dev).double(), T.stitch(ints, 2, 6))


def test_two_launches_give_equal_bits(dev):
    tiles = T.make_tiles((16, 12, 3), (13, 16, 3), 2, 8, torch.float16, seed=12)
    a, b = _run(tiles, 6, 10, torch.float16, dev), _run(tiles, 6, 10, torch.float16, dev)
    assert torch.equal(a.view(torch.int16), b.view(torch.int16))


def test_python_side_refuses_what_the_launcher_refuses(dev):
    from uni_renderer_amd import ops

    t = lambda h, w: torch.zeros(1, h, w, 3, dtype=torch.float16, device=dev)
    with pytest.raises(NotImplementedError, match="2 \\* blend"):
        ops.blend_tiles([[t(7, 16)], [t(16, 16)]], 4, 12)
    with pytest.raises(ValueError, match="expected"):
        ops.blend_tiles([[t(16, 16), t(15, 16)]], 4, 12)
    with pytest.raises(ValueError, match="contiguous NHWC"):
        ops.blend_tiles([[t(16, 32)[:, :, ::2]]], 4, 12)


# ---------------------------------------------------------------------------------------------------------------------
# network level
# ---------------------------------------------------------------------------------------------------------------------
def _product(oracle, dtype, dev, sample_size):
    from uni_renderer_amd.vae import AutoencoderKL

    c = oracle.cfg
    m = AutoencoderKL(in_channels=c["in_channels"], out_channels=c["out_channels"], latent_channels=c["latent_channels"],
                      block_out_channels=c["block_out_channels"], layers_per_block=c["layers_per_block"],
                      norm_num_groups=c["norm_num_groups"], scaling_factor=c["scaling_factor"], sample_size=sample_size,
                      down_block_types=("DownEncoderBlock2D",) * len(c["block_out_channels"]),
                      up_block_types=("UpDecoderBlock2D",) * len(c["block_out_channels"]))
    m.load_state_dict(oracle.state_dict())
    return m.to(dtype).to(dev).eval()


@functools.lru_cache(maxsize=None)
def _tiny():
    """The tiny oracle VAE (2 levels: sample tile 16, latent tile 8) with its tiled references, computed once."""
    o = V.build(V.TINY_VAE_CONFIG, seed=21)
    g = torch.Generator().manual_seed(22)
    z, x = torch.randn(2, 4, 17, 14, generator=g), torch.randn(2, 3, 34, 28, generator=g)
    return o, z, x, T.oracle_tiled_decode(o, z, 8, 16), T.oracle_tiled_moments(o, x, 8, 16)


@pytest.mark.parametrize("dtype,tol", [(torch.float16, 4e-3), (torch.bfloat16, 3e-2)])
def test_tiny_vae_tiled_decode_and_encode_vs_oracle(dev, dtype, tol):
    o, z, x, img, (mean, logvar) = _tiny()
    m = _product(o, dtype, dev, 16)
    assert (m.tile_sample_min_size, m.tile_latent_min_size) == (16, 8)
    out = m.tiled_decode(z.to(dev).to(dtype)).sample
    post = m.tiled_encode(x.to(dev).to(dtype)).latent_dist
    errs = dict(vae="tiny tiled", dtype=str(dtype), decode=rel_l2(out, img), mean=rel_l2(post.mean, mean), logvar=rel_l2(post.logvar, logvar))
    print(json.dumps(errs))
    assert out.shape == (2, 3, 34, 28) and out.dtype == dtype and post.parameters.shape == (2, 8, 17, 14)
    assert errs["decode"] < tol and errs["mean"] < tol and errs["logvar"] < tol
    # tiling changes the result: the tiled reference is not the plain decode
    assert rel_l2(o.decode(z), img) > 10 * tol


def test_sd_size_vae_tiled_decode_vs_oracle(dev):
    o = V.build(V.SD_VAE_CONFIG, seed=23)
    m = _product(o, torch.float16, dev, 128)
    z = torch.randn(1, 4, 28, 28, generator=torch.Generator().manual_seed(24))
    img = T.oracle_tiled_decode(o, z, 16, 128)
    out = m.tiled_decode(z.to(dev).half(), return_dict=False)[0]
    err = rel_l2(out, img)
    print(json.dumps(dict(vae="sd tiled", decode=err)))
    assert out.shape == (1, 3, 224, 224) and err < 3e-3


def test_plain_path_slicing_and_dispatch(dev):
    o, z, x, _, _ = _tiny()
    m = _product(o, torch.float16, dev, 16)
    zd, xd = z.to(dev).half(), x.to(dev).half()
    small = zd[:, :, :8, :8].contiguous()
    g = torch.Generator().manual_seed(25)
    z3, x3 = torch.randn(3, 4, 8, 6, generator=g).to(dev).half(), torch.randn(3, 3, 16, 12, generator=g).to(dev).half()
    plain, plain3 = m.decode(small).sample, m.decode(z3).sample
    moments3 = m.encode(x3).latent_dist.parameters
    big = m.decode(zd).sample                                      # tiling off: one plain decode of the 17 x 14 latent
    # with tiling on, an input no larger than the tile takes the plain path: the same bits
    m.enable_tiling()
    assert torch.equal(m.decode(small).sample, plain)
    assert torch.equal(m.encode(x3).latent_dist.parameters, moments3)
    # ... and a larger one the tiled path
    tiled = m.tiled_decode(zd).sample
    assert torch.equal(m.decode(zd).sample, tiled) and torch.equal(m.decode(zd, return_dict=False)[0], tiled)
    assert not torch.equal(tiled, big)
    assert torch.equal(m.encode(xd).latent_dist.parameters, m.tiled_encode(xd).latent_dist.parameters)
    # slicing: one sample at a time, concatenated -- alone and together with tiling
    m.enable_slicing()
    assert torch.equal(m.decode(zd).sample, tiled)
    m.disable_tiling()
    assert torch.equal(m.decode(z3).sample, torch.cat([m.decode(z3[i:i + 1]).sample for i in range(3)]))
    assert torch.equal(m.encode(x3).latent_dist.parameters,
                       torch.cat([m.encode(x3[i:i + 1]).latent_dist.parameters for i in range(3)]))
    assert m.decode(z3).sample.shape == plain3.shape
    m.disable_slicing()
    assert torch.equal(m.decode(z3).sample, plain3) and torch.equal(m.decode(zd).sample, big)


def test_pipeline_with_vae_tiling_enabled(dev):
    """The flow of test_vae_gpu.test_pipeline_with_the_product_vae_on_both_ends with ``pipe.enable_vae_tiling()`` and a VAE of
    sample_size 16 on 32 x 32 images, against the oracle flow whose VAE encode / decode are the tiled restatement."""
    from uni_renderer_amd import vae as vae_mod
    from uni_renderer_amd.pipeline import ATTR_GROUPS, UniRendererPipeline
    from uni_renderer_amd.schedulers import DDIMScheduler

    unet_o, enc_o, dec_o = O.build_triplet(O.TINY_CONFIG, seed=28)
    unet, enc, dec = build_product_from_oracle(unet_o, enc_o, dec_o, torch.float16, dev)
    vo = V.build(V.TINY_VAE_CONFIG, seed=15)
    vae = _product(vo, torch.float16, dev, 16)
    pipe = UniRendererPipeline(vae=vae, unet=unet, controlnet=enc, controldec=dec)
    pipe.vae_scale_factor = 2
    pipe.set_progress_bar_config(disable=True)
    pipe.enable_vae_tiling()
    assert vae.use_tiling
    g = torch.Generator().manual_seed(16)
    image, masks = torch.rand(2, 3, 32, 32, generator=g) * 2 - 1, torch.rand(2, 3, 32, 32, generator=g) * 2 - 1
    ehs = torch.randn(1, 77, 64, generator=g) * 0.5
    noise = torch.randn(2, 4, 16, 16, generator=g)
    orig_sample = vae_mod.DiagonalGaussianDistribution.sample
    vae_mod.DiagonalGaussianDistribution.sample = lambda self, generator=None: self.mean  # deterministic: the mode
    try:
        out = pipe.real_image2mask_3mod_albedo(prompt_embeds=ehs.to(dev).half(), image=image.to(dev).half(), masks=masks.to(dev).half(),
                                               latents=noise, num_inference_steps=2, guidance_scale=0.0, output_type="pt")
    finally:
        vae_mod.DiagonalGaussianDistribution.sample = orig_sample
    sf = vo.cfg["scaling_factor"]
    lat_img, lat_mask = T.oracle_tiled_moments(vo, image, 8, 16)[0] * sf, T.oracle_tiled_moments(vo, masks, 8, 16)[0] * sf
    assert rel_l2(vo.encode_moments(image)[0] * sf, lat_img) > 1e-1           # the tiled latents are other latents
    s = DDIMScheduler()
    s.set_timesteps(2)
    lat = {n: noise.clone() for n in ATTR_GROUPS}
    e = ehs.repeat(2, 1, 1)
    for t in s.timesteps:
        cond = torch.cat([lat_mask] + [lat[n] for n in ATTR_GROUPS], 1)
        r = O.dual_stream_step(unet_o, enc_o, dec_o, lat_img, cond, e, torch.zeros(2).long(), t.expand(2))
        for k, n in enumerate(ATTR_GROUPS):
            lat[n] = s.step(r["attr_pred"][:, 4 + 4 * k:8 + 4 * k], t, lat[n])[0]
    assert rel_l2(out[0], lat["material"]) < 1e-2
    for img, n in zip(out[1:], ATTR_GROUPS[1:]):
        ref = (T.oracle_tiled_decode(vo, lat[n] / sf, 8, 16) / 2 + 0.5).clamp(0, 1)
        assert img.shape == (2, 3, 32, 32) and rel_l2(img, ref) < 1.5e-2, (n, rel_l2(img, ref))
