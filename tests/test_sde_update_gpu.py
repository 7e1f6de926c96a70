"""GPU tests of ``ur_sde_update`` / ``ur_sampler_noise`` (csrc/sampler.hip) per element: the noise against the float64
restatement of its definition, the update exactly on small-integer data and against float64 on normal data, on guarded
buffers, for every dtype / layout / guidance / rounding mode; the kernel against the host schedulers bit for bit."""
import itertools

import numpy as np
import pytest
import torch

from util_models import ROOT  # noqa: F401  (path setup)
import util_stochastic as R
from util_sampler_update import HALF_ULP, SHAPES, Case as _Case, combine as _combine, guarded as _guarded, guards_intact as _guards_intact

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16, torch.float32]


def test_sampler_noise_matches_the_float64_definition(dev):
    """Bound, per element with radius r = sqrt(-2 ln u) and value z = r * trig, from the accuracy of the fp32 functions (the
    OpenCL full-profile limits, which the device library documents it meets: log 3 ulp, log1p 2 ulp, sqrt 3 ulp, sinpi / cospi
    4 ulp; 1 ulp <= 2^-23 relative) and the roundings of their arguments:
      * ln u is taken at an argument that is exact in fp32 (the kernel's two branches), so -2 ln u has relative error
        <= 3 * 2^-23 and r = sqrt(.) has <= 1.5 * 2^-23 + 3 * 2^-23;
      * the angle argument 2 u = fl(k + 0.5) 2^-23 carries one rounding, relative 2^-24: the angle moves by <= 2 pi 2^-24 and
        so does sin / cos; sincospi adds 4 * 2^-23;
      * the product r * trig one rounding, |z| 2^-24.
    => |err| <= r (4.5 * 2^-23 + 2 pi 2^-24 + 4 * 2^-23) + |z| 2^-24: 8.2e-6 at r = 5.9, 1.4e-6 at r = 1.  A wrong counter, key
    or element mapping misses by O(1)."""
    from uni_renderer_amd import ops

    worst = 0.0
    for seed, step, n in ((1234, 0, 4099), (1234, 5, 4099), ((0x7654_3210 << 32) | 0x0FED_CBA9, 49, 1027), (0, 0, 3), (7, 2, 35)):
        sd = torch.tensor([seed], dtype=torch.int64, device=dev)
        got = ops.sampler_noise(sd, step, (n,)).double().cpu().numpy()
        want, r = R.normal_f64(seed, step, n, parts=True)
        bound = r * (4.5 * 2.0 ** -23 + 2 * np.pi * 2.0 ** -24 + 4 * 2.0 ** -23) + np.abs(want) * 2.0 ** -24
        err = np.abs(got - want)
        worst = max(worst, float((err / bound).max()))
        print(f"seed {seed:#x} step {step} n {n}: max err {err.max():.3e}, max err / bound {float((err / bound).max()):.3f}")
        assert np.all(err <= bound), (seed, step, n, float(err.max()))
    # shape only names the element count: [2, 24, 5, 7] is the first 1680 elements of the same stream
    sd = torch.tensor([1234], dtype=torch.int64, device=dev)
    a = ops.sampler_noise(sd, 5, (2, 24, 5, 7))
    assert torch.equal(a.reshape(-1), ops.sampler_noise(sd, 5, (4099,))[:1680])
    # guarded output: a tail group writes n % 4 elements only
    buf, out = _guarded((35,), torch.float32, dev)
    ops.sampler_noise(sd, 5, (35,), out=out)
    assert _guards_intact(buf) and torch.equal(out, a.reshape(-1)[:35])
    with pytest.raises(RuntimeError):
        ops.sampler_noise(sd.int(), 0, (4,))
    with pytest.raises(RuntimeError):
        ops.sampler_noise(sd, -1, (4,))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16", "f32"])
def test_update_is_exact_on_small_integer_data_without_noise(dev, dtype):
    """pn = 0, integer data in [-2, 2] (guided predictions in [-10, 10]), rows of small dyadic weights: every intermediate is
    exact in fp32 and every result fits the 8-bit significand of bf16 (|x| <= 12, 27, 57.5, 67.5 after the four calls, in steps
    of 0.5), so the kernel must reproduce the float64 recurrence bit for bit --
    including the guidance combine, ``hist`` == m_i, the clamp of ``*step`` and untouched guards.  The seed pointer is a device
    int64 the rows with pn = 0 never read: its value must not matter."""
    from uni_renderer_amd import ops

    rows = torch.tensor([[1, 1, 0, 0], [-1, 1, 0.5, 0], [1, 1, -2, 0]], dtype=torch.float32)
    gen = torch.Generator().manual_seed(1)
    for (B, C, hw), cfg, rm in itertools.product(SHAPES, (False, True), (False, True)):
        c = _Case(dev, dtype, B, C, hw, cfg, 3, gen, integer=True)
        cc = C // 2  # cfg_channels < C
        x, m1 = c.x0.double(), torch.zeros_like(c.x0).double()
        for i in range(4):  # the fourth call has *step = 3 >= nsteps: row 2 again
            k = min(i, 2)
            c.seed.fill_(i * 977)
            ops.sde_update(c.preds[k], 4, c.lat, rows.to(dev), c.step, 3, c.seed, c.master, c.hist, round_master=rm,
                           guidance=2.0 if cfg else None, cfg_channels=cc if cfg else 0)
            ops.sampler_advance(c.step, torch.zeros(3, device=dev), 3)
            m = _combine(c.preds[k], cfg, 2.0, cc, B, C).double().cpu()
            x, m1 = rows[k, 0].double() * x + rows[k, 1].double() * m + rows[k, 2].double() * m1, m
            assert torch.equal(c.master.cpu().double(), x) and torch.equal(c.hist.cpu().double(), m), (B, C, hw, cfg, rm, i)
            assert torch.equal(c.lat[:B].cpu().double(), x), (B, C, hw, cfg, rm, i)
            if cfg:
                assert torch.equal(c.lat[B:], c.lat[:B])
            assert c.intact(), (B, C, hw, cfg, rm, i)
        assert int(c.step) == 4


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16", "f32"])
def test_update_with_noise_against_float64_on_guarded_buffers(dev, dtype):
    """N(0, 1) data, all four weights non-zero.  Each step is compared with the float64 update of the kernel's OWN previous
    state (master, hist) and its own noise (``sampler_noise``), so the bound is one step's: the four products and three sums are
    7 fp32 roundings, each of a value bounded by S = sum |p_k v_k|: |err| <= 7 * 2^-24 * S on the fp32 master; the storage
    dtype adds one rounding, 2^-11 (fp16) / 2^-8 (bf16) relative, to ``lat`` (and to ``master`` under round_master)."""
    from uni_renderer_amd import ops

    rows = torch.tensor([[0.9, 0.3, 0.0, 0.5], [0.7, 1.4, -0.6, 0.8], [0.2, 1.1, -0.3, 0.05]], dtype=torch.float32)
    gen = torch.Generator().manual_seed(2)
    worst = 0.0
    for (B, C, hw), cfg, rm in itertools.product(SHAPES, (False, True), (False, True)):
        c = _Case(dev, dtype, B, C, hw, cfg, 3, gen, integer=False)
        cc = C - 1
        for i in range(3):
            x_prev, h_prev = c.master.double().cpu(), c.hist.double().cpu()
            ops.sde_update(c.preds[i], 4, c.lat, rows.to(dev), c.step, 3, c.seed, c.master, c.hist, round_master=rm,
                           guidance=1.5 if cfg else None, cfg_channels=cc if cfg else 0)
            xi = ops.sampler_noise(c.seed, i, (B, C) + tuple(hw)).double().cpu()
            ops.sampler_advance(c.step, torch.zeros(3, device=dev), 3)
            m = _combine(c.preds[i], cfg, 1.5, cc, B, C).double().cpu()
            p = rows[i].double()
            terms = [p[0] * x_prev, p[1] * m, p[2] * h_prev, p[3] * xi]
            want = terms[0] + terms[1] + terms[2] + terms[3]
            bound32 = 7 * 2.0 ** -24 * sum(t.abs() for t in terms) + 1e-30
            store = HALF_ULP[dtype] * want.abs() + bound32 * (1 + HALF_ULP[dtype]) + (2.0 ** -25 if dtype == torch.float16 else 0.0)
            e_master = (c.master.double().cpu() - want).abs()
            e_lat = (c.lat[:B].double().cpu() - want).abs()
            worst = max(worst, float((e_master / (store if rm else bound32)).max()), float((e_lat / store).max()))
            assert bool((e_master <= (store if rm else bound32)).all()), (B, C, hw, cfg, rm, i)
            assert bool((e_lat <= store).all()), (B, C, hw, cfg, rm, i)
            assert torch.equal(c.hist.cpu().double(), m)
            assert torch.equal(c.lat[:B].float(), c.master) if rm else torch.equal(c.lat[:B], c.master.to(dtype))
            if cfg:
                assert torch.equal(c.lat[B:], c.lat[:B])
            assert c.intact(), (B, C, hw, cfg, rm, i)
    print("max err / bound", worst)


def _schedulers(n):
    from uni_renderer_amd.schedulers import DDIMScheduler, DDPMScheduler, DPMSolverMultistepScheduler

    kw = dict(prediction_type="sample", beta_schedule="scaled_linear", beta_start=0.00085, beta_end=0.012)
    for name, s, step_kw in (("ddim-eta1", DDIMScheduler(), dict(eta=1.0)), ("ddim-eta0.3", DDIMScheduler(), dict(eta=0.3)),
                             ("ddpm", DDPMScheduler(steps_offset=1, **kw), {}),
                             ("dpm++2m", DPMSolverMultistepScheduler(**kw), {}),
                             ("sde-dpm++2m", DPMSolverMultistepScheduler(algorithm_type="sde-dpmsolver++", lower_order_final=False, **kw), {})):
        s.set_timesteps(n)
        yield name, s, step_kw, (s.coefficient_table(step_kw["eta"]) if "eta" in step_kw else s.coefficient_table())


@pytest.mark.parametrize("dtype,lat_dtype", [(torch.float16, torch.float32), (torch.float16, torch.float16),
                                             (torch.float32, torch.float32), (torch.bfloat16, torch.bfloat16)],
                         ids=["f16-lat32", "f16-lat16", "f32", "bf16-lat16"])
def test_kernel_equals_the_host_scheduler_step_bitwise(dev, dtype, lat_dtype):
    """3 steps of ``ur_sde_update`` == 3 host ``step`` calls on the same table with the noise of ``sampler_noise``: same fp32
    products, same order, no contraction, one rounding where the host rounds (``round_master`` = latents kept in the storage
    dtype).  With and without guidance (the host gets the prediction combined in its dtype, as the step-by-step loop does)."""
    from uni_renderer_amd import ops

    gen = torch.Generator().manual_seed(3)
    B, C, hw, n = 2, 24, (5, 7), 3
    rm = lat_dtype != torch.float32
    for (name, s, step_kw, tab), cfg in itertools.product(list(_schedulers(n)), (False, True)):
        c = _Case(dev, dtype, B, C, hw, cfg, n, gen, integer=False)
        s.set_timesteps(n)  # a fresh multistep history
        if rm:
            c.master.copy_(c.x0.to(lat_dtype).float())
        x = c.master.to(lat_dtype, copy=True)  # not a view of the buffer the kernel updates
        tvals = s.timesteps.float().to(dev)
        for i, t in enumerate(s.timesteps):
            ops.sde_update(c.preds[i], 4, c.lat, tab.to(dev), c.step, n, c.seed, c.master, c.hist, round_master=rm,
                           guidance=2.5 if cfg else None, cfg_channels=4 if cfg else 0)
            ops.sampler_advance(c.step, tvals, n)
            xi = ops.sampler_noise(c.seed, i, (B, C) + hw)
            x = s.step(_combine(c.preds[i], cfg, 2.5, 4, B, C), t, x, variance_noise=xi, **step_kw)[0]
            assert x.dtype == lat_dtype and torch.equal(c.master, x.float()), (name, cfg, i)
            assert torch.equal(c.lat[:B], x.to(dtype)), (name, cfg, i)
        assert c.intact()


def test_runs_are_bit_stable_and_the_seed_reaches_every_element(dev):
    from uni_renderer_amd import ops

    rows = torch.tensor([[0.9, 0.3, 0.0, 0.5], [0.7, 1.4, -0.6, 0.8]], dtype=torch.float32, device=dev)
    outs = []
    for seed in (11, 11, 12):
        c = _Case(dev, torch.float16, 2, 24, (5, 7), True, 2, torch.Generator().manual_seed(4), integer=False)
        c.seed.fill_(seed)
        for i in range(2):
            ops.sde_update(c.preds[i], 4, c.lat, rows, c.step, 2, c.seed, c.master, c.hist, guidance=2.0, cfg_channels=4)
            ops.sampler_advance(c.step, torch.zeros(2, device=dev), 2)
        outs.append((c.master.clone(), c.lat.clone()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert bool((outs[0][0] != outs[2][0]).all())  # only the seed BUFFER changed: nothing of it is a launch argument


def test_argument_checks(dev):
    from uni_renderer_amd import ops

    c = _Case(dev, torch.float16, 1, 4, (8, 8), False, 1, torch.Generator().manual_seed(5), integer=True)
    rows = torch.tensor([[1.0, 1.0, 0.0, 0.0]], device=dev)
    ok = dict(pred_nhwc=c.preds[0], c0=4, lat_nchw=c.lat, coef=rows, step=c.step, nsteps=1, seed=c.seed, master=c.master, hist=c.hist)
    ops.sde_update(**ok)
    bad = [dict(coef=torch.zeros(1, 8, device=dev)), dict(coef=rows.double()), dict(step=c.step.long()), dict(seed=c.seed.int()),
           dict(seed=c.seed.cpu()), dict(master=c.master.half()), dict(hist=c.hist[:, :2]), dict(pred_nhwc=c.preds[0].float()),
           dict(lat_nchw=c.lat_full[:, 4:8].permute(0, 1, 3, 2)), dict(guidance=2.0), dict(cfg_channels=5), dict(nsteps=2),
           dict(c0=26), dict(pred_nhwc=c.preds[0][:, :4])]
    for kw in bad:
        with pytest.raises(RuntimeError):
            ops.sde_update(**dict(ok, **kw))
    assert c.intact()
