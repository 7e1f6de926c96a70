"""GPU tests of the sampling loops with MultiDiffusion views (``enable_multidiffusion``): the on-device loop (step graph +
update kernel + ``ur_view_blend`` + advance, replayed) against the step-by-step loop, both against the literal Panorama loop
on the CPU oracle networks (tests/util_multidiffusion.py), and the structure of the switch.  Tiny networks in fp16, one
24 x 32 latent, window 16, stride 8: a batch of 6 views, 12 under guidance."""
import pytest
import torch

from conftest import rel_l2
from util_models import O, OracleScheduler, build_product_from_oracle
import util_multidiffusion as R

pytestmark = pytest.mark.gpu
GROUPS = R.GROUPS
H, W, WINDOW, STRIDE = 24, 32, 16, 8
SD = dict(prediction_type="sample", beta_schedule="scaled_linear", beta_start=0.00085, beta_end=0.012)


def _new_pipe(nets):
    from uni_renderer_amd.pipeline import UniRendererPipeline

    pipe = UniRendererPipeline(unet=nets[0], controlnet=nets[1], controldec=nets[2])
    pipe.set_progress_bar_config(disable=True)
    return pipe


@pytest.fixture(scope="module")
def rig(dev):
    models = O.build_triplet(O.TINY_CONFIG, seed=21)
    nets = build_product_from_oracle(*models, torch.float16, dev)
    pipe = _new_pipe(nets)
    pipe.enable_multidiffusion(window_size=WINDOW, stride=STRIDE)
    g = torch.Generator().manual_seed(5)
    t = dict(img=torch.randn(1, 4, H, W, generator=g), mask=torch.randn(1, 4, H, W, generator=g),
             ehs=torch.randn(1, 77, 64, generator=g) * 0.5, noise=torch.randn(1, 4, H, W, generator=g),
             attr=torch.randn(1, 28, H, W, generator=g))
    return pipe, nets, models, t


def _attach(pipe, name):
    """Fresh scheduler objects on every latent group; returns the ``eta`` of the call."""
    from uni_renderer_amd.pipeline import SCHEDULER_NAMES
    from uni_renderer_amd.schedulers import DDIMScheduler, DPMSolverMultistepScheduler, UniPCMultistepScheduler

    make = {"ddim": DDIMScheduler, "unipc": UniPCMultistepScheduler, "ddim-eta1": DDIMScheduler,
            "sde-dpm++2m": lambda: DPMSolverMultistepScheduler(algorithm_type="sde-dpmsolver++", **SD)}[name]
    for n in SCHEDULER_NAMES:
        setattr(pipe, f"scheduler_{n}", make())
    return 1.0 if name == "ddim-eta1" else 0.0


def _inverse(pipe, t, dev, steps, guidance, eta=0.0, ehs_dtype=torch.float16, **kw):
    t = dict(t, **kw)
    return pipe.real_image2mask_3mod_albedo(
        prompt_embeds=t["ehs"].to(dev).to(ehs_dtype), image_latents=t["img"].to(dev), mask_latents=t["mask"].to(dev),
        latents=t["noise"], num_inference_steps=steps, guidance_scale=guidance, output_type="latent", eta=eta,
        generator=torch.Generator().manual_seed(3))


def _render(pipe, t, dev, steps, guidance, eta=0.0, ehs_dtype=torch.float16, **kw):
    t = dict(t, **kw)
    return pipe.mask2image_3mod_albedo(
        prompt_embeds=t["ehs"].to(dev).to(ehs_dtype), attr_latents=t["attr"].to(dev), latents=t["noise"],
        num_inference_steps=steps, guidance_scale=guidance, output_type="latent", eta=eta,
        generator=torch.Generator().manual_seed(3))


def _both(pipe, run, *a, **kw):
    """(on-device loop, its second call, step-by-step loop) as tuples of tensors"""
    tup = lambda x: x if isinstance(x, tuple) else (x,)
    pipe.use_fused_sampler = True
    n0 = len(pipe._sample_graphs)
    f1 = tup(run(pipe, *a, **kw))
    n1 = len(pipe._sample_graphs)
    f2 = tup(run(pipe, *a, **kw))
    assert len(pipe._sample_graphs) == n1 >= max(n0, 1)  # the second call re-uses the captured loop graph
    pipe.use_fused_sampler = False
    try:
        s = tup(run(pipe, *a, **kw))
    finally:
        pipe.use_fused_sampler = True
    return f1, f2, s


@pytest.mark.parametrize("guidance", [0.0, 2.0])
@pytest.mark.parametrize("name", ["ddim", "unipc", "sde-dpm++2m"])
def test_fused_view_loop_equals_step_by_step_view_loop(dev, rig, name, guidance):
    """Both directions, with the bounds tests/test_pipeline_gpu.py asserts for the same comparison without views: 2e-3 / 6e-3
    (guidance 0 / not) over several steps, 3e-3 / 8e-3 for UniPC, 1e-6 for one step -- the blend is the same launch on both
    sides, so it adds nothing to them."""
    pipe, _, _, t = rig
    eta = _attach(pipe, name)
    many = (3e-3 if guidance == 0 else 8e-3) if name == "unipc" else (2e-3 if guidance == 0 else 6e-3)
    edt = torch.float32 if name == "unipc" else torch.float16  # as the UniPC test of test_pipeline_gpu.py: fp32 prompt
    for run, steps in ((_inverse, 5), (_render, 4)):
        f1, f2, s = _both(pipe, run, t, dev, steps, guidance, eta, edt)
        key = list(pipe._sample_graphs)[-1]
        assert ("views", 2, 3, WINDOW, WINDOW, STRIDE, STRIDE) in key
        for x, y, z in zip(f1, f2, s):
            assert x.shape == (1, 4, H, W) and x.dtype == torch.float32 and bool(torch.isfinite(x).all())
            assert torch.equal(x, y)
            print(name, guidance, run.__name__, steps, "steps: fused vs step-by-step rel_l2", rel_l2(x, z), "bound", many)
            assert rel_l2(x, z) < many, (run.__name__, rel_l2(x, z))
        f1, _, s = _both(pipe, run, t, dev, 1, guidance, eta, edt)
        for x, z in zip(f1, s):
            print(name, guidance, run.__name__, "1 step: rel_l2", rel_l2(x, z))
            assert rel_l2(x, z) < 1e-6, (run.__name__, rel_l2(x, z))


def _plain_oracle_inverse(models, t, steps, kind):
    unet_o, enc_o, dec_o = models
    sched = {n: OracleScheduler(kind, steps) for n in GROUPS}
    lat = {n: t["noise"].clone() for n in GROUPS}
    for ts in sched["material"].timesteps:
        cond = torch.cat([t["mask"]] + [lat[n] for n in GROUPS], 1)
        out = O.dual_stream_step(unet_o, enc_o, dec_o, t["img"], cond, t["ehs"], torch.zeros(1).long(), ts.expand(1))
        for k, n in enumerate(GROUPS):
            lat[n] = sched[n].step(out["attr_pred"][:, 4 + 4 * k:8 + 4 * k], ts, lat[n])[0]
    return lat


@pytest.mark.parametrize("kind,steps,bound", [("ddim", 3, 1e-2), ("unipc", 6, 1.5e-2)])
def test_view_loops_match_the_oracle_panorama_loop(dev, rig, kind, steps, bound):
    """The literal Panorama loop on the CPU oracle (views one at a time, one scheduler per (view, group), value / count) with
    the bounds test_pipeline_gpu.py asserts for the plain loops against the plain oracle loop (1e-2 DDIM over 3 steps, 1.5e-2
    UniPC over 6); the plain loop on the same 24 x 32 inputs is measured here as the yardstick."""
    pipe, nets, models, t = rig
    _attach(pipe, kind)
    views = R.windows(H, W, WINDOW, STRIDE)
    ref, _ = R.panorama_inverse(models, t["img"], t["mask"], t["ehs"], t["noise"], steps, views, kind)
    for fused in (True, False):
        pipe.use_fused_sampler = fused
        out = _inverse(pipe, t, dev, steps, 0.0)
        pipe.use_fused_sampler = True
        got = [rel_l2(o, ref[n]) for o, n in zip(out, GROUPS)]
        print(kind, "fused" if fused else "step-by-step", "view loop vs oracle Panorama loop:", max(got), "bound", bound)
        assert max(got) < bound, got
    plain = _new_pipe(nets)
    _attach(plain, kind)
    yard = _plain_oracle_inverse(models, t, steps, kind)
    pl = max(rel_l2(o, yard[n]) for o, n in zip(_inverse(plain, t, dev, steps, 0.0), GROUPS))
    print(kind, "plain loop vs plain oracle loop on the same inputs (yardstick):", pl)
    assert pl < bound
    if kind == "ddim":  # rendering direction, and guidance on the inverse one
        refr = R.panorama_render(models, t["attr"], t["ehs"], t["noise"], steps, views, kind)
        got = rel_l2(_render(pipe, t, dev, steps, 0.0), refr)
        print("rendering view loop vs oracle Panorama loop:", got)
        assert got < bound
        refg, _ = R.panorama_inverse(models, t["img"], t["mask"], t["ehs"], t["noise"], steps, views, kind, guidance=2.0)
        got = [rel_l2(o, refg[n]) for o, n in zip(_inverse(pipe, t, dev, steps, 2.0), GROUPS)]
        print("guided view loop vs oracle Panorama loop:", max(got))
        assert max(got) < bound, got


def test_views_interact(dev, rig):
    """The same windows sampled WITHOUT the blend (the six crops as a plain batch of six) end somewhere else: rel-L2 > 1e-2 (on
    the CPU oracle, these inputs and 3 DDIM steps: 0.260 with ``util_multidiffusion.panorama_inverse(blend=False)``; the
    pipeline on the MI355X: 0.260).  A blend that does nothing fails here."""
    from uni_renderer_amd.multidiffusion import gather_views, view_geometry

    pipe, nets, _, t = rig
    _attach(pipe, "ddim")
    geo = view_geometry(H, W, WINDOW, STRIDE)
    crops = {k: gather_views(t[k], geo) for k in ("img", "mask", "noise")}
    plain = _new_pipe(nets)
    alone = _inverse(plain, t, dev, 3, 0.0, **crops)
    for fused in (True, False):
        pipe.use_fused_sampler = fused
        out = _inverse(pipe, t, dev, 3, 0.0)
        pipe.use_fused_sampler = True
        d = [rel_l2(gather_views(o, geo), a) for o, a in zip(out, alone)]
        print("blended views vs the same windows alone:", d)
        assert alone[0].shape == (6, 4, WINDOW, WINDOW) and min(d) > 1e-2, d


def test_switch_off_and_single_window_are_todays_path_and_make_no_launch(dev, rig, monkeypatch):
    from uni_renderer_amd import ops

    pipe, nets, _, t = rig
    small = {k: v[:, :, :16, :16].contiguous() for k, v in t.items() if k != "ehs"}
    never, other = _new_pipe(nets), _new_pipe(nets)

    def refuse(*a, **k):
        raise AssertionError("view_blend launched for a call without views")

    monkeypatch.setattr(ops, "view_blend", refuse)
    for fused in (True, False):
        never.use_fused_sampler = other.use_fused_sampler = fused
        for guidance in (0.0, 2.0):
            ref = _inverse(never, t, dev, 3, guidance, **small) + (_render(never, t, dev, 3, guidance, **small),)
            keys = set(never._sample_graphs), set(never._graphs)
            other.enable_multidiffusion(window_size=WINDOW, stride=STRIDE)
            one = _inverse(other, t, dev, 3, guidance, **small) + (_render(other, t, dev, 3, guidance, **small),)  # 16 x 16: a single window
            other.disable_multidiffusion()
            off = _inverse(other, t, dev, 3, guidance, **small) + (_render(other, t, dev, 3, guidance, **small),)
            assert all(torch.equal(a, b) for a, b in zip(ref, off)) and all(torch.equal(a, b) for a, b in zip(ref, one))
            assert (set(other._sample_graphs), set(other._graphs)) == keys  # no graph key changes


def test_view_batch_size_chunks_the_step_by_step_loop(dev, rig):
    """``view_batch_size=2``: three network calls of two views (four rows under guidance) per step instead of one of six; the
    blend is the same.  Bound: the 4e-3 of test_repeat_averaging_folds_into_one_batch (another batch size picks other tiles)."""
    pipe, _, _, t = rig
    _attach(pipe, "ddim")
    pipe.use_fused_sampler = False
    try:
        for guidance in (0.0, 2.0):
            pipe.enable_multidiffusion(window_size=WINDOW, stride=STRIDE)
            whole = _inverse(pipe, t, dev, 3, guidance) + (_render(pipe, t, dev, 3, guidance),)
            pipe.enable_multidiffusion(window_size=WINDOW, stride=STRIDE, view_batch_size=2)
            n0 = len(pipe._graphs)
            part = _inverse(pipe, t, dev, 3, guidance) + (_render(pipe, t, dev, 3, guidance),)
            assert len(pipe._graphs) > n0  # step graphs for the chunk's batch size
            for a, b in zip(whole, part):
                print("view_batch_size 2 vs all views, guidance", guidance, rel_l2(b, a))
                assert rel_l2(b, a) < 4e-3, rel_l2(b, a)
    finally:
        pipe.use_fused_sampler = True
        pipe.enable_multidiffusion(window_size=WINDOW, stride=STRIDE)


def test_the_geometry_is_part_of_the_sampling_graph_key(dev, rig):
    pipe, _, _, t = rig
    _attach(pipe, "ddim")
    pipe.use_fused_sampler = True
    a = _render(pipe, t, dev, 2, 0.0)
    n0 = len(pipe._sample_graphs)
    try:
        pipe.enable_multidiffusion(window_size=WINDOW, stride=4)  # 3 x 5 = 15 views
        b = _render(pipe, t, dev, 2, 0.0)
        assert len(pipe._sample_graphs) == n0 + 1 and rel_l2(b, a) > 1e-3
    finally:
        pipe.enable_multidiffusion(window_size=WINDOW, stride=STRIDE)
    c = _render(pipe, t, dev, 2, 0.0)
    assert len(pipe._sample_graphs) == n0 + 1 and torch.equal(a, c)  # back: the old graph, the old bits
