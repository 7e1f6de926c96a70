#!/usr/bin/env python3
"""Sampling loops with the samplers of ``ur_sde_update`` against the deterministic ones (tools/loop_bench.py's setting: the
SD-1.x sized networks of bench.py, B = 4, 64 x 64 latents, 50 steps, guidance 0, fp16), fused and step by step, and the update
kernel alone against ``ur_unipc_update``.

MODE=loops   (default) every sampler, fused and step by step;
MODE=ddim0   only DDIM eta = 0, fused -- runs on a tree without the new samplers too (the parent of this change);
MODE=kernels only the isolated update launches.
One JSON line per measurement; ``all`` holds every repetition so that the reader sees the spread."""
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROOT = os.environ.get("UR_TREE", ROOT)  # another (built) checkout of the package: the A side of an A/B against an older commit
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bench  # noqa: E402
from ab_gemm import time_graph  # noqa: E402
from uni_renderer_amd import ops, schedulers as S  # noqa: E402
from uni_renderer_amd.pipeline import SCHEDULER_NAMES, UniRendererPipeline  # noqa: E402

SD = dict(prediction_type="sample", beta_schedule="scaled_linear", beta_start=0.00085, beta_end=0.012)


def samplers(mode):
    yield "ddim_eta0", (lambda: S.DDIMScheduler()), 0.0
    if mode == "ddim0":
        return
    yield "unipc", (lambda: S.UniPCMultistepScheduler()), 0.0
    yield "ddim_eta1", (lambda: S.DDIMScheduler()), 1.0
    yield "ddpm", (lambda: S.DDPMScheduler(steps_offset=1, **SD)), 0.0
    yield "dpmpp_2m", (lambda: S.DPMSolverMultistepScheduler(**SD)), 0.0
    yield "sde_dpmpp_2m", (lambda: S.DPMSolverMultistepScheduler(algorithm_type="sde-dpmsolver++", **SD)), 0.0


def loops(dev, dt, mode, B=4, L=64, steps=50, reps=5):
    unet, enc, dec = bench.build_models(dev, dt)
    pipe = UniRendererPipeline(unet=unet, controlnet=enc, controldec=dec)
    pipe.set_progress_bar_config(disable=True)
    g = torch.Generator(device=dev).manual_seed(3)
    img = torch.randn(B, 4, L, L, device=dev, generator=g).to(dt)
    msk = torch.randn(B, 4, L, L, device=dev, generator=g).to(dt)
    ehs = (torch.randn(B, 77, 768, device=dev, generator=g) * 0.5).to(dt)
    attr = torch.randn(B, 28, L, L, device=dev, generator=g).to(dt)
    for name, make, eta in samplers(mode):
        for n in SCHEDULER_NAMES:
            setattr(pipe, f"scheduler_{n}", make())
        extra = dict(eta=eta) if eta else {}
        calls = (("inverse", lambda: pipe.real_image2mask_3mod_albedo(prompt_embeds=ehs, image_latents=img, mask_latents=msk,
                                                                      num_inference_steps=steps, guidance_scale=0.0,
                                                                      output_type="latent", **extra)),
                 ("render", lambda: pipe.mask2image_3mod_albedo(prompt_embeds=ehs, attr_latents=attr, num_inference_steps=steps,
                                                                guidance_scale=0.0, output_type="latent", **extra)))
        for fused in ((True,) if mode == "ddim0" else (True, False)):
            pipe.use_fused_sampler = fused
            for direction, fn in calls:
                fn()  # capture + warm
                torch.cuda.synchronize()
                ts = []
                for _ in range(reps):
                    t0 = time.perf_counter()
                    fn()
                    torch.cuda.synchronize()
                    ts.append(1e3 * (time.perf_counter() - t0))
                print(json.dumps(dict(loop=f"{direction}_{steps}", sampler=name, fused=fused, ms_median=round(statistics.median(ts), 2),
                                      ms_min=round(min(ts), 2), ms_max=round(max(ts), 2), all=[round(t, 2) for t in ts])), flush=True)
        pipe.use_fused_sampler = True


def kernels(dev, dt, timed=True):
    for shape in ((4, 24, 64, 64), (4, 4, 64, 64)):
        B, C, H, W = shape
        n = 50
        pred = torch.randn(B, H, W, 28, device=dev).to(dt)
        lat = torch.zeros(B, 28, H, W, device=dev, dtype=dt)[:, 4:4 + C]
        step = torch.zeros(1, dtype=torch.int32, device=dev)
        seed = torch.tensor([12345], dtype=torch.int64, device=dev)
        master, last, hist1 = (torch.randn(B, C, H, W, device=dev) for _ in range(3))
        hist2 = torch.zeros(2, B, C, H, W, device=dev)
        tab = lambda pn: torch.tensor([[0.9, 0.2, -0.1, pn]] * n, device=dev)
        tab8 = torch.tensor([[0.9, 0.1, 0.0, 0.0, 0.9, 0.2, -0.1, 0.0]] * n, device=dev)
        fns = dict(sde_update_with_noise=lambda: ops.sde_update(pred, 4, lat, tab_n, step, n, seed, master, hist1),
                   sde_update_pn0=lambda: ops.sde_update(pred, 4, lat, tab_0, step, n, seed, master, hist1),
                   unipc_update=lambda: ops.unipc_update(pred, 4, lat, tab8, step, n, last, master, hist2),
                   sampler_noise=lambda: ops.sampler_noise(seed, 3, shape, out=hist1))
        tab_n, tab_0 = tab(0.5), tab(0.0)
        row = dict(shape=list(shape), dtype=str(dt))
        for k, f in fns.items():
            if timed:
                row[k + "_us"] = round(time_graph(f), 2)
            else:
                for _ in range(5):
                    f()
                torch.cuda.synchronize()
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    dev, dt = torch.device("cuda:0"), torch.float16
    mode = os.environ.get("MODE", "loops")
    if mode == "kernels":
        kernels(dev, dt)
    else:
        loops(dev, dt, mode)
        if mode == "loops":
            kernels(dev, dt)
