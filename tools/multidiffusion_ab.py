#!/usr/bin/env python3
"""MultiDiffusion views (``enable_multidiffusion``) measured: SD-1.x sized networks of bench.py, fp16, guidance 0, DDIM, one box,
one session.  One JSON line per measurement; ``all`` holds every repetition so that the reader sees the spread.

MODE=kernel  the blend launch alone at [9, 24, 64, 64] (window 64, stride 32 on 128 x 128) and [81, 24, 64, 64] (stride 8),
             against the torch composition of the same arithmetic (V slice-adds, a division, V gathers into master and the
             latent slice) and against a copy of the bytes it moves -- each captured into a graph of 20 and replayed;
MODE=views   the 50-step inverse and rendering loop on ONE 1024 x 1024 image (a 128 x 128 latent): natively, with nine views
             (stride 32) fused and step by step, with 81 views (stride 8; STRIDE8=0 skips it) -- time and peak memory;
MODE=off     the 512 x 512 loops (B = 4) with the switch off -- runs on a tree without the feature too (UR_TREE=<the parent's
             checkout>, built): the only performance condition of the feature is that this equals the parent;
MODE=all     (default) kernel, views, off."""
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROOT = os.environ.get("UR_TREE", ROOT)  # another (built) checkout of the package: the A side of an A/B against the parent commit
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import uni_renderer_amd  # noqa: E402  (first: ab_gemm puts its own tree in front of the path)
from uni_renderer_amd import ops  # noqa: E402
from uni_renderer_amd.pipeline import UniRendererPipeline  # noqa: E402
import bench  # noqa: E402
from ab_gemm import time_graph  # noqa: E402


def out(**row):
    print(json.dumps(row), flush=True)


def kernel(dev, dt):
    from uni_renderer_amd.multidiffusion import cover_count, view_geometry

    for stride in (32, 8):
        geo = view_geometry(128, 128, 64, stride)
        V, C = geo.num_views, 24
        for halves in (1, 2):
            master = torch.randn(V, C, 64, 64, device=dev)
            buf = torch.zeros(halves * V, 28, 64, 64, device=dev, dtype=dt)
            lat = buf[:, 4:]
            glob = torch.zeros(1, C, 128, 128, device=dev)
            count = cover_count(geo, dev)
            views = geo.views

            def composed():  # the same arithmetic in torch: V slice-adds, one division, V gathers (+ the casts into the slice)
                glob.zero_()
                for v, (h0, h1, w0, w1) in enumerate(views):
                    glob[:, :, h0:h1, w0:w1] += master[v]
                glob.div_(count)
                for v, (h0, h1, w0, w1) in enumerate(views):
                    master[v].copy_(glob[0, :, h0:h1, w0:w1])
                for h in range(halves):
                    lat[h * V:(h + 1) * V].copy_(master)

            src, dst = torch.empty_like(master), torch.empty_like(master)
            lsrc = torch.zeros(halves * V, C, 64, 64, device=dev, dtype=dt)

            def copy_bytes():  # what the launch moves: master read and written, the latent slice written, global written
                dst.copy_(src)
                lat.copy_(lsrc)
                glob.copy_(glob2)

            glob2 = torch.zeros_like(glob)
            row = dict(measure="blend_alone", shape=[V, C, 64, 64], stride=stride, halves=halves, max_cover=geo.max_cover,
                       bytes=int(2 * master.numel() * 4 + lat.numel() * 2 + glob.numel() * 4))
            row["view_blend_us"] = round(time_graph(lambda: ops.view_blend(master, lat, glob, geo, halves=halves, round_master=True)), 2)
            row["torch_composition_us"] = round(time_graph(composed), 2)
            row["torch_launches"] = 2 * V + 2 + halves
            row["copy_of_its_bytes_us"] = round(time_graph(copy_bytes), 2)
            out(**row)


def timed(fn, reps):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    fn()  # capture + warm
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(1e3 * (time.perf_counter() - t0))
    return dict(ms_median=round(statistics.median(ts), 2), ms_min=round(min(ts), 2), ms_max=round(max(ts), 2),
                all=[round(t, 2) for t in ts], peak_mem_gb=round(torch.cuda.max_memory_allocated() / 2 ** 30, 2))


def inputs(dev, dt, B, L):
    g = torch.Generator(device=dev).manual_seed(3)
    return dict(img=torch.randn(B, 4, L, L, device=dev, generator=g).to(dt), msk=torch.randn(B, 4, L, L, device=dev, generator=g).to(dt),
                ehs=(torch.randn(B, 77, 768, device=dev, generator=g) * 0.5).to(dt),
                attr=torch.randn(B, 28, L, L, device=dev, generator=g).to(dt))


def calls(pipe, t, steps):
    return (("inverse", lambda: pipe.real_image2mask_3mod_albedo(prompt_embeds=t["ehs"], image_latents=t["img"], mask_latents=t["msk"],
                                                                 num_inference_steps=steps, guidance_scale=0.0, output_type="latent")),
            ("render", lambda: pipe.mask2image_3mod_albedo(prompt_embeds=t["ehs"], attr_latents=t["attr"], num_inference_steps=steps,
                                                           guidance_scale=0.0, output_type="latent")))


def views(pipe, dev, dt, steps=50):
    t = inputs(dev, dt, 1, 128)
    configs = [("native_1024", None, True, 3), ("views9_stride32", 32, True, 3), ("views9_stride32", 32, False, 3)]
    if os.environ.get("STRIDE8", "1") != "0":
        configs += [("views81_stride8", 8, True, 2), ("views81_stride8", 8, False, 1)]
    for name, stride, fused, reps in configs:
        if stride is None:
            pipe.disable_multidiffusion()
        else:
            pipe.enable_multidiffusion(window_size=64, stride=stride)
        pipe.use_fused_sampler = fused
        for direction, fn in calls(pipe, t, steps):
            try:
                out(measure="loop_1024", loop=f"{direction}_{steps}", config=name, fused=fused, **timed(fn, reps))
            except (RuntimeError, torch.cuda.OutOfMemoryError) as e:  # does not fit: say so instead of a number
                out(measure="loop_1024", loop=f"{direction}_{steps}", config=name, fused=fused, error=str(e)[:200])
        pipe.invalidate_graphs()  # the next configuration's graphs and pools start from an empty pipeline
        torch.cuda.empty_cache()
    pipe.disable_multidiffusion()
    pipe.use_fused_sampler = True


def off(pipe, dev, dt, steps=50, reps=5):
    t = inputs(dev, dt, 4, 64)
    pipe.use_fused_sampler = True
    for direction, fn in calls(pipe, t, steps):
        out(measure="loop_512_switch_off", package=os.path.dirname(uni_renderer_amd.__file__), loop=f"{direction}_{steps}", **timed(fn, reps))


if __name__ == "__main__":
    dev, dt = torch.device("cuda:0"), torch.float16
    mode = os.environ.get("MODE", "all")
    if mode in ("kernel", "all"):
        kernel(dev, dt)
    if mode in ("views", "off", "all"):
        unet, enc, dec = bench.build_models(dev, dt)
        pipe = UniRendererPipeline(unet=unet, controlnet=enc, controldec=dec)
        pipe.set_progress_bar_config(disable=True)
        if mode in ("off", "all"):
            off(pipe, dev, dt)
        if mode in ("views", "all"):
            pipe.invalidate_graphs()
            views(pipe, dev, dt)
