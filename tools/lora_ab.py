#!/usr/bin/env python3
"""LoRA merge at SD-1.x UNet size, fp16, adapter on every attention and feed-forward projection, rank 4 / 16 / 64 / 128:
  (a) the grouped merge alone: the launches of ur_lora_merge_multi over all items from item tables built beforehand, ms and
      GB/s against 2 x the bytes of the adapted weights -- and, beside it, the same through lora.merge_items, which also
      builds the tables (Python + ctypes, host time that may or may not hide behind the kernels);
  (b) the same merge written in torch, per layer: fp32 addmm of the factors onto base, then a cast-and-copy into the weight;
  (c) a whole scale switch as a user sees it: one pipeline call of one step at a NEW scale (merge + repacking + graph
      re-capture + the step) against the same call repeated at the scale already merged.
(a) and (b) are alternated in one process; medians of REPS runs after WARM warm-up runs, timed with HIP events on the stream."""
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from uni_renderer_amd import lora  # noqa: E402
from uni_renderer_amd.pipeline import UniRendererPipeline  # noqa: E402

KINDS = ("attn1.to_q", "attn1.to_k", "attn1.to_v", "attn1.to_out.0", "attn2.to_q", "attn2.to_k", "attn2.to_v", "attn2.to_out.0",
         "ff.net.0.proj", "ff.net.2")
WARM, REPS = 2, 9


def adapter(unet, rank, dev, seed=0):
    g = torch.Generator(device=dev).manual_seed(seed)
    sd = {}
    for n, m in unet.named_modules():
        if isinstance(m, torch.nn.Linear) and n.endswith(KINDS):
            N, K = m.weight.shape
            sd[n + ".lora.down.weight"] = torch.randn(rank, K, device=dev, generator=g) * K ** -0.5
            sd[n + ".lora.up.weight"] = torch.randn(N, rank, device=dev, generator=g) * 0.02
    return sd


def timed(fn):
    ts = []
    for i in range(WARM + REPS):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn(i)
        e1.record()
        torch.cuda.synchronize()
        if i >= WARM:
            ts.append(e0.elapsed_time(e1))
    return statistics.median(ts), min(ts), max(ts)


def merge_ab(unet, dev):
    for rank in (4, 16, 64, 128):
        unet.load_attn_procs(adapter(unet, rank, dev))
        st = unet._lora
        rows = []
        for name, (up, down, rscale) in st.assembled().items():
            rows.append((st.base[name], unet.get_submodule(name).weight.detach(), up, down, rscale))
        nbytes = 2 * sum(r[1].numel() * r[1].element_size() for r in rows)
        scales = (0.3, 1.0)

        from uni_renderer_amd import _lib
        from uni_renderer_amd.ops import _stream

        lib, dt = _lib.load(), _lib.ABI.UR_DT_F16
        tables = [lora.item_tables([r + (sc,) for r in rows], lora.multi_max()) for sc in scales]

        def grouped(i):  # launches only
            for table, k in tables[i % 2]:
                _lib.check(lib.ur_lora_merge_multi(table, k, dt, _stream()), "ur_lora_merge_multi")

        def grouped_call(i):  # what lora.py calls: tables built inside
            lora.merge_items([r + (scales[i % 2],) for r in rows], torch.float16)

        def torch_per_layer(i):
            s = scales[i % 2]
            for base, w, up, down, rscale in rows:
                w.copy_(torch.addmm(base.float(), up * rscale, down, alpha=s))

        a, c, b = timed(grouped), timed(grouped_call), timed(torch_per_layer)
        # the two agree to the fp16 rounding of the result (same scale on the last run of each)
        grouped(1)
        got = [r[1].clone() for r in rows[:8]]
        torch_per_layer(1)
        diff = max(float((g.float() - r[1].float()).abs().max() / r[1].float().abs().max()) for g, r in zip(got, rows))
        print(json.dumps(dict(rank=rank, items=len(rows), launches=-(-len(rows) // lora.multi_max()), adapted_weight_MB=round(nbytes / 2 / 2**20, 1),
                              grouped_ms=dict(median=round(a[0], 3), min=round(a[1], 3), max=round(a[2], 3)),
                              grouped_GBps=round(nbytes / a[0] / 1e6, 1),
                              merge_items_call_ms=dict(median=round(c[0], 3), min=round(c[1], 3), max=round(c[2], 3)),
                              torch_per_layer_ms=dict(median=round(b[0], 3), min=round(b[1], 3), max=round(b[2], 3)),
                              torch_over_grouped=round(b[0] / a[0], 2), max_rel_diff_first8=diff)), flush=True)
        for base, w, *_ in rows:  # the timed writes went around the model's bookkeeping: put base back by hand
            w.copy_(base)
        unet.unload_lora(keep_weights=True)


def switch(models, dev, rank=16, B=4, L=64):
    pipe = UniRendererPipeline(unet=models[0], controlnet=models[1], controldec=models[2])
    pipe.set_progress_bar_config(disable=True)
    g = torch.Generator(device=dev).manual_seed(3)
    kw = dict(prompt_embeds=(torch.randn(1, 77, 768, device=dev, generator=g) * 0.5).half(),
              attr_latents=torch.randn(B, 28, L, L, device=dev, generator=g), latents=torch.randn(B, 4, L, L, device=dev, generator=g),
              num_inference_steps=1, guidance_scale=0.0, output_type="latent")

    def call(scale):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pipe.mask2image_3mod_albedo(**kw, cross_attention_kwargs={"scale": scale})
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0)

    pipe.mask2image_3mod_albedo(**kw)  # everything captured once without an adapter
    pipe.load_lora_weights(adapter(models[0], rank, dev))
    call(1.0)
    new, same = [], []
    for s in (0.3, 0.8, 0.5, 1.0, 0.6):
        new.append(call(s))
        same.append(call(s))
    print(json.dumps(dict(scale_switch_rank=rank, batch=B, latent=L, steps=1,
                          call_at_new_scale_ms=dict(median=round(statistics.median(new), 1), all=[round(t, 1) for t in new]),
                          call_at_merged_scale_ms=dict(median=round(statistics.median(same), 1), all=[round(t, 1) for t in same]))), flush=True)
    pipe.unload_lora_weights()


if __name__ == "__main__":
    dev = torch.device("cuda:0")
    models = bench.build_models(dev, torch.float16)
    with torch.no_grad():
        merge_ab(models[0], dev)
        if os.environ.get("MODE") != "merge":
            switch(models, dev)
