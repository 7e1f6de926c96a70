#!/usr/bin/env python3
"""IP-Adapter A/B on one box, one session (SD-1.x sizes, B = 4, 512^2, fp16): writes profiles/ip_adapter_ab.txt.

  python tools/ip_adapter_ab.py [--parent DIR] [--out FILE]

1. ``ur_ip_attention_add`` at the four levels of the UNet (N = 4 image tokens), both thread mappings, against the same
   arithmetic in torch on the same tensors (the two projections excluded: SDPA over the N keys, scale, add) and against its own
   byte count over the copy rate measured for that byte count.
2. The captured grouped step and the 50-step rendering loop, adapter off and on, in child processes of this tree; with
   ``--parent DIR`` (a built checkout of the parent commit) the adapter-off numbers of the parent too, the processes alternated
   ``tree, parent, tree, parent``: the spread between the two processes of one tree is what a difference is read against.
   Every child also reports the launches of one eager grouped step and a checksum of the captured step's outputs.

``--child`` is the per-process half (prints one JSON line); it only uses what the parent commit has too unless ``--adapter``.
"""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEVELS = [(4096, 40), (1024, 80), (256, 160), (64, 160)]  # (tokens, head width) of the 64x64 .. 8x8 levels, 8 heads
CLIP_DIM, N_TOKENS, STD, SCALE = 1024, 4, 0.02, 1.0


def _adapter(unet, torch):
    """A random adapter in the original key layout (what tests/util_ip_adapter.ip_state_dict builds)."""
    from uni_renderer_amd.ip_adapter import attn_processor_ids

    g = torch.Generator().manual_seed(7)
    sd, mods = {}, dict(unet.named_modules())
    for i, path in attn_processor_ids(unet).items():
        if path.endswith("attn2"):
            inner, cross = mods[path].to_k.weight.shape
            for nm in ("to_k_ip", "to_v_ip"):
                sd[f"ip_adapter.{i}.{nm}.weight"] = torch.randn(inner, cross, generator=g) * STD
    sd["image_proj.proj.weight"] = torch.randn(N_TOKENS * cross, CLIP_DIM, generator=g) * CLIP_DIM ** -0.5
    sd["image_proj.proj.bias"] = torch.zeros(N_TOKENS * cross)
    sd["image_proj.norm.weight"], sd["image_proj.norm.bias"] = torch.ones(cross), torch.zeros(cross)
    return sd


def kernels(lines):
    import torch
    import torch.nn.functional as F

    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from ab_gemm import time_graph
    from uni_renderer_amd import ops

    dev, dt, B, H, N = torch.device("cuda:0"), torch.float16, 4, 8, N_TOKENS
    lines.append(f"1. ur_ip_attention_add, B = {B}, H = {H}, N = {N}, fp16; us per launch = median of 5 graph replays of 20 launches;")
    lines.append("   bytes = o read + o written + q read + k_ip / v_ip once per sample; copy = dst.copy_(src) moving the same bytes")
    lines.append("   (read + write), its rate measured in this session; torch = SDPA over the N keys + scale + add on the same tensors")
    for T, d in LEVELS:
        C = H * d
        g = torch.Generator(device=dev).manual_seed(T + d)
        rnd = lambda *s: torch.randn(*s, device=dev, generator=g).to(dt)
        o, q, k, v = rnd(B, T, C), rnd(B, T, C), rnd(B, N, C), rnd(B, N, C)
        nbytes = (3 * B * T * C + 2 * B * N * C) * 2
        src, dst = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev), torch.empty(nbytes // 2, dtype=torch.uint8, device=dev)
        kw = dict(B=B, H=H, T=T, d=d, ldq=C)
        ours = time_graph(lambda: ops.ip_attention_add(o, q, k, v, 1e-3, **kw))
        per_head = time_graph(lambda: ops.ip_attention_add(o, q, k, v, 1e-3, flags=ops.IPA_THREAD_PER_HEAD, **kw))
        # q carries d^-1/2 log2 e in the step; torch's SDPA applies d^-1/2 itself: same work
        split = lambda t: t.view(B, -1, H, d).transpose(1, 2)

        def torch_arith():
            ip = F.scaled_dot_product_attention(split(q), split(k), split(v))
            o.add_(ip.transpose(1, 2).reshape(B, T, C), alpha=1e-3)

        torch_arith()  # eager first: a backend that refuses the shape fails here, outside a capture
        torch.cuda.synchronize()
        tt = time_graph(torch_arith)
        cp = time_graph(lambda: dst.copy_(src))
        walks = {w: time_graph(lambda: ops.ip_attention_add(o, q, k, v, 1e-3, flags=w << ops.IPA_WALK_SHIFT, **kw)) for w in (1, 2, 4, 8, 16)}
        rate = nbytes / (cp * 1e-6) / 1e12
        lines.append(f"   T {T:5d} x C {C:4d} (d {d:3d})   lanes-per-head {ours:7.2f} us   thread-per-head {per_head:7.2f} us   "
                     f"torch {tt:7.2f} us ({tt / ours:4.1f}x)   copy of {nbytes / 1e6:6.2f} MB {cp:7.2f} us ({rate:4.2f} TB/s)   "
                     f"kernel / copy {ours / cp:4.2f}")
        lines.append("        groups walked per workgroup (the launcher's choice above): " + "   ".join(f"{w}: {t:.2f} us" for w, t in walks.items()))
    return lines


def child(adapter: bool):
    """One process: adapter-off captured step + rendering loop (+ the same with the adapter when ``adapter``)."""
    import torch

    sys.path.insert(0, os.getcwd())  # the tree this child was started in
    import bench
    from uni_renderer_amd import ops
    from uni_renderer_amd.fused import GroupedDualStreamStep
    from uni_renderer_amd.graph import GraphedDualStreamStep
    from uni_renderer_amd.pipeline import UniRendererPipeline

    dev, dt, B, L = torch.device("cuda:0"), torch.float16, 4, 64
    models = bench.build_models(dev, dt)
    inputs = bench.make_inputs(B, L, dev, dt, seed=100)
    res = {}

    def measure(tag, ip_kw):
        rec = []
        ops.profile_into(rec)
        with torch.no_grad():
            GroupedDualStreamStep(*models)(*inputs)
        ops.profile_into(None)
        torch.cuda.synchronize()
        r = GraphedDualStreamStep(*models, batch=B, latent_hw=L, cross_dim=768, dtype=dt, device=dev)
        r.load_inputs(*inputs)
        r.capture()
        ts = []
        for _ in range(4):
            for _ in range(5):
                r.replay()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(30):
                r.replay()
            torch.cuda.synchronize()
            ts.append(1e3 * (time.perf_counter() - t0) / 30)
        h = hashlib.sha256()
        for k in ("img_pred", "attr_pred"):
            h.update(r.out[k].contiguous().cpu().numpy().tobytes())
        res[tag] = dict(launches=len(rec), step_ms=[round(t, 4) for t in ts], step_ms_median=round(statistics.median(ts), 4),
                        outputs_sha256=h.hexdigest()[:16])
        pipe = UniRendererPipeline(unet=models[0], controlnet=models[1], controldec=models[2], **ip_kw.get("pipe", {}))
        pipe.set_progress_bar_config(disable=True)
        g = torch.Generator(device=dev).manual_seed(3)
        ehs = (torch.randn(B, 77, 768, device=dev, generator=g) * 0.5).to(dt)
        attr = torch.randn(B, 28, L, L, device=dev, generator=g).to(dt)
        noise = torch.randn(B, 4, L, L, device=dev, generator=g).to(dt)
        fn = lambda: pipe.mask2image_3mod_albedo(prompt_embeds=ehs, attr_latents=attr, latents=noise, num_inference_steps=50,
                                                 guidance_scale=0.0, output_type="latent", **ip_kw.get("call", {}))
        lat = fn()
        torch.cuda.synchronize()
        ls = []
        for _ in range(3):
            t0 = time.perf_counter()
            lat = fn()
            torch.cuda.synchronize()
            ls.append(time.perf_counter() - t0)
        res[tag].update(render50_ms=[round(1e3 * t, 2) for t in ls], render50_ms_best=round(1e3 * min(ls), 2),
                        render50_sha256=hashlib.sha256(lat.contiguous().cpu().numpy().tobytes()).hexdigest()[:16])

    measure("off", {})
    if adapter:
        import types

        class Enc(torch.nn.Module):  # stands in for the CLIP vision tower: fixed embeddings
            def __init__(self):
                super().__init__()
                self.w = torch.nn.Parameter(torch.randn(3 * 8 * 8, CLIP_DIM, generator=torch.Generator().manual_seed(3)) * 0.1)

            def forward(self, px):
                return types.SimpleNamespace(image_embeds=px.flatten(1) @ self.w)

        unet = models[0]
        unet._load_ip_adapter_weights(_adapter(unet, torch))
        unet.set_ip_adapter_scale(SCALE)
        px = torch.randn(1, 3, 8, 8, generator=torch.Generator().manual_seed(1))
        enc = Enc().to(dev).to(dt)
        with torch.no_grad():
            unet.set_ip_adapter_image_embeds(enc(px.to(dev).to(dt)).image_embeds.repeat(B, 1))
        measure("on", dict(pipe=dict(image_encoder=enc), call=dict(ip_adapter_image=px)))
        unet.unload_ip_adapter()
    print("AB_CHILD " + json.dumps(res), flush=True)


def run_child(tree, adapter):
    cmd = [sys.executable, os.path.abspath(__file__), "--child"] + (["--adapter"] if adapter else [])
    p = subprocess.run(cmd, cwd=tree, capture_output=True, text=True, timeout=900)
    for ln in p.stdout.splitlines():
        if ln.startswith("AB_CHILD "):
            return json.loads(ln[len("AB_CHILD "):])
    raise RuntimeError(f"child in {tree} failed (rc {p.returncode}):\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--adapter", action="store_true")
    ap.add_argument("--parent", default="", help="a built checkout of the parent commit")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ip_adapter_ab.txt"))
    a = ap.parse_args()
    if a.child:
        return child(a.adapter)
    sys.path.insert(0, ROOT)
    lines = ["IP-Adapter (ur_ip_attention_add, csrc/ipadapter.hip) -- one MI355X, one session, fp16, B = 4; tools/ip_adapter_ab.py", ""]

    def flush():
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")

    kernels(lines)
    flush()
    order = [("tree", ROOT, True)] + ([("parent", a.parent, False)] if a.parent else []) + [("tree", ROOT, True)] + \
            ([("parent", a.parent, False)] if a.parent else [])
    runs = []
    for name, tree, adapter in order:
        runs.append((name, run_child(tree, adapter)))
        print(name, json.dumps(runs[-1][1]), flush=True)
    lines += ["", "2. captured grouped step (bench.py's networks and inputs: enc + unet + dec, 512^2, B = 4; 4 x 30 replays, ms/step) and the",
              "   50-step rendering loop of the pipeline (mask2image_3mod_albedo, DDIM on the device, hoisted; 3 calls, ms/call), one",
              "   process per line, in the order run; launches = the wrappers' launches of one eager grouped step; sha = outputs"]
    for name, r in runs:
        for tag, v in r.items():
            lines.append(f"   {name:6s} adapter {tag:3s}  step {' '.join(f'{t:.4f}' for t in v['step_ms'])}  median {v['step_ms_median']:.4f}   "
                         f"render50 {' '.join(f'{t:.2f}' for t in v['render50_ms'])}  best {v['render50_ms_best']:.2f}   "
                         f"launches {v['launches']}   sha step {v['outputs_sha256']} loop {v['render50_sha256']}")
    tree_off = [r["off"] for n, r in runs if n == "tree"]
    par_off = [r["off"] for n, r in runs if n == "parent"]
    on = [r["on"] for n, r in runs if n == "tree" and "on" in r]
    med = lambda rs, k: [v[k] for v in rs]
    lines.append("")
    lines.append(f"   adapter off, this tree, two processes: step {med(tree_off, 'step_ms_median')} (spread "
                 f"{max(med(tree_off, 'step_ms_median')) - min(med(tree_off, 'step_ms_median')):.4f} ms), render50 {med(tree_off, 'render50_ms_best')} "
                 f"(spread {max(med(tree_off, 'render50_ms_best')) - min(med(tree_off, 'render50_ms_best')):.2f} ms)")
    if par_off:
        lines.append(f"   adapter off, parent commit, two processes: step {med(par_off, 'step_ms_median')} (spread "
                     f"{max(med(par_off, 'step_ms_median')) - min(med(par_off, 'step_ms_median')):.4f} ms), render50 {med(par_off, 'render50_ms_best')} "
                     f"(spread {max(med(par_off, 'render50_ms_best')) - min(med(par_off, 'render50_ms_best')):.2f} ms)")
        same = (len({v["launches"] for v in tree_off + par_off}) == 1, len({v["outputs_sha256"] for v in tree_off + par_off}) == 1,
                len({v["render50_sha256"] for v in tree_off + par_off}) == 1)
        lines.append(f"   adapter off vs parent: same launch count {same[0]}, captured step outputs bit-identical {same[1]}, "
                     f"50-step latents bit-identical {same[2]}")
    if on:
        d_step = statistics.mean(med(on, "step_ms_median")) - statistics.mean(med(tree_off, "step_ms_median"))
        d_loop = statistics.mean(med(on, "render50_ms_best")) - statistics.mean(med(tree_off, "render50_ms_best"))
        lines.append(f"   adapter on: step {med(on, 'step_ms_median')} ({d_step:+.4f} ms: {on[0]['launches'] - tree_off[0]['launches']} more launches), "
                     f"render50 {med(on, 'render50_ms_best')} ({d_loop:+.2f} ms per 50 steps)")
    flush()
    print("\n".join(lines))


if __name__ == "__main__":
    main()
