#!/usr/bin/env python3
"""FreeU off / on: captured-step time (bench.py's networks and inputs, alternated) and per-launch kernel time against the
one-launch GroupNorm at the same maps.  MODE=kernels runs only the isolated launches (for a rocprofv3 kernel trace)."""
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bench  # noqa: E402
from ab_gemm import time_graph  # noqa: E402
from uni_renderer_amd import ops  # noqa: E402
from uni_renderer_amd.graph import GraphedDualStreamStep  # noqa: E402

SD14 = dict(s1=0.9, s2=0.2, b1=1.2, b2=1.4)


def kernels(dev, dt, B=4, timed=True):
    rows = []
    for hw, ch, cs in [(8, 1280, 1280), (16, 1280, 1280), (16, 1280, 640), (32, 640, 640), (32, 640, 320)]:
        x = torch.randn(B, hw, hw, ch, device=dev).to(dt)
        x.lo = ops.lo_encode(torch.randn(B, hw, hw, ch, device=dev) * 1e-4, dt)
        sk = torch.randn(B, hw, hw, cs, device=dev).to(dt)
        sk.lo = ops.lo_encode(torch.randn(B, hw, hw, cs, device=dev) * 1e-4, dt)
        g, b = torch.randn(ch + cs, device=dev), torch.randn(ch + cs, device=dev)
        f_free = lambda: ops.freeu(x, sk, 1.0, 0.9, out=sk)  # b = 1: repeated in-place launches stay finite
        f_gn = lambda: ops.groupnorm(x, g, b, 1e-5, x1=sk, silu=True, fused=True)
        if timed:
            rows.append(dict(hw=hw, ch=ch, cs=cs, B=B, freeu_us=round(time_graph(f_free), 2), groupnorm_fused_us=round(time_graph(f_gn), 2)))
            print(json.dumps(rows[-1]), flush=True)
        else:
            for _ in range(5):
                f_free()
                f_gn()
            torch.cuda.synchronize()
    return rows


def step_ab(dev, dt, rounds=4, steps=30):
    models = bench.build_models(dev, dt)
    inputs = bench.make_inputs(4, 64, dev, dt, seed=100)
    runners = {}
    for name in ("off", "on"):
        models[0].enable_freeu(**SD14) if name == "on" else models[0].disable_freeu()
        r = GraphedDualStreamStep(*models, batch=4, latent_hw=64, cross_dim=768, dtype=dt, device=dev)
        r.load_inputs(*inputs)
        r.capture()
        runners[name] = r
    models[0].disable_freeu()
    ts = {"off": [], "on": []}
    for _ in range(rounds):
        for name, r in runners.items():
            for _ in range(5):
                r.replay()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                r.replay()
            torch.cuda.synchronize()
            ts[name].append(1e3 * (time.perf_counter() - t0) / steps)
    out = {k: dict(ms_per_step_median=round(statistics.median(v), 4), all=[round(t, 4) for t in v]) for k, v in ts.items()}
    d = (runners["on"].out["img_pred"].float() - runners["off"].out["img_pred"].float()).norm() / runners["off"].out["img_pred"].float().norm()
    out["img_pred_on_vs_off_rel_l2"] = float(d)
    out["attr_pred_equal"] = bool(torch.equal(runners["on"].out["attr_pred"], runners["off"].out["attr_pred"]))
    print(json.dumps(dict(captured_step_B4_512sq_fp16=out)), flush=True)


if __name__ == "__main__":
    dev, dt = torch.device("cuda:0"), torch.float16
    if os.environ.get("MODE") == "kernels":
        kernels(dev, dt, timed=False)
    else:
        kernels(dev, dt)
        step_ab(dev, dt)
