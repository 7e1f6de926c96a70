#!/usr/bin/env python3
"""The measurements behind ``training_utils.EMAModel`` (profiles/ema_ab.txt).

MODE=update (default)  the whole EMA update of the fp32 masters of the three SD-1.x sized networks of bench.py, one process:
    * ``EMAModel.step`` (ur_ema_advance + ur_ema_multi) launched from Python, and the same as one HIP-graph replay;
    * the per-parameter torch loop as diffusers 0.24 writes it, ``s.sub_(one_minus_decay * (s - p))``;
    * its ``torch._foreach_sub`` / ``_foreach_mul_`` / ``_foreach_sub_`` form;
    every arm as a host clock around the update and a device synchronise, and the achieved bytes per second against the
    12 B per parameter the update needs.
MODE=steps  the cfg-4 graphed training step (tools/train_bench.py --graph) in processes of their own, alternating: this tree
    without and with ``--ema`` and, if ``UR_PARENT_TREE`` names a built checkout of the parent commit, that tree (twice per
    round: the spread between two processes of one tree).  Starts one process at a time and stops at the first that fails.
One JSON line per measurement; ``all`` holds every repetition so that the reader sees the spread."""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COPY_RATE = 6.3e12  # bytes / s a float4 copy achieves on one MI355X (8.0 TB/s HBM3E peak by the data sheet)


def _stats(name, ts, nbytes=None, **extra):
    row = dict(arm=name, ms_median=round(statistics.median(ts), 3), ms_min=round(min(ts), 3), ms_max=round(max(ts), 3),
               all=[round(t, 3) for t in ts], **extra)
    if nbytes is not None:
        rate = nbytes / (statistics.median(ts) * 1e-3)
        row.update(tb_per_s_at_12B_per_param=round(rate / 1e12, 3), share_of_copy_rate=round(rate / COPY_RATE, 3))
    print(json.dumps(row), flush=True)


def update(reps=10):
    import torch

    sys.path.insert(0, ROOT)
    import bench
    from uni_renderer_amd import EMAModel

    dev = torch.device("cuda:0")
    nets = bench.build_models(dev, torch.float32)
    for m in nets:
        m.requires_grad_(True)
    params = [p for m in nets for p in m.parameters()]
    n = sum(p.numel() for p in params)
    ema = EMAModel(params)
    ema.optimization_step = 1000  # a decay in (0, 1): the arithmetic does not depend on it, the torch arms get the same value
    omd = 1.0 - ema.get_decay(1001)
    shadows = [s.clone() for s in ema.shadow_params]
    with torch.no_grad():
        for p in params:  # the parameters moved since the shadows were taken (values do not change the time; NaN / denormals would)
            p.mul_(1.001)
    print(json.dumps(dict(tensors=len(params), parameters=n, launches=1 + -(-len(params) // 64), bytes_at_12B=12 * n,
                          ms_at_copy_rate=round(12 * n / COPY_RATE * 1e3, 3),
                          aligned_16B=sum(p.data_ptr() % 16 == 0 for p in params))), flush=True)

    def timed(fn):
        for _ in range(2):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append(1e3 * (time.perf_counter() - t0))
        return ts

    @torch.no_grad()
    def loop():
        for s, p in zip(shadows, params):
            s.sub_(omd * (s - p))

    @torch.no_grad()
    def foreach():
        t = torch._foreach_sub(shadows, params)
        torch._foreach_mul_(t, omd)
        torch._foreach_sub_(shadows, t)

    ema.step(params)  # builds the item tables
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ema.step(params)
    for rnd in range(3):  # arms alternate: a drift of the box shows as a drift of every arm
        _stats("EMAModel.step eager", timed(lambda: ema.step(params)), 12 * n, round=rnd)
        _stats("EMAModel.step graph replay", timed(graph.replay), 12 * n, round=rnd)
        _stats("torch loop (diffusers 0.24)", timed(loop), 12 * n, round=rnd, bytes_it_moves=20 * n)
        _stats("torch._foreach form", timed(foreach), 12 * n, round=rnd, bytes_it_moves=20 * n)
    print(json.dumps(dict(peak_mem_gb=round(torch.cuda.max_memory_allocated() / 2**30, 1))), flush=True)


def steps(rounds=3, n_steps=10):
    parent = os.environ.get("UR_PARENT_TREE")
    arms = [("here", ROOT, []), ("here --ema", ROOT, ["--ema"])]
    if parent:
        arms = [("parent", parent, []), ("parent again", parent, [])] + arms
    results = {name: [] for name, _, _ in arms}
    for rnd in range(rounds):
        for name, tree, extra in arms:
            cmd = [sys.executable, os.path.join(tree, "tools", "train_bench.py"), "--graph", "--steps", str(n_steps)] + extra
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=420, cwd=tree)
            if r.returncode != 0:
                print(json.dumps(dict(arm=name, round=rnd, failed=r.returncode, stderr=r.stderr[-2000:])), flush=True)
                raise SystemExit(1)  # nothing more is started after a failure
            row = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
            results[name].append(row["ms_per_step"])
            print(json.dumps(dict(arm=name, round=rnd, ms_per_step=row["ms_per_step"], loss=row["loss"], peak_mem_gb=row["peak_mem_gb"],
                                  phase_ms=row["phase_ms"], ema=row.get("ema"))), flush=True)
    for name, ts in results.items():
        _stats(name, ts)


if __name__ == "__main__":
    if os.environ.get("MODE", "update") == "steps":
        steps(rounds=int(os.environ.get("ROUNDS", "3")))
    else:
        update(reps=int(os.environ.get("REPS", "10")))
