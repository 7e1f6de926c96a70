"""RCCL on the leased GPU (missing #2 / weak #11): the `nccl` backend with world_size 1 runs the same
collectives the 8-GPU job issues -- all-reduce, reduce-scatter + in-place all-gather, bf16 transport, the barrier and
max-reduce of bench.py -- on RCCL's own stream, so the stream ordering between the HIP kernels that produce the gradients
and the collectives that consume them is exercised for real (the gloo tests cannot).  Plus: `python bench.py --gpus 1`
and the self-spawn path (`--gpus N` with no launcher) start and print one JSON line."""
import json
import os
import socket
import subprocess
import sys

import pytest
import torch

from util_models import ROOT

pytestmark = pytest.mark.gpu

WORKER = r'''
import os, sys, json
import torch, torch.distributed as dist
sys.path.insert(0, os.environ["UR_ROOT"])
from uni_renderer_amd.parallel import GradientBuckets, init_distributed, max_over_ranks
rank, world, local = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"]), int(os.environ["LOCAL_RANK"])
dev = torch.device("cuda", local)
torch.cuda.set_device(dev)
dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
assert dist.get_backend() == "nccl"
out = {}
torch.manual_seed(0)
def net():
    torch.manual_seed(1)
    return torch.nn.Sequential(torch.nn.Linear(256, 512), torch.nn.SiLU(), torch.nn.Linear(512, 300), torch.nn.SiLU(),
                               torch.nn.Linear(300, 64)).to(dev)
x = torch.randn(64, 256, device=dev)
ref = net()
ref(x).square().mean().backward()
gref = [p.grad.clone() for p in ref.parameters()]
for algo in ("all_reduce", "rs_ag"):
    for comm in (None, torch.bfloat16):
        for overlap in (True, False):
            m = net()
            gb = GradientBuckets([m], bucket_mb=0.25, comm_dtype=comm, algorithm=algo, overlap=overlap, force_collectives=True)
            assert len(gb.buckets) >= 3
            for it in range(2):  # second iteration: buffers reused, hooks re-armed
                gb.zero_grad()
                m(x).square().mean().backward()
                gb.finish()
                torch.cuda.synchronize()
                err = max(float((p.grad - g).abs().max() / g.abs().max()) for p, g in zip(m.parameters(), gref))
                tol = 1e-6 if comm is None else 1e-2
                assert err < tol, (algo, comm, overlap, it, err)
            out[f"{algo}/{comm}/{overlap}"] = dict(err=err, from_hooks=gb.launched_from_hooks, buckets=len(gb.buckets))
            if overlap:
                assert gb.launched_from_hooks > 0  # the collectives were enqueued while autograd was still running
dist.barrier()
out["max_over_ranks"] = max_over_ranks(0.25, device=dev)
dist.destroy_process_group()
print("RESULT " + json.dumps(out))
'''


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_rccl_world1_collectives_of_the_gradient_buckets(tmp_path):
    script = tmp_path / "worker.py"
    script.write_text(WORKER)
    env = dict(os.environ, RANK="0", WORLD_SIZE="1", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()),
               UR_ROOT=ROOT, HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, str(script)], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    res = json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
    print(json.dumps(res))
    assert res["max_over_ranks"] == 0.25
    assert set(k.split("/")[0] for k in res if "/" in k) == {"all_reduce", "rs_ag"}


def test_bench_runs_with_the_drivers_command_line_and_spawns_its_own_ranks():
    """`python bench.py --gpus 1 ...` (the driver's N = 1 command) and, with no launcher around it, `--gpus N`: bench.py
    must start its own N ranks (here N = visible GPUs = 1 is the only N the box can run; the spawn path is the same code
    for every N and is exercised by forcing it through torch.distributed.run for N = 1)."""
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--no-cpu-baseline",
           "--no-roofline", "--batch", "1", "--latent", "16"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["n_gpus"] == 1 and line["steps"] == 3 and line["value"] > 0
    # more GPUs than the box has: a clear refusal, not a hang and not the old "launch with torch.distributed.run" exit
    n = torch.cuda.device_count() + 1
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(n), "--steps", "1", "--warmup", "0"], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and f"only {n - 1} GPU" in (r.stderr + r.stdout)
    # the launcher path with one rank over RCCL (what `--gpus N` spawns for N > 1)
    port = _free_port()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=1", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
           "--no-cpu-baseline", "--no-roofline", "--batch", "1", "--latent", "16"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert line["n_gpus"] == 1


def test_bench_line_carries_the_contract_fields_with_a_live_roofline():
    """One --full run (roofline on, live PMC traffic attempted, CPU baseline off for time) at a small configuration:
    the JSON line has every field of the bench contract, and the roofline object is self-consistent."""
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", TMPDIR="/tmp")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--steps", "3", "--warmup", "1", "--no-cpu-baseline",
           "--batch", "2", "--latent", "32"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=1200, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
              "dtype", "data", "config", "roofline"):
        assert k in line, k
    assert line["steps"] == 3 and line["warmup"] == 1 and line["n_gpus"] == 1 and line["higher_is_better"] is True
    assert line["scaling"] == "weak" and line["vs_baseline"] is None and "workload" in line["config"] and "model" not in line["config"]
    roof = line["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in roof, k
    assert roof["bound"] in ("hbm", "mfma") and abs(roof["frac"] - roof["achieved"] / roof["peak"]) < 1e-3
    if roof["traffic"] is not None:
        assert roof["traffic"] > 0 and roof["traffic_source"].startswith(("LIVE", "STATIC"))


def test_plain_bench_run_times_only_and_dumps_the_last_steps_outputs(tmp_path):
    """A plain run (no --full) prints the headline line without the --full legs, and --dump-outputs writes the last timed
    step's outputs as float32 .npy files: the same arrays on a second run with the same arguments."""
    import numpy as np

    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    got = []
    for run in ("a", "b"):
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "4", "--warmup", "1", "--batch", "2", "--latent", "16",
               "--dump-outputs", str(tmp_path / run)]
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-3000:]
        line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
        assert line["steps"] == 4 and line["ms_per_step"] > 0
        assert not {"roofline", "loop", "cpu_baseline", "kernel_classes"} & set(line)
        got.append({n: np.load(tmp_path / run / f"{n}.npy") for n in ("img_pred", "attr_pred")})
    assert sorted(os.listdir(tmp_path / "a")) == ["attr_pred.npy", "img_pred.npy"]
    for n, shape in (("img_pred", (2, 4, 16, 16)), ("attr_pred", (2, 28, 16, 16))):
        a, b = got[0][n], got[1][n]
        assert a.dtype == np.float32 and a.shape == shape and np.isfinite(a).all() and np.abs(a).max() > 0
        assert np.array_equal(a, b), n


GRAPH_WORKER = r'''
import os, sys, json
import torch, torch.distributed as dist
sys.path.insert(0, os.environ["UR_ROOT"]); sys.path.insert(0, os.path.join(os.environ["UR_ROOT"], "tests"))
from util_models import O, build_product_from_oracle
from uni_renderer_amd.optim import FusedAdamW
from uni_renderer_amd.parallel import GradientBuckets
from uni_renderer_amd.train_step import GraphedTrainStep, train_step
dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)

def setup(algo, comm, overlap):
    nets = build_product_from_oracle(*O.build_triplet(O.TINY_CONFIG, seed=44), torch.float32, dev)
    for m in nets:
        m.train(); m.requires_grad_(True)
    b = GradientBuckets(nets, bucket_mb=0.5, comm_dtype=comm, algorithm=algo, overlap=overlap, force_collectives=True)
    return nets, FusedAdamW([p for m in nets for p in m.parameters()], lr=2e-4), b

def batch(it):
    x, c, ehs, ti, ta = [t.to(dev) for t in O.make_inputs(2, 16, 64, seed=120 + it)]
    g = torch.Generator().manual_seed(121 + it)
    return dict(x_t=x, cond=c, ehs=ehs, t_img=ti, t_attr=ta, target_img=torch.randn(2, 4, 16, 16, generator=g).to(dev),
                target_attr=torch.randn(2, 28, 16, 16, generator=g).to(dev))

out = {}
for algo in ("all_reduce", "rs_ag"):
    for comm in (None, torch.bfloat16):
        nets_e, opt_e, b_e = setup(algo, comm, True)
        eager = [train_step(nets_e, batch(it), optimizer=opt_e, buckets=b_e, dtype=torch.bfloat16)["loss"] for it in range(3)]
        nets_s, opt_s, b_s = setup(algo, comm, False)           # forward + backward graph | eager collectives | update graph
        serial = GraphedTrainStep(nets_s, batch(0), opt_s, buckets=b_s, dtype=torch.bfloat16, warmup=0)
        assert not serial.capture_collectives
        ls = [float(serial.step(batch(it))["loss"]) for it in range(3)]
        nets_g, opt_g, b_g = setup(algo, comm, True)             # ONE graph, collectives captured as parallel branches
        assert len(b_g.buckets) >= 3
        fused = GraphedTrainStep(nets_g, batch(0), opt_g, buckets=b_g, dtype=torch.bfloat16, warmup=0)
        assert fused.capture_collectives and fused.g_up is None
        lg = [float(fused.step(batch(it))["loss"]) for it in range(3)]
        torch.cuda.synchronize()
        same = all(torch.equal(a, b) and torch.equal(a, c) for a, b, c in zip((p for m in nets_e for p in m.parameters()),
                   (p for m in nets_g for p in m.parameters()), (p for m in nets_s for p in m.parameters())))
        ph = fused.phase_times(); ps = serial.phase_times()
        out[f"{algo}/{comm}"] = dict(eager=eager, fused=lg, serial=ls, params_equal=bool(same), forked=fused.collectives_from_hooks,
                                     buckets=len(b_g.buckets), phases_fused=sorted(ph), phases_serial=sorted(ps))
try:
    GraphedTrainStep(nets_g, batch(0), opt_g, buckets=b_g, dtype=torch.bfloat16, warmup=0, capture_collectives=False)
    out["refuses_hooks_without_capture"] = False
except ValueError:
    out["refuses_hooks_without_capture"] = True
dist.barrier()
dist.destroy_process_group()
print("RESULT " + json.dumps(out))
'''


def test_graphed_train_step_with_the_rccl_collectives_captured_in_the_graph(tmp_path):
    """the graphed training step used to run replay -> collectives -> update serially.  With RCCL the bucket
    collectives are now captured INTO the step graph: the buckets' hooks enqueue them on RCCL's stream as the backward completes
    each bucket (a fork inside the capture), ``finish()`` joins.  World size 1 on the leased GPU runs the real RCCL kernels as
    graph nodes: three steps must equal the eager hook-overlapped step and the serial three-phase graphed step bit for bit
    (losses and parameters), for all-reduce and reduce-scatter + all-gather, fp32 and bf16 transport, and some collectives
    must have been forked from inside the backward."""
    script = tmp_path / "graph_worker.py"
    script.write_text(GRAPH_WORKER)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()), UR_ROOT=ROOT, HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, str(script)], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    res = json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
    print(json.dumps(res))
    assert res.pop("refuses_hooks_without_capture") is True
    assert len(res) == 4
    for k, v in res.items():
        assert v["eager"] == v["fused"] == v["serial"], (k, v)
        assert v["params_equal"], k
        assert v["forked"] > 0 and v["buckets"] >= 3, (k, v)
        assert v["phases_fused"] == ["overlapped_total"] and v["phases_serial"] == ["collectives", "replay", "update"]
