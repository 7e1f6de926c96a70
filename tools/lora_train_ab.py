"""The two kernels of LoRA training at SD-1.x UNet size (profiles/lora_train_ab.txt, section 1): ur_lora_merge_cast_multi
(fp32 base -> bf16 W') and ur_lora_grad_multi (bf16 dW' -> fp32 d_up / d_down) over the 160 attention / feed-forward matrices
of bench.py's UNet, rank 4 / 16 / 64, launches from item tables built beforehand and the same with the tables built per call.
HIP events on the stream, median (min .. max) of 9 runs after 2 warm-up runs.  GB/s of the gradient kernel = the bytes of dW'
(read twice per 16 ranks by construction, counted ONCE) / time."""
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

TARGETS = ("to_q", "to_k", "to_v", "to_out.0", "ff.net.0.proj", "ff.net.2")


def timed(fn, runs=9, warm=2):
    ms = []
    for i in range(runs + warm):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        if i >= warm:
            ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def main():
    dev = torch.device("cuda", 0)
    unet = bench.build_models(dev, torch.float32)[0]
    shapes = [(n, m.weight) for n, m in unet.named_modules() if isinstance(m, torch.nn.Linear) and any(n.endswith("." + t) for t in TARGETS)]
    g = torch.Generator(device=dev).manual_seed(3)
    dws = [torch.randn(w.shape, device=dev, generator=g).to(torch.bfloat16) for _, w in shapes]
    outs = [torch.empty(w.shape, device=dev, dtype=torch.bfloat16) for _, w in shapes]
    dw_bytes = sum(t.numel() * 2 for t in dws)
    for rank in (4, 16, 64):
        ups = [torch.randn(w.shape[0], rank, device=dev, generator=g) * 0.02 for _, w in shapes]
        downs = [torch.randn(rank, w.shape[1], device=dev, generator=g) / rank for _, w in shapes]
        d_ups, d_downs = [torch.empty_like(u) for u in ups], [torch.empty_like(d) for d in downs]
        mrows = [(w.detach(), o, u, d, None, 1.0) for (_, w), o, u, d in zip(shapes, outs, ups, downs)]
        grows = [(dw, u, d, None, du, dd, 1.0) for dw, u, d, du, dd in zip(dws, ups, downs, d_ups, d_downs)]
        mt, gt = lora.item_tables(mrows, lora.multi_max()), lora.grad_item_tables(grows, lora.multi_max())
        m_l = timed(lambda: lora.launch_merge_cast(mt, torch.float32, torch.bfloat16))
        g_l = timed(lambda: lora.launch_grad(gt, torch.bfloat16))
        m_t = timed(lambda: lora.merge_cast_items(mrows, torch.float32, torch.bfloat16))
        g_t = timed(lambda: lora.grad_items(grows, torch.bfloat16))
        t0 = time.perf_counter()
        for _ in range(20):
            lora.grad_item_tables(grows, lora.multi_max())
        host = (time.perf_counter() - t0) / 20 * 1e3
        print(json.dumps(dict(rank=rank, items=len(shapes), launches=len(gt), dW_MB=round(dw_bytes / 2**20, 1),
                              merge_cast_ms=[round(v, 3) for v in m_l], merge_cast_with_tables_ms=[round(v, 3) for v in m_t],
                              merge_cast_GBps=round((dw_bytes * 3) / m_l[0] / 1e6),  # fp32 in (2x) + bf16 out
                              grad_ms=[round(v, 3) for v in g_l], grad_with_tables_ms=[round(v, 3) for v in g_t],
                              grad_GBps_of_dW=round(dw_bytes / g_l[0] / 1e6), grad_table_build_host_ms=round(host, 3))))


if __name__ == "__main__":
    main()
