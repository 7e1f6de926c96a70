"""A/B of training the ControlNet conditioning embedding on the direct narrow-channel backward kernels (csrc/condconv_bwd.hip)
against the route the package had without them: every narrow layer padded to 64 channels on ``autograd_ops.conv3x3`` /
``backward.conv3x3_backward``.  SD-1.x shape: B = 4, 512 x 512 image, 64 x 64 latent, fp16 and bf16.  One process, HIP events,
warm-up, legs alternated three times; medians per visit and their spread.

  per layer    forward / dgrad / wgrad of the new kernels, the same three on the padded route, algorithmic bytes (operands once,
               results once) against the bytes the new kernels move (dgrad: the same; wgrad: + the fp32 partials twice)
  SiLU         the elementwise SiLU forward and backward passes of the chain, as a share of the narrow route's chain time
  whole step   ControlNet trainable, UNet frozen, FusedAdamW: step time, peak memory, saved-activation bytes of the embedding,
               on both routes
  inference    the no-grad ControlNet forward (a code path this tool's subject does not touch), for comparison with
               profiles/cond_embed_ab.txt

    python tools/controlnet_train_ab.py [--out profiles/controlnet_train_ab.txt] [--reps 10] [--batch 4] [--size 512] [--no-step]
"""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from uni_renderer_amd import autograd_ops as A, backward as BW, ops  # noqa: E402
from uni_renderer_amd.layers import f32, pack_cond_conv3x3, pack_cond_conv3x3_rot, pack_conv3x3  # noqa: E402

WIDTHS = (16, 32, 96, 256)


def layers():
    out, c = [(3, WIDTHS[0], 1)], WIDTHS[0]
    for nxt in WIDTHS[1:]:
        out += [(c, c, 1), (c, nxt, 2)]
        c = nxt
    return out


def up64(c):
    return (c + 63) // 64 * 64


def timed(fn, reps):
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts)


def visits(fns, reps, n=3):
    """{name: [median ms per visit]} with the legs alternated."""
    for f in fns.values():
        f()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(n):
        for k, f in fns.items():
            out[k].append(timed(f, reps))
    return out


def ms(v):
    return f"{statistics.median(v):.3f} (+-{(max(v) - min(v)) / 2:.3f})"


def padded_embedding_forward(emb, cond, dt, bgr=False):
    """The embedding under autograd on the 64-channel route: image and every channel count zero padded to a multiple of 64,
    ``autograd_ops.conv3x3`` + ``autograd_ops.SiLU``; the gradients reach the same parameters (through F.pad's backward)."""
    x = F.pad((cond.flip(1) if bgr else cond).permute(0, 2, 3, 1).to(dt), (0, 64 - cond.shape[1])).contiguous()
    for conv in [emb.conv_in] + list(emb.blocks):
        co, ci = conv.weight.shape[:2]
        w = F.pad(conv.weight, (0, 0, 0, 0, 0, up64(ci) - ci, 0, up64(co) - co))
        b = F.pad(conv.bias, (0, up64(co) - co))
        x = A.SiLU.apply(A.conv3x3(x, A.pack_conv_weight(w, dt), b, stride=conv.stride[0]))
    return x[..., :emb.blocks[-1].out_channels].contiguous()


def per_layer(say, dt, B, S, reps, dev):
    g = torch.Generator().manual_seed(0)
    H = S
    tot = {"narrow": 0.0, "padded": 0.0, "silu": 0.0}
    say(f"## per layer, {dt}: ms = median over 3 visits (+- half the spread over the visits)")
    say("layer          map     algorithmic MB (fwd / dgrad / wgrad)    narrow fwd      dgrad          wgrad       | padded fwd      dgrad          wgrad       | wgrad moves MB")
    for i, (cin, cout, s) in enumerate(layers()):
        img = i == 0
        Ho = (H - 1) // s + 1
        w4 = torch.randn(cout, cin, 3, 3, generator=g) / (9 * cin) ** 0.5
        x = (torch.rand(B, cin, H, H, generator=g).to(dev) if img else torch.randn(B, H, H, cin, generator=g).to(dev, dt))
        dy = torch.randn(B, Ho, Ho, cout, generator=g).to(dev, dt)
        wa, ba = pack_cond_conv3x3(w4, dt, s, image=img).to(dev), torch.zeros(cout, device=dev)
        wr = None if img else pack_cond_conv3x3_rot(w4, dt).to(dev)
        ci, co = up64(cin), up64(cout)
        wb4 = torch.zeros(co, ci, 3, 3)
        wb4[:cout, :cin] = w4
        wb, bb = pack_conv3x3(wb4, dt).to(dev), torch.zeros(co, device=dev)
        xb = (F.pad(x.permute(0, 2, 3, 1).to(dt), (0, ci - cin)) if img else F.pad(x, (0, ci - cin))).contiguous()
        dyb = F.pad(dy, (0, co - cout)).contiguous()
        fns = {
            "nf": lambda: ops.cond_conv3x3(x, wa, ba, n_out=cout, stride=s, dtype=dt, image=img),
            "nw": lambda: ops.cond_conv3x3_wgrad(x, dy, stride=s, image=img),
            "pf": lambda: ops.conv3x3(xb, wb, bb, stride=s),
            "pw": lambda: BW.conv3x3_backward(xb, wb, dyb, stride=s, need_dx=False),
        }
        if not img:
            fns["nd"] = lambda: ops.cond_conv3x3_dgrad(dy, wr, in_hw=(H, H), n_in=cin, stride=s)
            fns["pd"] = lambda: BW.conv3x3_backward(xb, wb, dyb, need_bias=False, stride=s, need_dw=False)
        v = visits(fns, reps)
        xbytes, ybytes = x.numel() * x.element_size(), dy.numel() * 2
        ws = ops._lib.load().ur_cond_conv3x3_wgrad_workspace(B, H, H, cin, cout, s, int(img), 0)
        alg = (xbytes + ybytes + wa.numel() * 2, 0 if img else xbytes + ybytes + wr.numel() * 2, xbytes + ybytes + cout * cin * 36)
        col = lambda k: ms(v[k]) if k in v else "      -       "
        say(f"{cin:>3} -> {cout:<3} s{s}  {H:>4}^2   {alg[0] / 1e6:>8.1f} / {alg[1] / 1e6:>8.1f} / {alg[2] / 1e6:>8.1f}     "
            f"{col('nf')}  {col('nd')}  {col('nw')} | {col('pf')}  {col('pd')}  {col('pw')} | {(alg[2] + 2 * ws) / 1e6:>8.1f}")
        for k in v:
            tot["narrow" if k[0] == "n" else "padded"] += statistics.median(v[k])
        # SiLU forward + backward over this layer's output (the derivative reads the saved pre-activation and dy)
        pre = torch.randn(B, Ho, Ho, cout, generator=g).to(dev, dt)
        sv = visits({"sf": lambda: A.SiLU.apply(pre), "sb": lambda: BW.silu_backward(pre, dy)}, reps)
        tot["silu"] += statistics.median(sv["sf"]) + statistics.median(sv["sb"])
        H = Ho
    say(f"sum over the seven layers, {dt}: narrow fwd + dgrad + wgrad {tot['narrow']:.3f} ms, padded {tot['padded']:.3f} ms "
        f"(padded / narrow = {tot['padded'] / tot['narrow']:.2f}); elementwise SiLU forward + backward passes {tot['silu']:.3f} ms "
        f"= {100 * tot['silu'] / (tot['narrow'] + tot['silu']):.1f} % of the narrow route's chain with them")
    return tot


def whole_step(say, dt, B, S, reps, dev):
    import uni_renderer_amd as U
    from uni_renderer_amd.optim import FusedAdamW

    torch.manual_seed(0)
    g = torch.Generator().manual_seed(1)
    unet = U.UNet2DConditionModel(cross_attention_dim=768).to(dev).eval().requires_grad_(False)
    unet.compute_dtype = dt
    cn = U.ControlNetModel.from_unet(unet).to(dev).train().requires_grad_(True)
    cn.compute_dtype = dt
    for m in [cn.controlnet_cond_embedding.conv_out] + list(cn.controlnet_down_blocks) + [cn.controlnet_mid_block]:
        torch.nn.init.normal_(m.weight, std=0.02)
    opt = FusedAdamW(cn.parameters(), lr=1e-5)
    L = S // 8
    x = torch.randn(B, 4, L, L, generator=g).to(dev)
    img = torch.rand(B, 3, S, S, generator=g).to(dev)
    ehs = (torch.randn(B, 77, 768, generator=g) * 0.5).to(dev)
    t = torch.full((B,), 500, device=dev)
    target = torch.randn(B, unet.config["out_channels"], L, L, generator=g).to(dev)
    emb = cn.controlnet_cond_embedding
    narrow = emb.forward_autograd
    routes = {"narrow": narrow, "padded": lambda c, d, bgr=False: padded_embedding_forward(emb, c, d, bgr)}

    def step():
        opt.zero_grad(set_to_none=True)
        res, mid = cn(x, t, ehs, img, return_dict=False)
        out = unet(x, t, ehs, down_block_additional_residuals=res, mid_block_additional_residual=mid, return_dict=False)[0]
        loss = F.mse_loss(out.float(), target)
        loss.backward()
        opt.step()
        return loss

    say(f"## whole training step, {dt}: ControlNet trainable (SD-1.x size), UNet frozen, FusedAdamW, B = {B}, latent {L} x {L}")
    res = {}
    for name, fwd in routes.items():
        emb.forward_autograd = fwd
        saved = [0]

        def pack(tn):
            saved[0] += tn.numel() * tn.element_size()
            return tn

        with torch.autograd.graph.saved_tensors_hooks(pack, lambda tn: tn):
            h = fwd(img, dt)
        del h
        for _ in range(2):
            step()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        step()
        torch.cuda.synchronize()
        res[name] = dict(saved=saved[0], peak=torch.cuda.max_memory_allocated())
    v = {k: [] for k in routes}
    for _ in range(3):
        for name, fwd in routes.items():
            emb.forward_autograd = fwd
            step()
            v[name].append(timed(step, reps))
    emb.forward_autograd = narrow
    for name in routes:
        say(f"{name:>7} route: step {ms(v[name])} ms (visits {', '.join(f'{q:.2f}' for q in v[name])}); peak memory "
            f"{res[name]['peak'] / 2 ** 20:.0f} MiB; tensors saved for the embedding's backward {res[name]['saved'] / 2 ** 20:.0f} MiB")
    d = statistics.median(v["padded"]) - statistics.median(v["narrow"])
    sp = max(max(q) - min(q) for q in v.values())
    say(f"padded - narrow = {d:.3f} ms per step; largest spread over the visits of a leg {sp:.3f} ms -> "
        f"{'the narrow route wins by more than the spread' if d > sp else 'NO difference beyond the spread' if abs(d) <= sp else 'the narrow route LOSES by more than the spread'}")
    with torch.no_grad():
        iv = visits({"inf": lambda: cn(x, t, ehs, img, return_dict=False)}, reps)
    say(f"inference (no autograd) ControlNetModel forward, same network: {ms(iv['inf'])} ms (visits {', '.join(f'{q:.3f}' for q in iv['inf'])})")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "controlnet_train_ab.txt"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--no-step", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say(f"# tools/controlnet_train_ab.py: B = {a.batch}, {a.size} x {a.size}, {torch.cuda.get_device_name(0)}; HIP events, {a.reps} "
        f"repetitions per visit, 3 visits per leg, legs alternated, one process")
    for dt in (torch.float16, torch.bfloat16):
        per_layer(say, dt, a.batch, a.size, a.reps, dev)
        if not a.no_step:
            whole_step(say, dt, a.batch, a.size, a.reps, dev)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
