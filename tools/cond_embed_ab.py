"""A/B of the ControlNet conditioning embedding's seven narrow 3x3 convs (3 -> 16 -> 16 -> 32 -> 32 -> 96 -> 96 -> 256,
SiLU after each, three stride-2 steps) at B = 4, 512 x 512, fp16:

  (a) seven ``ops.cond_conv3x3`` launches (csrc/condconv.hip), the first reading the caller's NCHW fp32 image;
  (b) the same convs on ``ops.igemm`` as it has to run them: ``to_nhwc`` of the image into 64 channels, every channel count
      zero-padded to a multiple of 64 (K granularity of the implicit GEMM), ``act=ACT_SILU``, ``n_store`` padding so that
      the next layer reads zeros in its padded channels.

HIP events in one process, no profiler: warm-up, then the two legs alternated three times, >= 20 repetitions of the whole
chain per visit; medians per visit and their spread over the visits.  Per layer (timed on its own the same way): the
algorithmic bytes -- the input once, the output once, the packed weights -- and the GB/s they amount to.  The chain's byte
floor counts the image once and every intermediate written once and read once.  Also: ``ControlNetModel.forward`` minus
``AttributeEncoderModel.forward`` at the same shape (SD-1.5 size, latent 64 x 64) = what the embedding adds to a forward.

    python tools/cond_embed_ab.py [--out profiles/cond_embed_ab.txt] [--reps 20] [--batch 4] [--size 512]
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from uni_renderer_amd import ops  # noqa: E402
from uni_renderer_amd.layers import f32, pack_cond_conv3x3, pack_conv3x3  # noqa: E402

WIDTHS = (16, 32, 96, 256)


def layers():
    """[(cin, cout, stride)] of the seven narrow convs."""
    out, c = [(3, WIDTHS[0], 1)], WIDTHS[0]
    for nxt in WIDTHS[1:]:
        out += [(c, c, 1), (c, nxt, 2)]
        c = nxt
    return out


def up64(c):
    return (c + 63) // 64 * 64


def timed(fn, reps):
    """Median milliseconds of ``fn()`` over ``reps`` event-timed calls."""
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cond_embed_ab.txt"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--no-forward", action="store_true", help="skip the ControlNetModel / AttributeEncoderModel forwards")
    a = ap.parse_args()
    dev, dt = torch.device("cuda:0"), torch.float16
    B, S = a.batch, a.size
    g = torch.Generator().manual_seed(0)
    img = torch.rand(B, 3, S, S, generator=g).to(dev)
    convs = []
    for cin, cout, s in layers():
        w = torch.randn(cout, cin, 3, 3, generator=g) / (9 * cin) ** 0.5
        b = torch.randn(cout, generator=g) * 0.1
        convs.append(dict(cin=cin, cout=cout, s=s, w=w, b=b))
    for i, c in enumerate(convs):
        c["wa"] = pack_cond_conv3x3(c["w"], dt, c["s"], image=i == 0).to(dev)
        c["ba"] = f32(c["b"]).to(dev)
        ci, co = up64(c["cin"]), up64(c["cout"])
        wb = torch.zeros(co, ci, 3, 3)
        wb[:c["cout"], :c["cin"]] = c["w"]
        c["wb"] = pack_conv3x3(wb, dt).to(dev)
        c["bb"] = torch.nn.functional.pad(c["b"], (0, co - c["cout"])).float().to(dev)

    def layer_a(i, x):
        c = convs[i]
        return ops.cond_conv3x3(x, c["wa"], c["ba"], n_out=c["cout"], stride=c["s"], act=ops.ACT_SILU, dtype=dt, image=i == 0)

    def layer_b(i, x):
        c = convs[i]
        Bx, H, W, ci = x.shape
        Ho, Wo = (H - 1) // c["s"] + 1, (W - 1) // c["s"] + 1
        co = up64(c["cout"])
        out = torch.empty(Bx, Ho, Wo, co, dtype=dt, device=dev)
        ops.igemm(x0=x, w=c["wb"], out=out, M=Bx * Ho * Wo, N=c["cout"], K=9 * ci, c0=ci, ldx0=ci, ldw=9 * ci, ldc=co, taps=9,
                  conv=(Bx, H, W, Ho, Wo), stride=c["s"], bias=c["bb"], rows_per_b=Ho * Wo, n_store=co, act=ops.ACT_SILU)
        return out

    def chain_a():
        x = img
        for i in range(len(convs)):
            x = layer_a(i, x)
        return x

    def chain_b():
        x = ops.to_nhwc(img, dt, 64)
        for i in range(len(convs)):
            x = layer_b(i, x)
        return x

    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say(f"# tools/cond_embed_ab.py: B = {B}, {S} x {S}, fp16, {torch.cuda.get_device_name(0)}; HIP events, {a.reps} repetitions per visit,")
    say("# legs alternated three times; (a) ops.cond_conv3x3 x 7, (b) to_nhwc + ops.igemm x 7 on channels padded to 64")
    ya, yb = chain_a(), chain_b()
    torch.cuda.synchronize()
    diff = float((ya.float() - yb[..., :WIDTHS[-1]].float()).norm() / yb[..., :WIDTHS[-1]].float().norm())
    say(f"rel-L2 of (a) against (b) on the 256-channel map: {diff:.2e}")
    for _ in range(3):
        chain_a()
        chain_b()
    torch.cuda.synchronize()
    visits = {"a": [], "b": []}
    for _ in range(3):
        visits["a"].append(timed(chain_a, a.reps))
        visits["b"].append(timed(chain_b, a.reps))
    for k in "ab":
        v = visits[k]
        say(f"chain ({k}): medians per visit {', '.join(f'{t:.3f}' for t in v)} ms; median {statistics.median(v):.3f}, spread {max(v) - min(v):.3f} ms")
    ma, mb = statistics.median(visits["a"]), statistics.median(visits["b"])
    sb = max(visits["b"]) - min(visits["b"])
    say(f"(b) - (a) = {mb - ma:.3f} ms ((b) / (a) = {mb / ma:.2f}); spread of (b) over its visits {sb:.3f} ms -> "
        f"{'(a) beats (b) by more than the spread of (b)' if mb - ma > sb else '(a) does NOT beat (b) by more than the spread of (b)'}")

    # per layer: inputs of each layer taken from an (a) / (b) pass
    xa, xb = [img], [ops.to_nhwc(img, dt, 64)]
    for i in range(len(convs)):
        xa.append(layer_a(i, xa[-1]))
        xb.append(layer_b(i, xb[-1]))
    torch.cuda.synchronize()
    floor = 0
    say("layer         map       bytes (MB)   (a) ms   GB/s   (b) ms   GB/s of the same bytes")
    for i, c in enumerate(convs):
        H = xa[i].shape[2] if i == 0 else xa[i].shape[1]
        nbytes = xa[i].numel() * xa[i].element_size() + xa[i + 1].numel() * 2 + c["wa"].numel() * 2
        floor += xa[i].numel() * (xa[i].element_size() if i == 0 else 2) + xa[i + 1].numel() * 2
        ta = statistics.median([timed(lambda: layer_a(i, xa[i]), a.reps) for _ in range(3)])
        tb = statistics.median([timed(lambda: layer_b(i, xb[i]), a.reps) for _ in range(3)])
        say(f"{c['cin']:>3} -> {c['cout']:<3} s{c['s']}  {H:>4}^2   {nbytes / 1e6:>9.1f}   {ta:>7.3f}  {nbytes / ta / 1e6:>6.0f}  {tb:>7.3f}  {nbytes / tb / 1e6:>6.0f}")
    say(f"byte floor of the chain (image once, every intermediate written once and read once): {floor / 1e6:.1f} MB "
        f"= {floor / B / 1e6:.1f} MB per sample; (a) moves it at {floor / ma / 1e6:.0f} GB/s, (b) at {floor / mb / 1e6:.0f} GB/s")

    if not a.no_forward:
        import uni_renderer_amd as U

        torch.manual_seed(0)
        net = U.ControlNetModel(cross_attention_dim=768)
        for m in [net.controlnet_cond_embedding.conv_out] + list(net.controlnet_down_blocks) + [net.controlnet_mid_block]:
            torch.nn.init.normal_(m.weight, std=0.02)
        enc = U.AttributeEncoderModel(cross_attention_dim=768)
        enc.load_state_dict({k: v for k, v in net.state_dict().items() if not k.startswith("controlnet_cond_embedding.")})
        net, enc = net.to(dt).to(dev).eval(), enc.to(dt).to(dev).eval()
        x = torch.randn(B, 4, S // 8, S // 8, generator=g).to(dev)
        ehs = (torch.randn(B, 77, 768, generator=g) * 0.5).to(dev)
        t = torch.full((B,), 500, device=dev)
        with torch.no_grad():
            f_net = lambda: net(x, t, ehs, img, return_dict=False)
            f_enc = lambda: enc(x, t, ehs, controlnet_cond=x)
            for _ in range(3):
                f_net()
                f_enc()
            torch.cuda.synchronize()
            vn, ve = [], []
            for _ in range(3):
                vn.append(timed(f_net, a.reps))
                ve.append(timed(f_enc, a.reps))
        mn, me = statistics.median(vn), statistics.median(ve)
        say(f"eager forward at B = {B}, latent {S // 8} x {S // 8}: ControlNetModel {mn:.3f} ms (visits {', '.join(f'{v:.3f}' for v in vn)}), "
            f"AttributeEncoderModel {me:.3f} ms (visits {', '.join(f'{v:.3f}' for v in ve)}); difference {mn - me:.3f} ms "
            f"= {100 * (mn - me) / mn:.1f} % of the ControlNet forward (embedding chain + its conv_out)")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
