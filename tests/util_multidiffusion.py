"""Independent restatements for the MultiDiffusion tests: the windows and the blend in float64 numpy, a numpy fp32 emulation of
the kernel's exact operation order (sequential fp32 adds in ascending view index, one IEEE division, then the roundings), and
the literal Panorama loop (diffusers' StableDiffusionPanoramaPipeline: views ONE AT A TIME through the network, one scheduler
per view, ``value`` / ``count`` accumulation) on the CPU oracle networks.  Nothing here imports the package."""
import numpy as np
import torch

from util_models import O, OracleScheduler

GROUPS = ("material", "normal", "albedo", "spec_light", "diff_light", "env")
U32 = 2.0 ** -24  # unit roundoff of fp32


def windows(H, W, window, stride):
    """(h0, h1, w0, w1) per view, row-major; an axis not longer than the window has one window of its own length."""
    def axis(L):
        if L <= window:
            return [(0, L)]
        assert (L - window) % stride == 0, (L, window, stride)
        return [(k * stride, k * stride + window) for k in range((L - window) // stride + 1)]

    return [(h0, h1, w0, w1) for (h0, h1) in axis(H) for (w0, w1) in axis(W)]


def cut(x, views):
    """[N, C, H, W] -> [N * V, C, wh, ww], sample n's view v at n * V + v (numpy or torch)."""
    lib = torch if torch.is_tensor(x) else np
    parts = [x[:, :, h0:h1, w0:w1] for (h0, h1, w0, w1) in views]
    st = lib.stack(parts, 1)
    return st.reshape((x.shape[0] * len(views), x.shape[1]) + tuple(st.shape[-2:]))


def counts(views, H, W):
    c = np.zeros((H, W), dtype=np.int64)
    for (h0, h1, w0, w1) in views:
        c[h0:h1, w0:w1] += 1
    return c


def blend_f64(master, views, H, W):
    """float64: (global [N, C, H, W], sum of |entries| per global element, count [H, W])."""
    m = np.asarray(master, dtype=np.float64)
    V = len(views)
    N, C = m.shape[0] // V, m.shape[1]
    m = m.reshape(N, V, C, *m.shape[-2:])
    value, mag = np.zeros((N, C, H, W)), np.zeros((N, C, H, W))
    for v, (h0, h1, w0, w1) in enumerate(views):
        value[:, :, h0:h1, w0:w1] += m[:, v]
        mag[:, :, h0:h1, w0:w1] += np.abs(m[:, v])
    cnt = counts(views, H, W)
    return value / cnt, mag, cnt


def bound(g64, mag, cnt):
    """|fp32 blend - float64 blend| per global element: k - 1 ordered fp32 adds, each with relative error u on a partial sum
    of at most sum|m|, then a division with relative error u:  (k - 1) u sum|m| / k + u |g|  (first order; the tests add the
    1 + k u second-order factor)."""
    k = cnt.astype(np.float64)
    return ((k - 1) * U32 * mag / k + U32 * np.abs(g64)) * (1 + k * U32)


def blend_fp32_emulation(master, views, H, W, lat_dtype=torch.float32, round_master=False, halves=1):
    """The kernel's bits: (master_out fp32 numpy, lat_out torch [halves * NV, ...] of lat_dtype, global fp32 numpy)."""
    m = np.asarray(master, dtype=np.float32)
    V = len(views)
    N, C = m.shape[0] // V, m.shape[1]
    mv = m.reshape(N, V, C, *m.shape[-2:])
    value = np.zeros((N, C, H, W), dtype=np.float32)
    for v, (h0, h1, w0, w1) in enumerate(views):  # ((0 + m0) + m1) + ...: one fp32 rounding per add
        value[:, :, h0:h1, w0:w1] = value[:, :, h0:h1, w0:w1] + mv[:, v]
    with np.errstate(invalid="ignore"):
        g = (value / counts(views, H, W).astype(np.float32)).astype(np.float32)  # IEEE division
    gt = torch.from_numpy(g).to(lat_dtype)  # ONE rounding to the latent dtype (round to nearest even)
    if round_master:
        g = gt.to(torch.float32).numpy()
    lat = cut(gt, views)
    return cut(g, views), torch.cat([lat] * halves), g


def panorama_inverse(models, img, mask, ehs, noise, steps, views, kind="ddim", guidance=0.0, blend=True):
    """Inverse rendering on the oracle networks over the global tensors ``img`` / ``mask`` / ``noise`` [N, 4, H, W]: per step,
    per view one ``O.dual_stream_step`` on the view's crop, one scheduler per (view, group), value / count.  ``blend=False``:
    the same windows sampled independently (the views never see each other).  Returns ({group: global latent}, [views])."""
    unet_o, enc_o, dec_o = models
    N, _, H, W = noise.shape
    sched = {(v, n): OracleScheduler(kind, steps) for v in range(len(views)) for n in GROUPS}
    ts = OracleScheduler(kind, steps).timesteps
    cfg = guidance != 0
    e = ehs.repeat(N, 1, 1)
    if cfg:
        e = torch.cat([torch.zeros_like(e), e])
    dup = (lambda t: torch.cat([t, t])) if cfg else (lambda t: t)
    lat = {n: noise.clone() for n in GROUPS}
    own = {(v, n): noise[:, :, h0:h1, w0:w1].clone() for v, (h0, h1, w0, w1) in enumerate(views) for n in GROUPS}
    cnt = torch.from_numpy(counts(views, H, W)).to(noise.dtype)
    for t in ts:
        value = {n: torch.zeros_like(noise) for n in GROUPS}
        for v, (h0, h1, w0, w1) in enumerate(views):
            crop = lambda x: x[:, :, h0:h1, w0:w1]
            cur = {n: (crop(lat[n]) if blend else own[(v, n)]) for n in GROUPS}
            cond = torch.cat([dup(crop(mask))] + [dup(cur[n]) for n in GROUPS], 1)
            B = cond.shape[0]
            out = O.dual_stream_step(unet_o, enc_o, dec_o, dup(crop(img)), cond, e, torch.zeros(B).long(), t.expand(B))
            pred = out["attr_pred"][:, 4:]
            for k, n in enumerate(GROUPS):
                p = pred[:, 4 * k:4 * k + 4]
                if cfg:
                    pc, pu = p.chunk(2)
                    p = pu + guidance * (pc - pu) if n == "material" else pc
                own[(v, n)] = sched[(v, n)].step(p, t, cur[n])[0]
                value[n][:, :, h0:h1, w0:w1] += own[(v, n)]
        lat = {n: value[n] / cnt for n in GROUPS}
    return lat, own


def panorama_render(models, attr, ehs, noise, steps, views, kind="ddim"):
    """Rendering (encoder + UNet, guidance 0) the same way: the global image latent [N, 4, H, W]."""
    unet_o, enc_o, dec_o = models
    N, _, H, W = noise.shape
    sched = [OracleScheduler(kind, steps) for _ in views]
    e = ehs.repeat(N, 1, 1)
    lat = noise.clone()
    cnt = torch.from_numpy(counts(views, H, W)).to(noise.dtype)
    for t in OracleScheduler(kind, steps).timesteps:
        value = torch.zeros_like(noise)
        for v, (h0, h1, w0, w1) in enumerate(views):
            x = lat[:, :, h0:h1, w0:w1]
            r = O.dual_stream_step(unet_o, enc_o, dec_o, x, attr[:, :, h0:h1, w0:w1], e, t.expand(N), torch.zeros(N).long(),
                                   run_decoder=False)
            value[:, :, h0:h1, w0:w1] += sched[v].step(r["img_pred"], t, x)[0]
        lat = value / cnt
    return lat
