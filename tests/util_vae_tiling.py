"""Helpers of the VAE tiling tests: a float64 restatement of diffusers 0.24's SEQUENTIAL IN-PLACE tile stitch
(``AutoencoderKL.blend_v`` / ``blend_h`` and the loops of ``tiled_decode`` / ``tiled_encode``, over a list of lists of NCHW
tensors), the four-tile closed form ``ur_blend_tiles`` evaluates with its per-element error bound, the variant that blends
against raw neighbours (what the kernel must NOT compute), and guarded buffers for tiles and outputs."""
import torch

from util_lora import Guarded, ulp  # noqa: F401  (Guarded: outputs between canaries; re-exported for the tests)

U32 = 2.0 ** -24  # unit roundoff of fp32


# ---------------------------------------------------------------------------------------------------------------------
# the restatement: diffusers' loops as diffusers writes them
# ---------------------------------------------------------------------------------------------------------------------
def blend_v(a, b, blend_extent):
    blend_extent = min(a.shape[2], b.shape[2], blend_extent)
    for y in range(blend_extent):
        b[:, :, y, :] = a[:, :, -blend_extent + y, :] * (1 - y / blend_extent) + b[:, :, y, :] * (y / blend_extent)
    return b


def blend_h(a, b, blend_extent):
    blend_extent = min(a.shape[3], b.shape[3], blend_extent)
    for x in range(blend_extent):
        b[:, :, :, x] = a[:, :, :, -blend_extent + x] * (1 - x / blend_extent) + b[:, :, :, x] * (x / blend_extent)
    return b


def stitch(tiles, blend, limit, dtype=torch.float64):
    """``tiles[i][j]``: NCHW tensors.  Copies them to ``dtype``, then the second loop nest of ``tiled_decode``: the blends
    write into the tiles, and the neighbour a blend reads is the already blended one."""
    rows = [[t.detach().cpu().to(dtype).clone() for t in row] for row in tiles]
    result_rows = []
    for i, row in enumerate(rows):
        result_row = []
        for j, tile in enumerate(row):
            if i > 0:
                tile = blend_v(rows[i - 1][j], tile, blend)
            if j > 0:
                tile = blend_h(row[j - 1], tile, blend)
            result_row.append(tile[:, :, :limit, :limit])
        result_rows.append(torch.cat(result_row, dim=3))
    return torch.cat(result_rows, dim=2)


def stitch_raw_neighbours(tiles, blend, limit, dtype=torch.float64):
    """The WRONG stitch: every blend reads the raw, unblended neighbour.  Equal to ``stitch`` on the edges, different in the
    corners y < e_v, x < e_h."""
    raw = [[t.detach().cpu().to(dtype).clone() for t in row] for row in tiles]
    rows = [[t.clone() for t in row] for row in raw]
    result_rows = []
    for i, row in enumerate(rows):
        result_row = []
        for j, tile in enumerate(row):
            if i > 0:
                tile = blend_v(raw[i - 1][j], tile, blend)
            if j > 0:
                tile = blend_h(raw[i][j - 1], tile, blend)
            result_row.append(tile[:, :, :limit, :limit])
        result_rows.append(torch.cat(result_row, dim=3))
    return torch.cat(result_rows, dim=2)


# ---------------------------------------------------------------------------------------------------------------------
# the closed form over the RAW tiles, and the error bound of its fp32 evaluation
# ---------------------------------------------------------------------------------------------------------------------
def _lerp(a, b, w):
    """(value, error bound) of ``a (1 - w) + b w`` for operands (value, error bound), as the kernel evaluates it in fp32:
    wh = fl(w) (w an fp32 quotient: relative error u), uh = fl(1 - wh), p = fl(a uh), result = fl(fma(b, wh, p)).  To first
    order uh = (1 - w) + eta with |eta| <= u w + u (1 - w); p adds u |a| (1 - w); b wh carries u |b| w; the fma's rounding adds
    u (|a| (1 - w) + |b| w).  In all: u (|a| (w + 3 (1 - w)) + 2 |b| w), plus the operands' own errors times their weights."""
    (va, ea), (vb, eb) = a, b
    val = va * (1 - w) + vb * w
    err = ea * (1 - w) + eb * w + U32 * (va.abs() * (w + 3 * (1 - w)) + 2 * vb.abs() * w)
    return val, err


def closed_form(tiles, blend, limit):
    """``(value, fp32 error bound)`` in float64 of the stitch as ``ur_blend_tiles`` computes it, from the raw tiles alone:
        y >= ev, x >= eh   T
        y <  ev, x >= eh   lerp(A, T, wy)
        y >= ev, x <  eh   lerp(L, T, wx)
        y <  ev, x <  eh   lerp(lerp(AL, L, wy), lerp(lerp(AL, A, wx), T, wy), wx)
    with A / L / AL read at the last ev rows / eh columns of the tile above / to the left / above-left."""
    raw = [[t.detach().cpu().double() for t in row] for row in tiles]
    val_rows, err_rows = [], []
    for i, row in enumerate(raw):
        vals, errs = [], []
        for j, t in enumerate(row):
            h, w = t.shape[2:]
            ev = min(raw[i - 1][j].shape[2], h, blend) if i > 0 else 0
            eh = min(row[j - 1].shape[3], w, blend) if j > 0 else 0
            wy = (torch.arange(ev, dtype=torch.float64) / max(ev, 1)).view(1, 1, ev, 1)
            wx = (torch.arange(eh, dtype=torch.float64) / max(eh, 1)).view(1, 1, 1, eh)
            v, e = t.clone(), torch.zeros_like(t)
            z = lambda x: (x, torch.zeros_like(x))
            if ev:
                a = raw[i - 1][j][:, :, -ev:, :]
                av, ae = a.clone(), torch.zeros_like(a)
                if eh:
                    al = raw[i - 1][j - 1][:, :, -ev:, -eh:]
                    av[..., :eh], ae[..., :eh] = _lerp(z(al), z(a[..., :eh]), wx)
                v[:, :, :ev], e[:, :, :ev] = _lerp((av, ae), z(t[:, :, :ev]), wy)
            if eh:
                l = row[j - 1][:, :, :, -eh:]
                lv, le = l.clone(), torch.zeros_like(l)
                if ev:
                    al = raw[i - 1][j - 1][:, :, -ev:, -eh:]
                    lv[:, :, :ev], le[:, :, :ev] = _lerp(z(al), z(l[:, :, :ev]), wy)
                v[..., :eh], e[..., :eh] = _lerp((lv, le), (v[..., :eh].clone(), e[..., :eh].clone()), wx)
            vals.append(v[:, :, :limit, :limit])
            errs.append(e[:, :, :limit, :limit])
        val_rows.append(torch.cat(vals, 3))
        err_rows.append(torch.cat(errs, 3))
    return torch.cat(val_rows, 2), torch.cat(err_rows, 2)


def bound(tiles, blend, limit, out_dtype):
    """Per-element bound on |kernel - float64 stitch|: the first-order fp32 bound of ``closed_form`` (times 1 + 2^-20 for the
    higher orders) plus, for a 16-bit output, half an ulp of the output dtype at |value| + that bound (the one rounding; an
    fp32 output is the fp32 value itself)."""
    val, err = closed_form(tiles, blend, limit)
    err = err * (1 + 2.0 ** -20)
    if out_dtype != torch.float32:
        err = err + 0.5 * ulp(val.abs() + err, out_dtype)
    return err


def corner_mask(tiles, blend, limit):
    """Boolean [Hout][Wout]: the output pixels with y < e_v and x < e_h of their tile (the four-tile regions)."""
    hs, ws = [r[0].shape[2] for r in tiles], [t.shape[3] for t in tiles[0]]
    ys = torch.cat([torch.arange(min(limit, h)) < (min(hs[i - 1], h, blend) if i else 0) for i, h in enumerate(hs)])
    xs = torch.cat([torch.arange(min(limit, w)) < (min(ws[j - 1], w, blend) if j else 0) for j, w in enumerate(ws)])
    return ys[:, None] & xs[None, :]


# ---------------------------------------------------------------------------------------------------------------------
# the oracle VAE, tiled: the first loop nest of tiled_decode / tiled_encode over oracle/vae_oracle.py, stitched in fp32
# ---------------------------------------------------------------------------------------------------------------------
def oracle_tiled_decode(o, z, tile_latent, tile_sample, factor=0.25):
    overlap, blend = int(tile_latent * (1 - factor)), int(tile_sample * factor)
    rows = [[o.decode(z[:, :, i:i + tile_latent, j:j + tile_latent]) for j in range(0, z.shape[3], overlap)]
            for i in range(0, z.shape[2], overlap)]
    return stitch(rows, blend, tile_sample - blend, torch.float32)


def oracle_tiled_moments(o, x, tile_latent, tile_sample, factor=0.25):
    """(mean, logvar clamped to [-30, 20]) from the blended raw moments, as DiagonalGaussianDistribution reads them."""
    overlap, blend = int(tile_sample * (1 - factor)), int(tile_latent * factor)
    with torch.no_grad():
        rows = [[o.quant_conv(o.encoder(x[:, :, i:i + tile_sample, j:j + tile_sample])) for j in range(0, x.shape[3], overlap)]
                for i in range(0, x.shape[2], overlap)]
    mean, logvar = stitch(rows, blend, tile_latent - blend, torch.float32).chunk(2, dim=1)
    return mean, logvar.clamp(-30.0, 20.0)


# ---------------------------------------------------------------------------------------------------------------------
# tiles on the device, between NaN bands
# ---------------------------------------------------------------------------------------------------------------------
def make_tiles(hs, ws, B, C, dtype, seed, integer=False):
    """NCHW CPU tiles ``[B, C, h_i, w_j]`` in ``dtype``: integers in [-64, 64] or N(0, 1) values."""
    g = torch.Generator().manual_seed(seed)
    if integer:
        return [[torch.randint(-64, 65, (B, C, h, w), generator=g).to(dtype) for w in ws] for h in hs]
    return [[torch.randn(B, C, h, w, generator=g).to(dtype) for w in ws] for h in hs]


def device_tiles(tiles, dev, batched=False, offset=0, guard=64):
    """The NHWC device tiles of NCHW CPU ``tiles``, each inside its own buffer of NaNs with ``guard + offset`` NaNs in front and
    ``guard`` behind, so that any read outside a tile poisons a result.  ``batched``: a tile is the slice ``[:, 0]`` of a
    ``[B, 2, h, w, C]`` tensor whose other half is NaN: its sample stride is 2 h w C."""
    out, keep = [], []
    for row in tiles:
        orow = []
        for t in row:
            B, C, h, w = t.shape
            n = B * (2 if batched else 1) * h * w * C
            buf = torch.full((guard + offset + n + guard,), float("nan"), dtype=t.dtype, device=dev)
            body = buf[guard + offset:guard + offset + n]
            view = body.view(B, 2, h, w, C)[:, 0] if batched else body.view(B, h, w, C)
            view.copy_(t.permute(0, 2, 3, 1).to(dev))
            keep.append(buf)
            orow.append(view)
        out.append(orow)
    return out, keep
