#!/usr/bin/env python3
"""VAE tiling A/B on one MI355X: SD-size ``AutoencoderKL`` (random weights), fp16, B = 1, latent 128 x 128 (a 1024 x 1024 image).

  * ``tiled_decode`` with the fused stitch (``ur_blend_tiles``: one launch);
  * the same decoded tiles stitched the way diffusers 0.24 does it: a layout conversion per tile, ``blend_v`` / ``blend_h`` as
    Python loops of small strided torch ops, the crops and two ``torch.cat`` per grid (written below);
  * the plain ``decode``;
  * the tiled decode with every tile in a network call of its own instead of equal tiles as one batch (written below: the
    package has no such mode);
  * peak allocated memory, plain against tiled.

Writes ``profiles/vae_tiling_ab.txt`` (or the path given as the first argument).  Nothing is asserted but that the two stitches
agree to fp16 rounding; the file records what was measured and on how many runs."""
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from uni_renderer_amd import ops  # noqa: E402
from uni_renderer_amd.vae import AutoencoderKL  # noqa: E402

ROUNDS, ITERS, WARMUP = 5, 5, 3


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


def torch_stitch(tiles, blend, limit):
    """diffusers' stitch over the NHWC network outputs: NCHW copies (the blends write into them), then its second loop nest."""
    rows = [[ops.to_nchw(t) for t in row] for row in tiles]
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


def one_per_call(vae, z):
    """The tiled decode with nine network calls, one per tile, instead of four batched ones; the same fused stitch."""
    ay, ax = vae._tile_axes(z.shape[2], z.shape[3], True)
    tiles = [[vae._decode_nhwc(z[:, :, py:py + ly, px:px + lx]) for px, lx in zip(ax.positions, ax.lengths)]
             for py, ly in zip(ay.positions, ay.lengths)]
    return ops.blend_tiles(tiles, ay.blend, ay.limit)


def timed(fn, iters=ITERS):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / iters


def peak_mib(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


@torch.no_grad()
def main(path):
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    vae = AutoencoderKL().half().to(dev).eval()
    z = torch.randn(1, 4, 128, 128, device=dev).half()
    tiles, blend, limit = vae._network_tiles(z, True)
    ntiles = sum(len(r) for r in tiles)

    cases = {
        "tiled_decode, fused stitch": lambda: vae.tiled_decode(z),
        "tiled_decode, torch stitch": lambda: torch_stitch(*vae._network_tiles(z, True)),
        "tiled_decode, 1 tile / call": lambda: one_per_call(vae, z),
        "plain decode": lambda: vae.decode(z),
        "stitch alone, fused": lambda: ops.blend_tiles(tiles, blend, limit),
        "stitch alone, torch": lambda: torch_stitch(tiles, blend, limit),
    }
    assert not vae.use_tiling
    a, b = ops.blend_tiles(tiles, blend, limit), torch_stitch(tiles, blend, limit)
    diff = float((a.float() - b.float()).abs().max() / b.float().abs().max())
    assert a.shape == b.shape == (1, 3, 1024, 1024) and diff < 1e-2, diff  # the torch path rounds to fp16 after every blend
    times = {k: [] for k in cases}
    for fn in cases.values():
        for _ in range(WARMUP):
            fn()
    for _ in range(ROUNDS):  # alternated: every round times every case once
        for k, fn in cases.items():
            times[k].append(timed(fn))
    peaks = {k: peak_mib(cases[k]) for k in ("plain decode", "tiled_decode, fused stitch", "tiled_decode, torch stitch",
                                             "tiled_decode, 1 tile / call")}

    med = {k: statistics.median(v) for k, v in times.items()}
    lines = [
        "VAE tiling (AutoencoderKL.enable_tiling; ur_blend_tiles, csrc/vaetile.hip) -- one MI355X, SD-size VAE, random weights, fp16,",
        f"B = 1, latent 128 x 128 -> 1024 x 1024; tools/vae_tiling_bench.py.  {ntiles} tiles ({len(tiles)} x {len(tiles[0])}), blend {blend}, limit {limit}.",
        f"Host clock around {ITERS} calls ending in a device synchronise, {ROUNDS} rounds with the cases alternated, {WARMUP} warm-up calls each;",
        "ms per call: every round, then the median.  Eager launches (no graph): the torch stitch is bound by its launch count.",
        "",
    ]
    for k, v in times.items():
        lines.append(f"  {k:<28s} " + " ".join(f"{t:9.3f}" for t in v) + f"   median {med[k]:9.3f} ms")
    fs, ts = med["stitch alone, fused"], med["stitch alone, torch"]
    lines += [
        "",
        f"  stitch alone: fused {fs:.3f} ms against torch {ts:.3f} ms = {ts / fs:.1f}x" + ("" if fs < ts else "   (the fused stitch is NOT faster)"),
        f"  tiled_decode: fused stitch {med['tiled_decode, fused stitch']:.3f} ms against torch stitch {med['tiled_decode, torch stitch']:.3f} ms;"
        f" one tile per call {med['tiled_decode, 1 tile / call']:.3f} ms; plain decode {med['plain decode']:.3f} ms",
        f"  fused against torch stitch of the same tiles: max |difference| / max |value| = {diff:.2e} (the torch path rounds to fp16 after every blend)",
        "",
        "peak allocated memory above the weights and the latent, one call (MiB).  Equal tiles run as one batch (the four 512 x 512",
        "tiles of this grid in one network call); '1 tile / call' is this tool's own loop, not a mode of the package:",
    ]
    lines += [f"  {k:<28s} {v:10.1f}" for k, v in peaks.items()]
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "vae_tiling_ab.txt"))
