"""VAE tiling and slicing without a device: the tile geometry, the closed form of the sequential in-place stitch (and that it
is NOT the blend against raw neighbours), the surface on ``AutoencoderKL`` / ``UniRendererPipeline`` and the launcher's
argument checks."""
import ctypes

import pytest
import torch

import util_vae_tiling as T


# ---------------------------------------------------------------------------------------------------------------------
# geometry
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile", [8, 64])
@pytest.mark.parametrize("scale", [2, 8])
def test_decode_geometry_covers_every_length(tile, scale):
    from uni_renderer_amd.vae import tile_axis

    for length in range(tile + 1, 4 * tile + 1):
        ax = tile_axis(length, tile, tile * scale, 0.25, lambda n: n * scale)
        overlap, blend = int(tile * 0.75), int(tile * scale * 0.25)
        assert ax.blend == blend and ax.limit == tile * scale - blend
        assert ax.positions == tuple(range(0, length, overlap))
        assert all(p + n <= length and n == min(tile, length - p) for p, n in zip(ax.positions, ax.lengths))
        assert ax.out_lengths == tuple(n * scale for n in ax.lengths)
        assert sum(ax.kept) == scale * length, (length, ax)
        assert all(n >= 2 * blend for n in ax.out_lengths[:-1]), (length, ax)
        assert ax.extents[0] == 0 and all(e == min(a, b, blend) for e, a, b in zip(ax.extents[1:], ax.out_lengths, ax.out_lengths[1:]))
        assert ax.kept == tuple(min(ax.limit, n) for n in ax.out_lengths)


@pytest.mark.parametrize("tile", [8, 64])
@pytest.mark.parametrize("scale", [2, 8])
def test_encode_geometry_is_the_mirror_image(tile, scale):
    """Stepping in pixels, blending in latents: for every pixel length that is a multiple of the scale."""
    from uni_renderer_amd.vae import tile_axis

    sample = tile * scale
    for length in range(sample + scale, 4 * sample + 1, scale):
        ax = tile_axis(length, sample, tile, 0.25, lambda n: n // scale)
        assert ax.blend == int(tile * 0.25) and ax.limit == tile - ax.blend
        assert ax.positions == tuple(range(0, length, int(sample * 0.75)))
        assert sum(ax.kept) == length // scale, (length, ax)
        assert all(n >= 2 * ax.blend for n in ax.out_lengths[:-1])


def test_geometry_refuses_what_the_closed_form_does_not_cover():
    from uni_renderer_amd.vae import tile_axis

    with pytest.raises(NotImplementedError, match="tile_overlap_factor"):
        tile_axis(20, 8, 16, 0.5, lambda n: 2 * n)
    with pytest.raises(NotImplementedError):
        tile_axis(20, 8, 16, 0.34, lambda n: 2 * n)
    tile_axis(20, 8, 16, 1.0 / 3.0, lambda n: 2 * n)
    with pytest.raises(ValueError, match="no output"):  # a one-pixel encode tile has no latent
        tile_axis(25, 16, 8, 0.25, lambda n: n // 2)


def test_the_vae_geometry_is_the_issue_examples():
    import uni_renderer_amd as U

    vae = U.AutoencoderKL()  # SD: 512 px / 64 latents
    ay, ax = vae._tile_axes(128, 128, decode=True)
    assert ay == ax and ay.positions == (0, 48, 96) and ay.lengths == (64, 64, 32) and ay.blend == 128 and ay.limit == 384
    assert ay.kept == (384, 384, 256) and sum(ay.kept) == 1024
    tiny = U.AutoencoderKL(block_out_channels=(64, 128), layers_per_block=1, sample_size=16,
                           down_block_types=("DownEncoderBlock2D",) * 2, up_block_types=("UpDecoderBlock2D",) * 2)
    ay, ax = tiny._tile_axes(17, 14, decode=True)
    assert ay.out_lengths == (16, 16, 10) and ax.out_lengths == (16, 16, 4) and (sum(ay.kept), sum(ax.kept)) == (34, 28)
    ay, ax = tiny._tile_axes(34, 28, decode=False)
    assert ay.out_lengths == (8, 8, 5) and ax.out_lengths == (8, 8, 2) and (ay.blend, ay.limit) == (2, 6)
    assert (sum(ay.kept), sum(ax.kept)) == (17, 14)


# ---------------------------------------------------------------------------------------------------------------------
# the closed form
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hs,ws,blend,limit", [((16, 16, 10), (16, 16, 2), 4, 12), ((16, 12, 3), (13, 16, 5), 6, 10),
                                               ((16,), (16, 16, 7), 4, 12), ((16, 16, 1), (16,), 8, 8)])
def test_sequential_stitch_equals_the_four_tile_closed_form(hs, ws, blend, limit):
    tiles = T.make_tiles(hs, ws, 2, 3, torch.float64, seed=1)
    seq = T.stitch(tiles, blend, limit)
    val, err = T.closed_form(tiles, blend, limit)
    assert seq.shape == (2, 3, sum(min(limit, h) for h in hs), sum(min(limit, w) for w in ws))
    assert torch.equal(seq, val)  # the same float64 operations in the same order
    assert float(err.max()) < 1e-5 and bool((err >= 0).all())


def test_sequential_stitch_is_not_the_blend_against_raw_neighbours():
    """The aliasing the kernel must reproduce: in place, the neighbour a blend reads has been blended already."""
    hs, ws, blend, limit = (16, 16, 10), (16, 16, 2), 4, 12
    tiles = T.make_tiles(hs, ws, 1, 3, torch.float64, seed=2)
    seq, raw = T.stitch(tiles, blend, limit), T.stitch_raw_neighbours(tiles, blend, limit)
    corner = T.corner_mask(tiles, blend, limit)
    assert int(corner.sum()) == (4 + 4) * (4 + 2)
    assert torch.equal(seq[..., ~corner], raw[..., ~corner])           # edges and interiors: two tiles or one
    d = (seq - raw).abs()[..., corner]
    assert float((d > 1e-3).double().mean()) > 0.9, float((d > 1e-3).double().mean())


# ---------------------------------------------------------------------------------------------------------------------
# surface
# ---------------------------------------------------------------------------------------------------------------------
def test_flags_defaults_and_tile_sizes():
    import uni_renderer_amd as U

    vae = U.AutoencoderKL()
    assert (vae.use_tiling, vae.use_slicing) == (False, False)
    assert (vae.tile_sample_min_size, vae.tile_latent_min_size, vae.tile_overlap_factor) == (512, 64, 0.25)
    vae.enable_tiling()
    assert vae.use_tiling is True
    vae.enable_tiling(False)
    assert vae.use_tiling is False
    vae.enable_tiling()
    vae.disable_tiling()
    assert vae.use_tiling is False
    vae.enable_slicing()
    assert vae.use_slicing is True
    vae.disable_slicing()
    assert vae.use_slicing is False
    small = U.AutoencoderKL(block_out_channels=(64, 128), sample_size=16, down_block_types=("DownEncoderBlock2D",) * 2,
                            up_block_types=("UpDecoderBlock2D",) * 2)
    assert (small.tile_sample_min_size, small.tile_latent_min_size) == (16, 8)
    for name in ("tiled_decode", "tiled_encode", "enable_tiling", "disable_tiling", "enable_slicing", "disable_slicing"):
        assert callable(getattr(U.AutoencoderKL, name)), name


def test_pipeline_delegates_to_the_vae():
    import uni_renderer_amd as U

    vae = U.AutoencoderKL(block_out_channels=(64, 128), down_block_types=("DownEncoderBlock2D",) * 2,
                          up_block_types=("UpDecoderBlock2D",) * 2)
    pipe = U.UniRendererPipeline(vae=vae)
    pipe.enable_vae_tiling()
    assert vae.use_tiling and not vae.use_slicing
    pipe.enable_vae_slicing()
    assert vae.use_tiling and vae.use_slicing
    pipe.disable_vae_tiling()
    assert not vae.use_tiling and vae.use_slicing
    pipe.disable_vae_slicing()
    assert not vae.use_tiling and not vae.use_slicing


def test_symbols_are_exported_and_the_tiled_paths_have_no_cpu_fallback():
    import uni_renderer_amd as U
    from uni_renderer_amd import _lib, ops

    lib = _lib.load()
    for name in ("ur_blend_tiles", "ur_blend_tiles_max", "ur_blend_tiles_item_words"):
        assert name in _lib.SYMBOLS and hasattr(lib, name)
    assert lib.ur_blend_tiles_item_words() == ops.BLEND_ITEM_WORDS == 4
    assert ops.blend_tiles_max() == lib.ur_blend_tiles_max() >= 16      # a 3 x 3 grid and a row above fit one launch
    assert _lib.ABI_VERSION == 17
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.blend_tiles([[torch.zeros(1, 4, 4, 3, dtype=torch.float16)]], 1, 3)
    vae = U.AutoencoderKL(block_out_channels=(64, 128), sample_size=16, down_block_types=("DownEncoderBlock2D",) * 2,
                          up_block_types=("UpDecoderBlock2D",) * 2).half()
    vae.tile_overlap_factor = 0.5
    with pytest.raises(NotImplementedError, match="tile_overlap_factor"):
        vae.tiled_decode(torch.zeros(1, 4, 12, 12, dtype=torch.float16))


# ---------------------------------------------------------------------------------------------------------------------
# the launcher's checks (no launch happens: every case returns before it)
# ---------------------------------------------------------------------------------------------------------------------
_P = 0x7F0000001000  # a plausible, 16-byte aligned, never dereferenced device address


def _table(hs, ws, stride=None):
    words = []
    for i, h in enumerate(hs):
        for j, w in enumerate(ws):
            words += [_P + 0x100000 * (i * len(ws) + j), (h * w * 3) if stride is None else stride, h, w]
    return (ctypes.c_int64 * len(words))(*words)


def _call(table, rows=3, cols=3, above=0, B=1, C=3, blend=4, limit=12, out=_P - 0x1000, Hout=34, Wout=30, plane=None,
          tdt=0, odt=0):
    from uni_renderer_amd import _lib

    plane = Hout * Wout if plane is None else plane
    return _lib.load().ur_blend_tiles(table, rows, cols, above, B, C, blend, limit, out, Hout, Wout, plane, tdt, odt, None)


def test_launcher_rejects_bad_arguments_without_gpu():
    from uni_renderer_amd import _lib, ops

    A = _lib.ABI
    hs, ws = (16, 16, 10), (16, 16, 6)       # kept 12 + 12 + 10 = 34 rows, 12 + 12 + 6 = 30 columns
    ok = lambda: _table(hs, ws)
    bad = A.UR_E_BADARG
    assert _call(None) == bad                                             # null table
    assert _call(ok(), out=None) == bad                                   # null output
    assert _call(ok(), out=_P + 1) == bad                                 # misaligned output
    assert _call(ok(), out=_P + 2, odt=A.UR_DT_F32) == bad
    for kw in (dict(rows=0), dict(rows=-1), dict(cols=0), dict(cols=-2), dict(blend=-1), dict(limit=0), dict(limit=-5),
               dict(B=0), dict(C=0), dict(above=2), dict(above=-1), dict(Hout=33), dict(Hout=35), dict(Wout=29), dict(Wout=31),
               dict(Hout=0), dict(Wout=0), dict(plane=34 * 30 - 1), dict(tdt=2), dict(tdt=-1), dict(tdt=5), dict(odt=3),
               dict(odt=-1)):
        assert _call(ok(), **kw) == bad, kw
    for word, value in ((0, 0), (0, _P + 1), (1, -1), (2, 0), (2, -4), (3, 0), (3, -1), (2, 15), (3, 17), (2, 2 ** 31)):
        for tile in (0, 4, 8):                                            # every tile is checked, the last one too
            t = ok()
            t[4 * tile + word] = value
            assert _call(t) == bad, (word, value, tile)
    # with a row above: the first table row is read-only and adds nothing to Hout
    assert _call(_table((16,) + hs, ws), above=1, Hout=34 + 12) == bad
    # refused shapes: too many tiles, too many channels, a tile with a successor shorter than 2 * blend
    nmax = ops.blend_tiles_max()
    assert _call(_table((16,) * (nmax + 1), (16,)), rows=nmax + 1, cols=1, Hout=12 * (nmax + 1), Wout=12) == A.UR_E_UNSUPPORTED
    assert _call(_table((16,) * (nmax + 1), (16,)), rows=nmax, cols=1, above=1, Hout=12 * nmax, Wout=12) == A.UR_E_UNSUPPORTED
    assert _call(ok(), C=9) == A.UR_E_UNSUPPORTED
    assert _call(ok(), blend=9, limit=7, Hout=21, Wout=20) == A.UR_E_UNSUPPORTED
    assert _call(_table((16, 7, 10), ws), Hout=12 + 7 + 10) == A.UR_E_UNSUPPORTED
    assert _call(_table((7,) + hs, ws), above=1) == A.UR_E_UNSUPPORTED
    # a bad tile behind a refused shape is still a bad argument
    t = _table((16, 7, 10), ws)
    t[4 * 8 + 0] = 0
    assert _call(t, Hout=12 + 7 + 10) == bad
    t = _table((16,) * (nmax + 1), (16,))
    t[4 * nmax + 3] = 0
    assert _call(t, rows=nmax + 1, cols=1, Hout=12 * (nmax + 1), Wout=12) == bad
