"""GPU tests of ``ur_view_blend`` (csrc/multidiff.hip) per element: ``master``, ``lat`` and ``global`` against the numpy fp32
emulation of the kernel's operation order (bit-equal: the kernel has only ordered adds, one correctly rounded division and
one rounding, so the equality is derived, not measured), against float64 exactly on integer data and within the derived bound
on N(0, 1) data, with NaN guards round all three buffers and everything the kernel must not touch compared bitwise."""
import ctypes

import numpy as np
import pytest
import torch

import util_multidiffusion as R
from uni_renderer_amd import multidiffusion as M

pytestmark = pytest.mark.gpu
GUARD = 64  # elements of NaN in front of and behind every buffer

#            H   W  window stride C
GEOMETRIES = [(16, 12, 8, 4, 3),   # the vector path: stride and window multiples of 4
              (6, 6, 4, 1, 3),     # counts 1, 2, 3 per axis
              (14, 14, 8, 2, 2),   # stride 2: one element per thread
              (16, 16, 8, 1, 2),   # 81 views, the cover cap of 64
              (16, 16, 8, 8, 3),   # no overlap
              (8, 8, 8, 8, 5),     # one view
              (24, 32, 16, 8, 24),  # the pipeline tests' geometry: 24 attribute channels ...
              (24, 32, 16, 8, 4)]   # ... and the 4 image channels
INT_BITS = {torch.float32: torch.int32, torch.float16: torch.int16, torch.bfloat16: torch.int16}


def _bits(t, nan_payloads=True):
    """The bits; ``nan_payloads=False``: every NaN as one value (a NaN's payload and sign through an add, a division and a
    conversion are the hardware's business)."""
    if not nan_payloads:
        return torch.nan_to_num(t.float(), nan=12345.0, posinf=float("inf"), neginf=-float("inf"))
    return t.view(INT_BITS[t.dtype])


def _guarded(n, dtype, dev):
    """A flat NaN buffer of n elements plus guards, and its payload."""
    flat = torch.full((n + 2 * GUARD,), float("nan"), dtype=dtype, device=dev)
    return flat, flat[GUARD:GUARD + n]


def _run(dev, geo, C, N, halves, dt, round_master, data, extra, with_lat=True, nan_payloads=True):
    """One launch on guarded buffers; asserts the bits of all three buffers and returns the global (numpy)."""
    from uni_renderer_amd import ops

    V, plane = geo.num_views, geo.wh * geo.ww
    NV = N * V
    m_flat, m_pay = _guarded(NV * C * plane, torch.float32, dev)
    master = m_pay.view(NV, C, geo.wh, geo.ww)
    master.copy_(data)
    g_flat, g_pay = _guarded(N * C * geo.height * geo.width, torch.float32, dev)
    glob = g_pay.view(N, C, geo.height, geo.width)
    # lat: channels 4.. of a (C + 4)-channel buffer with `extra` elements between two samples and one more sample behind
    bs, rows = (C + 4) * plane + extra, halves * NV + 1
    l_flat, l_pay = _guarded(rows * bs, dt, dev)
    gen = torch.Generator().manual_seed(1)
    buf = torch.as_strided(l_pay, (rows, C + 4, geo.wh, geo.ww), (bs, plane, geo.ww, 1))
    buf.copy_(torch.randn(buf.shape, generator=gen).to(dt))
    lat = buf[:halves * NV, 4:]
    want_l = l_flat.clone()
    em_m, em_l, em_g = R.blend_fp32_emulation(data.numpy(), geo.views, geo.height, geo.width, dt, round_master, halves)
    if with_lat:
        torch.as_strided(want_l[GUARD:GUARD + rows * bs], (rows, C + 4, geo.wh, geo.ww), (bs, plane, geo.ww, 1))[:halves * NV, 4:] = em_l.to(dev)
    ops.view_blend(master, lat if with_lat else None, glob, geo, halves=halves, round_master=round_master)
    torch.cuda.synchronize()
    tag = (tuple(geo), C, N, halves, dt, round_master, extra, with_lat)
    # lat: the slice is the emulation; the mask channels, the gaps, the sample behind and the NaN guards are untouched
    assert torch.equal(_bits(l_flat, nan_payloads), _bits(want_l, nan_payloads)), tag
    want_m = torch.full_like(m_flat, float("nan"))
    want_m[GUARD:-GUARD] = torch.from_numpy(em_m).reshape(-1).to(dev)
    assert torch.equal(_bits(m_flat, nan_payloads), _bits(want_m, nan_payloads)), tag
    want_g = torch.full_like(g_flat, float("nan"))
    want_g[GUARD:-GUARD] = torch.from_numpy(em_g).reshape(-1).to(dev)
    assert torch.equal(_bits(g_flat, nan_payloads), _bits(want_g, nan_payloads)), tag
    return glob.cpu().numpy()


@pytest.mark.parametrize("H,W,window,stride,C", GEOMETRIES)
def test_view_blend_bits_guards_and_bounds(dev, H, W, window, stride, C):
    geo = M.view_geometry(H, W, window, stride)
    assert geo.views == R.windows(H, W, window, stride)
    gen = torch.Generator().manual_seed(H * 1000 + W * 10 + stride)
    case = 0
    for N in (1, 3):
        shape = (N * geo.num_views, C, geo.wh, geo.ww)
        normal = torch.randn(shape, generator=gen)
        ints = torch.randint(-15, 16, shape, generator=gen).float()
        g64n, magn, cnt = R.blend_f64(normal.numpy(), geo.views, H, W)
        g64i, magi, _ = R.blend_f64(ints.numpy(), geo.views, H, W)
        pow2 = (cnt & (cnt - 1)) == 0
        for halves in (1, 2):
            for dt in (torch.float32, torch.float16, torch.bfloat16):
                for rm in (False, True):
                    extra = (0, 8, 3)[case % 3]  # batch strides that keep / break the 16-byte alignment of the vector path
                    case += 1
                    g = _run(dev, geo, C, N, halves, dt, rm, normal, extra)
                    if not rm:  # N(0, 1): the derived bound (with round_master the 16-bit rounding comes on top: bits only)
                        assert (np.abs(g.astype(np.float64) - g64n) <= R.bound(g64n, magn, cnt)).all()
                    # small integers: |sum| <= 15 * 64, means over 1, 2, 4, ... views are k / 64 at most: exact in fp32 and, for
                    # counts <= 4 (|mean| <= 15 in quarters: 6 bits), in fp16 and bf16 too
                    g = _run(dev, geo, C, N, halves, dt, rm, ints, extra)
                    exact = pow2 if (not rm or dt == torch.float32) else (pow2 & (cnt <= 4))
                    assert np.array_equal(g.astype(np.float64)[:, :, exact], g64i[:, :, exact])
                    if not rm:
                        assert (np.abs(g.astype(np.float64) - g64i) <= R.bound(g64i, magi, cnt)).all()
    _run(dev, geo, C, 1, 1, torch.float32, False, normal[:geo.num_views], 0, with_lat=False)  # no latent slice: master, global


@pytest.mark.parametrize("H,W,window,stride,C,N", [(128, 128, 64, 32, 24, 6),  # vector path: 589 824 groups of four
                                                   (62, 62, 8, 6, 24, 6),      # element path: 553 536 elements
                                                   (128, 128, 64, 8, 24, 1)])  # the 81 views of diffusers' defaults at 1024 x 1024
def test_view_blend_past_one_grid_and_at_the_real_size(dev, H, W, window, stride, C, N):
    """The launch takes at most 2048 workgroups of 256 threads and strides over the rest: more than 524 288 work items on
    either path; and the largest real case (window 64, stride 8: 81 views, 64 over the centre).  Bits and guards as above."""
    geo = M.view_geometry(H, W, window, stride)
    data = torch.randn(N * geo.num_views, C, geo.wh, geo.ww, generator=torch.Generator().manual_seed(H + stride))
    g = _run(dev, geo, C, N, 2, torch.float16, False, data, 8)
    g64, mag, cnt = R.blend_f64(data.numpy(), geo.views, H, W)
    assert (np.abs(g.astype(np.float64) - g64) <= R.bound(g64, mag, cnt)).all()


def test_view_blend_keeps_signs_nans_and_infinities_of_its_inputs(dev):
    """0 + (-0) = +0 (the sum starts from zero, as the torch definition), a NaN or an infinity in one view reaches exactly the
    global elements that view covers."""
    geo = M.view_geometry(16, 12, 8, 4)
    data = torch.randn(geo.num_views, 2, 8, 8, generator=torch.Generator().manual_seed(2))
    data[0, 0, 0, 0] = -0.0
    data[1, 1, 5, 5] = float("nan")
    data[4, 0, 2, 3] = float("inf")
    g = _run(dev, geo, 2, 1, 2, torch.float16, True, data, 8, nan_payloads=False)
    assert np.signbit(g[0, 0, 0, 0]) == False and int(np.isnan(g).sum()) == 1 and int(np.isinf(g).sum()) == 1  # noqa: E712


def test_view_blend_error_codes(dev):
    from uni_renderer_amd import _lib, ops

    lib, E = _lib.load(), _lib.ABI
    m = torch.zeros(81 * 9 * 9, device=dev)
    g = torch.zeros(17 * 17, device=dev)
    lat = torch.zeros(2 * 81 * 9 * 9, device=dev, dtype=torch.float16)
    P = lambda t: ctypes.c_void_p(t.data_ptr())

    def call(master=m, lt=lat, bs=81, glob=g, N=1, C=1, rows=9, cols=9, wh=9, ww=9, sy=1, sx=1, halves=1, rm=0, dtype=E.UR_DT_F16):
        return lib.ur_view_blend(P(master) if master is not None else None, P(lt) if lt is not None else None, bs,
                                 P(glob) if glob is not None else None, N, C, rows, cols, wh, ww, sy, sx, halves, rm, dtype, None)

    assert call() == E.UR_E_UNSUPPORTED  # 9 x 9 = 81 views cover the centre pixel
    assert call(rows=8, cols=8, wh=8, ww=8) == 0  # 64 do
    assert call(rows=2, cols=2, wh=4, ww=4, sy=5, sx=4) == E.UR_E_BADARG  # a stride above the window: uncovered pixels
    assert call(rows=2, cols=2, wh=4, ww=4, sy=4, sx=4, bs=16) == 0
    for bad in (dict(master=None), dict(glob=None), dict(N=0), dict(C=0), dict(rows=0), dict(ww=0), dict(sx=0), dict(halves=0),
                dict(halves=3), dict(dtype=7), dict(rows=2, cols=2, wh=4, ww=4, sy=4, sx=4, bs=15)):
        assert call(**bad) == E.UR_E_BADARG, bad
    torch.cuda.synchronize()
    with pytest.raises(NotImplementedError, match="81"):
        ops.view_blend(m.view(81, 1, 9, 9), None, g.view(1, 1, 17, 17), M.ViewGeometry(9, 9, 9, 9, 1, 1))
    with pytest.raises(RuntimeError, match="contiguous channel planes"):
        ops.view_blend(torch.zeros(4, 2, 4, 4, device=dev), torch.zeros(4, 4, 4, 2, device=dev).permute(0, 3, 1, 2),
                       torch.zeros(1, 2, 8, 8, device=dev), M.ViewGeometry(2, 2, 4, 4, 4, 4))
