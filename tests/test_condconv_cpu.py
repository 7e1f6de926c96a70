"""Host side of ur_cond_conv3x3 without a GPU: the launcher's refusals, the packed weight image, and the proof that the
per-element bound of test_condconv_gpu.py (util_condconv.bound) fits a correct kernel with room and rejects the three
indexing errors a halo-staged conv is prone to."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import util_condconv as CCV
from util_igemm import TOL, check_elem


def _call(lib, **kw):
    a = dict(x=4096, x_dtype=0, x_nchw=0, w=8192, bias=12288, out=16384, B=1, H=8, W=8, Cin=16, Cout=16, stride=1, act=0,
             dtype=0)
    a.update(kw)
    return lib.ur_cond_conv3x3(a["x"], a["x_dtype"], a["x_nchw"], a["w"], a["bias"], a["out"], a["B"], a["H"], a["W"],
                               a["Cin"], a["Cout"], a["stride"], a["act"], a["dtype"], None)


def test_launcher_refuses_before_any_launch():
    """The addresses are never dereferenced: every call below returns from the argument checks."""
    from uni_renderer_amd import _lib

    lib = _lib.load()
    BAD, UNS = _lib.ABI.UR_E_BADARG, _lib.ABI.UR_E_UNSUPPORTED
    for name in ("x", "w", "bias", "out"):
        assert _call(lib, **{name: None}) == BAD, name
    assert _call(lib, B=0) == BAD and _call(lib, H=0) == BAD and _call(lib, W=-1) == BAD
    assert _call(lib, dtype=2) == BAD and _call(lib, dtype=7) == BAD
    assert _call(lib, x_dtype=1) == BAD          # NHWC input in another type than the compute dtype
    assert _call(lib, x_nchw=1, Cin=3, x_dtype=5) == BAD
    assert _call(lib, act=_lib.ABI.UR_ACT_GEGLU) == BAD
    assert _call(lib, out=16384 + 8) == BAD and _call(lib, x=4096 + 2) == BAD  # alignment
    assert _call(lib, stride=3) == UNS and _call(lib, stride=0) == UNS
    assert _call(lib, Cin=24) == UNS and _call(lib, Cin=272) == UNS and _call(lib, Cin=3) == UNS
    assert _call(lib, Cout=272) == UNS and _call(lib, Cout=24) == UNS
    assert _call(lib, x_nchw=1, Cin=5, x_dtype=2) == UNS
    # the k chunk the weight image is laid out by
    k = lib.ur_cond_conv3x3_kchunk
    assert [k(16, 1, 0), k(32, 1, 0), k(96, 1, 0), k(48, 1, 0), k(32, 2, 0), k(96, 2, 0), k(3, 1, 1), k(4, 2, 1)] == [16, 32, 32, 16, 16, 16, 8, 8]
    assert k(24, 1, 0) == UNS and k(16, 3, 0) == UNS and k(5, 1, 1) == UNS


def test_ops_wrapper_has_no_cpu_fallback():
    from uni_renderer_amd import ops

    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.cond_conv3x3(torch.zeros(1, 4, 4, 16, dtype=torch.float16), torch.zeros(1), torch.zeros(16), n_out=16)


@pytest.mark.parametrize("cin,cout,stride,image", [(16, 16, 1, False), (16, 32, 2, False), (32, 32, 1, False), (32, 96, 2, False),
                                                   (96, 96, 1, False), (96, 256, 2, False), (48, 80, 1, False), (80, 48, 2, False),
                                                   (3, 16, 1, True), (1, 16, 1, True), (4, 32, 2, True)])
def test_packed_weights_round_trip(cin, cout, stride, image):
    """A float64 conv over the weights read back from the PACKED image (by the header's formula, not by the packer's code)
    equals F.conv2d over the originals; padding entries are zero; the image has the documented size."""
    from uni_renderer_amd import ops
    from uni_renderer_amd.layers import pack_cond_conv3x3

    g = torch.Generator().manual_seed(cin * 1000 + cout)
    w4 = torch.randn(cout, cin, 3, 3, generator=g, dtype=torch.float64)
    x = torch.randn(2, cin, 9, 11, generator=g, dtype=torch.float64)
    cc = ops.cond_conv_kchunk(cin, stride, image)
    packed = pack_cond_conv3x3(w4, torch.float64, stride, image=image)
    assert packed.numel() == ops.cond_conv_weight_numel(cin, cout, stride, image)
    back, pad_zero = CCV.unpack(packed, cin, cout, cc)
    assert pad_zero
    xp = F.pad(x, (0, 0, 0, 0, 0, back.shape[1] - cin))
    assert torch.equal(CCV.conv64(xp, back, stride), CCV.conv64(x, w4, stride))
    if image and cin > 1:  # bgr: the flip happens on the weights' input-channel axis, the image is read as it lies
        back_bgr, _ = CCV.unpack(pack_cond_conv3x3(w4, torch.float64, stride, image=True, bgr=True), cin, cout, cc)
        assert torch.equal(back_bgr[:, :cin], w4.flip(1)) and not torch.equal(back_bgr, back)
        # (the channel order of the sum differs, so float64 agrees to its own rounding, not bit for bit)
        torch.testing.assert_close(CCV.conv64(xp, back_bgr, stride), CCV.conv64(x.flip(1), w4, stride), rtol=0, atol=1e-12)


@pytest.mark.parametrize("dtype", CCV.DTYPES)
def test_exact_family_is_exact(dtype):
    """Every exact-family problem of the GPU file holds integers below 2^24 (asserted by ``problem``) and a correct kernel
    reproduces the reference bit for bit."""
    for cin, cout, stride in CCV.CHAIN + CCV.EXTRA:
        p = CCV.problem(cin, cout, stride, 5, 7, dtype)
        assert torch.equal(CCV.emulate(p), p["ref"])
    for cin, xdt in CCV.IMAGE:
        p = CCV.problem(cin, 16, 1, 5, 7, dtype, image=True, x_dtype=xdt)
        assert torch.equal(CCV.emulate(p), p["ref"])


@pytest.mark.parametrize("dtype", CCV.DTYPES)
def test_bound_fits_a_correct_kernel_with_room(dtype):
    """The float64 emulation with exactly a correct kernel's roundings (input to dtype, exact sum rounded to fp32, fp32 SiLU,
    one output rounding) against the per-element bound, on every layer.  The margin of one half is held where a margin can
    exist, as test_igemm_bounds_cpu.py holds it: the fp32 value BEFORE the storage rounding stays within HALF of the fp32
    part of the bound.  The stored value is held to the whole bound: round-to-nearest itself reaches u |v| just above a
    power of two (the emulation's stored values reach 0.94 of the bound in fp16 and 0.97 in bf16 from that rounding alone), so no correct
    kernel can stay within half of the u |v| term."""
    worst32 = worst = 0.0
    cases = [CCV.problem(cin, cout, stride, 33, 19, dtype, family="gauss") for cin, cout, stride in CCV.CHAIN + CCV.EXTRA]
    cases.append(CCV.problem(3, 16, 1, 33, 19, dtype, family="gauss", image=True, x_dtype=torch.float32))
    for p in cases:
        what = f"{p['cin']}->{p['cout']} s{p['stride']}"
        _, r32 = check_elem(CCV.finish32(p["pre"], p), p["ref"], p["fp"], TOL[dtype], what + " before storing", frac=0.5)
        _, r = check_elem(CCV.emulate(p), p["ref"], CCV.bound(p), TOL[dtype], what)
        worst32, worst = max(worst32, r32), max(worst, r)
    print(f"{dtype}: worst |err| / fp32 part before storing {worst32:.3f}, worst |err| / bound of the stored value {worst:.3f}")


@pytest.mark.parametrize("dtype", CCV.DTYPES)
def test_bound_rejects_damaged_outputs(dtype):
    s1 = CCV.problem(32, 32, 1, 33, 19, dtype, family="gauss")
    s2 = CCV.problem(16, 32, 2, 33, 19, dtype, family="gauss")
    for name, p, bad in [("corner tap dropped", s1, CCV.damaged_corner_tap(s1)),
                         ("corner tap dropped, stride 2", s2, CCV.damaged_corner_tap(s2)),
                         ("halo row of the neighbouring sample", s1, CCV.damaged_neighbour_halo(s1)),
                         ("last odd column shifted", s2, CCV.damaged_last_odd_column(s2))]:
        assert not torch.equal(bad, CCV.emulate(p)), name
        with pytest.raises(AssertionError, match="worst"):
            check_elem(bad, p["ref"], CCV.bound(p), TOL[dtype], name)
