"""Host side of ur_cond_conv3x3_dgrad / ur_cond_conv3x3_wgrad without a GPU: the proof that the bounds of util_condconv_bwd.py
fit correct fp32 arithmetic in two summation orders on every problem and reject the damaged outputs, the ``w_rot`` image read
back by the header's formula, the launchers' refusals (they come before any launch) and the ``bgr`` gradient flip."""
import pytest
import torch

import util_condconv_bwd as CB
from uni_renderer_amd import _lib, ops

UR_E_BADARG, UR_E_UNSUPPORTED = _lib.ABI.UR_E_BADARG, _lib.ABI.UR_E_UNSUPPORTED

IDS = [f"{a}to{b}s{s}" for a, b, s in CB.LAYERS]


@pytest.mark.parametrize("dtype", CB.DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("layer", CB.LAYERS, ids=IDS)
def test_correct_fp32_arithmetic_stays_inside_the_bounds(layer, dtype):
    cin, cout, s = layer
    worst = {"dx": 0.0, "dw": 0.0, "db": 0.0}
    for H, W in CB.MAPS:
        p = CB.problem(cin, cout, s, H, W, dtype, family="gauss")
        for order in ("seq", "pair"):
            worst["dx"] = max(worst["dx"], CB.over(CB.emulate_dx(p, order), p["dx"], CB.bound_dx(p)))
            dw, db = CB.emulate_dw(p, order)
            worst["dw"] = max(worst["dw"], CB.over(dw, p["dw"], CB.bound_dw(p)))
            worst["db"] = max(worst["db"], CB.over(db, p["db"], CB.bound_db(p)))
    print(f"{layer} {dtype}: worst |err| / bound dx {worst['dx']:.3f} dw {worst['dw']:.3f} db {worst['db']:.3f}")
    assert max(worst.values()) <= 1.0


@pytest.mark.parametrize("dtype", CB.DTYPES, ids=["fp16", "bf16"])
def test_image_mode_emulation_stays_inside_the_bound(dtype):
    for cin, xdt in CB.IMAGE:
        p = CB.problem(cin, 16, 1, 33, 19, dtype, family="gauss", image=True, x_dtype=xdt)
        dw, db = CB.emulate_dw(p, "pair")
        assert CB.over(dw, p["dw"], CB.bound_dw(p)) <= 1.0 and CB.over(db, p["db"], CB.bound_db(p)) <= 1.0


@pytest.mark.parametrize("dtype", CB.DTYPES, ids=["fp16", "bf16"])
def test_emulation_is_exact_on_integer_data(dtype):
    for cin, cout, s in [(16, 32, 2), (32, 32, 1)]:
        p = CB.problem(cin, cout, s, 33, 19, dtype)
        assert torch.equal(CB.emulate_dx(p, "pair"), p["dx"])
        dw, db = CB.emulate_dw(p, "pair")
        assert torch.equal(dw, p["dw"]) and torch.equal(db, p["db"])


@pytest.mark.parametrize("family", ["int", "gauss"])
@pytest.mark.parametrize("dtype", CB.DTYPES, ids=["fp16", "bf16"])
def test_damaged_outputs_are_rejected(dtype, family):
    def rejected(got, ref, bound):
        return not torch.equal(got, ref) if family == "int" else CB.over(got, ref, bound) > 1.0

    s1 = CB.problem(32, 32, 1, 33, 19, dtype, family=family)
    s2 = CB.problem(32, 96, 2, 33, 19, dtype, family=family)
    for name, p, fn in [("corner tap", s1, CB.damaged_dx_corner_tap), ("neighbour halo", s1, CB.damaged_dx_neighbour_halo),
                        ("parity classes", s2, CB.damaged_dx_parity_swapped), ("last odd column", s2, CB.damaged_dx_last_odd_column)]:
        assert rejected(fn(p), p["dx"], CB.bound_dx(p)), f"dgrad with a damaged {name} passes"
    for p in (s1, s2):
        dw, db = CB.damaged_dw_tail_chunk(p)
        assert rejected(dw, p["dw"], CB.bound_dw(p)) and rejected(db, p["db"], CB.bound_db(p)), "a dropped tail chunk passes"
        assert rejected(CB.damaged_dw_taps_transposed(p), p["dw"], CB.bound_dw(p)), "ky / kx transposed passes"


@pytest.mark.parametrize("layer", CB.LAYERS, ids=IDS)
def test_rot_image_read_by_the_header_formula(layer):
    from uni_renderer_amd import packs as R
    from uni_renderer_amd.layers import Conv2d, PackCache, one, pack_cond_conv3x3_rot

    cin, cout, s = layer
    w4 = torch.randn(cout, cin, 3, 3, generator=torch.Generator().manual_seed(cin + cout), dtype=torch.float64)
    cc = ops.cond_conv_kchunk(cout, 1, False)
    packed = pack_cond_conv3x3_rot(w4, torch.float64)
    assert packed.numel() == ops.cond_conv_weight_numel(cout, cin, 1, False)
    back, pad_zero = CB.unpack_rot(packed, cin, cout, cc)
    assert torch.equal(back, w4) and pad_zero
    conv = Conv2d(cin, cout, 3, padding=1, stride=s)
    got = one(PackCache(), R.cond_conv3x3_rot, conv, torch.float16)
    assert torch.equal(got, pack_cond_conv3x3_rot(conv.weight, torch.float16))
    assert R.cond_conv3x3_rot.params(conv) == (conv.weight,)


def _args(**kw):
    a = dict(B=1, H=8, W=8, Cin=16, Cout=16, stride=1, dtype=ops.DT[torch.float16], p=1 << 12)
    a.update(kw)
    return a


def _dgrad(lib, **kw):
    a = _args(**kw)
    p = a["p"]
    return lib.ur_cond_conv3x3_dgrad(kw.get("dy", p), kw.get("w", p), kw.get("dx", p), a["B"], a["H"], a["W"], a["Cin"], a["Cout"],
                                     a["stride"], a["dtype"], None)


def _wgrad(lib, **kw):
    a = _args(**kw)
    p = a["p"]
    nchw = kw.get("x_nchw", 0)
    return lib.ur_cond_conv3x3_wgrad(kw.get("x", p), kw.get("x_dtype", a["dtype"]), nchw, kw.get("dy", p), kw.get("dw", p),
                                     kw.get("db", p), kw.get("ws", p), kw.get("ws_bytes", 1 << 40), a["B"], a["H"], a["W"], a["Cin"],
                                     a["Cout"], a["stride"], kw.get("splits", 0), a["dtype"], None)


def test_bad_arguments_return_their_codes_without_a_launch():
    """The pointers are never dereferenced and no GPU is present: every refusal comes before a launch."""
    lib = _lib.load()
    for call in (_dgrad, _wgrad):
        assert call(lib, B=0) == UR_E_BADARG and call(lib, H=-1) == UR_E_BADARG and call(lib, dtype=99) == UR_E_BADARG
        assert call(lib, dy=None) == UR_E_BADARG and call(lib, dy=(1 << 12) + 2) == UR_E_BADARG
        assert call(lib, stride=3) == UR_E_UNSUPPORTED and call(lib, Cout=24) == UR_E_UNSUPPORTED
        assert call(lib, Cin=272) == UR_E_UNSUPPORTED and call(lib, Cout=512) == UR_E_UNSUPPORTED
    assert _dgrad(lib, w=None) == UR_E_BADARG and _dgrad(lib, dx=None) == UR_E_BADARG and _dgrad(lib, Cin=3) == UR_E_UNSUPPORTED
    assert _wgrad(lib, dw=None, db=None) == UR_E_BADARG and _wgrad(lib, ws=None) == UR_E_BADARG
    assert _wgrad(lib, splits=-1) == UR_E_BADARG and _wgrad(lib, splits=1 << 20) == UR_E_UNSUPPORTED
    assert _wgrad(lib, ws_bytes=16) == UR_E_BADARG and _wgrad(lib, x_dtype=ops.DT_ANY[torch.float32]) == UR_E_BADARG
    assert _wgrad(lib, x_nchw=1, Cin=5) == UR_E_UNSUPPORTED and _wgrad(lib, Cin=3) == UR_E_UNSUPPORTED
    ws = lib.ur_cond_conv3x3_wgrad_workspace
    assert ws(1, 8, 8, 16, 16, 1, 0, 3) == 3 * (16 * 16 * 9 + 16) * 4
    assert ws(1, 8, 8, 3, 16, 1, 1, 2) == 2 * (16 * 16 * 9 + 16) * 4  # image mode: the partials are 16 channels wide
    assert ws(2, 33, 19, 16, 16, 1, 0, 0) == ws(2, 33, 19, 16, 16, 1, 0, 0) > 0
    assert ws(1, 8, 8, 24, 16, 1, 0, 0) == UR_E_UNSUPPORTED and ws(0, 8, 8, 16, 16, 1, 0, 0) == UR_E_BADARG


def test_python_layer_refuses_cpu_tensors_and_wrong_shapes():
    z = torch.zeros
    with pytest.raises(RuntimeError):
        ops.cond_conv3x3_dgrad(z(1, 4, 4, 16, dtype=torch.float16), z(1, dtype=torch.float16), in_hw=(4, 4), n_in=16)
    with pytest.raises(RuntimeError):
        ops.cond_conv3x3_wgrad(z(1, 4, 4, 16, dtype=torch.float16), z(1, 4, 4, 16, dtype=torch.float16))


def test_bgr_gradient_is_the_flip_along_the_channel_axis():
    """A `bgr` first layer convolves flip(W) with the image as it lies, so d loss / d W = flip(d loss / d flip(W)): the float64
    autograd of that statement, which autograd_ops.CondConv3x3 restates with the kernel's gradient."""
    g = torch.Generator().manual_seed(5)
    img = torch.randn(2, 3, 9, 7, generator=g, dtype=torch.float64)
    w = torch.randn(16, 3, 3, 3, generator=g, dtype=torch.float64, requires_grad=True)
    dy = torch.randn(2, 16, 9, 7, generator=g, dtype=torch.float64)
    torch.nn.functional.conv2d(img.flip(1), w, padding=1).backward(dy)  # the reference: the image flipped to rgb
    as_it_lies = CB.wgrad64(dy, img, 1)                               # what the kernel computes on the image in memory
    assert torch.allclose(as_it_lies.flip(1), w.grad, rtol=1e-12, atol=1e-12)
    assert not torch.allclose(as_it_lies, w.grad, rtol=1e-3, atol=1e-3)
