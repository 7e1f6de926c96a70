"""ur_cond_conv3x3_dgrad / ur_cond_conv3x3_wgrad (csrc/condconv_bwd.hip) on the GPU, per element: exact on integer data for every
layer x map x dtype and every forced split, within the derived bounds on N(0, 1) data (util_condconv_bwd.py;
test_condconv_bwd_cpu.py shows that the bounds fit correct arithmetic and reject the damaged outputs), bit-reproducible.  Every
operand sits in a NaN-filled guard buffer and every output in a sentinel buffer that must come back untouched outside its
extent; no element is left out of a comparison."""
import pytest
import torch

import util_condconv_bwd as CB
from util_igemm import check_exact

pytestmark = pytest.mark.gpu

IDS = [f"{a}to{b}s{s}" for a, b, s in CB.LAYERS]
IMG_IDS = [f"{c}ch_{str(xdt)[6:]}" for c, xdt in CB.IMAGE]


@pytest.mark.parametrize("dtype", CB.DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("layer", CB.LAYERS, ids=IDS)
def test_exact_on_integer_data(dev, layer, dtype):
    cin, cout, s = layer
    for H, W in CB.MAPS:
        p = CB.problem(cin, cout, s, H, W, dtype)
        check_exact(CB.launch_dgrad(p, dev), p["dx"], CB.what(p) + " dx")
        dw, db = CB.launch_wgrad(p, dev)
        check_exact(dw.reshape(cout, -1), p["dw"].reshape(cout, -1), CB.what(p) + " dw")
        check_exact(db[None], p["db"][None], CB.what(p) + " db")


@pytest.mark.parametrize("dtype", CB.DTYPES, ids=["fp16", "bf16"])
def test_exact_with_three_samples(dev, dtype):
    for cin, cout, s in [(16, 32, 2), (32, 32, 1), (96, 256, 2)]:
        p = CB.problem(cin, cout, s, 33, 19, dtype, B=3)
        check_exact(CB.launch_dgrad(p, dev), p["dx"], CB.what(p) + " dx")
        dw, db = CB.launch_wgrad(p, dev)
        check_exact(dw.reshape(cout, -1), p["dw"].reshape(cout, -1), CB.what(p) + " dw")
        check_exact(db[None], p["db"][None], CB.what(p) + " db")


@pytest.mark.parametrize("splits", CB.SPLITS)
def test_wgrad_exact_for_every_split(dev, splits):
    for cin, cout, s, (H, W), dtype in [(16, 32, 2, (33, 19), torch.float16), (96, 96, 1, (40, 72), torch.bfloat16),
                                        (80, 48, 2, (40, 72), torch.float16), (32, 32, 1, (5, 7), torch.bfloat16)]:
        p = CB.problem(cin, cout, s, H, W, dtype)
        dw, db = CB.launch_wgrad(p, dev, splits=splits)
        check_exact(dw.reshape(cout, -1), p["dw"].reshape(cout, -1), CB.what(p) + f" dw splits={splits}")
        check_exact(db[None], p["db"][None], CB.what(p) + f" db splits={splits}")


@pytest.mark.parametrize("dtype", CB.DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("layer", CB.LAYERS, ids=IDS)
def test_gaussian_data_within_the_bounds(dev, layer, dtype):
    cin, cout, s = layer
    worst = {"dx": 0.0, "dw": 0.0, "db": 0.0}
    for H, W in CB.MAPS:
        p = CB.problem(cin, cout, s, H, W, dtype, family="gauss")
        dx = CB.launch_dgrad(p, dev)
        dw, db = CB.launch_wgrad(p, dev)
        assert torch.isfinite(dx).all() and torch.isfinite(dw).all() and torch.isfinite(db).all(), CB.what(p)
        worst["dx"] = max(worst["dx"], CB.over(dx, p["dx"], CB.bound_dx(p)))
        worst["dw"] = max(worst["dw"], CB.over(dw, p["dw"], CB.bound_dw(p)))
        worst["db"] = max(worst["db"], CB.over(db, p["db"], CB.bound_db(p)))
    print(f"{layer} {dtype}: worst |err| / bound dx {worst['dx']:.3f} dw {worst['dw']:.3f} db {worst['db']:.3f}")
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize("dtype", CB.DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("image", CB.IMAGE, ids=IMG_IDS)
def test_image_mode_wgrad(dev, image, dtype):
    cin, xdt = image
    for s, cout, (H, W) in [(1, 16, (33, 19)), (2, 32, (40, 72)), (1, 16, (5, 7))]:
        p = CB.problem(cin, cout, s, H, W, dtype, image=True, x_dtype=xdt)
        dw, db = CB.launch_wgrad(p, dev)
        check_exact(dw.reshape(cout, -1), p["dw"].reshape(cout, -1), CB.what(p) + " dw")
        check_exact(db[None], p["db"][None], CB.what(p) + " db")
        q = CB.problem(cin, cout, s, H, W, dtype, family="gauss", image=True, x_dtype=xdt)
        dw, db = CB.launch_wgrad(q, dev, splits=3)
        assert CB.over(dw, q["dw"], CB.bound_dw(q)) <= 1.0 and CB.over(db, q["db"], CB.bound_db(q)) <= 1.0, CB.what(q)


def test_dw_only_and_db_only(dev):
    p = CB.problem(32, 96, 2, 33, 19, torch.float16)
    dw, db = CB.launch_wgrad(p, dev, need_bias=False)
    assert db is None
    check_exact(dw.reshape(96, -1), p["dw"].reshape(96, -1), "dw only")
    dw, db = CB.launch_wgrad(p, dev, need_dw=False)
    assert dw is None
    check_exact(db[None], p["db"][None], "db only")


def test_twenty_launches_give_identical_bytes(dev):
    p = CB.problem(32, 96, 2, 33, 19, torch.float16, family="gauss")
    dx0, (dw0, db0) = CB.launch_dgrad(p, dev), CB.launch_wgrad(p, dev)
    for _ in range(19):
        assert torch.equal(CB.launch_dgrad(p, dev), dx0)
        dw, db = CB.launch_wgrad(p, dev)
        assert torch.equal(dw, dw0) and torch.equal(db, db0)


def test_bad_arguments_return_their_codes_without_a_launch(dev):
    from uni_renderer_amd import _lib, ops

    lib = _lib.load()
    BAD, UNS = _lib.ABI.UR_E_BADARG, _lib.ABI.UR_E_UNSUPPORTED
    t = torch.zeros(1 << 16, dtype=torch.float16, device=dev)
    out = torch.full((1 << 16,), 7.0, dtype=torch.float32, device=dev)
    a, o, h = t.data_ptr(), out.data_ptr(), ops.DT[torch.float16]
    assert lib.ur_cond_conv3x3_dgrad(a, a, o, 1, 8, 8, 16, 24, 1, h, None) == UNS
    assert lib.ur_cond_conv3x3_dgrad(a, a + 2, o, 1, 8, 8, 16, 16, 1, h, None) == BAD
    assert lib.ur_cond_conv3x3_dgrad(a, a, o, 1, 8, 8, 16, 16, 4, h, None) == UNS
    assert lib.ur_cond_conv3x3_wgrad(a, h, 0, a, None, None, o, 1 << 18, 1, 8, 8, 16, 16, 1, 0, h, None) == BAD
    assert lib.ur_cond_conv3x3_wgrad(a, h, 0, a, o, o, o, 64, 1, 8, 8, 16, 16, 1, 0, h, None) == BAD      # workspace too small
    assert lib.ur_cond_conv3x3_wgrad(a, h, 0, a, o, o, o, 1 << 18, 1, 8, 8, 24, 16, 1, 0, h, None) == UNS
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()), "a refused call wrote to its output"
    with pytest.raises(ValueError):
        ops.cond_conv3x3_dgrad(t[:1024].view(1, 8, 8, 16), t[:16], in_hw=(8, 8), n_in=16)
    with pytest.raises(ValueError):
        ops.cond_conv3x3_wgrad(t[:1024].view(1, 8, 8, 16), t[:512].view(1, 4, 4, 32), stride=1)
