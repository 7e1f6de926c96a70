"""ur_cond_conv3x3 (csrc/condconv.hip) on the GPU, per element: exact on integer data, within the derived bound with SiLU on
N(0, 1) data (util_condconv.py; test_condconv_cpu.py shows that the bound fits correct arithmetic and rejects a dropped
corner tap, a halo row of the neighbouring sample and a shifted last odd column), bit-reproducible.  Every operand sits in
a NaN-filled guard buffer and the output in a sentinel buffer that must come back untouched outside [B, Ho, Wo, Cout]."""
import pytest
import torch

import util_condconv as CCV
from util_igemm import TOL, check_elem, check_exact

pytestmark = pytest.mark.gpu

LAYERS = [(cin, cout, s, False, None) for cin, cout, s in CCV.CHAIN + CCV.EXTRA] + [(c, 16, 1, True, xdt) for c, xdt in CCV.IMAGE]
IDS = [f"{cin}to{cout}s{s}" + (f"_image_{str(xdt)[6:]}" if img else "") for cin, cout, s, img, xdt in LAYERS]


@pytest.mark.parametrize("dtype", CCV.DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("layer", LAYERS, ids=IDS)
def test_exact_on_integer_data(dev, layer, dtype):
    cin, cout, s, img, xdt = layer
    for H, W in CCV.MAPS:
        p = CCV.problem(cin, cout, s, H, W, dtype, image=img, x_dtype=xdt)
        got, what = CCV.launch(p, dev)
        check_exact(got, p["ref"], what)


@pytest.mark.parametrize("dtype", CCV.DTYPES, ids=["fp16", "bf16"])
def test_exact_with_three_samples_and_stride_2_image(dev, dtype):
    for cin, cout, s, img, xdt in [(16, 32, 2, False, None), (32, 32, 1, False, None), (3, 32, 2, True, torch.float32)]:
        p = CCV.problem(cin, cout, s, 33, 19, dtype, B=3, image=img, x_dtype=xdt)
        got, what = CCV.launch(p, dev)
        check_exact(got, p["ref"], what)


@pytest.mark.parametrize("dtype", CCV.DTYPES, ids=["fp16", "bf16"])
def test_bgr_weights_read_the_image_as_it_lies(dev, dtype):
    """`bgr` is a flip of the first layer's input-channel axis at pack time: the kernel, launched on an image in BGR order
    with those weights, gives exactly the conv of the RGB-ordered weights over the channel-flipped image -- and not the
    conv over the image as it lies.  This is where the channel order is pinned: behind the whole network its effect
    (1e-4 of the outputs of the tiny configuration) is below any parity bound."""
    for cin, xdt in [(3, torch.float32), (4, torch.float16)]:
        p = CCV.problem(cin, 16, 1, 33, 19, dtype, image=True, x_dtype=xdt)
        flipped = dict(p, x=p["x"].flip(1).contiguous())  # the caller's image in BGR order
        got, what = CCV.launch(flipped, dev, bgr=True)
        check_exact(got, p["ref"], what + " bgr")
        plain, _ = CCV.launch(flipped, dev)
        assert not torch.equal(plain, p["ref"]), "the channel order does not matter on this data"


@pytest.mark.parametrize("dtype", CCV.DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("layer", LAYERS, ids=IDS)
def test_silu_within_the_bound(dev, layer, dtype):
    cin, cout, s, img, xdt = layer
    worst = 0.0
    for H, W in [(33, 19), (16, 16)]:
        p = CCV.problem(cin, cout, s, H, W, dtype, family="gauss", image=img, x_dtype=xdt)
        got, what = CCV.launch(p, dev)
        rel, r = check_elem(got, p["ref"], CCV.bound(p), TOL[dtype], what)
        worst = max(worst, r)
    print(f"{IDS[LAYERS.index(layer)]} {dtype}: worst |err| / bound {worst:.3f}")


def test_twenty_launches_give_identical_bytes(dev):
    p = CCV.problem(32, 96, 2, 33, 19, torch.float16, family="gauss")
    first, _ = CCV.launch(p, dev)
    for _ in range(19):
        got, what = CCV.launch(p, dev)
        assert torch.equal(got, first), what
