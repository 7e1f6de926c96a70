"""tests/util_igemm.py checked without a GPU (runs in -m "not gpu"):

  * reference: the explicit float64 im2col equals F.conv2d in float64 for every gather mode (stride 1, stride 2 on an odd
    map, nearest-2x, pad = 0 as F.pad(x, (0, 1, 0, 1)), two sources), and the ``cblock``-packed weights with a 1x1 tail
    walk the same sum as conv2d + conv1x1;
  * exactness: every "int" problem of test_igemm_range_gpu.py satisfies |value before out_scale| <= 256 and is
    representable in its storage type (make_problem asserts it; here every one is built);
  * emulation: torch-float32 emulations of a correct kernel (64-wide chunks forwards, backwards, 3 and 7 split-K slabs;
    the ur_common.h activation formulas; ops.lo_encode) stay within HALF of the fp32 part of every bound before the
    storage rounding and within the whole bound after it, on "gauss" and "act", both dtypes;
  * sensitivity: the rounded reference stands in for a kernel output and is damaged in five ways; the new checkers must
    reject each.  The whole-tensor rel-L2 assertion of test_ops_gpu.py is evaluated on the same tensors and its verdict
    printed: it accepts (a), (d) and (e) in both dtypes and (b) in bf16; (c), a whole wrong row of 297, it rejects.
"""
import pytest
import torch
import torch.nn.functional as F

import util_igemm as ug

DTYPES = ug.DTYPES
ids = lambda t: str(t).replace("torch.", "") if isinstance(t, torch.dtype) else None
f64 = torch.float64


def _conv2d(x_nhwc, w_oihw, stride, ups, pad):
    x = x_nhwc.permute(0, 3, 1, 2)
    if ups:
        x = F.interpolate(x, scale_factor=2.0, mode="nearest")
    if pad == 0:
        x = F.pad(x, (0, 1, 0, 1))
    return F.conv2d(x, w_oihw, None, stride=stride, padding=pad).permute(0, 2, 3, 1)


@pytest.mark.parametrize("mode", ["s1", "s2_odd", "ups", "s2_pad0", "s2_pad0_even", "two_sources"])
def test_im2col_reference_equals_conv2d(mode):
    from uni_renderer_amd.layers import pack_conv3x3
    g = torch.Generator().manual_seed(11)
    stride, ups, pad = {"s1": (1, False, 1), "s2_odd": (2, False, 1), "ups": (1, True, 1), "s2_pad0": (2, False, 0),
                        "s2_pad0_even": (2, False, 0), "two_sources": (1, False, 1)}[mode]
    H, W = (5, 6) if ups else ((8, 10) if mode == "s2_pad0_even" else (9, 11))
    x = torch.randn(3, H, W, 24, generator=g, dtype=f64)
    if mode == "two_sources":
        x = torch.cat([x[..., :16], x[..., 16:]], -1)  # k = tap * (c0 + c1) + c: the sources side by side in every tap
    w = torch.randn(20, 24, 3, 3, generator=g, dtype=f64)
    ref = _conv2d(x, w, stride, ups, pad)
    Ho, Wo = ug.out_hw(H, W, stride, ups, pad)
    assert ref.shape == (3, Ho, Wo, 20)
    got = ug.im2col(x, stride, ups, pad).reshape(3 * Ho * Wo, -1) @ pack_conv3x3(w, f64).T
    assert torch.allclose(got.view(3, Ho, Wo, 20), ref, rtol=0, atol=1e-12)


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
def test_problem_reference_equals_conv2d_plus_conv1x1(dtype):
    """make_problem's reference (tap-outer) for a cblock-packed conv with a two-source 1x1 tail, bias, per-sample row,
    residual and scale; and the kernel-order weights are the product's packer applied to the same OIHW tensor."""
    from uni_renderer_amd.layers import pack_conv3x3
    p = ug.make_problem(dict(mode="conv", family="gauss", dtype=dtype, B=2, H=5, W=7, N=24, c0=128, cblock=64, ct0=64, ct1=64,
                             streams=2, **ug.EPI))
    for s in range(2):
        x = p["x0"][s].view(2, 5, 7, 128)
        y = _conv2d(x, p["w4"][s], 1, False, 1).reshape(70, 24)
        y = y + torch.cat([p["t0"][s], p["t1"][s]], -1) @ p["wt"][s].T + p["bias"][s]
        y = (y + p["rowadd"][s][torch.arange(70) // 35] + p["res"][s]) * 0.5
        assert torch.allclose(p["ref"][s], y, rtol=0, atol=1e-12)
        wk = torch.cat([pack_conv3x3(p["w4"][s], f64, cblock=64), p["wt"][s]], -1)
        assert torch.equal(p["w"][s], wk)
        # block-outer order: k = (c // 64) * 576 + tap * 64 + c % 64
        assert torch.equal(p["w"][s][:, 576 + 3 * 64 + 5], p["w4"][s][:, 64 + 5, 1, 0])


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
def test_every_int_problem_of_the_gpu_file_is_exact(dtype):
    assert ug.int_problems(dtype) >= 20
    # the figures quoted in the docstring: M = 300, N = 328 at K = 1728 (density 1/8) and K = 6400 (1/32)
    for K in (1728, 6400):
        p = ug.make_problem(dict(mode="gemm", dtype=dtype, M=300, N=328, c0=K, rows_per_b=100, **ug.EPI))
        print({"K": K, "max_abs_before_scale": float((p["ref"] / 0.5).abs().max())})


def test_exactness_violation_fails_loudly():
    with pytest.raises(AssertionError, match="exact family"):
        ug.make_problem(dict(mode="gemm", M=64, N=64, c0=64 * 3000, bias=True))


EMU_SPECS = [("gauss", "silu"), ("gauss", "geglu"), ("gauss", "hilo"), ("act", "silu"), ("act", "geglu"), ("act", "hilo")]


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("family,which", EMU_SPECS)
def test_fp32_emulation_within_half_of_the_fp32_part(dtype, family, which):
    spec = {n: s for n, s, _, _ in ug.specs_g(dtype, family)}[which]
    _emulation(ug.problem(**spec), f"{family} {which}")


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
def test_fp32_emulation_long_k_conv(dtype):
    _emulation(ug.problem(**ug.spec_g_long_conv(dtype)), "act conv K 5760")


def _emulation(p, what):
    b, dt = ug.bounds(p), p["dtype"]
    worst = 0.0
    for order, slabs in (("fwd", 1), ("rev", 1), ("fwd", 3), ("fwd", 7)):
        y32, hi, lo = ug.emulate(p, order, slabs)
        w = f"{what} {order} slabs {slabs}"
        _, r = ug.check_elem(y32, p["ref"], b["fp"], float("inf"), w + " fp32 value", frac=0.5, rel=False)
        worst = max(worst, r)
        ug.check_elem(hi, p["ref"], b["hi"], ug.TOL[dt], w + " stored")
        if lo is not None:
            ug.check_elem(hi + lo, p["ref"], b["pair"], ug.TOL[dt], w + " pair")
    if p["act"] == "geglu":
        assert bool(((p["gate"] > -12) & (p["gate"] < -6)).any()), "no gate in [-12, -6]"
    print({"emulation": what, "dtype": str(dt), "worst_fp32_err_over_fp32_part": worst})


# ---------------------------------------------------------------------------------------------------------------
def _rejected(fn, *a, **kw):
    try:
        fn(*a, **kw)
    except AssertionError:
        return True
    return False


def _report(name, dtype, new_rejects, old_figure):
    print({"sensitivity": name, "dtype": str(dtype), "new_checkers_reject": new_rejects, "old_rel_l2": old_figure,
           "old_tolerance": ug.TOL[dtype], "old_assertion_accepts": old_figure < ug.TOL[dtype]})


def _standin(dtype, conv=False, **extra):
    """The 128 | 64 GEMM of case group (a), or its 9 x 11 conv (K = 1728)."""
    shape = dict(mode="conv", B=3, H=9, W=11) if conv else dict(mode="gemm", M=300, rows_per_b=100)
    p = ug.problem(family="gauss", dtype=dtype, N=328, c0=128, c1=64, seed=3, **shape, **dict(ug.EPI, **extra))
    got = ug.rnd(p["ref"], dtype)
    ug.check_elem(got, p["ref"], ug.bounds(p)["hi"], ug.TOL[dtype], "undamaged stand-in")
    return p, got.clone()


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
def test_sensitivity_a_one_element(dtype):
    """(a) one element of 300 x 328 off by 4 u |v| (the element of median magnitude of its row), at K = 192.  The fp32 part
    of the bound grows with K -- at K = 1728 it is ~6 u |v| for fp16 -- so an error of a few u in ONE element of a long-K
    output is below what any order-independent bound can resolve; the exact family has no such limit."""
    p, got = _standin(dtype)
    c = int(p["ref"][0, 150].abs().argsort()[164])
    got[0, 150, c] += 4 * ug.U[dtype] * p["ref"][0, 150, c].abs()
    rej = _rejected(ug.check_elem, got, p["ref"], ug.bounds(p)["hi"], ug.TOL[dtype], "a")
    old = ug.old_rel_l2(got, p["ref"])
    _report("a", dtype, rej, old)
    assert rej and old < ug.TOL[dtype]


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
def test_sensitivity_b_last_columns_from_the_neighbouring_row(dtype):
    p, got = _standin(dtype)
    got[0, 98, -8:] = got[0, 99, -8:]  # m = 98 | 99: the last pixel of sample 0 takes the first of sample 1
    rej = _rejected(ug.check_elem, got, p["ref"], ug.bounds(p)["hi"], ug.TOL[dtype], "b")
    _report("b", dtype, rej, ug.old_rel_l2(got, p["ref"]))
    assert rej


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
def test_sensitivity_c_border_pixel_reads_the_previous_line(dtype):
    """(c) output pixel (b 1, oy 4, ox 0): its three kx = 0 taps read the pixel in front of the line in the buffer (the last
    pixel of the previous line) instead of zero padding."""
    p, got = _standin(dtype, conv=True)
    B, H, W, Ho, Wo = p["conv"]
    C = p["c0"] + p["c1"]
    xc = torch.cat([p["x0"][0], p["x1"][0]], -1)                       # [B * H * W, C]
    b_, oy = 1, 4
    m = b_ * Ho * Wo + oy * Wo
    cols = ug.im2col(xc.view(B, H, W, C))[m].clone()                   # [9, C]
    for ky in range(3):
        iy = oy - 1 + ky
        cols[ky * 3] = xc[b_ * H * W + iy * W - 1]
    pre = cols.reshape(-1) @ p["wref"][0].T + p["bias"][0] + p["rowadd"][0][m // p["rows_per_b"]]
    got[0, m] = ug.rnd((pre + p["res"][0, m]) * p["out_scale"], dtype)
    rej = _rejected(ug.check_elem, got, p["ref"], ug.bounds(p)["hi"], ug.TOL[dtype], "c")
    old = ug.old_rel_l2(got, p["ref"])
    _report("c", dtype, rej, old)
    assert rej


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
def test_sensitivity_d_one_low_part_column_zeroed(dtype):
    from uni_renderer_amd import ops
    p, hi = _standin(dtype, res_lo=True)
    lo = ops.lo_float(ops.lo_encode((p["ref"] - hi).float(), dtype)).double()
    b = ug.bounds(p)
    ug.check_elem(hi + lo, p["ref"], b["pair"], ug.TOL[dtype], "undamaged pair")
    lo[..., 37] = 0.0
    rej = _rejected(ug.check_elem, hi + lo, p["ref"], b["pair"], ug.TOL[dtype], "d")
    _report("d", dtype, rej, ug.old_rel_l2(hi + lo, p["ref"]))
    assert rej


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
def test_sensitivity_e_one_element_outside_the_named_region(dtype):
    """(e) one element behind column n_store of one row, and one in the first guard row behind M, for both the output
    type and the low part's byte; the undamaged buffers pass."""
    from uni_renderer_amd import ops
    M, ns, ldc = 300, 192, 200
    for t in (dtype, ops.lo_dtype(dtype)):
        named = ug.region2d((M + 2 * ug.GUARD_ROWS, ldc), ug.GUARD_ROWS, M, ns)
        buf = ug.sentinel(named.shape, t, "cpu")
        buf[named] = 0
        ug.assert_untouched(buf, named, "undamaged")
        for r, c in ((ug.GUARD_ROWS + 17, ns), (ug.GUARD_ROWS + M, 0), (ug.GUARD_ROWS - 1, ldc - 1)):
            bad = buf.clone()
            bad[r, c] = 0
            assert _rejected(ug.assert_untouched, bad, named, "e"), (t, r, c)
    _report("e", dtype, True, 0.0)  # the old assertion never looks outside [M][N]


def test_exact_checker_names_rows_and_columns():
    exp = torch.zeros(1, 6, 8, dtype=f64)
    got = exp.clone()
    got[0, 4, 7] = 1.0
    with pytest.raises(AssertionError, match=r"1 rows \[4\].*1 columns \[7\]"):
        ug.check_exact(got, exp, "x")
    got[0, 4, 7] = float("nan")
    with pytest.raises(AssertionError, match="1 NaN"):
        ug.check_exact(got, exp, "x")
    ug.check_exact(exp.clone(), exp, "x")
