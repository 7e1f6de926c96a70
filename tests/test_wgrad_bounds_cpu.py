"""tests/util_wgrad.py checked without a GPU (runs in -m "not gpu"):

  * reference: float64 dw = dy^T . im2col(x) and db = sum_p dy equal float64 autograd of F.conv2d / F.linear for every conv
    mode of test_wgrad_range_gpu.py (stride 1 / 2, odd input at stride 2, pad = 0 as F.pad(x, (0, 1, 0, 1)) + padding 0);
  * exactness: every exact-family problem of the GPU file satisfies its condition (the builders assert it; here every one
    is built), and a violation fails loudly;
  * emulation: a torch-float32 emulation of a correct kernel (32-row stages forwards and backwards, 1 / 3 / 7 slices summed
    in slice order) stays within HALF of the fp32 part of the dw bound before the storage rounding, within the whole bound
    after it, and its db within the db bound;
  * sensitivity: a correct result is damaged in the ways this kind of kernel goes wrong -- row P - 1 dropped, one border
    tap of one sample read from the neighbouring line, (ky, kx) swapped, dw transposed, db over P - 1 rows, one element
    written outside [N][K], outside [N], behind the slab -- and the new checks must reject each, on the exact family
    (check_exact) and on the toleranced one (check_elem).  The criteria of test_wgrad_gpu.py are evaluated next to them
    and their verdict printed.  What they let through, by arithmetic on the operands alone: their dw figure is the LARGEST
    error of the matrix over the largest reference element, so a dropped row (largest error max_n |dy[P-1][n]| .
    max_k |x[P-1][k]|, about 3 x 3 for N(0, 1) rows of a few hundred elements) passes in bf16 once 1.2e-2 . max |ref|
    (about 4.5 sqrt(P)) exceeds it -- from P of a few 10^4, e.g. the 65536-row problem below, where a TYPICAL element moves
    by 0.4 (less than its bf16 spacing) and the derived fp32 bound itself is far wider than that: only the exact family sees such a row there -- and
    the db criterion 2e-4 . max sum |dy| exceeds one dy element from P of about 2 . 10^4.  Anything outside [N][K], [N] or
    the slab they never look at.  At the small shapes of the new tests both old criteria reject the structured errors too;
    what they cannot show at any shape is WHICH elements are wrong, and nothing about the guards.
"""
import pytest
import torch
import torch.nn.functional as F

import util_igemm as ug
import util_wgrad as uw

DTYPES = uw.DTYPES
ids = lambda t: str(t).replace("torch.", "") if isinstance(t, torch.dtype) else None
f64 = torch.float64

CONV_MODES = {"s1": dict(Hin=4, Win=8, stride=1), "s2": dict(Hin=8, Win=16, stride=2), "s2_odd": dict(Hin=7, Win=15, stride=2),
              "s2_pad0": dict(Hin=8, Win=8, stride=2, pad=0), "s1_tall": dict(Hin=16, Win=8, stride=1)}


@pytest.mark.parametrize("mode", sorted(CONV_MODES))
def test_reference_equals_autograd_of_conv2d(mode):
    p = uw.make_problem(dict(kind="conv", family="gauss", dtype=torch.float16, B=3, C=64, N=24, **CONV_MODES[mode]))
    B, Hin, Win, Ho, Wo = p["conv"]
    x = p["x"].permute(0, 3, 1, 2)
    pad = p["pad"]
    if pad == 0:
        x = F.pad(x, (0, 1, 0, 1))
    w = torch.zeros(24, 64, 3, 3, dtype=f64, requires_grad=True)
    b = torch.zeros(24, dtype=f64, requires_grad=True)
    y = F.conv2d(x, w, b, stride=p["stride"], padding=pad)
    assert y.shape == (B, 24, Ho, Wo)
    y.backward(p["dy"].view(B, Ho, Wo, 24).permute(0, 3, 1, 2))
    assert torch.allclose(p["dw"], w.grad.permute(0, 2, 3, 1).reshape(24, 9 * 64), rtol=0, atol=1e-11)
    assert torch.allclose(p["db"], b.grad, rtol=0, atol=1e-11)


def test_reference_equals_autograd_of_linear():
    p = uw.make_problem(dict(kind="linear", family="gauss", dtype=torch.bfloat16, P=77, N=24, K=40))
    w = torch.zeros(24, 40, dtype=f64, requires_grad=True)
    b = torch.zeros(24, dtype=f64, requires_grad=True)
    F.linear(p["x"], w, b).backward(p["dy"])
    assert torch.allclose(p["dw"], w.grad, rtol=0, atol=1e-11) and torch.allclose(p["db"], b.grad, rtol=0, atol=1e-11)


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
def test_every_exact_problem_of_the_gpu_file_is_exact(dtype):
    assert uw.int_problems(dtype) >= 90
    for P, N, K in uw.LINEAR + [(300, 1280, 64)]:
        p = uw.problem(**uw.spec_linear(dtype, P, N, K))
        print({"linear": (P, N, K), "max_abs_dw": float(p["dw"].abs().max()), "max_abs_db": float(p["db"].abs().max())})
    print({"conv_max_abs_dw": max(float(uw.problem(**s)["dw"].abs().max()) for _, s, _ in uw.specs_conv(dtype))})
    for fam, name, s in [("dgrad", n, s) for n, s in uw.specs_bwd_dx()] + [("wgrad", n, s) for n, s in uw.specs_bwd_dw()]:
        q = uw.bwd_problem("conv", fam, dtype, **s)
        print({"bwd": name, "family": fam, "max_abs_dx": float(q["dx"].abs().max()), "max_abs_dw": float(q["dw"].abs().max())})
    q = uw.bwd_problem("linear", "dgrad", dtype, **uw.SPEC_BWD_LINEAR)
    print({"bwd": "linear", "max_abs_dx": float(q["dx"].abs().max()), "max_abs_dw": float(q["dw"].abs().max())})


def test_exactness_violation_fails_loudly():
    with pytest.raises(AssertionError, match="exact family"):
        uw.make_problem(dict(kind="linear", P=400000, N=16, K=16))


def test_packed_weights_of_the_backward_problems_are_the_products_layout():
    """make_bwd packs [N][(ky, kx, c)] by hand (independent of the package); the package's packer gives the same matrix."""
    from uni_renderer_amd.layers import pack_conv3x3
    q = uw.bwd_problem("conv", "dgrad", torch.float16, **dict(uw.specs_bwd_dx())["s1_9x11_N72"])
    assert torch.equal(q["w"], pack_conv3x3(q["w4"], f64))


# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("which", [0, 1], ids=["linear", "conv"])
def test_fp32_emulation_within_half_of_the_fp32_part(dtype, which):
    name, spec = uw.specs_toleranced(dtype)[which]
    p = uw.problem(**spec)
    worst = worst_db = 0.0
    for order in ("fwd", "rev"):
        for slices in (1, 3, 7):
            b = uw.bounds(p, slices)
            dw32, dw, db32 = uw.emulate(p, order, slices)
            what = f"{name} {order} slices {slices}"
            _, r = uw.check_elem(dw32, p["dw"], b["fp"], float("inf"), what + " fp32 value", frac=0.5, rel=False)
            worst = max(worst, r)
            uw.check_elem(dw, p["dw"], b["dw"], uw.TOL[dtype], what + " stored")
            _, r = uw.check_elem(db32, p["db"], b["db"], float("inf"), what + " db", rel=False)
            worst_db = max(worst_db, r)
    print({"emulation": name, "dtype": str(dtype), "worst_fp32_err_over_fp32_part": worst, "worst_db_err_over_bound": worst_db})


# ---------------------------------------------------------------------------------------------------------------
def _rejected(fn, *a, **kw):
    try:
        fn(*a, **kw)
    except AssertionError:
        return True
    return False


def _report(name, dtype, family, new_rejects, old_err):
    print({"sensitivity": name, "dtype": str(dtype), "family": family, "new_check_rejects": new_rejects,
           "old_max_err_over_max_ref": old_err, "old_tolerance": uw.TOL[dtype], "old_assertion_accepts": old_err <= uw.TOL[dtype]})


def _new_check(p, got, what):
    """The check test_wgrad_range_gpu.py applies to a dw of this problem's family."""
    if p["family"] == "int":
        uw.check_exact(got, p["dw"], what)
    else:
        uw.check_elem(got, p["dw"], uw.bounds(p)["dw"], uw.TOL[p["dtype"]], what)


def _standins(dtype, conv):
    """(exact, toleranced) problems: the 300 x 328 x 200 linear layer, or the B = 3, 4 x 8, C = 192 conv."""
    if conv:
        s = dict(kind="conv", dtype=dtype, N=328, B=3, Hin=4, Win=8, C=192)
        return uw.problem(**s), uw.problem(family="gauss", **s)
    return uw.problem(**uw.spec_linear(dtype, 300, 328, 200)), uw.problem(**uw.spec_linear(dtype, 300, 328, 200, family="gauss"))


def _damaged(p, dw):
    """``dw`` (float64, exact arithmetic on damaged operands) as a kernel would store it."""
    return ug.rnd(dw, p["dtype"])


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
def test_undamaged_standins_pass(dtype):
    for conv in (False, True):
        for p in _standins(dtype, conv):
            _new_check(p, _damaged(p, p["dw"]), "undamaged")


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
def test_sensitivity_row_p_minus_1_dropped(dtype):
    for p in _standins(dtype, False):
        got = _damaged(p, p["dy"][:-1].T @ p["xcol"][:-1])
        rej = _rejected(_new_check, p, got, "row dropped")
        _report("row P - 1 dropped", dtype, p["family"], rej, uw.old_dw_err(got, p["dw"]))
        assert rej


def test_old_criteria_accept_a_dropped_row_of_a_long_problem():
    """P = 65536, N = K = 64, N(0, 1), bf16: the arithmetic of the module docstring, asserted from the operands before the
    old figures are evaluated.  (The derived fp32 bound is wider than the damage here as well: (P + 9) 2^-23 A is about
    300 per element.  Only exact data resolves one row of 65536.)"""
    dt = torch.bfloat16
    p = uw.make_problem(dict(kind="linear", family="gauss", dtype=dt, P=65536, N=64, K=64, seed=2))
    largest_damage = float(p["dy"][-1].abs().max() * p["x"][-1].abs().max())
    assert largest_damage <= uw.TOL[dt] * float(p["dw"].abs().max()), "the arithmetic says the old dw criterion accepts"
    assert float(p["dy"][-1].abs().max()) <= 2e-4 * float(p["Ady"].max()), "the arithmetic says the old db criterion accepts"
    got = _damaged(p, p["dy"][:-1].T @ p["xcol"][:-1])
    old = uw.old_dw_err(got, p["dw"])
    old_db = uw.old_db_accepts(p["dy"][:-1].sum(0).float().double(), p["db"], p["Ady"])
    moved = float((got - ug.rnd(p["dw"], dt)).abs().median())
    print({"sensitivity": "row P - 1 of 65536 dropped", "old_max_err_over_max_ref": old, "old_tolerance": uw.TOL[dt],
           "old_db_accepts": old_db, "median_element_moved_by": moved, "median_fp32_part_of_new_bound": float(uw.bounds(p)["fp"].median())})
    assert old <= uw.TOL[dt] and old_db


def _conv_damage(p, fn):
    """dw of conv problem ``p`` with its im2col [P, 9, C] changed by ``fn(cols, x)`` in place."""
    cols = p["xcol"].reshape(p["P"], 9, p["C"]).clone()
    fn(cols, p["x"])
    return _damaged(p, p["dy"].T @ cols.reshape(p["P"], -1))


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
def test_sensitivity_border_tap_reads_the_neighbouring_line(dtype):
    """Sample 1, tap (ky 1, kx 0): the ox = 0 pixels read the pixel in front of their line in memory (the last pixel of the
    previous line) instead of the zero padding."""
    for p in _standins(dtype, True):
        B, Hin, Win, Ho, Wo = p["conv"]

        def fn(cols, x, b=1):
            flat = x.reshape(B * Hin * Win, -1)
            for oy in range(Ho):
                cols[b * Ho * Wo + oy * Wo, 3] = flat[b * Hin * Win + oy * Win - 1]

        got = _conv_damage(p, fn)
        rej = _rejected(_new_check, p, got, "border tap")
        _report("border tap of one sample from the neighbouring line", dtype, p["family"], rej, uw.old_dw_err(got, p["dw"]))
        assert rej


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
def test_sensitivity_ky_kx_swapped(dtype):
    for p in _standins(dtype, True):
        def fn(cols, x):
            cols[:] = cols.reshape(-1, 3, 3, cols.shape[-1]).transpose(1, 2).reshape(cols.shape)

        got = _conv_damage(p, fn)
        rej = _rejected(_new_check, p, got, "ky kx")
        _report("(ky, kx) swapped", dtype, p["family"], rej, uw.old_dw_err(got, p["dw"]))
        assert rej


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
def test_sensitivity_dw_transposed(dtype):
    """A square problem (N = K = 200), where a transposed result has the right shape."""
    for fam in ("int", "gauss"):
        p = uw.problem(**uw.spec_linear(dtype, 300, 200, 200, family=fam))
        got = _damaged(p, p["dw"].T.contiguous())
        rej = _rejected(_new_check, p, got, "transposed")
        _report("dw transposed", dtype, fam, rej, uw.old_dw_err(got, p["dw"]))
        assert rej


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
def test_sensitivity_db_over_p_minus_1_rows(dtype):
    for p in _standins(dtype, False):
        got = p["dy"][:-1].sum(0).float().double()
        if p["family"] == "int":
            rej = _rejected(uw.check_exact, got[None], p["db"][None], "db")
        else:
            rej = _rejected(uw.check_elem, got, p["db"], uw.bounds(p)["db"], float("inf"), "db", rel=False)
        print({"sensitivity": "db over P - 1 rows", "dtype": str(dtype), "family": p["family"], "new_check_rejects": rej,
               "old_assertion_accepts": uw.old_db_accepts(got, p["db"], p["Ady"])})
        assert rej


@pytest.mark.parametrize("dtype", DTYPES + [torch.float32], ids=ids)
def test_sensitivity_one_element_outside_the_named_region(dtype):
    """One element behind column K of a row, in the guard rows in front of and behind dw (fp16 / bf16); in front of and
    behind db and behind the slab floats (fp32).  The undamaged buffers pass.  The old assertions never look there."""
    N, K = 328, 200
    if dtype == torch.float32:
        cases = [(uw.sentinel((N + 2 * uw.GUARD_ROWS,), dtype, "cpu"), uw.region1d(N + 2 * uw.GUARD_ROWS, uw.GUARD_ROWS, N),
                  [(uw.GUARD_ROWS - 1,), (uw.GUARD_ROWS + N,)]),
                 (uw.sentinel((1000 + uw.TAIL,), dtype, "cpu"), uw.region1d(1000 + uw.TAIL, 0, 1000), [(1000,), (1000 + uw.TAIL - 1,)])]
    else:
        named = ug.region2d((N + 2 * uw.GUARD_ROWS, K + 8), uw.GUARD_ROWS, N, K)
        cases = [(uw.sentinel(named.shape, dtype, "cpu"), named,
                  [(uw.GUARD_ROWS + 17, K), (uw.GUARD_ROWS + N, 0), (uw.GUARD_ROWS - 1, K + 7)])]
    for buf, named, spots in cases:
        buf[named] = 0
        uw.assert_untouched(buf, named, "undamaged")
        for spot in spots:
            bad = buf.clone()
            bad[spot] = 0
            assert _rejected(uw.assert_untouched, bad, named, "outside"), (dtype, spot)
        half = buf.clone()   # one changed bit of the low half of an fp32 sentinel: a 16-bit view of one half would miss it
        if dtype == torch.float32:
            half.view(torch.int32)[spots[0]] ^= 1
            assert _rejected(uw.assert_untouched, half, named, "outside"), "low bit"
