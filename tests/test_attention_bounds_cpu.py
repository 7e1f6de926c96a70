"""The bounds of tests/util_attention.py, checked without a GPU (runs in -m "not gpu"):

  * emulation: float64 arithmetic with exactly the roundings a correct kernel makes (util_attention.emulate_forward /
    emulate_backward) stays within HALF of every element-wise bound and half of the per-row rel-L2 tolerance wherever
    the GPU tests apply it, on every data family -- the bounds are satisfiable with a factor 2 of room, independent of the
    code under test.  Two exceptions, both the analytic worst case and documented at EMU_FRAC / EMU_FRAC_LSE: dv (3.44 u
    of its 4 u when lse error, rounding of P ~ 1 and output rounding align) and lse (1.44 u of its 2 u).
  * sensitivity: the float64 reference rounded to the storage type stands in for a kernel output and is damaged in one
    place; the per-row helpers must reject it.  The earlier assertion (whole-tensor rel-L2 at the old tolerance, lse at
    2e-3 / 1.5e-2) is evaluated on the same tensors and its verdict printed: it accepts (a), (c), (d) and (e).
"""
import pytest
import torch

import util_attention as ua

DTYPES = ua.DTYPES
ids = lambda t: str(t).replace("torch.", "") if isinstance(t, torch.dtype) else None


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("prescaled", [False, True], ids=["scaled", "prescaled"])
@pytest.mark.parametrize("family", ua.FAMILIES)
def test_forward_emulation_within_half_of_the_bounds(dtype, prescaled, family):
    """Reference 0 / 3.3 / 7.9 log2 units below the row maximum (what the lazy rescale may leave), rounded to the storage
    type in the pre-scaled mode (the slot kernel's reference), ragged (77) and multi-tile (512) key counts."""
    for Tq, Tk, d in ((96, 77, 40), (64, 512, 40), (64, 333, 80)):
        case = ua.make_case(family, 1, 2, Tq, Tk, d, dtype, prescaled=prescaled, seed=1)
        o, A, lse = ua.forward_ref(case)
        for below in (0.0, 3.3, 7.9):
            oe, le = ua.emulate_forward(case, below, round_ref=prescaled)
            what = f"{family} Tk {Tk} d {d} reference {below} below the maximum"
            ua.check_forward(oe, o, A, dtype, what, frac=0.5)
            if not prescaled:  # lse exists for scale > 0 only
                ua.check_lse(le, lse, dtype, what, frac=ua.EMU_FRAC_LSE)


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("family", ["flat", "peaky", "sink_last", "ramp_8.5", "offset_v"])
def test_forward_emulation_4096_keys(dtype, family):
    case = ua.make_case(family, 1, 1, 64, 4096, 40, dtype, prescaled=True, seed=2)
    o, A, _ = ua.forward_ref(case)
    for below in (0.0, 7.9):
        oe, _ = ua.emulate_forward(case, below, round_ref=True)
        ua.check_forward(oe, o, A, dtype, f"{family} 4096 keys, reference {below} below", frac=0.5)


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("family", ua.BWD_FAMILIES)
def test_flash_backward_emulation_within_the_bounds(dtype, family):
    for Tq, Tk, d in ((128, 77, 40), (128, 128, 80), (64, 128, 32), (128, 77, 160)):
        case = ua.make_case(family, 1, 2, Tq, Tk, d, dtype, seed=1)
        ref = ua.backward_ref(case)
        ua.check_backward(ua.emulate_backward(case), ref, dtype, f"{family} {Tq}x{Tk} d {d}", family, frac=ua.EMU_FRAC)


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("family", ua.MAT_FAMILIES)
def test_materialised_backward_emulation_within_the_bounds(dtype, family):
    for Tq, Tk, d in ((200, 77, 40), (96, 96, 80)):
        case = ua.make_case(family, 1, 2, Tq, Tk, d, dtype, seed=1)
        ref = ua.backward_ref(case, materialised=True)
        ua.check_backward(ua.emulate_backward(case, materialised=True), ref, dtype, f"{family} {Tq}x{Tk} d {d}", family,
                          path="materialised", frac=ua.EMU_FRAC)


# ---------------------------------------------------------------------------------------------------------------
def _rejected(fn, *a, **kw):
    try:
        fn(*a, **kw)
    except AssertionError:
        return True
    return False


def _forward_standin(family, Tk, dtype):
    case = ua.make_case(family, 1, 1, 1024, Tk, 40, dtype, seed=3)
    o, A, lse = ua.forward_ref(case)
    got = ua.rnd(o, dtype)
    ua.check_forward(got, o, A, dtype, "undamaged stand-in")
    return case, o, A, lse, got


def _report(name, dtype, new_rejects, old_figure, old_tol):
    print({"sensitivity": name, "dtype": str(dtype), "new_helpers_reject": new_rejects, "old_figure": old_figure,
           "old_tolerance": old_tol, "old_assertion_accepts": old_figure < old_tol})


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
def test_sensitivity_a_one_element(dtype):
    """(a) one element of one row moved by 1 % of its A (fp16).  bf16: 3 u = 1.17 % and the stand-in's own rounding may
    take u |o| <= 0.39 % off, so no bound of this form can see 1 %; the bf16 case moves 2 %."""
    _, o, A, _, got = _forward_standin("flat", 256, dtype)
    move = 0.01 if dtype == torch.float16 else 0.02
    got[0, 0, 700, 17] += move * A[0, 0, 700, 17]
    rej = _rejected(ua.check_forward, got, o, A, dtype, "a")
    old = ua.old_rel_l2(got, o)
    _report("a", dtype, rej, old, ua.TOL_FWD[dtype])
    assert rej and old < ua.TOL_FWD[dtype]


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
def test_sensitivity_b_row_replaced_by_its_neighbour(dtype):
    _, o, A, _, got = _forward_standin("flat", 256, dtype)
    got[0, 0, 511] = got[0, 0, 510]
    rej = _rejected(ua.check_forward, got, o, A, dtype, "b")
    _report("b", dtype, rej, ua.old_rel_l2(got, o), ua.TOL_FWD[dtype])
    assert rej


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
def test_sensitivity_c_last_valid_key_dropped_for_one_row(dtype):
    """(c) key 76 of 77 missing from ONE query row of 1024 (numerator and denominator): the row whose weight on that key
    is the median of the 1024 (P ~ 0.5 %), not a row picked for a heavy last key."""
    case, o, A, _, got = _forward_standin("flat", 77, dtype)
    S2 = (case["q"][0, 0] @ case["k"][0, 0].T) * case["c"]
    r = int(torch.softmax(S2 * 0.6931471805599453, -1)[:, 76].argsort()[512])
    S2 = (case["q"][0, 0, r] @ case["k"][0, 0, :76].T) * case["c"]
    got[0, 0, r] = ua.rnd(torch.softmax(S2 * 0.6931471805599453, -1) @ case["v"][0, 0, :76], dtype)
    rej = _rejected(ua.check_forward, got, o, A, dtype, "c")
    old = ua.old_rel_l2(got, o)
    _report("c", dtype, rej, old, ua.TOL_FWD[dtype])
    assert rej and old < ua.TOL_FWD[dtype]


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
def test_sensitivity_d_lse_of_one_row(dtype):
    _, _, _, lse, _ = _forward_standin("flat", 77, dtype)
    got = lse.float().double()
    ua.check_lse(got, lse, dtype, "undamaged lse")
    off = 0.0015 if dtype == torch.float16 else 0.012
    got[0, 0, 300] += off
    rej = _rejected(ua.check_lse, got, lse, dtype, "d")
    old = float((got - lse).abs().max())
    _report("d", dtype, rej, old, ua.OLD_LSE[dtype])
    assert rej and old < ua.OLD_LSE[dtype]


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
def test_sensitivity_e_one_dv_row_scaled(dtype):
    """(e) one of 1024 dv rows of a peaky case scaled by 1.05."""
    case = ua.make_case("peaky", 1, 1, 1024, 1024, 40, dtype, seed=3)
    ref = ua.backward_ref(case)
    got = {n: ua.rnd(ref[n], dtype) for n in ("dq", "dk", "dv")}
    ua.check_backward(got, ref, dtype, "undamaged stand-in", "peaky")
    got["dv"][0, 0, 38] *= 1.05
    rej = _rejected(ua.check_backward, got, ref, dtype, "e", "peaky")
    old = ua.old_rel_l2(got["dv"], ref["dv"])
    _report("e", dtype, rej, old, ua.TOL_BWD[dtype])
    assert rej and old < ua.TOL_BWD[dtype]
