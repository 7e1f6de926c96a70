"""ur_tchain (csrc/tchain.hip) per element, on guarded buffers.  test_tchain_gpu.py asserts one whole-tensor rel-L2 per
output on N(0, 1) data in compact tensors the wrapper allocates: low parts that are all zero or shifted by a row, a store
behind row M or into V^T token columns T .. ld_vt, one wrong element, a slightly wrong 8-row slice of the last wave of a
ragged tile, or a wrong column of the weight-stream decode never show there.  Here (tests/util_tchain.py):

  * groups (a) and (b) use the EXACT family "gamma0": integer data, 0 / +-1 weights and LayerNorm gamma = 0, so that every
    sum in any order is exact in fp32 and every output must be torch.equal to the float64 reference, low parts zero; y and
    the FF out differ from row to row; a mismatch is reported with its rows and columns;
  * every input sits inside NaN, every output inside sentinels (GUARD_ROWS rows on both sides; V^T with ld_vt = Tpad + 8 and
    a guard sample on each side; z_consts larger than the const block); nothing outside the named regions may change;
  * groups (c) and (d) hold N(0, 1) data -- and residuals ~ 16 with coarse ulps -- to the element bounds derived in
    util_tchain's docstring and to the per-row rel-L2 of test_tchain_gpu.py, and print the worst |err| / bound, the worst
    row rel-L2 and the share of susceptible operands;
  * group (e) runs the cases of (c) twice and requires identical bits.

Shapes: M = 200 (two tiles, the last with 72 rows: its third wave has 8, its fourth none; with S = 2 it overhangs the
other stream's rows), M = 5, M = 129 (one row in the second tile); PRE at (B, T) = (3, 96), (5, 32), (2, 64): sample
boundaries inside tiles, Tpad != T and == T.  PRE takes whole samples of a multiple of 32 tokens only: M = 200 is a
descriptor it must refuse.
"""
import pytest
import torch

import util_igemm as ug
import util_tchain as ut

pytestmark = pytest.mark.gpu

DTYPES = ug.DTYPES
ids = lambda t: str(t).replace("torch.", "") if isinstance(t, torch.dtype) else None


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("case", [n for n, _ in ut.specs_a(torch.float16)])
def test_a_exact(dev, dtype, case):
    """(a) modes Q / FF / PRE, S = 1 and 2 with different weights and consts per stream, with and without low parts."""
    p = ut.problem(**dict(ut.specs_a(dtype))[case])
    ut.check_exact_outputs(p, ut.launch(p, dev))


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("case", [n for n, _ in ut.specs_b(torch.float16)])
def test_b_exact_head_major(dev, dtype, case):
    """(b) q / k as [sample][head][token][40] images: the token matrices permuted, inside the same guards; y, y.lo and V^T
    unchanged."""
    p = ut.problem(**dict(ut.specs_b(dtype))[case])
    ut.check_exact_outputs(p, ut.launch(p, dev, head_major_qk=True), head_major_qk=True)


def test_a_pre_refuses_rows_that_are_not_whole_samples_of_32_tokens(dev):
    """M = 200 / 5 / 129 do not exist for PRE: rows_per_b must be a multiple of 32 that divides M."""
    p = dict(ut.problem(mode="pre", dtype=torch.float16, S=1, B=2, T=64))
    for T in (100, 40, 96):  # 128 rows: 100 and 96 do not divide them, 40 is no multiple of 32
        with pytest.raises(RuntimeError):
            ut.launch(dict(p, T=T), dev)


def _toleranced(dev, name, spec, figs_out=None):
    p = ut.problem(**spec)
    got = ut.launch(p, dev)
    figs = ut.check_toleranced_outputs(p, got)
    print({"case": name, "dtype": str(p["dtype"]), "susceptible": {k: round(v, 4) for k, v in p["sus"].items()},
           "row_rel_l2, err_over_bound": {k: (f"{a:.2e}", f"{b:.3g}") for k, (a, b) in figs.items()}})
    return p, got


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("case", [n for n, _ in ut.specs_c(torch.float16)])
def test_c_gauss(dev, dtype, case):
    """(c) N(0, 1) data, all three modes, S = 2; eps 1e-5, and one Q case with eps 1e-6 whose every 5th row is a constant
    plus 1-ulp noise (rstd ~ 1e3)."""
    p, _ = _toleranced(dev, "(c) " + case, dict(ut.specs_c(dtype))[case])
    if case.startswith("q_flat"):
        y = p["ref"]["y"][:, p["flat_rows"]]
        assert float(y.var(-1, unbiased=False).max()) < 10 * (2 * ug.U[dtype]) ** 2


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("case", [n for n, _ in ut.specs_d(torch.float16)])
def test_d_gauss_large_residuals(dev, dtype, case):
    """(d) res and blk ~ N(0, 16^2): the low part carries its 3 (fp16) / 8 (bf16) bits at a coarse ulp."""
    _toleranced(dev, "(d) " + case, dict(ut.specs_d(dtype))[case])


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
def test_e_two_runs_identical_bits(dev, dtype):
    """(e) every case of (c) twice: identical bits in every output."""
    for name, spec in ut.specs_c(dtype):
        p = ut.problem(**spec)
        first, second = ut.launch(p, dev), ut.launch(p, dev)
        for k in first:
            assert torch.equal(first[k], second[k]), f"(e) {name} {dtype}: {k} differs in {int((first[k] != second[k]).sum())} elements"
