"""tests/util_tchain.py checked without a GPU (runs in -m "not gpu"):

  * reference: make_problem's float64 reference equals the chain written with independent torch float64 calls (F.linear,
    F.layer_norm, F.gelu) and the same rounding points, one small problem per mode; the packed weight stream is the stored
    matrices (decoded through the documented layout for one probe element per matrix);
  * exactness: every gamma0 problem of test_tchain_range_gpu.py passes its assertions (make_problem raises otherwise), and
    a draw that violates them fails loudly;
  * the GEGLU program's formula in float32 with the kernel's constants gives exactly 2 gate value for integer gates 7 .. 16;
  * emulation: an fp32 emulation of a correct kernel (64-wide k chunks forwards and backwards, two-pass LayerNorm, the
    program's formula, ops.lo_encode) stays within HALF of fp + D before the storage rounding and within the whole bound
    after it, for every toleranced problem of the GPU file, both dtypes;
  * sensitivity: the rounded reference stands in for a kernel output and is damaged; the new checkers must reject each
    damage in both dtypes.  The whole-tensor rel-L2 assertions of test_tchain_gpu.py are evaluated on the same tensors and
    their verdicts printed (-s): they accept 1 in bf16, 2, 3, 4 in bf16 and 5, and never look at 6 and 7.  Two limits of
    the toleranced checker are printed as well: it rejects a zero FF out.lo only on the case "ff_po1" (dense Wpo: D is wider
    than a low part), and it does not see 8 ulp in one fp16 q element (the exact checker does, in both dtypes).
"""
import pytest
import torch
import torch.nn.functional as F

import util_igemm as ug
import util_tchain as ut

DTYPES = ug.DTYPES
ids = lambda t: str(t).replace("torch.", "") if isinstance(t, torch.dtype) else None
f64 = torch.float64
C = ut.C


# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("mode", ["q", "pre", "ff"])
def test_reference_is_the_operation(dtype, mode):
    shape = dict(B=2, T=32) if mode == "pre" else dict(M=37)
    p = ut.make_problem(dict(mode=mode, family="gauss", dtype=dtype, S=2, seed=5, **shape))
    r = lambda t: t.to(dtype).to(f64)
    for s in range(2):
        y = F.linear(p["a0"][s], p["w0"][s], p["b0"][s])
        if mode != "pre":
            y = y + p["res"][s] + p["res_lo"][s]
        assert torch.allclose(p["ref"]["y"][s], y, rtol=0, atol=1e-12)
        xn = r(F.layer_norm(y, (C,), p["gamma"][s], p["beta"][s], p["eps"]))
        assert float((xn != p["xn"][s]).double().mean()) < 1e-3  # two float64 evaluation orders: a tie may round the other way
        xn = p["xn"][s]
        if mode == "q":
            assert torch.equal(p["wq"][s], r((p["wq_raw"][s].float() * p["scale"]).double()))
            assert torch.allclose(p["ref"]["q"][s], F.linear(xn, p["wq"][s]), rtol=0, atol=1e-12)
        elif mode == "pre":
            for n in "qkv":
                assert torch.allclose(p["ref"][n][s], F.linear(xn, p["w" + n][s]), rtol=0, atol=1e-12)
            vt = ut.vt_of(p, p["ref"]["v"])
            assert vt.shape == (2, 2, C, 32) and torch.equal(vt[s, 1, 7, 5], p["ref"]["v"][s, 32 + 5, 7])
        else:
            hc = F.linear(xn, p["w1"][s], p["b1"][s])
            h = hc[:, :ut.FF] * F.gelu(hc[:, ut.FF:])                 # diffusers' GEGLU: value * gelu(gate), erf form
            h2 = r(2 * h)
            assert float((h2 != p["h2"][s]).double().mean()) < 1e-3
            # the host halves w2 instead: the same sum while 0.5 * w2 is not subnormal (a power of two changes no rounding)
            w2 = r(p["w2_raw"][s])
            big = w2.abs() >= 2.0 ** -13
            assert torch.equal((2 * p["w2s"][s])[big], w2[big])
            y3 = y + p["b2"][s] + F.linear(p["h2"][s], p["w2s"][s])
            assert float((r(y3) != p["y3"][s]).double().mean()) < 1e-3
            out = F.linear(p["y3"][s], p["wpo"][s], p["bpo"][s]) + p["blk"][s] + p["blk_lo"][s]
            assert torch.allclose(p["ref"]["out"][s], out, rtol=0, atol=1e-12)


def test_packed_stream_holds_the_stored_matrices():
    """The GPU tests take the stream from the product's packer; here one probe per matrix is read back through the layout
    tchain.py documents (stage images of 64 k, chunk XOR-swizzle by (row >> 1) & 7, KPERM behind the first GEMM, the FF
    order A0 A1 | A0 A1 B ... | B), so that reference and stream provably describe the same matrices."""
    from uni_renderer_amd import tchain
    dt = torch.float16
    p = ut.make_problem(dict(mode="ff", family="gauss", dtype=dt, S=1, M=8, seed=2))
    ws, cs = ut.pack(p)
    img = ws[0].double().view(-1, tchain.STAGE // 2)
    inv = [tchain.KPERM16.index(i) for i in range(16)]  # packed position of original column i of a 16-group

    def at(stage, row, k, rows_off=0, permuted=True):
        """element (row, original k) of the [rows, 64] image at element offset rows_off * 64 of ``stage``."""
        kk = k % 64
        if permuted:
            kk = (kk // 16) * 16 + inv[kk % 16]
        chunk, e = kk // 8, kk % 8
        pos = chunk ^ ((row >> 1) & 7)
        return float(img[stage, (rows_off + row) * 64 + pos * 8 + e])

    n, k = 77, 200
    assert at(k // 64, n, k, permuted=False) == float(p["w0"][0, n, k])                        # leading GEMM: stages 0 .. 4
    j, half, hid, kc = 3, 1, 3 * 64 + 32 + 9, 2                                                # A1(3): stage 5 + 2 + 3 * 2 + 1
    st = 5 + 2 + 3 * (j - 1) + half
    assert at(st, 9, 64 * kc + 21, rows_off=64 * kc) == float(p["w1"][0, hid, 64 * kc + 21])               # value row
    assert at(st, 32 + 9, 64 * kc + 21, rows_off=64 * kc) == float(p["w1"][0, ut.FF + hid, 64 * kc + 21])  # gate row
    assert at(5 + 2 + 3 * j + 2, n, 64 * j + 40) == float(p["w2s"][0, n, 64 * j + 40])         # B(3) follows A0(4) A1(4)
    last = img.shape[0] - 5
    assert at(last - 1, n, 64 * 19 + 3) == float(p["w2s"][0, n, 64 * 19 + 3])                  # B(19) closes the FF
    assert at(last + k // 64, n, k) == float(p["wpo"][0, n, k])
    assert torch.equal(cs[0, :C].double(), p["b0"][0]) and torch.equal(cs[0, 960 + ut.FF:960 + 2 * ut.FF].double(), p["b1"][0, ut.FF:])


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
def test_every_gamma0_problem_of_the_gpu_file_is_exact(dtype):
    ranges = ut.gamma0_problems(dtype)
    assert len(ranges) >= 16
    for name, r in ranges.items():
        print({"gamma0": name, "dtype": str(dtype), "max_abs": r})


def test_exactness_violation_fails_loudly(monkeypatch):
    draw = ut._draw

    def low_gate_bias(p, g):
        d = draw(p, g)
        d["b1"][:, ut.FF:] = 5.0
        return d

    monkeypatch.setattr(ut, "_draw", low_gate_bias)
    with pytest.raises(AssertionError, match="exact family"):
        ut.make_problem(dict(mode="ff", M=8))


def test_geglu_program_is_exact_for_integer_gates_7_to_16():
    """2 value gelu(gate) = 2 gate value exactly: p t exp2(-zc^2) is below 2^-25, the erf rounds to 1."""
    gate = torch.arange(7, 17, dtype=torch.float32)[:, None]
    value = torch.arange(-9, 10, dtype=torch.float32)[None, :]
    zero = torch.zeros((), dtype=torch.float32)
    got = ut.geglu_program_f32(value - 1.0, zero + 1.0, gate - 10.0, zero + 10.0)  # through the bias additions, as the kernel
    assert torch.equal(got, (2 * gate * value).expand_as(got))
    # and the formula is the GELU elsewhere: within the allowance of the bound's derivation
    g = torch.linspace(-8, 8, 4001, dtype=torch.float32)
    err = (ut.geglu_program_f32(zero + 1.0, zero, g, zero).double() - ut.gelu2_64(g.double())).abs()
    assert bool((err <= 2 * ug.c_gelu(g.double())).all())
    print({"geglu_program": "worst error / allowance", "value": float((err / (2 * ug.c_gelu(g.double())).clamp_min(1e-300)).max())})


# ---------------------------------------------------------------------------------------------------------------
def _all_toleranced(dtype):
    return [("c_" + n, s) for n, s in ut.specs_c(dtype)] + [("d_" + n, s) for n, s in ut.specs_d(dtype)]


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("case", [n for n, _ in _all_toleranced(torch.float16)])
def test_fp32_emulation_within_half_of_the_fp32_part(dtype, case):
    p = ut.problem(**dict(_all_toleranced(dtype))[case])
    figs = {}
    for order in ("fwd", "rev"):
        emu = ut.emulate(p, order)
        got = {}
        for name, (v32, hi, lo) in emu.items():
            b = ut.bounds(p, name)
            _, figs[f"{name}_{order}_fp32"] = ug.check_elem(v32, p["ref"][name], b["fp"], float("inf"), f"{case} {order} {name} fp32 value",
                                                           frac=0.5, rel=False)
            if name == "v":
                got["vt"] = ut.vt_of(p, hi)
            else:
                got[name] = hi
            if lo is not None:
                got[name + "_lo"] = lo
        for k, v in ut.check_toleranced_outputs(p, got).items():
            figs[f"{k}_{order}"] = v
    print({"emulation": case, "dtype": str(dtype), "susceptible": {k: round(v, 4) for k, v in p["sus"].items()},
           "row_rel_l2, err_over_bound | fp32_err_over_fp_plus_D":
               {k: (tuple(f"{x:.3g}" for x in v) if isinstance(v, tuple) else f"{v:.3g}") for k, v in figs.items()},
           "median_bound_over_u_v": {n: f"{float((ut.bounds(p, n)['hi'] / (ug.U[dtype] * p['ref'][n].abs()).clamp_min(1e-30)).median()):.3g}"
                                     for n in ut.OUTPUTS[p['mode']]}})


# ---------------------------------------------------------------------------------------------------------------
def _rejected(fn, *a, **kw):
    try:
        fn(*a, **kw)
    except AssertionError:
        return True
    return False


def _old(got, p, name, pair):
    """What test_tchain_gpu.py asserts about this output: one whole-tensor rel-L2 per stream, (figure, tolerance)."""
    v = got[name] + (got[name + "_lo"] if pair else 0.0)
    tol = ut.OLD_PAIR_TOL[p["dtype"]] if (pair and name == "y") else ut.TOL[p["dtype"]]
    return max(ug.old_rel_l2(v[s], p["ref"][name][s]) for s in range(p["S"])), tol


def _report(name, dtype, new_rejects, old):
    fig, tol = old
    print({"sensitivity": name, "dtype": str(dtype), "new_checkers_reject": new_rejects, "old_rel_l2": f"{fig:.3g}",
           "old_tolerance": tol, "old_assertion_accepts": fig < tol})


def _standin(dtype, which):
    spec = dict(ut.specs_c(dtype) + ut.specs_d(dtype))[which]
    p = ut.problem(**spec)
    got = ut.standin(p)
    ut.check_toleranced_outputs(p, got)
    return p, {k: v.clone() for k, v in got.items()}


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
def test_sensitivity_1_y_lo_all_zero(dtype):
    p, got = _standin(dtype, "q")
    got["y_lo"].zero_()
    rej = _rejected(ut.check_toleranced_outputs, p, got)
    _report("1 y.lo = 0", dtype, rej, _old(got, p, "y", True))
    assert rej


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
def test_sensitivity_2_y_lo_of_a_row_from_the_next_row(dtype):
    p, got = _standin(dtype, "q")
    got["y_lo"][1, 150] = got["y_lo"][1, 151]
    rej = _rejected(ut.check_toleranced_outputs, p, got)
    _report("2 y.lo[r] = y.lo[r + 1]", dtype, rej, _old(got, p, "y", True))
    assert rej


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
def test_sensitivity_3_ff_out_lo_zero(dtype):
    """On "ff_po1_res16", the case built so that D_out does not swamp the pair bound.  On the dense-Wpo FF problems the
    worst-case D is wider than a low part and an all-zero out.lo is NOT rejected by the element bound (printed)."""
    p, got = _standin(dtype, "ff_po1_res16")
    got["out_lo"].zero_()
    rej = _rejected(ut.check_toleranced_outputs, p, got)
    _report("3 ff out.lo = 0 (po1, res 16)", dtype, rej, _old(got, p, "out", True))
    pd, gd = _standin(dtype, "ff")
    gd["out_lo"].zero_()
    _report("3' ff out.lo = 0 (dense Wpo: D wider than the low part)", dtype, _rejected(ut.check_toleranced_outputs, pd, gd),
            _old(gd, pd, "out", True))
    assert rej


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
def test_sensitivity_4_two_tokens_of_a_vt_channel_swapped(dtype):
    p, got = _standin(dtype, "pre")
    a, b = got["vt"][1, 2, 77, 40].clone(), got["vt"][1, 2, 77, 41].clone()
    got["vt"][1, 2, 77, 40], got["vt"][1, 2, 77, 41] = b, a
    rej = _rejected(ut.check_toleranced_outputs, p, got)
    tok = {"v": got["vt"].transpose(2, 3).reshape(p["ref"]["v"].shape)}
    _report("4 V^T tokens swapped", dtype, rej, _old(tok, p, "v", False))
    assert rej


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
def test_sensitivity_5_one_q_element_off_by_8_ulp(dtype):
    """What resolves 8 ulp of ONE element behind a rounded operand: the exact family always (any element, both dtypes:
    asserted); the toleranced bound in bf16 (asserted at the element of median magnitude of its row).  In fp16 the
    worst-case fp32 error of y (c(320) A ~ 7e-4) is as large as an ulp of xn, every operand is susceptible and D ~ 100
    u |v| at a median element: the toleranced bound does NOT see 8 ulp there, not even at the largest element of the row
    (printed): an order-independent fp32 bound over K = 320 dense N(0, 1) terms has no room for it.  For fp16 this damage is
    the exact family's to catch."""
    def damage(got, r, c):
        v = got["q"][0, r, c]
        got["q"][0, r, c] = v + 8 * 2 * ug.U[dtype] * 2.0 ** torch.floor(torch.log2(v.abs()))

    verdict = {}
    for where, pick in (("median", lambda a: int(a.argsort()[C // 2])), ("largest", lambda a: int(a.argmax()))):
        p, got = _standin(dtype, "q")
        damage(got, 150, pick(p["ref"]["q"][0, 150].abs()))
        verdict[where] = _rejected(ut.check_toleranced_outputs, p, got)
        _report(f"5 one q element + 8 ulp ({where} element of row 150)", dtype, verdict[where], _old(got, p, "q", False))
    assert verdict["median"] or dtype == torch.float16
    p = ut.problem(mode="q", dtype=dtype, S=1, M=200)
    got = {k: v.clone() for k, v in ut.standin(p).items()}
    r, c = (p["ref"]["q"][0].abs() > 0).nonzero()[0].tolist()
    damage(got, r, c)
    assert _rejected(ut.check_exact_outputs, p, got)


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
def test_sensitivity_6_and_7_stores_outside_the_named_region(dtype):
    """6: a store in row M (the first guard row behind the output), for the output type and the low part's byte; 7: a store
    in V^T column T, and in the guard sample behind.  The undamaged buffers pass.  The old test never looks there."""
    from uni_renderer_amd import ops
    M, G = 200, ut.GUARD_ROWS
    for t in (dtype, ops.lo_dtype(dtype)):
        named = ug.region2d((M + 2 * G, C), G, M, C)
        buf = ug.sentinel(named.shape, t, "cpu")
        buf[named] = 0
        ug.assert_untouched(buf, named, "undamaged")
        for r in (G + M, G - 1):
            bad = buf.clone()
            bad[r, 5] = 0
            assert _rejected(ug.assert_untouched, bad, named, "6"), (t, r)
    B, T = 3, 96
    vt = ug.sentinel((B + 2, C, ut.ld_vt_of(T)), dtype, "cpu")
    named = torch.zeros(vt.shape, dtype=torch.bool)
    named[1:-1, :, :T] = True
    vt[named] = 0
    ug.assert_untouched(vt, named, "undamaged")
    for idx in ((2, 17, T), (B + 1, 0, 0), (0, C - 1, T - 1)):
        bad = vt.clone()
        bad[idx] = 0
        assert _rejected(ug.assert_untouched, bad, named, "7"), idx
    print({"sensitivity": "6 / 7 stores outside the named region", "dtype": str(dtype), "new_checkers_reject": True,
           "old_assertion_accepts": "never looks (columns T .. Tpad must be ZERO there: a stored zero passes)"})


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("mode", ["q", "ff"])
def test_sensitivity_exact_family_weight_column_from_its_kperm_neighbour(dtype, mode):
    """A decode that forgets KPERM for one column: column 4 of every 16-group of the second matrix (Wq; in FF: W1) read
    from packed position 4, which holds column 8.  The exact family must see it."""
    from uni_renderer_amd import tchain
    p = ut.problem(mode=mode, dtype=dtype, S=1, M=200)
    name = "wq" if mode == "q" else "w1"
    assert tchain.KPERM16[4] == 8
    bad = dict(p)
    for k in ("wq", "wq_raw", "w1"):
        if k in p:
            bad[k] = p[k].clone()
    cols = torch.arange(4, C, 16)  # in every 16-group
    bad[name][..., cols] = p[name][..., cols + 4]
    # the reference recomputed over the damaged matrix is what such a kernel would store
    xn = p["xn"]
    if mode == "q":
        got = dict(ut.standin(p), q=torch.einsum("smk,snk->smn", xn, bad["wq"]))
    else:
        hc = torch.einsum("smk,snk->smn", xn, bad["w1"]) + p["b1"][:, None]
        h2 = ug.rnd(hc[..., :ut.FF] * ut.gelu2_64(hc[..., ut.FF:]), dtype)
        y3 = ug.rnd(p["ref"]["y"] + p["b2"][:, None] + torch.einsum("smk,snk->smn", h2, p["w2s"]), dtype)
        out = torch.einsum("smk,snk->smn", y3, p["wpo"]) + p["bpo"][:, None] + p["blk"] + p["blk_lo"]
        hi, lo = ug._lo_pair(out, dtype)
        got = dict(out=hi, out_lo=lo)
    ut.check_exact_outputs(p, ut.standin(p))
    assert _rejected(ut.check_exact_outputs, p, got)
