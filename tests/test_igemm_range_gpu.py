"""ur_igemm (csrc/igemm.hip, igemm_epi.h, igemm_pp.hip) per element, on guarded layouts.  test_ops_gpu.py asserts one
whole-tensor rel-L2 on N(0, 1) operands in compact tensors: one wrong border pixel, a wrong row at a sample boundary inside
a tile, the last columns of a ragged N tile, a write behind n_store or a gather that reads in front of the buffer never
show there.  Here (tests/util_igemm.py):

  * groups (a) - (e) use the EXACT family: small integers, +-1 weights -- every partial sum in any order is an exact fp32
    integer and the result is representable in fp16 and bf16, so the output must be torch.equal to the float64 reference,
    on every tile build, with and without split-K; a mismatch is reported with its rows and columns;
  * every operand sits inside a NaN-filled buffer (ld > c, whole guard lines around an image) and every output inside a
    sentinel-filled one; nothing outside [M][n_store] (for V^T: [samples][N - vt_n0][vt_rows]) may change;
  * group (f) runs one N(0, 1) conv twice per tile and requires identical bits;
  * group (g) holds SiLU, GEGLU and the (hi, lo) pair to the element-wise bounds derived in util_igemm's docstring and to
    the per-row rel-L2 of test_ops_gpu.py, on N(0, 1) and on post-activation data, and prints the worst |err| / bound.

Shapes are the smallest that reach the edges: M = 300 (5 / 3 / 2 row tiles, the last with 44 rows), N = 328 (>= 2 column
tiles for every BN, the last ragged and no multiple of 16), 9 x 11 images with B = 3 (sample boundaries inside tiles).
Every descriptor is inside what igemm_run accepts, except the n_store case a tile's column grid cannot cover, which must
be refused with UR_E_BADARG before any launch (include/ur_kernels.h, n_store).
"""
import pytest
import torch

import util_igemm as ug

pytestmark = pytest.mark.gpu

DTYPES = ug.DTYPES
ids = lambda t: str(t).replace("torch.", "") if isinstance(t, torch.dtype) else None


def _need(tile):
    """Skip the cases of an opt-in kernel build (csrc/Makefile: PP=1) the loaded library does not contain."""
    from uni_renderer_amd import ops
    if tile in ug.PP_TILES and not ops.pp_built():
        pytest.skip("ping-pong tiles: opt-in build (make PP=1)")


def _bn(tile):
    from uni_renderer_amd import ops
    return ops.tile_table()[tile][1]


def _exact(p, dev, tile, what, **kw):
    """launch + torch.equal against the reference (columns n_out .. n_store: zero; low part: zero)."""
    got, lo = ug.launch(p, dev, tile, **kw)
    n = p["n_out"]
    ug.check_exact(got[..., :n], p["ref"], what)
    if got.shape[-1] > n:
        ug.check_exact(got[..., n:], torch.zeros_like(got[..., n:]), what + ": columns N .. n_store")
    if lo is not None:
        ug.check_exact(lo, torch.zeros_like(lo), what + ": out_lo")


# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("tile", ug.ALL_TILES)
def test_a_every_tile_exact(dev, dtype, tile):
    """(a) GEMM over two sources 128 | 64 with bias + rowadd + res, scale 0.5; K = 64 .. 320 (1, 2, 3, 5 chunks against
    rings of 2 - 5 slots); M = 5; conv s1 / s2 (pad 1 and 0) / nearest-2x."""
    _need(tile)
    for name, spec in ug.specs_a(dtype):
        _exact(ug.problem(**spec), dev, tile, f"(a) {name} tile {tile}")


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("hilo", [False, True], ids=["plain", "hilo"])
@pytest.mark.parametrize("tile", ug.REP)
def test_b_splitk_exact(dev, dtype, hilo, tile):
    """(b) uneven slices, one chunk per slice, the clamp; slices starting inside a channel block and inside the 1x1 tail;
    both second-pass kernels (M = 2970: the one without pipelined loads); with and without the (hi, lo) pair."""
    _need(tile)
    for name, spec, sks in ug.specs_b(dtype):
        p = ug.problem(**spec)
        for sk in sks:
            _exact(p, dev, tile, f"(b) {name} tile {tile} splitk {sk} hilo {hilo}", splitk=sk, hilo=hilo)


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("tile", ug.REP)
def test_c_n_store(dev, dtype, tile):
    """(c) n_store > N writes zeros in columns N .. n_store - 1, columns >= n_store keep the sentinel (ldc = 200), with and
    without split-K -- for every tile whose column grid ceil(N / BN) * BN reaches n_store.  A 160-wide tile at N = 150,
    n_store = 192 does not: the library must refuse that descriptor (UR_E_BADARG) and leave the output alone."""
    _need(tile)
    for name, spec, ns, ldc in ug.specs_c(dtype):
        p = ug.problem(**spec)
        for sk in (1, 2):
            what = f"(c) {name} tile {tile} splitk {sk}"
            if ug.roundup(p["N"], _bn(tile)) >= ns:
                _exact(p, dev, tile, what, splitk=sk, n_store=ns, ldc=ldc)
            else:
                with pytest.raises(RuntimeError, match="UR_E_BADARG"):
                    ug.launch(p, dev, tile, splitk=sk, n_store=ns, ldc=ldc)


def test_c_planned_tiles_cover_n_store(dev):
    """ops.igemm never hands the library a planned tile whose grid stops short of n_store (ops.vt_proj, the VAE's scores):
    a tuning-table row naming a 160-wide tile for T = 150 is replaced, and the pad columns are zero."""
    from uni_renderer_amd import ops
    dtype = torch.float16
    c = ug.case_zx_div(dtype)
    key = f"{c['Co']},150,{c['Ci']},1,{c['S'] * c['B']}"
    x = torch.cat([c["x"], c["x"][:, :73]], 1).contiguous()  # 150 tokens per sample
    ops.load_tuning_table()
    ops._tune_table[key] = (44, 1)
    ops._plan_cache.clear()
    try:
        vt = ops.vt_proj(x.to(dtype).to(dev), c["wv"].to(dtype).to(dev), streams=c["S"])
    finally:
        ops.load_tuning_table()
    ref = torch.stack([c["wv"][z // c["B"]] @ x[z].T for z in range(x.shape[0])])
    assert vt.shape == (6, c["Co"], 192)
    ug.check_exact(vt[..., :150].double().cpu(), ref, "vt_proj T = 150")
    assert float(vt[..., 150:].float().abs().max()) == 0.0


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("S", [1, 2], ids=["z1", "z2"])
@pytest.mark.parametrize("tile", ug.REP)
def test_d_transposed_value_output(dev, dtype, S, tile):
    """(d) out_vt with vt_rows = 77 (sample boundaries inside every tile), ldvt = 128, shared x (zx = 0), with and without
    split-K: token columns >= 77 of V^T, guard samples around it and the columns >= vt_n0 of ``out`` keep the sentinel."""
    from uni_renderer_amd import ops
    _need(tile)
    c = ug.case_vt(dtype, S)
    p, B, T, C = c["p"], c["B"], c["T"], c["C"]
    M, N, K = p["M"], p["N"], p["K"]
    x = ug.embed(p["x0"][0], K + 24, 8, 3, 3, dtype, dev)
    w = ug.embed(p["w"].reshape(S * N, K), K + 16, 8, 2, 2, dtype, dev)
    bias = ug.embed(p["bias"], N + 8, 4, 1, 1, torch.float32, dev)
    ldc, ldvt = 2 * C + 8, 128
    for sk in (1, 2):
        _, out, check_out = ug.sentinel_out(S * M, ldc, 2 * C, dtype, dev)
        vt = ug.sentinel((S * B + 2, C, ldvt), dtype, dev)  # one guard sample in front and behind
        ops.igemm(x0=x, w=w, out=out, M=M, N=N, K=K, c0=K, ldx0=x.stride(0), ldw=w.stride(0), ldc=ldc, n_store=2 * C,
                  bias=bias, out_scale=0.5, zbatch=S, zx=0, zw=N * w.stride(0), zbias=bias.stride(0), zout=M * ldc,
                  out_vt=vt[1:], vt_n0=2 * C, vt_rows=T, zvt=B * C * ldvt, tile=tile, splitk=sk)
        torch.cuda.synchronize()
        what = f"(d) tile {tile} z {S} splitk {sk}"
        qk = check_out(what + " out")
        named = torch.zeros(vt.shape, dtype=torch.bool)
        named[1:-1, :, :T] = True
        ug.assert_untouched(vt, named, what + " out_vt")
        ug.check_exact(qk.double().view(S, M, 2 * C), c["qk"], what + " q | k")
        ug.check_exact(vt.cpu()[1:-1, :, :T].double().view(S, B, C, T), c["vt"], what + " V^T")


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("tile", ug.REP)
def test_d_transposed_value_output_through_linear(dev, dtype, tile):
    """(d) the 64 k-token form the self-attention uses: ops.linear(vt_cols=...), two streams, with and without split-K."""
    from uni_renderer_amd import ops
    _need(tile)
    S, B, T, C = 2, 3, 64, 176
    p = ug.problem(mode="gemm", dtype=dtype, M=B * T, N=3 * C, c0=128, streams=S, bias=True, out_scale=0.5, seed=8)
    x, w, b = (p[k].to(dtype if k != "bias" else torch.float32).to(dev) for k in ("x0", "w", "bias"))
    full = p["pre"]
    for sk in (1, 2):
        qk, vt = ops.linear(x.view(S * B, T, 128), w, b, streams=S, out_scale=0.5, vt_cols=C, vt_tokens=T, tile=tile, splitk=sk)
        what = f"(d) linear vt_cols tile {tile} splitk {sk}"
        ug.check_exact(qk.double().cpu().view(S, B * T, 2 * C), full[..., :2 * C] * 0.5, what + " q | k")
        ug.check_exact(vt.double().cpu().view(S, B, C, T), full[..., 2 * C:].reshape(S, B, T, C).transpose(2, 3), what + " V^T")


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("tile", ug.REP)
def test_e_strides_and_z(dev, dtype, tile):
    """(e) x0 and w aliasing one [B, T, 2C] matrix with ldx0 = ldw = 2C > K (the VAE attention's scores, n_store = ldc = 128);
    zx_div = B with a weight shared by a stream's samples (ops.vt_proj's descriptor); two streams whose residual is the other
    stream's tensor (pointer at the second half, zres < 0); a grouped conv with per-stream bias and rowadd."""
    from uni_renderer_amd import ops
    _need(tile)
    # q . k^T
    c = ug.case_qk(dtype)
    B, T, C = c["B"], c["T"], c["C"]
    qk = ug.embed(c["qk"].reshape(B * T, 2 * C), 2 * C + 16, 8, 3, 3, dtype, dev)
    ld = qk.stride(0)
    _, out, check_out = ug.sentinel_out(B * T, 128, 128, dtype, dev)
    ops.igemm(x0=qk, w=qk[:, C:], out=out, M=T, N=T, K=C, c0=C, ldx0=ld, ldw=ld, ldc=128, n_store=128, out_scale=0.5,
              zbatch=B, zx=T * ld, zw=T * ld, zout=T * 128, tile=tile, splitk=1)
    torch.cuda.synchronize()
    got = check_out(f"(e) q.k^T tile {tile}").double().view(B, T, 128)
    ug.check_exact(got[..., :T], c["ref"], f"(e) q.k^T tile {tile}")
    ug.check_exact(got[..., T:], torch.zeros(B, T, 128 - T, dtype=torch.float64), f"(e) q.k^T tile {tile}: columns T .. 128")
    # zx_div
    c = ug.case_zx_div(dtype)
    S, B, T, Co, Ci = c["S"], c["B"], c["T"], c["Co"], c["Ci"]
    wv = ug.embed(c["wv"].reshape(S * Co, Ci), Ci + 24, 8, 3, 3, dtype, dev)
    x = ug.embed(c["x"].reshape(S * B * T, Ci), Ci + 16, 8, 2, 2, dtype, dev)
    _, out, check_out = ug.sentinel_out(S * B * Co, 136, 128, dtype, dev)
    ops.igemm(x0=wv, w=x, out=out, M=Co, N=T, K=Ci, c0=Ci, ldx0=wv.stride(0), ldw=x.stride(0), ldc=136, n_store=128,
              zbatch=S * B, zx=Co * wv.stride(0), zx_div=B, zw=T * x.stride(0), zout=Co * 136, tile=tile, splitk=1)
    torch.cuda.synchronize()
    got = check_out(f"(e) zx_div tile {tile}").double().view(S * B, Co, 128)
    ug.check_exact(got[..., :T], c["ref"], f"(e) zx_div tile {tile}")
    ug.check_exact(got[..., T:], torch.zeros(S * B, Co, 128 - T, dtype=torch.float64), f"(e) zx_div tile {tile}: columns T .. 128")
    # residual = the other stream's tensor
    c = ug.case_exchange(dtype)
    p = c["p"]
    M, N, K = p["M"], p["N"], p["K"]
    x = ug.embed(p["x0"].reshape(2 * M, K), K + 24, 8, 3, 3, dtype, dev)
    w = ug.embed(p["w"].reshape(2 * N, K), K + 16, 8, 2, 2, dtype, dev)
    bias = ug.embed(p["bias"], N + 8, 4, 1, 1, torch.float32, dev)
    res = ug.embed(p["res"].reshape(2 * M, N), N + 8, 0, 2, 2, dtype, dev)
    ldc = N + 8
    for sk in (1, 2):
        _, out, check_out = ug.sentinel_out(2 * M, ldc, N, dtype, dev)
        ops.igemm(x0=x, w=w, out=out, M=M, N=N, K=K, c0=K, ldx0=x.stride(0), ldw=w.stride(0), ldc=ldc, bias=bias,
                  res=res[M:], ldres=res.stride(0), zbatch=2, zx=M * x.stride(0), zw=N * w.stride(0), zbias=bias.stride(0),
                  zres=-M * res.stride(0), zout=M * ldc, tile=tile, splitk=sk)
        torch.cuda.synchronize()
        got = check_out(f"(e) exchange tile {tile} splitk {sk}").double().view(2, M, N)
        ug.check_exact(got, c["ref"], f"(e) exchange tile {tile} splitk {sk}")
    # grouped conv
    p = ug.problem(**ug.spec_e_grouped(dtype))
    for sk in (1, 3):
        _exact(p, dev, tile, f"(e) grouped conv tile {tile} splitk {sk}", splitk=sk)


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("tile", ug.REP)
def test_f_two_runs_identical_bits(dev, dtype, tile):
    """(f) one N(0, 1) conv, run twice on the same inputs (plain and split-K 3): identical bits, and within the bounds."""
    _need(tile)
    p = ug.problem(**ug.spec_f(dtype))
    b = ug.bounds(p)
    for sk in (1, 3):
        first, _ = ug.launch(p, dev, tile, splitk=sk)
        second, _ = ug.launch(p, dev, tile, splitk=sk)
        assert torch.equal(first, second), f"(f) tile {tile} splitk {sk}: two runs differ in {int((first != second).sum())} elements"
        ug.check_elem(first, p["ref"], b["hi"], ug.TOL[dtype], f"(f) tile {tile} splitk {sk}")


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("family", ["gauss", "act"])
@pytest.mark.parametrize("tile", ug.REP)
def test_g_toleranced(dev, dtype, family, tile):
    """(g) SiLU, GEGLU (N = 336 -> 168 columns; every 7th group of gates shifted into [-12, -6], where 0.5 x + 0.5 |x| erf
    cancels), the (hi, lo) pair with and without split-K; on "act" data also one K = 5760 conv."""
    _need(tile)
    cases = ug.specs_g(dtype, family)
    if family == "act":
        cases = cases + [("conv_K5760", ug.spec_g_long_conv(dtype), False, (1,))]
    figs = {}
    for name, spec, hilo, sks in cases:
        p = ug.problem(**spec)
        b = ug.bounds(p)
        if name == "geglu":
            assert bool(((p["gate"] > -12) & (p["gate"] < -6)).any())
        for sk in sks:
            what = f"(g) {family} {name} tile {tile} splitk {sk}"
            got, lo = ug.launch(p, dev, tile, splitk=sk, hilo=hilo)
            figs[f"{name}_sk{sk}"] = ug.check_elem(got, p["ref"], b["hi"], ug.TOL[dtype], what) + (ug.fp_part_used(got, p),)
            if hilo:
                figs[f"{name}_sk{sk}_pair"] = ug.check_elem(got + lo, p["ref"], b["pair"], ug.TOL[dtype], what + " pair")
    print({"case": f"(g) {family} tile {tile} {dtype}", "row_rel_l2, err_over_bound, fp32_part_used":
           {k: (f"{v[0]:.2e}",) + tuple(f"{x:.3f}" for x in v[1:]) for k, v in figs.items()}})
