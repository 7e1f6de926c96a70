"""ur_wgrad / ur_wgrad_group (csrc/wgrad.hip) and the rest of backward.conv3x3_backward / linear_backward per element, on
guarded layouts (tests/util_wgrad.py).  test_wgrad_gpu.py asserts one whole-matrix figure on N(0, 1) operands in compact
tensors and test_backward_gpu.py one whole-tensor rel-L2 at one shape each: which elements are wrong, a read of row P or of
pixel -1, a store behind [N][K] or behind the slab never show there.  Here:

  * the EXACT family (small integers against sparse +-1: every partial sum under any order and any slicing of P is an
    exact fp32 integer, the result representable in fp16 and bf16) must come out torch.equal to the float64 reference, on
    every tile, for every slice count -- trailing empty slices included --, single and grouped; a mismatch is reported
    with its rows and columns;
  * dy and x lie in NaN-filled buffers (column slices, guard stages / guard lines around them), dw, db and ``partial`` in
    sentinel-filled ones; nothing outside [N][K], [N] and the slab floats may change;
  * descriptor fields the wrappers never set run through a hand-filled ur_wgrad_desc: lddw > K, conv ldx > C, pad = 0;
  * the N(0, 1) family is held to the element-wise bounds derived in util_wgrad's docstring, and the worst figures printed;
  * dx (rotated weights from ``weight_rot`` and from ``_rot_weights``, zero insertion for stride 2, 28 -> 64 channel
    padding), the im2col + transposes weight gradient of maps whose sides are no powers of two, and linear_backward with dy
    a column slice of a wider gradient, against float64 autograd of F.conv2d / F.linear on the CPU, exactly.

Shapes are the smallest that reach the edges: P = 300 (10 stages of 32 rows, the last with 12), N = 328 and K = 200 (ragged
on every tile width, no multiples of 16, grids that are no multiples of 8), images of 2 x 4 .. 16 x 8 output pixels with
sample boundaries inside a stage.
"""
import pytest
import torch

import util_wgrad as uw

pytestmark = pytest.mark.gpu

DTYPES = uw.DTYPES
ids = lambda t: str(t).replace("torch.", "") if isinstance(t, torch.dtype) else None


def _exact(got, p, what):
    dw, db = got[0], got[1]
    uw.check_exact(dw, p["dw"], what + " dw")
    if db is not None:
        uw.check_exact(db[None], p["db"][None], what + " db")


# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("tile", uw.TILES)
def test_exact_linear(dev, dtype, tile):
    """P = 300 (10 stages, the last with 12 rows), 5 (less than a stage), 33, 2085 (66 stages); with and without db; the
    hand-filled descriptor (every output guarded, lddw = K + 8) and backward.wgrad with the library's slice count."""
    for P, N, K in uw.LINEAR:
        p = uw.problem(**uw.spec_linear(dtype, P, N, K))
        for need_db in (True, False):
            _exact(uw.launch_direct(p, dev, tile, 1, need_db), p, uw.describe(p, tile, 1) + f" db {need_db}")
            _exact(uw.launch_wrapper(p, dev, tile, 0, need_db), p, "backward.wgrad " + uw.describe(p, tile, 0) + f" db {need_db}")
    if tile == 1:
        for P, N, K in uw.LINEAR:  # tile 0: the library's choice of tile as well
            p = uw.problem(**uw.spec_linear(dtype, P, N, K))
            _exact(uw.launch_wrapper(p, dev, 0, 0, True), p, "backward.wgrad " + uw.describe(p, 0, 0))


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("tile", uw.TILES)
def test_exact_slices(dev, dtype, tile):
    """P = 300 in 2, 3, 4, 7 (two trailing slices without work: their slabs must still be zeros) and 10 slices; P = 2085 in
    the library's count and in 64; bit-identical to one slice; the sentinel tail behind ``partial`` intact."""
    for (P, N, K), slices in ((uw.LINEAR[0], uw.SLICES_300), (uw.LINEAR[3], uw.SLICES_2085)):
        p = uw.problem(**uw.spec_linear(dtype, P, N, K))
        one = uw.launch_direct(p, dev, tile, 1)
        _exact(one, p, uw.describe(p, tile, 1))
        for s in slices:
            got = uw.launch_direct(p, dev, tile, s)
            what = uw.describe(p, tile, got[2])
            if s:
                assert got[2] == s
            _exact(got, p, what)
            assert torch.equal(got[0], one[0]) and torch.equal(got[1], one[1]), what + ": differs from one slice"
        _exact(uw.launch_direct(p, dev, tile, slices[-1], need_db=False), p, uw.describe(p, tile, slices[-1]) + " without db")
        _exact(uw.launch_wrapper(p, dev, tile, 3), p, "backward.wgrad " + uw.describe(p, tile, 3))


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("tile", uw.TILES)
def test_exact_conv(dev, dtype, tile):
    """B = 5 of 2 x 4 (sample boundaries every 8 rows), B = 3 of 4 x 8 at C = 192 (tap boundary inside a k tile), B = 2 of
    16 x 8, each at stride 1 and 2; stride 2 on an odd 7 x 15 input; pad = 0 (stride 2, 8 x 8 -> 4 x 4: taps beyond the last
    line / column only); ldx = C + 8.  N = 328, slices 1 and 3 -- 2 where P = 40 or 48 has only two stages: the library
    refuses more slices than stages (UR_E_BADARG, asserted), backward.wgrad clamps the same way."""
    for name, spec, ldx_pad in uw.specs_conv(dtype):
        p = uw.problem(**spec)
        stages = -(-p["P"] // uw.STAGE)
        if stages < 3:
            with pytest.raises(RuntimeError, match="UR_E_BADARG"):
                uw.launch_direct(p, dev, tile, 3, ldx_pad=8)
        for s in (1, min(3, stages)):  # every hand-filled descriptor reads pixels of C + 8 elements ...
            _exact(uw.launch_direct(p, dev, tile, s, ldx_pad=8), p, f"{name}: " + uw.describe(p, tile, s))
        if not ldx_pad:                # ... and once the compact image the wrapper names
            _exact(uw.launch_direct(p, dev, tile, 1), p, f"{name}: compact " + uw.describe(p, tile, 1))
        if p["pad"] == 1:
            _exact(uw.launch_wrapper(p, dev, tile, 0), p, f"{name}: backward.wgrad " + uw.describe(p, tile, 0))


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("tile", uw.TILES)
def test_exact_grouped(dev, dtype, tile):
    """3 x (300, 328, 200) in 3 slices with db absent in the middle problem; UR_WGRAD_GROUP_MAX x (40, 64, 64); 4 convs
    (B = 3, 4 x 8, C = 64, stride 2) in 2 slices.  Every problem has its own guarded buffers and is compared with float64."""
    for name, specs, slices, no_db in uw.specs_group(dtype):
        probs = [uw.problem(**s) for s in specs]
        for i, (p, got) in enumerate(zip(probs, uw.launch_group(probs, dev, tile, slices, no_db))):
            assert (got[1] is None) == (i in no_db)
            _exact(got, p, f"group {name} problem {i} tile {tile}")


# ---------------------------------------------------------------------------------------------------------------
_worst = {}


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("tile", uw.TILES)
def test_toleranced(dev, dtype, tile):
    """N(0, 1) operands: |dw - ref| <= u |ref| + (P + slices + 8) 2^-23 A + TINY and |db - ref| <= (P + slices) 2^-24
    sum |dy| element by element, per-row rel-L2 below test_wgrad_gpu.py's TOL; slices 1 and 4 (the conv has P = 96, three
    stages: 4 slices are refused with UR_E_BADARG, asserted, and it runs in 3)."""
    for name, spec in uw.specs_toleranced(dtype):
        p = uw.problem(**spec)
        stages = -(-p["P"] // uw.STAGE)
        if stages < 4:
            with pytest.raises(RuntimeError, match="UR_E_BADARG"):
                uw.launch_direct(p, dev, tile, 4)
        for s in (1, min(4, stages)):
            dw, db, used = uw.launch_direct(p, dev, tile, s, ldx_pad=8 if p["conv"] is not None else 0)
            assert used == s
            b = uw.bounds(p, s)
            what = f"{name}: " + uw.describe(p, tile, s)
            rel, ratio = uw.check_elem(dw, p["dw"], b["dw"], uw.TOL[dtype], what + " dw")
            _, rdb = uw.check_elem(db, p["db"], b["db"], float("inf"), what + " db", rel=False)
            w = _worst.setdefault((str(dtype), name), [0.0, 0.0, 0.0, 0.0])
            for i, v in enumerate((rel, ratio, uw.fp_part_used(dw, p, s), rdb)):
                w[i] = max(w[i], v)
    for (dt, name), w in sorted(_worst.items()):
        if dt == str(dtype):
            print({"toleranced": name, "dtype": dt, "tiles_so_far": tile, "worst_row_rel_l2": w[0], "worst_err_over_bound": w[1],
                   "fp32_part_used": w[2], "worst_db_err_over_bound": w[3]})


# ---------------------------------------------------------------------------------------------------------------
# backward.conv3x3_backward / linear_backward against float64 autograd on the CPU
def _conv_backward(q, dev, **kw):
    from uni_renderer_amd import backward as bw
    dt = q["dtype"]
    x, w, dy = (q[k].to(dt).to(dev) for k in ("x", "w", "dy"))
    dx, dw, db = bw.conv3x3_backward(x, w, dy, True, stride=q["stride"], **kw)
    torch.cuda.synchronize()
    assert dx.dtype == dt and dw.dtype == dt and db.dtype == torch.float32
    return dx.double().cpu(), dw.double().cpu(), db.double().cpu(), (x, w, dy)


def _check_bwd(got, q, what):
    dx, dw, db = got[:3]
    uw.check_exact(dx.reshape(-1, dx.shape[-1]), q["dx"].reshape(-1, dx.shape[-1]), what + " dx")
    uw.check_exact(dw, q["dw"], what + " dw")
    uw.check_exact(db[None], q["db"][None], what + " db")


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
def test_conv_data_gradient_exact(dev, dtype):
    """dx at stride 1 (9 x 11, N = 72), stride 2 (8 x 12 -> 4 x 6: zero insertion), N = 28 (padded to 64) and N = 128; the
    weight and bias gradients of the same calls (im2col + transposes: 9 x 11 and 4 x 6 are no powers of two) as well."""
    for name, s in uw.specs_bwd_dx():
        q = uw.bwd_problem("conv", "dgrad", dtype, **s)
        _check_bwd(_conv_backward(q, dev), q, f"conv3x3_backward {name} {dtype}")


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
def test_conv_data_gradient_with_cached_rotated_weights(dev, dtype, monkeypatch):
    """The rotated weights once from ``weight_rot`` (filled by rot_weights_many, as autograd_ops.PackConvWeights does; here
    _rot_weights must not run) and once from ``_rot_weights``: the same exact dx."""
    from uni_renderer_amd import backward as bw
    q = uw.bwd_problem("conv", "dgrad", dtype, **dict(uw.specs_bwd_dx())["s1_9x11_N128"])
    w = q["w"].to(dtype).to(dev)
    x, dy = q["x"].to(dtype).to(dev), q["dy"].to(dtype).to(dev)
    key = (w.data_ptr(), tuple(w.shape))
    assert bw.weight_rot.lookup(key) is None
    called = []
    real = bw._rot_weights
    monkeypatch.setattr(bw, "_rot_weights", lambda *a: (called.append(1), real(*a))[1])
    dx0 = bw.conv3x3_backward(x, w, dy)[0]
    assert called == [1]
    bw.weight_rot.put(key, w, bw.rot_weights_many([(w, q["C"])])[0])
    try:
        dx1 = bw.conv3x3_backward(x, w, dy)[0]
    finally:
        bw.weight_rot.pop(key, None)
    torch.cuda.synchronize()
    assert called == [1], "weight_rot was not consulted"
    for name, dx in (("_rot_weights", dx0), ("weight_rot", dx1)):
        uw.check_exact(dx.double().cpu().reshape(-1, q["C"]), q["dx"].reshape(-1, q["C"]), f"dx through {name} {dtype}")


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
def test_conv_weight_gradient_fallback_exact(dev, dtype, monkeypatch):
    """Maps whose sides are no powers of two take ur_im2col3x3_t + transposes: 6 x 12 at stride 1, 12 x 6 -> 6 x 3 at stride
    2.  With WGRAD forced off a 4 x 8 map takes the same route and must equal the ur_wgrad result bit for bit."""
    from uni_renderer_amd import backward as bw
    for name, s in uw.specs_bwd_dw():
        q = uw.bwd_problem("conv", "wgrad", dtype, **s)
        before = bw.wgrad_stats["problems"]
        _check_bwd(_conv_backward(q, dev), q, f"conv3x3_backward {name} {dtype}")
        assert bw.wgrad_stats["problems"] == before + 1
    q = uw.bwd_problem("conv", "wgrad", dtype, **uw.SPEC_BWD_FORCED)
    outs = {}
    for flag in (True, False):
        monkeypatch.setattr(bw, "WGRAD", flag)
        outs[flag] = _conv_backward(q, dev)
        _check_bwd(outs[flag], q, f"conv3x3_backward 4 x 8 WGRAD {flag} {dtype}")
    for a, b in zip(outs[True][:3], outs[False][:3]):
        assert torch.equal(a, b)


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("family", ["dgrad", "wgrad"])
@pytest.mark.parametrize("wgrad", [True, False], ids=["ur_wgrad", "transposes"])
def test_linear_backward_exact_from_a_column_slice(dev, dtype, family, wgrad, monkeypatch):
    """(2, 150, 200) -> 328 with dy columns 8 .. 336 of a 344-wide NaN-filled gradient: dx (a contraction over 328, no
    multiple of 64), dw (ur_wgrad reads the slice in place; with WGRAD off: transposed copies) and db."""
    from uni_renderer_amd import backward as bw
    q = uw.bwd_problem("linear", family, dtype, **uw.SPEC_BWD_LINEAR)
    N = q["N"]
    wide = torch.full((2, 150, N + 16), float("nan"), dtype=dtype)
    wide[..., 8:8 + N] = q["dy"].to(dtype)
    dy = wide.to(dev)[..., 8:8 + N]
    x, w = q["x"].to(dtype).to(dev), q["w"].to(dtype).to(dev)
    monkeypatch.setattr(bw, "WGRAD", wgrad)
    for need_dw in (True, False):
        dx, dw, db = bw.linear_backward(x, w, dy, need_dw=need_dw)
        torch.cuda.synchronize()
        what = f"linear_backward {family} {dtype} need_dw {need_dw}"
        assert dx.shape == x.shape
        uw.check_exact(dx.double().cpu().reshape(-1, 200), q["dx"].reshape(-1, 200), what + " dx")
        uw.check_exact(db.double().cpu()[None], q["db"][None], what + " db")
        if need_dw:
            uw.check_exact(dw.double().cpu(), q["dw"], what + " dw")
        else:
            assert dw is None
