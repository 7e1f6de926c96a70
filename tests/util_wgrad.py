"""ur_wgrad / ur_wgrad_group (csrc/wgrad.hip) and the rest of backward.conv3x3_backward / linear_backward per ELEMENT
against float64: problems, references with their bound terms, an fp32 emulation, checkers, guard / sentinel buffers and
launchers shared by test_wgrad_range_gpu.py (the kernels) and test_wgrad_bounds_cpu.py (the proof that the reference is
the operation, that the exact family is exact, that the bounds fit correct arithmetic with room and that the checkers
reject the errors they are for).  ``rnd``, ``im2col``, ``embed``, ``check_exact`` and ``check_elem`` are util_igemm's.

Reference (float64, on the STORED values)
    dw[n][k] = sum_p dy[p][n] xcol[p][k]        db[n] = sum_p dy[p][n]
  xcol = x for a linear layer; for a 3x3 conv util_igemm.im2col(x, stride, pad=...) reshaped to [P, 9 C], k = tap * C + c,
  the packed layout [N][(ky, kx, c)].  test_wgrad_bounds_cpu.py holds it against float64 autograd of F.linear / F.conv2d.

Exact family ("int")
  x integers in [-3, 3]; dy +-1 with density 1/8 (1/32 when P > 1000), zero elsewhere.  Every product and every partial
  sum, in ANY order and under any slicing of P, is an integer of magnitude <= 3 P < 2^24, exact in fp32; dw must be
  torch.equal to the reference in fp16 AND bf16 while max |dw| <= 256 (8 significant bits), db in fp32 always.
  ``make_problem`` asserts that on the float64 reference and fails loudly (no re-draw).  On these draws (printed by
  test_wgrad_bounds_cpu.py): linear max |dw| 54 at (P, N, K) = (300, 328, 200), 76 at (2085, 328, 200), 52 at
  (300, 1280, 64); conv <= 51 at P <= 512.
  The backward entry points (``make_bwd``) have two such families: "wgrad" (x integers, dy and w sparse +-1) and "dgrad"
  (dy integers in [-3, 3], w and x sparse +-1, density 1/32 above 4000 terms): dx sums 9 N terms (N for a linear layer),
  dw P terms, and all three of dx, dw, db must be exact; max |dx|, max |dw| <= 256 asserted (conv dx: 74 at N = 72, 102
  at N = 128; linear dx: 53 at N = 328).

Toleranced family ("gauss"): N(0, 1) dy and x rounded to the storage type
  u = 2^-11 (fp16) / 2^-8 (bf16); A[n][k] = sum_p |dy xcol|; ``splits`` the slice count of the launch.
      |dw - ref| <= u |ref| + (P + splits + 8) 2^-23 A + TINY               (``bounds(p, splits)["dw"]``)
      |db - ref| <= (P + splits) 2^-24 sum_p |dy|                           (``bounds(p, splits)["db"]``)
  util_igemm's convention: products of two fp16 / bf16 numbers are exact in fp32; a sum of P terms in any order has
  |error| <= (P - 1) 2^-24 sum |terms| to first order (Higham 4.2); the MFMA's internal alignment / rounding is not
  documented, so every term of dw is charged 2^-23 instead of 2^-24; the slab fold adds ``splits`` more additions.  db is
  a plain fp32 sum in some order (lane partial sums, stages, two shuffles, slabs).  u |ref| is the storage rounding (the
  second-order u times the fp32 part lies inside the factor 2 of the charge).  Also: per-row rel-L2 < TOL of
  test_wgrad_gpu.py (1.5e-3 / 1.2e-2).
  What is NOT derived is the factor 2 on the summation term.  test_wgrad_bounds_cpu.py therefore holds an fp32 emulation
  of a correct kernel (``emulate``: torch float32, 32-row stages forwards and backwards, 1 / 3 / 7 slices summed in slice
  order) to HALF of the fp32 part before the storage rounding and to the whole bound after it.
  Worst GPU figures (MI355X, tiles 1 - 6; slices 1 and 4 -- 3 for the conv, whose P = 96 has three stages; row rel-L2 /
  |err| / bound / share of the fp32 part used once u |ref| is taken off / db |err| / bound), as printed by test_toleranced:
      fp16  linear 300 x 328 x 200  2.5e-4 / 0.70 / 0.0003 / 0.0009     conv B 3, 4 x 8, C 192  2.2e-4 / 0.95 / 0.0016 / 0.0027
      bf16  linear 300 x 328 x 200  1.9e-3 / 0.95 / 0.0000 / 0.0004     conv B 3, 4 x 8, C 192  1.8e-3 / 0.99 / 0.0001 / 0.0010
  identical on every tile (the order of the sum over p does not depend on the tile).  The u |ref| term -- a rounding of
  nearly half an ulp just above a power of two -- is what the stored elements use; the CPU emulations use at most 0.011
  of the fp32 part and 0.003 of the db bound.

Guards
  dy is a column slice at element offset 8 of a NaN-filled buffer with lddy = N + 24 and 32 NaN rows (one stage) in front
  and behind; x of a linear layer likewise; an NHWC image gets whole NaN guard lines of W + 2 pixels in front and behind
  and, through the direct descriptor, ldx = C + 8.  A read of row P, of pixel -1 or of the column behind N / K turns the
  result into NaN instead of a plausible number, and stays inside the test's own allocation.  dw lies in a buffer of the
  bit pattern of -1234 with 8 guard rows on both sides and lddw = K + 8, db in an fp32 one with 8 guard elements on both
  sides, ``partial`` is ur_wgrad_partial_floats floats plus a sentinel tail; ``assert_untouched`` requires every element
  outside [N][K], [N] and the slab floats to hold the sentinel still, bit for bit (16- and 32-bit views).

Launchers
  ``launch_direct`` fills backward._WgradDesc itself (lddw > K, conv ldx > C, pad = 0, any ``splits``, every output
  guarded); ``launch_wrapper`` goes through backward.wgrad (the wrapper allocates dw / db / partial: guarded inputs
  only) and ``launch_group`` through backward.wgrad_group (guarded inputs, dw / db in guarded buffers of lddw = K).
"""
import ctypes as C

import torch
import torch.nn.functional as F

import util_igemm as ug
from util_igemm import TINY, U, check_elem, check_exact, embed, im2col, rnd  # noqa: F401  (re-exported for the tests)

DTYPES = ug.DTYPES
TOL = {torch.float16: 1.5e-3, torch.bfloat16: 1.2e-2}  # tests/test_wgrad_gpu.py, here per row
TILES = [1, 2, 3, 4, 5, 6]
STAGE = 32        # contraction rows per stage (csrc/wgrad.hip: WG_BKP)
GUARD_ROWS = 8    # sentinel rows / elements in front of and behind dw / db
TAIL = 4096       # sentinel floats behind ``partial``
SENTINEL = ug.SENTINEL
f64 = torch.float64

DEFAULTS = dict(kind="linear", family="int", dtype=torch.float16, seed=0,
                P=0, N=0, K=0,                                # linear
                B=0, Hin=0, Win=0, C=0, stride=1, pad=1)      # conv: N as above, K = 9 C, P = B Hout Wout


def _sparse(g, dens, *shape):
    sign = 2 * torch.randint(0, 2, shape, generator=g).to(f64) - 1
    return torch.where(torch.rand(*shape, generator=g) < dens, 1.0, 0.0).to(f64) * sign


def _ints(g, *shape):
    return torch.randint(-3, 4, shape, generator=g).to(f64)


def xcol_of(p, x=None):
    x = p["x"] if x is None else x
    if p["conv"] is None:
        return x
    return im2col(x, p["stride"], pad=p["pad"]).reshape(p["P"], p["K"])


def make_problem(spec):
    """-> dict: the spec's entries plus dy [P, N], x ([P, K] or NHWC [B, Hin, Win, C]) -- stored values as float64 --,
    xcol [P, K], dw [N, K], db [N] (float64 references), A = |dy|^T |xcol|, Ady = sum_p |dy|, P, K,
    conv = (B, Hin, Win, Hout, Wout) or None."""
    p = dict(DEFAULTS)
    unknown = set(spec) - set(p)
    assert not unknown, unknown
    p.update(spec)
    dt, N = p["dtype"], p["N"]
    if p["kind"] == "conv":
        Ho, Wo = ug.out_hw(p["Hin"], p["Win"], p["stride"], False, p["pad"])
        p.update(P=p["B"] * Ho * Wo, K=9 * p["C"], conv=(p["B"], p["Hin"], p["Win"], Ho, Wo))
        xshape = (p["B"], p["Hin"], p["Win"], p["C"])
    else:
        assert p["kind"] == "linear", p["kind"]
        p["conv"] = None
        xshape = (p["P"], p["K"])
    P, K = p["P"], p["K"]
    g = torch.Generator().manual_seed(1000003 * p["seed"] + 7 * P + 13 * N + K)
    if p["family"] == "int":
        x = _ints(g, *xshape)
        dy = _sparse(g, 1 / 32 if P > 1000 else 1 / 8, P, N)
    else:
        assert p["family"] == "gauss", p["family"]
        x = rnd(torch.randn(*xshape, generator=g, dtype=f64), dt)
        dy = rnd(torch.randn(P, N, generator=g, dtype=f64), dt)
    p.update(x=x, dy=dy)
    xc = xcol_of(p)
    p.update(xcol=xc, dw=dy.T @ xc, db=dy.sum(0), A=dy.abs().T @ xc.abs(), Ady=dy.abs().sum(0))
    if p["family"] == "int":
        assert_exact_family(p["dw"], p["A"], dt, str(spec))
    return p


def assert_exact_family(dw, A, dtype, what):
    """The exactness condition: sums of |products| below 2^24 (fp32-exact under any order) and max |dw| <= 256."""
    assert float(A.max()) < 2.0 ** 24, f"exact family: sum |terms| reaches {float(A.max())} >= 2^24 ({what})"
    worst = float(dw.abs().max())
    assert worst <= 256.0, f"exact family: max |dw| = {worst} > 256 ({what}): not exact in bf16"
    assert torch.equal(rnd(dw, dtype), dw), f"exact family: the reference is not representable in {dtype} ({what})"


def bounds(p, splits=1):
    """-> dict(dw = bound on |dw - ref|, fp = its fp32 part, db = bound on |db - ref|)."""
    dt = p["dtype"]
    fp = (p["P"] + splits + 8) * 2.0 ** -23 * p["A"]
    return dict(dw=U[dt] * p["dw"].abs() + fp + TINY[dt], fp=fp, db=(p["P"] + splits) * 2.0 ** -24 * p["Ady"])


def fp_part_used(got, p, splits=1):
    """Largest share of the fp32 part of the dw bound an element needs once u |ref| is taken off."""
    dt = p["dtype"]
    e = (got - p["dw"]).abs() - U[dt] * p["dw"].abs() - TINY[dt]
    return float((e.clamp_min(0) / bounds(p, splits)["fp"].clamp_min(1e-300)).max())


def emulate(p, order="fwd", slices=1):
    """fp32 emulation of a correct kernel -> (dw32 [N, K] before the storage rounding, dw stored, db32), as float64.
    P is summed in 32-row stages (``order`` fwd | rev inside a slice), ``slices`` slices of ceil(stages / slices)
    stages each -- trailing ones may be empty, as in the kernel -- whose sums are added in slice order."""
    f32 = torch.float32
    dy, xc = p["dy"].to(f32), p["xcol"].to(f32)
    P, N, K = p["P"], p["N"], p["K"]
    steps = -(-P // STAGE)
    per = -(-steps // slices)
    acc, accb = torch.zeros(N, K, dtype=f32), torch.zeros(N, dtype=f32)
    for z in range(slices):
        st = list(range(z * per, min(steps, (z + 1) * per)))
        if order == "rev":
            st.reverse()
        part, partb = torch.zeros(N, K, dtype=f32), torch.zeros(N, dtype=f32)
        for s in st:
            r = slice(s * STAGE, min(P, (s + 1) * STAGE))
            part = part + dy[r].T @ xc[r]
            partb = partb + dy[r].sum(0)
        acc, accb = acc + part, accb + partb
    return acc.double(), acc.to(p["dtype"]).double(), accb.double()


def old_dw_err(got, ref):
    """test_wgrad_gpu._close's figure: max |got - ref| / max |ref| over the whole matrix (asserted <= TOL there)."""
    return float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-6))


def old_db_accepts(got, ref, Ady):
    """test_wgrad_gpu.py's db assertion: max |db - ref| <= 2e-4 max(1, max sum_p |dy|)."""
    return float((got - ref).abs().max()) <= 2e-4 * max(1.0, float(Ady.max()))


# ---------------------------------------------------------------------------------------------------------------
# guards
def sentinel(shape, dtype, dev):
    return torch.full(tuple(shape), SENTINEL, dtype=dtype, device=dev)


def _bits(t):
    return t.view({2: torch.int16, 4: torch.int32}[t.element_size()])


def assert_untouched(buf, written, what):
    """Every element of ``buf`` (fp16 / bf16 / fp32, any device) outside the boolean mask ``written`` still holds the
    sentinel, bit for bit."""
    b = buf.detach().cpu()
    sbits = int(_bits(sentinel((1,), b.dtype, "cpu"))[0])
    bad = (_bits(b) != sbits) & ~written
    if bad.any():
        idx = bad.nonzero()
        raise AssertionError(f"{what}: {int(bad.sum())} elements outside the region the descriptor names were overwritten; "
                             f"first (index): {[tuple(i.tolist()) for i in idx[:8]]}")


def region1d(n, lo, cnt):
    m = torch.zeros(n, dtype=torch.bool)
    m[lo:lo + cnt] = True
    return m


def dw_out(N, K, ld, dtype, dev):
    """-> (buffer [N + 2 GUARD_ROWS, ld], view of rows GUARD_ROWS .. + N, check(what) -> dw [N, K] float64 on the CPU)."""
    buf = sentinel((N + 2 * GUARD_ROWS, ld), dtype, dev)

    def check(what):
        assert_untouched(buf, ug.region2d(buf.shape, GUARD_ROWS, N, K), what + " dw")
        return buf.cpu()[GUARD_ROWS:GUARD_ROWS + N, :K].double()

    return buf, buf[GUARD_ROWS:GUARD_ROWS + N], check


def db_out(N, dev):
    buf = sentinel((N + 2 * GUARD_ROWS,), torch.float32, dev)

    def check(what):
        assert_untouched(buf, region1d(buf.numel(), GUARD_ROWS, N), what + " db")
        return buf.cpu()[GUARD_ROWS:GUARD_ROWS + N].double()

    return buf, buf[GUARD_ROWS:GUARD_ROWS + N], check


def partial_out(floats, dev):
    buf = sentinel((floats + TAIL,), torch.float32, dev)
    return buf, lambda what: assert_untouched(buf, region1d(buf.numel(), 0, floats), what + " partial")


def inputs(p, dev, ldx_pad=0):
    """(dy, x) of problem ``p`` on ``dev`` inside their NaN guards (built once per problem and layout; read-only).
    dy [P, N] with row stride N + 24; x [P, K] with row stride K + 24, or the NHWC image -- contiguous [B, Hin, Win, C]
    when ``ldx_pad`` is 0, else the [B Hin Win, C] pixel matrix with row stride C + ldx_pad."""
    key = ("inputs", str(dev), ldx_pad)
    if key not in p:
        dt = p["dtype"]
        dy = embed(p["dy"], p["N"] + 24, 8, STAGE, STAGE, dt, dev)
        if p["conv"] is None:
            x = embed(p["x"], p["K"] + 24, 8, STAGE, STAGE, dt, dev)
        else:
            B, Hin, Win, _, _ = p["conv"]
            x = embed(p["x"].reshape(B * Hin * Win, p["C"]), p["C"] + ldx_pad, 0, Win + 2, Win + 2, dt, dev)
            if not ldx_pad:
                x = x.view(B, Hin, Win, p["C"])
        p[key] = (dy, x)
    return p[key]


def describe(p, tile, splits):
    c = p["conv"]
    shape = f"conv B {c[0]} {c[1]}x{c[2]} -> {c[3]}x{c[4]} C {p['C']} stride {p['stride']} pad {p['pad']}" if c else "linear"
    return f"{shape} P {p['P']} N {p['N']} K {p['K']} {p['dtype']} tile {tile} slices {splits}"


def _fill_shape(d, p, ldx):
    d.taps, d.ldx = 1, ldx
    if p["conv"] is not None:
        B, Hin, Win, Ho, Wo = p["conv"]
        d.taps, d.C, d.B, d.Hin, d.Win, d.Hout, d.Wout, d.stride, d.pad = 9, p["C"], B, Hin, Win, Ho, Wo, p["stride"], p["pad"]


def launch_direct(p, dev, tile, splits=1, need_db=True, ldx_pad=0, lddw_pad=8):
    """ur_wgrad through a hand-filled descriptor, every operand guarded.  ``splits`` = 0: the library's choice
    (ur_wgrad_plan).  Asserts the guard regions and returns (dw [N, K], db [N] | None as float64, slices used)."""
    from uni_renderer_amd import _lib, backward as bw, ops
    lib = _lib.load()
    dt, P, N, K = p["dtype"], p["P"], p["N"], p["K"]
    dy, x = inputs(p, dev, ldx_pad)
    x2 = x.view(-1, x.shape[-1]) if (p["conv"] is not None and not ldx_pad) else x
    d = bw._WgradDesc()
    _fill_shape(d, p, x2.stride(0))
    _, dwv, check_dw = dw_out(N, K, K + lddw_pad, dt, dev)
    _, dbv, check_db = db_out(N, dev)
    zp = ops.zero_page(dev)
    d.dy, d.x, d.dw, d.db = dy.data_ptr(), x2.data_ptr(), dwv.data_ptr(), (dbv.data_ptr() if need_db else None)
    d.zero_page, d.zero_page_bytes = zp.data_ptr(), ops.ZERO_PAGE_BYTES
    d.lddy, d.lddw, d.P, d.N, d.K = dy.stride(0), K + lddw_pad, P, N, K
    d.tile, d.dtype, d.splits = tile, ops.DT[dt], max(splits, 1)
    if splits == 0:
        ns, nf = C.c_int32(0), C.c_int64(0)
        _lib.check(lib.ur_wgrad_plan(C.byref(d), C.byref(ns), C.byref(nf)), "ur_wgrad_plan")
        d.splits = ns.value
    check_part = None
    if d.splits > 1:
        part, check_part = partial_out(int(lib.ur_wgrad_partial_floats(C.byref(d))), dev)
        d.partial = part.data_ptr()
    _lib.check(lib.ur_wgrad(C.byref(d), ops._stream()), "ur_wgrad")
    torch.cuda.synchronize()
    what = describe(p, tile, d.splits) + f" ldx {x2.stride(0)} lddw {K + lddw_pad}"
    dw = check_dw(what)
    db = check_db(what)
    if check_part is not None:
        check_part(what)
    if not need_db:
        assert_untouched(dbv, torch.zeros(N, dtype=torch.bool), what + " db (absent)")
    return dw, (db if need_db else None), int(d.splits)


def launch_wrapper(p, dev, tile=0, splits=0, need_db=True):
    """backward.wgrad on the guarded inputs (pad 1 and ldx = C only: what the wrapper expresses) -> (dw, db) float64."""
    from uni_renderer_amd import backward as bw
    assert p["pad"] == 1
    dy, x = inputs(p, dev)
    conv = (p["conv"][3], p["conv"][4], p["stride"]) if p["conv"] is not None else None
    dw, db = bw.wgrad(dy, x, need_db, conv=conv, tile=tile, splits=splits)
    torch.cuda.synchronize()
    assert dw.shape == (p["N"], p["K"]) and (db is None) == (not need_db)
    return dw.double().cpu(), (db.double().cpu() if need_db else None)


def launch_group(probs, dev, tile=0, splits=0, no_db=()):
    """backward.wgrad_group over equally shaped problems, each with its own guarded buffers (``no_db``: indices of the
    problems without a bias gradient) -> [(dw, db | None)] float64; asserts the guards."""
    from uni_renderer_amd import backward as bw
    p0 = probs[0]
    conv = (p0["conv"][3], p0["conv"][4], p0["stride"]) if p0["conv"] is not None else None
    items, checks = [], []
    for i, p in enumerate(probs):
        assert (p["P"], p["N"], p["K"], p["conv"], p["dtype"]) == (p0["P"], p0["N"], p0["K"], p0["conv"], p0["dtype"])
        dy, x = inputs(p, dev)
        _, dwv, check_dw = dw_out(p["N"], p["K"], p["K"], p["dtype"], dev)
        dbbuf, dbv, check_db = db_out(p["N"], dev)
        items.append((dy, x, dwv, None if i in no_db else dbv))
        checks.append((check_dw, check_db, dbbuf))
    bw.wgrad_group(items, tile=tile, splits=splits, conv=conv)
    torch.cuda.synchronize()
    out = []
    for i, (check_dw, check_db, dbbuf) in enumerate(checks):
        what = f"group of {len(probs)} problem {i}: " + describe(probs[i], tile, splits)
        dw = check_dw(what)
        if i in no_db:
            assert_untouched(dbbuf, torch.zeros(dbbuf.numel(), dtype=torch.bool), what + " db (absent)")
            out.append((dw, None))
        else:
            out.append((dw, check_db(what)))
    return out


# ---------------------------------------------------------------------------------------------------------------
# the problems of test_wgrad_range_gpu.py (built once per dtype and shared; test_wgrad_bounds_cpu.py builds every "int"
# one to show that the exactness condition holds)
_cache = {}


def problem(**spec):
    key = tuple(sorted(spec.items()))
    if key not in _cache:
        _cache[key] = make_problem(spec)
    return _cache[key]


LINEAR = [(300, 328, 200), (5, 328, 200), (33, 64, 2560), (2085, 328, 200)]  # 10 stages (last: 12 rows) | < 1 | 2 | 66
SLICES_300 = (2, 3, 4, 7, 10)   # 7: per = 2, slices 5 and 6 empty
SLICES_2085 = (0, 64)           # the library's choice; 64: per = 2, 33 slices of work, 31 empty


def spec_linear(dtype, P, N, K, **kw):
    return dict(kind="linear", dtype=dtype, P=P, N=N, K=K, **kw)


def specs_conv(dtype):
    """(name, spec, ldx_pad != 0: only with pixels of C + ldx_pad elements).  N = 328 throughout."""
    c = dict(kind="conv", dtype=dtype, N=328)
    out = []
    for s in (1, 2):
        out += [(f"B5_2x4_C64_s{s}", dict(c, B=5, Hin=2 * s, Win=4 * s, C=64, stride=s), 0),
                (f"B3_4x8_C192_s{s}", dict(c, B=3, Hin=4 * s, Win=8 * s, C=192, stride=s), 0),
                (f"B2_16x8_C64_s{s}", dict(c, B=2, Hin=16 * s, Win=8 * s, C=64, stride=s), 0)]
    out += [("s2_odd_7x15", dict(c, B=3, Hin=7, Win=15, C=64, stride=2), 0),
            ("s2_pad0_8x8", dict(c, B=3, Hin=8, Win=8, C=64, stride=2, pad=0), 0),
            ("ldx_C+8", dict(c, B=3, Hin=4, Win=8, C=64, stride=1, seed=1), 8)]
    return out


def specs_group(dtype):
    """(name, [specs], slices, indices without db)."""
    from uni_renderer_amd import backward as bw
    return [("3_linear", [spec_linear(dtype, 300, 328, 200, seed=10 + i) for i in range(3)], 3, (1,)),
            ("max_linear", [spec_linear(dtype, 40, 64, 64, seed=20 + i) for i in range(bw.WGRAD_GROUP_MAX)], 1, ()),
            ("4_conv", [dict(kind="conv", dtype=dtype, N=328, B=3, Hin=8, Win=16, C=64, stride=2, seed=90 + i) for i in range(4)], 2, ())]


def specs_toleranced(dtype):
    return [("linear 300 x 328 x 200", spec_linear(dtype, 300, 328, 200, family="gauss")),
            ("conv B 3, 4 x 8, C 192", dict(kind="conv", family="gauss", dtype=dtype, N=328, B=3, Hin=4, Win=8, C=192))]


# ---------------------------------------------------------------------------------------------------------------
# backward.conv3x3_backward / linear_backward: exact problems whose reference is float64 autograd on the CPU
def make_bwd(kind, family, dtype, seed=0, **s):
    """kind "conv": B, H, W, C, N, stride -> x [B, H, W, C], w4 OIHW [N, C, 3, 3], w = its packed form [N][(ky, kx, c)],
    dy [B, Ho, Wo, N]; kind "linear": lead (tuple), K, N -> x [*lead, K], w [N, K], dy [*lead, N].  Stored values and the
    references dx, dw, db as float64.  family "wgrad": x integers, dy and w sparse +-1; "dgrad": dy integers, w and x sparse
    +-1 (density 1/8; 1/32 above 4000 terms)."""
    p = dict(kind=kind, family=family, dtype=dtype, **s)
    N = s["N"]
    g = torch.Generator().manual_seed(7000003 * seed + 31 * N + sum(v for v in s.values() if isinstance(v, int)))
    if kind == "conv":
        B, H, W, Cc, stride = s["B"], s["H"], s["W"], s["C"], s["stride"]
        Ho, Wo = ug.out_hw(H, W, stride)
        xshape, wshape, dyshape, terms_dx, terms_dw = (B, H, W, Cc), (N, Cc, 3, 3), (B, Ho, Wo, N), 9 * N, B * Ho * Wo
    else:
        lead, K = tuple(s["lead"]), s["K"]
        rows = 1
        for v in lead:
            rows *= v
        xshape, wshape, dyshape, terms_dx, terms_dw = lead + (K,), (N, K), lead + (N,), N, rows
    dens = lambda terms: 1 / 32 if terms > 4000 else 1 / 8
    w = _sparse(g, dens(terms_dx), *wshape)
    if family == "wgrad":
        x, dy = _ints(g, *xshape), _sparse(g, 1 / 32 if terms_dw > 1000 else 1 / 8, *dyshape)
    else:
        assert family == "dgrad", family
        x, dy = _sparse(g, dens(terms_dw), *xshape), _ints(g, *dyshape)
    xr, wr = x.clone().requires_grad_(), w.clone().requires_grad_()
    br = torch.zeros(N, dtype=f64, requires_grad=True)
    if kind == "conv":
        y = F.conv2d(xr.permute(0, 3, 1, 2), wr, br, stride=stride, padding=1)
        y.backward(dy.permute(0, 3, 1, 2))
        dw = wr.grad.permute(0, 2, 3, 1).reshape(N, 9 * Cc).contiguous()
        p["w4"], wp = w, w.permute(0, 2, 3, 1).reshape(N, 9 * Cc).contiguous()
    else:
        F.linear(xr, wr, br).backward(dy)
        dw, wp = wr.grad, w
    p.update(x=x, w=wp, dy=dy, dx=xr.grad, dw=dw, db=br.grad)
    for name in ("dx", "dw"):
        worst = float(p[name].abs().max())
        assert worst <= 256.0, f"exact family: max |{name}| = {worst} > 256 ({kind} {family} {s})"
        assert torch.equal(rnd(p[name], dtype), p[name])
    assert float(dy.abs().sum()) < 2.0 ** 24
    return p


_bwd_cache = {}


def bwd_problem(kind, family, dtype, **s):
    key = (kind, family, dtype, tuple(sorted((k, v) for k, v in s.items())))
    if key not in _bwd_cache:
        _bwd_cache[key] = make_bwd(kind, family, dtype, **s)
    return _bwd_cache[key]


def specs_bwd_dx():
    """conv3x3_backward, "dgrad" family: (name, shape)."""
    return [("s1_9x11_N72", dict(B=3, H=9, W=11, C=64, N=72, stride=1)),
            ("s2_8x12_N72", dict(B=3, H=8, W=12, C=64, N=72, stride=2)),
            ("s1_9x11_N28", dict(B=3, H=9, W=11, C=64, N=28, stride=1)),
            ("s1_9x11_N128", dict(B=3, H=9, W=11, C=64, N=128, stride=1))]   # N % 64 == 0: the one weight_rot serves


def specs_bwd_dw():
    """conv3x3_backward, "wgrad" family, maps whose sides are no powers of two: the im2col + transposes fallback."""
    return [("s1_6x12", dict(B=3, H=6, W=12, C=64, N=72, stride=1)),
            ("s2_12x6", dict(B=3, H=12, W=6, C=64, N=72, stride=2))]


SPEC_BWD_FORCED = dict(B=3, H=4, W=8, C=64, N=72, stride=1)        # ur_wgrad takes it; WGRAD off: the fallback
SPEC_BWD_LINEAR = dict(lead=(2, 150), K=200, N=328)


def int_problems(dtype):
    """Builds every exact-family problem of the GPU file (each asserts its exactness condition); -> their number."""
    n = 0
    for P, N, K in LINEAR:
        n += problem(**spec_linear(dtype, P, N, K)) is not None
    for _, s, _ in specs_conv(dtype):
        n += problem(**s) is not None
    for _, specs, _, _ in specs_group(dtype):
        for s in specs:
            n += problem(**s) is not None
    for fam, specs in (("dgrad", specs_bwd_dx()), ("wgrad", specs_bwd_dw() + [("forced", SPEC_BWD_FORCED)])):
        for _, s in specs:
            n += bwd_problem("conv", fam, dtype, **s) is not None
    for fam in ("dgrad", "wgrad"):
        n += bwd_problem("linear", fam, dtype, **SPEC_BWD_LINEAR) is not None
    return n
