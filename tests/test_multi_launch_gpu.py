"""The five multi-tensor launchers that share one segment table (csrc/ur_launch.h): ur_transpose2d_multi, ur_colsum_multi,
ur_adamw_multi, ur_cast_multi(_sumsq) and ur_add_hilo_multi.

Oracle: many items in one launch == the same items, same tensors, same addresses, one item per launch, bit for bit (plus the
single-tensor entry points where there is one).  Every output is a view of ONE flat buffer with a canary-filled gap between
neighbours, so a workgroup that looks up the wrong item or the wrong block of its item lands in a neighbour or in a gap and
fails the test.  Item counts 1, 2, 3, MAX - 1, MAX and MAX + 1 (two launches) of each launcher's own MAX; item sizes cycle
through {one unit minus the smallest legal step, three units, exactly one unit, one unit plus the smallest legal step}, which
puts a one-block item on both sides of every multi-block one."""
import pytest
import torch

pytestmark = pytest.mark.gpu

GAP = 64          # elements: the alignment of every view and the least canary gap between two of them
CANARY = -1000.0  # exact in fp32, fp16 and bf16 (0xA5 in the one-byte low parts of an fp16 stream)
HALVES = [torch.float16, torch.bfloat16]


def _counts(nmax):
    return [1, 2, 3, nmax - 1, nmax, nmax + 1]


class Flat:
    """One flat buffer holding a view of each of ``sizes`` elements, GAP-aligned, with >= GAP canary elements around each."""

    def __init__(self, sizes, dtype, dev):
        offs, off = [], GAP
        for n in sizes:
            offs.append(off)
            off += (n + GAP - 1) // GAP * GAP + GAP
        self.buf = torch.empty(off, dtype=dtype, device=dev)
        self.guard = torch.ones(off, dtype=torch.bool, device=dev)
        for o, n in zip(offs, sizes):
            self.guard[o:o + n] = False
        self.views = [self.buf[o:o + n] for o, n in zip(offs, sizes)]
        self.canary = 0xA5 if dtype == torch.uint8 else CANARY
        self.reset()

    def reset(self):
        self.buf.fill_(self.canary)

    def guards_intact(self) -> bool:
        return bool((self.buf[self.guard] == self.canary).all())


def _multi_equals_single(run, *flats):
    """``run(single)`` writes every output into ``flats``: once MAX items per launch, once one item per launch.  Both leave the
    same bits everywhere and the canaries alone."""
    run(False)
    torch.cuda.synchronize()
    many = [f.buf.clone() for f in flats]
    for f in flats:
        assert f.guards_intact()
        f.reset()
    run(True)
    torch.cuda.synchronize()
    for f, m in zip(flats, many):
        assert f.guards_intact()
        assert torch.equal(m, f.buf)


def _rand(g, dev, dtype, *shape):
    return torch.randn(*shape, generator=g).to(dtype).to(dev)


# ---- ur_transpose2d_multi: unit = one 64 x 64 tile; (R, C, batch), C a multiple of 8 ----
_TR_SHAPES = [(63, 56, 1), (192, 64, 1), (64, 64, 1), (65, 72, 1), (63, 56, 1), (64, 64, 3), (64, 64, 1), (65, 72, 1)]


@pytest.mark.parametrize("dtype", HALVES)
@pytest.mark.parametrize("n", _counts(32))
def test_transposes_of_one_launch_equal_one_launch_each(dev, dtype, n):
    from uni_renderer_amd import _lib, backward as bw

    assert bw.TRANSPOSE_MAX == 32
    g = torch.Generator().manual_seed(100 + n)
    shapes = [_TR_SHAPES[i % len(_TR_SHAPES)] for i in range(n)]
    xs = [_rand(g, dev, dtype, b, R, C) for R, C, b in shapes]
    flat = Flat([b * C * ((R + 7) // 8 * 8) for R, C, b in shapes], dtype, dev)

    def fill(d, x, i):
        R, C, b = shapes[i]
        Rp = (R + 7) // 8 * 8
        d.src, d.dst = x.data_ptr(), flat.views[i].data_ptr()
        d.ld_src, d.bs_src, d.ld_dst, d.bs_dst = C, R * C, Rp, C * Rp
        d.R, d.C, d.batch, d.rows_out = R, C, b, 0

    _multi_equals_single(lambda single: _lib.launch_chunked(
        "ur_transpose2d_multi", bw._TransposeDesc, xs, 1 if single else bw.TRANSPOSE_MAX, fill, bw.DT[dtype], None), flat)
    for x, v, (R, C, b) in zip(xs, flat.views, shapes):
        o = v.view(b, C, -1)
        assert torch.equal(o[..., :R], x.transpose(-1, -2)) and not o[..., R:].any()
        assert torch.equal(o, bw.transpose2d(x))  # the single-tensor entry point


# ---- ur_colsum_multi: unit = 32 columns; fp32 [M, N] -> [N], or the planar (channel, component) pair form ----
_CS_COLS = [31, 96, 32, 33]


@pytest.mark.parametrize("n", _counts(96))
def test_column_sums_of_one_launch_equal_one_launch_each(dev, n):
    from uni_renderer_amd import _lib, backward as bw

    assert bw.COLSUM_MULTI_MAX == 96
    g = torch.Generator().manual_seed(200 + n)
    items = []
    for i in range(n):
        N, M = _CS_COLS[i % 4], (5 + 7 * i) % 40 + 1
        items.append((_rand(g, dev, torch.float32, M, N), N % 2 == 0 and i % 3 == 1))
    flat = Flat([p.shape[1] for p, _ in items], torch.float32, dev)

    def fill(d, item, i):
        part, pair = item
        d.inp, d.out, d.M, d.N, d.pair = part.data_ptr(), flat.views[i].data_ptr(), part.shape[0], part.shape[1], int(pair)

    _multi_equals_single(lambda single: _lib.launch_chunked(
        "ur_colsum_multi", bw._ColsumItem, items, 1 if single else bw.COLSUM_MULTI_MAX, fill, None), flat)
    assert any(pair for _, pair in items) or n < 2
    for (part, pair), out in zip(items, flat.views):
        planar = (lambda t: t.view(-1, 2).t().reshape(-1)) if pair else (lambda t: t)
        # against float64 and the single-tensor entry point (another summation order; it takes multiples of 8 columns): each
        # fp32 sum of M terms is within M * 2^-24 * sum|x| of the exact one (first-order bound of recursive summation in any
        # order), so two of them are within twice that of each other
        bound = planar(part.abs().double().sum(0) * part.shape[0] * 2.0 ** -24)
        assert bool(((out.double() - planar(part.double().sum(0))).abs() <= bound).all())
        if part.shape[1] % 8 == 0:
            assert bool(((out.double() - planar(bw.colsum(part)).double()).abs() <= 2 * bound).all())


# ---- ur_add_hilo_multi: unit = 1024 eight-element vectors = 8192 elements; sizes are multiples of 8 ----
_ADD_SIZES = [8192 - 8, 3 * 8192, 8192, 8192 + 8]


@pytest.mark.parametrize("dtype", HALVES)
@pytest.mark.parametrize("n", _counts(16))
def test_hilo_adds_of_one_launch_equal_one_launch_each(dev, dtype, n):
    from uni_renderer_amd import _lib, ops

    assert ops.ADD_MULTI_MAX == 16
    g = torch.Generator().manual_seed(300 + n)
    pairs = []
    for i in range(n):
        ab = []
        for k in range(2):
            v = torch.randn(_ADD_SIZES[i % 4], generator=g).to(dev)
            hi = v.to(dtype)
            if (i + k) % 3 != 2:  # operands with and without a low part
                hi.lo = ops.lo_encode(v - hi.float(), dtype)
            ab.append(hi)
        pairs.append(tuple(ab))
    flat = Flat([a.numel() for a, _ in pairs], dtype, dev)
    flat_lo = Flat([a.numel() for a, _ in pairs], ops.lo_dtype(dtype), dev)

    def fill(d, pair, i):
        a, b = pair
        d.a, d.a_lo, d.b, d.b_lo = a.data_ptr(), ops._ptr(ops.lo_of(a)), b.data_ptr(), ops._ptr(ops.lo_of(b))
        d.out, d.out_lo, d.n = flat.views[i].data_ptr(), flat_lo.views[i].data_ptr(), a.numel()

    _multi_equals_single(lambda single: _lib.launch_chunked(
        "ur_add_hilo_multi", ops._AddItem, pairs, 1 if single else ops.ADD_MULTI_MAX, fill, ops.DT[dtype], None), flat, flat_lo)
    for (a, b), o, o_lo in zip(pairs, flat.views, flat_lo.views):
        r = ops.add(a, b, hilo=True)  # the single-tensor entry point (ur_add_hilo)
        assert torch.equal(o, r) and torch.equal(o_lo, r.lo)


# ---- ur_cast_multi / ur_cast_multi_sumsq: unit = 8192 elements ----
_CAST_SIZES = [8191, 3 * 8192, 8192, 8193]


@pytest.mark.parametrize("half", HALVES)
@pytest.mark.parametrize("to_f32,sumsq", [(False, False), (True, False), (True, True)])
@pytest.mark.parametrize("n", _counts(128))
def test_casts_of_one_launch_equal_one_launch_each(dev, half, to_f32, sumsq, n):
    from uni_renderer_amd import backward as bw

    assert bw.CAST_MAX_TENSORS == 128
    g = torch.Generator().manual_seed(400 + n)
    src_dt, dst_dt = (half, torch.float32) if to_f32 else (torch.float32, half)
    srcs = [_rand(g, dev, src_dt, _CAST_SIZES[i % 4]) for i in range(n)]
    flat = Flat([s.numel() for s in srcs], dst_dt, dev)
    parts = []

    def run(single):
        if not sumsq:
            for group in ([[i] for i in range(n)] if single else [range(n)]):
                bw.cast_many([srcs[i] for i in group], dst_dt, outs=[flat.views[i] for i in group])
        elif single:
            parts.append(torch.cat([bw.cast_many([s], dst_dt, sumsq=True, outs=[v])[1] for s, v in zip(srcs, flat.views)]))
        else:
            parts.append(bw.cast_many(srcs, dst_dt, sumsq=True, outs=flat.views)[1])

    _multi_equals_single(run, flat)
    for s, v in zip(srcs, flat.views):
        assert torch.equal(v, s.to(dst_dt))
    if sumsq:  # one partial per workgroup, in item order: the one-per-launch partials concatenated
        assert parts[0].numel() == sum((s.numel() + 8191) // 8192 for s in srcs) and torch.equal(parts[0], parts[1])


# ---- ur_adamw_multi (optim.FusedAdamW): unit = 16384 elements ----
_ADAMW_SIZES = [16383, 3 * 16384, 16384, 16385]


@pytest.mark.parametrize("n", _counts(64))
def test_adamw_over_one_launch_equals_one_launch_per_tensor(dev, n, monkeypatch):
    """Two optimizers over identical clones (parameters, gradients and both moments of each are views of flat buffers of one
    layout, canaries between them), two steps: one built normally, one stepping one tensor per launch."""
    from uni_renderer_amd import optim

    assert optim.MAX_TENSORS == 64
    g = torch.Generator().manual_seed(500 + n)
    sizes = [_ADAMW_SIZES[i % 4] for i in range(n)]
    p0 = [torch.randn(s, generator=g) for s in sizes]
    grads = [[torch.randn(s, generator=g) for s in sizes] for _ in range(2)]

    def two_steps(per_launch):
        monkeypatch.setattr(optim, "MAX_TENSORS", per_launch)
        flats = {k: Flat(sizes, torch.float32, dev) for k in "pgmv"}
        params = []
        for i, v in enumerate(flats["p"].views):
            v.copy_(p0[i])
            flats["m"].views[i].zero_()
            flats["v"].views[i].zero_()
            params.append(v.requires_grad_())
        opt = optim.FusedAdamW(params, lr=1e-2, weight_decay=1e-2)
        step = torch.zeros((), dtype=torch.float32, device=dev)
        for i, p in enumerate(params):
            opt.state[p] = {"step": step, "exp_avg": flats["m"].views[i], "exp_avg_sq": flats["v"].views[i]}
        for it in range(2):
            for i, p in enumerate(params):
                flats["g"].views[i].copy_(grads[it][i])
                p.grad = flats["g"].views[i]
            opt.step()
        torch.cuda.synchronize()
        assert len(opt.param_groups[0]["_ur_launches"][2]) == -(-n // per_launch) and float(step) == 2.0
        assert all(flats[k].guards_intact() for k in "pgmv")
        return [flats[k].buf.detach().clone() for k in "pmv"]

    many, single = two_steps(64), two_steps(1)
    assert all(torch.equal(a, b) for a, b in zip(many, single))
