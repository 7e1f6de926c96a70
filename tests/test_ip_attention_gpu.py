"""``ur_ip_attention_add`` (the image half of IP-Adapter's decoupled cross-attention) per element against float64 on the same
rounded inputs, within the bound derived in util_ip_adapter.py, on guarded buffers; the q layouts the step hands it; exact
cases; error codes."""
import json

import pytest
import torch

import util_ip_adapter as IP

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16]
SENT = 1234.0  # exactly representable in fp16 and bf16


class Guarded:
    """A tensor of ``shape`` inside a flat device buffer with ``band`` elements of ``fill`` on both sides."""

    def __init__(self, value, dev, fill, band=512):
        flat = torch.full((value.numel() + 2 * band,), fill, dtype=value.dtype)
        flat[band:band + value.numel()] = value.reshape(-1)
        self.flat, self.band, self.n, self.fill = flat.to(dev), band, value.numel(), fill
        self.t = self.flat[band:band + self.n].view(value.shape)

    def intact(self):
        lo, hi = self.flat[: self.band].cpu(), self.flat[self.band + self.n:].cpu()
        if self.fill != self.fill:
            return bool(torch.isnan(lo).all() and torch.isnan(hi).all())
        return bool((lo == self.fill).all() and (hi == self.fill).all())


def _data(B, T, H, d, N, dtype, seed=0):
    g = torch.Generator().manual_seed(1000 * T + 10 * d + N + seed)
    C = H * d
    rnd = lambda *s: torch.randn(*s, generator=g).to(dtype)
    return rnd(B, T, C), rnd(B, T, C), rnd(B, N, C), rnd(B, N, C)  # o, q (log2 units), k_ip, v_ip


def _launch(dev, o, q, k, v, scale, H, *, q_layout="token", rows=None, flags=0, kv_wide=False):
    """Runs the kernel on guarded copies; returns (result on the CPU, guards all intact)."""
    from uni_renderer_amd import ops

    B, T, C = o.shape
    d, N = C // H, k.shape[1]
    nan = float("nan")
    og = Guarded(o, dev, SENT)
    kw = dict(B=B, H=H, T=T, d=d)
    if q_layout == "token":
        qg = Guarded(q, dev, nan)
        kw.update(ldq=C)
    elif q_layout == "wide":  # [B, T, ldq] with the heads at q_off; every other column NaN
        ldq, q_off = 2 * C + 24, C + 16
        wide = torch.full((B, T, ldq), nan, dtype=q.dtype)
        wide[:, :, q_off:q_off + C] = q
        qg = Guarded(wide, dev, nan)
        kw.update(ldq=ldq, q_off=q_off)
    else:  # head-major image [B, H, T, d]
        qg = Guarded(q.view(B, T, H, d).permute(0, 2, 1, 3).contiguous().view(B, T, C), dev, nan)
        kw.update(ldq=C, q_hstride=T * d)
    if kv_wide:  # column slices of one [B, N, 2 C + 16] projection, NaN between and around them
        both = torch.full((B, N, 2 * C + 16), nan, dtype=k.dtype)
        both[:, :, 8:8 + C], both[:, :, 16 + C:] = k, v
        kg = vg = Guarded(both, dev, nan)
        kt, vt = kg.t[:, :, 8:8 + C], kg.t[:, :, 16 + C:]
    else:
        kg, vg = Guarded(k, dev, nan), Guarded(v, dev, nan)
        kt, vt = kg.t, vg.t
    if rows is not None:
        kt, vt = kt[rows[0]:rows[1]], vt[rows[0]:rows[1]]
    before = [x.flat.clone() for x in (qg, kg, vg)]
    out = ops.ip_attention_add(og.t, qg.t, kt, vt, scale, rows=rows, flags=flags, **kw)
    assert out is og.t
    torch.cuda.synchronize()
    same = all(torch.equal(a.view(torch.int16), x.flat.view(torch.int16)) for a, x in zip(before, (qg, kg, vg)))  # inputs untouched
    return og.t.cpu().clone(), (og.intact() and qg.intact() and kg.intact() and vg.intact() and same)


def _check(got, o, q, k, v, scale, H, dtype, tag):
    ref = IP.ip_reference(o, q, k, v, scale, H)
    err = (got.double() - ref).abs()
    ratio = float((err / IP.ip_bound(o, q, k, v, scale, H, dtype)).max())
    moved = float((ref - o.double()).abs().max())
    print(json.dumps(dict(tag=tag, max_err=float(err.max()), worst_err_over_bound=round(ratio, 4), max_change=round(moved, 3))))
    assert ratio <= 1.0, (tag, ratio)  # every element
    assert moved > 0.05  # the comparison sees the added term


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
def test_kernel_per_element_against_float64(dev, dtype):
    """N(0, 1) data, B = 2, H = 8, the sweep T in {64, 35} x d in {40, 80, 160} x N in {1, 4, 16} (one case per dtype: the
    eighteen launches are milliseconds): every element within the derived bound; guard bands intact; a second launch and the
    thread-per-(token, head) kernel give the same bits."""
    scale = 0.7
    for T in (64, 35):
        for d in (40, 80, 160):
            for N in (1, 4, 16):
                tag = f"{dtype}/T{T}/d{d}/N{N}"
                o, q, k, v = _data(2, T, 8, d, N, dtype)
                got, ok = _launch(dev, o, q, k, v, scale, 8)
                assert ok, tag
                _check(got, o, q, k, v, scale, 8, dtype, tag)
                again, ok2 = _launch(dev, o, q, k, v, scale, 8)
                assert ok2 and torch.equal(again.view(torch.int16), got.view(torch.int16)), tag
                alt, ok3 = _launch(dev, o, q, k, v, scale, 8, flags=1)
                assert ok3 and torch.equal(alt.view(torch.int16), got.view(torch.int16)), tag


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
def test_kernel_walks_several_groups_per_workgroup(dev, dtype):
    """A workgroup that walks 2 or 5 groups of (token, head) pairs with the next group's loads in flight (what the launcher
    chooses from 4096 groups per launch on; forced here through the flags) -- 34 groups of 48 pairs, 50 groups of 12, so the last
    workgroup of a sample stops early.  Same bound, every element; the same bits as the one-group launch, for both kernels."""
    from uni_renderer_amd import ops

    for T, d in ((203, 40), (75, 160)):
        o, q, k, v = _data(2, T, 8, d, 4, dtype, seed=4)
        got, ok = _launch(dev, o, q, k, v, 0.7, 8, flags=1 << ops.IPA_WALK_SHIFT)
        assert ok
        _check(got, o, q, k, v, 0.7, 8, dtype, f"walk/{dtype}/T{T}/d{d}")
        for walk in (2, 5):
            for per_head in (0, 1):
                alt, ok2 = _launch(dev, o, q, k, v, 0.7, 8, flags=per_head | (walk << ops.IPA_WALK_SHIFT))
                assert ok2 and torch.equal(alt.view(torch.int16), got.view(torch.int16)), (T, d, walk, per_head)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
def test_kernel_other_head_counts_and_widths(dev, dtype):
    """The power-of-two head widths (butterfly alone: the small test networks) and head counts other than 8."""
    for H, d in ((2, 32), (2, 64), (4, 128), (3, 40)):
        for T, N in ((35, 4), (64, 5)):
            o, q, k, v = _data(2, T, H, d, N, dtype, seed=3)
            got, ok = _launch(dev, o, q, k, v, -1.25, H)
            assert ok, (H, d, T, N)
            _check(got, o, q, k, v, -1.25, H, dtype, f"{dtype}/H{H}/d{d}/T{T}/N{N}")
            alt, _ = _launch(dev, o, q, k, v, -1.25, H, flags=1)
            assert torch.equal(alt.view(torch.int16), got.view(torch.int16)), (H, d, T, N)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
def test_kernel_q_layouts_equal_the_plain_launch(dev, dtype):
    """Token-major q with ldq > C and a q_off (NaN in every other column), and the chain path's head-major image: within the
    bound, and the same bits as the plain token-major launch.  Also k_ip / v_ip as column slices of one wider projection."""
    for layout, T, d in (("wide", 35, 80), ("wide", 64, 160), ("head_major", 64, 40), ("head_major", 96, 40)):
        o, q, k, v = _data(2, T, 8, d, 4, dtype, seed=1)
        base, ok = _launch(dev, o, q, k, v, 1.0, 8)
        got, ok2 = _launch(dev, o, q, k, v, 1.0, 8, q_layout=layout)
        assert ok and ok2, (layout, T, d)
        _check(got, o, q, k, v, 1.0, 8, dtype, f"{layout}/{dtype}/T{T}/d{d}")
        assert torch.equal(got.view(torch.int16), base.view(torch.int16)), (layout, T, d)
        wide_kv, ok3 = _launch(dev, o, q, k, v, 1.0, 8, q_layout=layout, kv_wide=True)
        assert ok3 and torch.equal(wide_kv.view(torch.int16), base.view(torch.int16)), (layout, T, d)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
def test_kernel_rows_leave_the_other_samples_alone(dev, dtype):
    """rows = (1, 2) of a two-sample launch: sample 0 bit-unchanged, sample 1 the full launch's bits."""
    o, q, k, v = _data(2, 35, 8, 80, 4, dtype, seed=2)
    full, _ = _launch(dev, o, q, k, v, 0.5, 8)
    part, ok = _launch(dev, o, q, k, v, 0.5, 8, rows=(1, 2))
    assert ok
    assert torch.equal(part[0].view(torch.int16), o[0].view(torch.int16))
    assert torch.equal(part[1].view(torch.int16), full[1].view(torch.int16))
    first, _ = _launch(dev, o, q, k, v, 0.5, 8, rows=(0, 1))
    assert torch.equal(first[1].view(torch.int16), o[1].view(torch.int16)) and torch.equal(first[0].view(torch.int16), full[0].view(torch.int16))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
def test_kernel_exact_on_identical_keys(dev, dtype):
    """Four identical keys: p = 1/4 exactly whatever q is; integer values that are multiples of 4 and a power-of-two scale make
    o + scale * mean(v) exact in every format involved: the result equals float64."""
    for d in (40, 80, 160):
        g = torch.Generator().manual_seed(d)
        B, T, H, N = 2, 35, 8, 4
        C = H * d
        o = torch.randint(-8, 9, (B, T, C), generator=g).to(dtype)
        q = torch.randn(B, T, C, generator=g).to(dtype)
        k = torch.randn(B, 1, C, generator=g).to(dtype).expand(B, N, C).contiguous()
        v = (4 * torch.randint(-6, 7, (B, N, C), generator=g)).to(dtype)
        for scale in (0.5, 2.0, -0.25):
            got, ok = _launch(dev, o, q, k, v, scale, H)
            ref = o.double() + scale * v.double().mean(1, keepdim=True)
            assert ok and torch.equal(got.double(), ref), (d, scale)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
def test_kernel_exact_on_a_dominant_key(dev, dtype):
    """One key per head whose score exceeds every other by more than 200 log2 units: the other weights are exp2(< -200) = 0 in
    fp32 and the result is o + scale * v_j exactly on integer data.  The dominant token differs per head and sample."""
    for d in (40, 80, 160):
        g = torch.Generator().manual_seed(d + 1)
        B, T, H, N = 2, 64, 8, 4
        C = H * d
        o = torch.randint(-8, 9, (B, T, C), generator=g).to(dtype)
        v = torch.randint(-16, 17, (B, N, C), generator=g).to(dtype)
        q = torch.zeros(B, T, C)
        q.view(B, T, H, d)[..., 0] = 16.0 * (1 + torch.randint(0, 2, (B, T, H), generator=g))  # 16 or 32: scores 256 / 512 vs 0
        jstar = torch.randint(0, N, (B, H), generator=g)
        k = torch.zeros(B, N, H, d)
        k[..., 0].scatter_(1, jstar[:, None, :], 16.0)
        k[..., 1:] = torch.randn(B, N, H, d - 1, generator=g)  # q is zero there
        got, ok = _launch(dev, o, q.to(dtype), k.view(B, N, C).to(dtype), v, 2.0, H)
        vh = v.double().view(B, N, H, d)
        pick = torch.gather(vh, 1, jstar[:, None, :, None].expand(B, 1, H, d)).reshape(B, 1, C)
        assert ok and torch.equal(got.double(), o.double() + 2.0 * pick)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
def test_kernel_scale_zero_leaves_o_alone(dev, dtype):
    """scale = 0 launched directly, through the wrapper and through the C entry point: o unchanged bit for bit (-0.0 included)."""
    from uni_renderer_amd import ops

    o, q, k, v = _data(2, 35, 8, 40, 4, dtype)
    o[0, 0, :8] = -0.0
    got, ok = _launch(dev, o, q, k, v, 0.0, 8)
    assert ok and torch.equal(got.view(torch.int16), o.view(torch.int16))
    od, qd, kd, vd = (t.to(dev) for t in (o, q, k, v))
    rc = ops._lib.load().ur_ip_attention_add(od.data_ptr(), qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), 0.0, 0.0, 2, 8, 35, 40, 4,
                                             320, 0, 0, 320, 0, ops.DT[dtype], None)
    torch.cuda.synchronize()
    assert rc == 0 and torch.equal(od.cpu().view(torch.int16), o.view(torch.int16))


def test_kernel_rejects_what_it_does_not_support(dev):
    from uni_renderer_amd import ops

    lib = ops._lib.load()
    z = lambda *s: torch.zeros(*s, dtype=torch.float16, device=dev)
    o, q, k, v = z(2, 16, 320), z(2, 16, 320), z(2, 4, 320), z(2, 4, 320)
    big = z(2, 17, 320)

    def rc(o=o, q=q, k=k, v=v, scale=1.0, qk=0.0, B=2, H=8, T=16, d=40, N=4, ldq=320, q_off=0, hs=0, ldkv=320, flags=0, dtype=0):
        p = lambda t: None if t is None else (t if isinstance(t, int) else t.data_ptr())
        return lib.ur_ip_attention_add(p(o), p(q), p(k), p(v), scale, qk, B, H, T, d, N, ldq, q_off, hs, ldkv, flags, dtype, None)

    BAD, UNS = ops.ABI.UR_E_BADARG, ops.ABI.UR_E_UNSUPPORTED
    assert rc() == 0
    assert rc(d=48, H=8, ldq=384, ldkv=384) == UNS and rc(d=24) == UNS          # head widths
    assert rc(H=16, d=160, ldq=2560, ldkv=2560) == UNS                          # H * d > 1280
    assert rc(k=big, v=big, N=17) == UNS                                       # more than 16 image tokens
    assert rc(qk=0.125) == UNS                                                 # scores not in log2 units
    assert rc(o=None) == BAD and rc(q=None) == BAD and rc(k=None) == BAD and rc(v=None) == BAD
    assert rc(B=0) == BAD and rc(T=0) == BAD and rc(N=0) == BAD and rc(H=0) == BAD
    assert rc(dtype=2) == BAD and rc(flags=2) == BAD and rc(scale=float("nan")) == BAD and rc(scale=float("inf")) == BAD
    assert rc(q=q.data_ptr() + 2) == BAD and rc(o=o.data_ptr() + 8) == BAD     # 16-byte alignment
    assert rc(ldq=324) == BAD and rc(q_off=4, ldq=328) == BAD and rc(ldkv=324) == BAD
    assert rc(ldq=312) == BAD and rc(q_off=8) == BAD and rc(ldkv=312) == BAD   # the heads do not fit the row
    assert rc(hs=8 * 40) == BAD and rc(hs=16 * 40 + 8) == BAD                  # head-major image outside its sample
    assert rc(hs=16 * 40) == 0
    torch.cuda.synchronize()
    with pytest.raises(ValueError, match="image tokens"):
        ops.ip_attention_add(o, q, big, big, 1.0, B=2, H=8, T=16, d=40, ldq=320)
    with pytest.raises(ValueError, match="rows"):
        ops.ip_attention_add(o, q, k, v, 1.0, B=2, H=8, T=16, d=40, ldq=320, rows=(1, 3))
    with pytest.raises(ValueError, match="contiguous"):
        ops.ip_attention_add(o[:, :, :160], q, k, v, 1.0, B=2, H=8, T=16, d=20, ldq=320)
    with pytest.raises(ValueError, match="k_ip / v_ip"):
        ops.ip_attention_add(o, q, k, v.float(), 1.0, B=2, H=8, T=16, d=40, ldq=320)
    with pytest.raises(ValueError, match="finite"):
        ops.ip_attention_add(o, q, k, v, float("nan"), B=2, H=8, T=16, d=40, ldq=320)
