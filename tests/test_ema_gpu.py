"""GPU tests of the EMA kernels (csrc/ema.hip) per element: ur_ema_advance against the float64 restatement of the schedule,
ur_ema_multi against the float64 definition (exactly on integer data, within the three roundings' bound otherwise) and bit for
bit against the three-rounding fp32 emulation of tests/util_ema.py, on guarded buffers at aligned and odd offsets."""
import ctypes

import numpy as np
import pytest
import torch

import util_ema as E

pytestmark = pytest.mark.gpu

CANARY, PAD = -6.02e23, 64
COPY = 0x100
DTYPES = [torch.float32, torch.float16, torch.bfloat16]


class Guarded:
    """n elements with PAD canaries on both sides (PAD elements keep the 16-byte alignment of the allocation for every dtype
    here; ``offset`` shifts the payload by that many further elements)."""

    def __init__(self, values, dtype, dev, offset=0):
        values = torch.as_tensor(values).reshape(-1)
        self.canary = torch.tensor(CANARY).to(dtype).item()  # (-inf in fp16: still a value no update produces)
        self.buf = torch.full((2 * PAD + offset + values.numel(),), self.canary, dtype=dtype, device=dev)
        self.lo, self.hi = PAD + offset, PAD + offset + values.numel()
        self.t = self.buf[self.lo:self.hi]
        self.t.copy_(values.to(dtype))

    def intact(self):
        return bool((self.buf[:self.lo] == self.canary).all()) and bool((self.buf[self.hi:] == self.canary).all())


def _lib():
    from uni_renderer_amd import _lib

    return _lib.load(), _lib


def _code(dtype):
    A = _lib()[1].ABI
    return {torch.float32: A.UR_DT_F32, torch.float16: A.UR_DT_F16, torch.bfloat16: A.UR_DT_BF16}[dtype]


def _advance(step_t, cur_t, omd_t, update_after_step=0, use_ema_warmup=False, inv_gamma=1.0, power=2 / 3, min_decay=0.0, decay=0.9999):
    from uni_renderer_amd.ops import _stream

    lib, L = _lib()
    sched = (ctypes.c_double * 4)(inv_gamma, power, min_decay, decay)
    L.check(lib.ur_ema_advance(ctypes.cast(step_t.data_ptr(), ctypes.POINTER(ctypes.c_int64)), update_after_step, int(use_ema_warmup),
                               sched, cur_t.data_ptr(), omd_t.data_ptr(), _stream()), "ur_ema_advance")


def _device_omd(dev, step, **kw):
    """(device fp32 scalar, its value): one_minus_decay as ur_ema_advance leaves it when it advances to ``step``."""
    st = torch.tensor(step - 1, dtype=torch.int64, device=dev)
    cur, omd = torch.zeros((), dtype=torch.float64, device=dev), torch.zeros((), dtype=torch.float32, device=dev)
    _advance(st, cur, omd, **kw)
    assert int(st) == step
    return omd, np.float32(omd.item())


def _multi(rows, omd_t):
    """One ur_ema_multi over rows of (shadow tensor, parameter tensor, flags)."""
    from uni_renderer_amd.ops import _stream

    lib, L = _lib()
    words = [w for s, p, f in rows for w in (s.data_ptr(), p.data_ptr(), s.numel(), _code(p.dtype) | f)]
    return lib.ur_ema_multi((ctypes.c_int64 * len(words))(*words), len(rows), omd_t.data_ptr(), _stream())


@pytest.mark.parametrize("kw", [dict(), dict(decay=0.5, min_decay=0.3, update_after_step=3),
                                dict(use_ema_warmup=True), dict(use_ema_warmup=True, inv_gamma=3.0, power=0.75, update_after_step=2, decay=0.8)],
                         ids=["default", "clamped", "warmup", "warmup-late"])
def test_advance_twelve_launches(dev, kw):
    st = torch.zeros((), dtype=torch.int64, device=dev)
    cur, omd = torch.full((), -1.0, dtype=torch.float64, device=dev), torch.full((), -1.0, dtype=torch.float32, device=dev)
    log_s, log_c, log_o = (torch.zeros(12, dtype=t.dtype, device=dev) for t in (st, cur, omd))
    for i in range(12):  # the state is only ever written by the kernel: the log copies are device reads
        _advance(st, cur, omd, **kw)
        log_s[i], log_c[i], log_o[i] = st, cur, omd
    torch.cuda.synchronize()
    assert log_s.tolist() == list(range(1, 13))
    want = np.array([E.get_decay(s, **kw) for s in range(1, 13)])
    want_o = np.array([E.one_minus_decay32(s, **kw) for s in range(1, 13)], dtype=np.float32)
    got_c, got_o = log_c.cpu().numpy(), log_o.cpu().numpy()
    assert want[0] == 0.0 and got_c[0] == 0.0 and got_o[0] == 1.0 and len(set(want.tolist())) > 3
    if not kw.get("use_ema_warmup"):
        # fp64 division and subtraction are correctly rounded on both sides, and so is the cast
        assert np.array_equal(got_c, want) and np.array_equal(got_o, want_o)
    else:
        # the device pow is not the host's: one fp32 ulp on what the update reads, a few fp64 ulps on cur_decay
        assert np.all(np.abs(got_o.astype(np.float64) - want_o.astype(np.float64)) <= np.spacing(want_o).astype(np.float64))
        assert np.all(np.abs(got_c - want) <= 1e-14) and np.array_equal(got_o, (1.0 - got_c).astype(np.float32))


def _layout(dev, dtype, rng, integers, B):
    """The fp32 / 16-bit cases: every size at offsets (0, 0) and (1, 1) behind a 16-byte boundary, two mixed ones and a copy row at
    either offset."""
    cases = [(n, off, off, 0) for n in (1, 3, 4, 5, 255, 1025, B, B + 1) for off in (0, 1)]
    cases += [(1025, 1, 0, 0), (1025, 0, 1, 0), (1029, 0, 0, COPY), (B + 3, 1, 1, COPY)]
    out = []
    for n, so, po, flags in cases:
        if integers:
            s, p = rng.integers(-64, 65, n).astype(np.float32), rng.integers(-64, 65, n).astype(np.float32)
        else:
            s, p = (3.0 * rng.standard_normal(n)).astype(np.float32), (3.0 * rng.standard_normal(n)).astype(np.float32)
        S, P = Guarded(torch.from_numpy(s), torch.float32, dev, so), Guarded(torch.from_numpy(p), dtype, dev, po)
        assert S.t.data_ptr() % 16 == 4 * so and P.t.data_ptr() % 16 == P.t.element_size() * po
        out.append(dict(n=n, S=S, P=P, flags=flags, s=E.widen(S.t), p=E.widen(P.t), p_raw=P.t.clone()))
    return out


def _check_guards(cases, what):
    for c in cases:
        assert c["S"].intact() and c["P"].intact(), (what, c["n"])
        assert torch.equal(c["P"].t.view(torch.uint8), c["p_raw"].view(torch.uint8)), (what, c["n"])  # never written, bit for bit


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "fp16", "bf16"])
def test_exact_on_integer_data(dev, dtype):
    B = _lib()[0].ur_ema_block_elems()
    omd, d = _device_omd(dev, 20, decay=0.5)  # (1 + 19) / (10 + 19) > 0.5: clamped
    assert d == np.float32(0.5)
    cases = _layout(dev, dtype, np.random.default_rng(11), True, B)
    assert _multi([(c["S"].t, c["P"].t, c["flags"]) for c in cases], omd) == 0
    torch.cuda.synchronize()
    _check_guards(cases, dtype)
    for c in cases:
        got = E.widen(c["S"].t).astype(np.float64)
        want = c["p"].astype(np.float64) if c["flags"] & COPY else E.definition64(c["s"], c["p"], 0.5)  # every operation is exact
        assert np.array_equal(got, want), (dtype, c["n"], c["flags"], int((got != want).sum()))
        assert c["flags"] & COPY or c["n"] < 255 or (np.any(got != c["p"]) and np.any(got != c["s"]))  # half-way between the two


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "fp16", "bf16"])
def test_random_data_is_the_three_rounding_emulation(dev, dtype):
    """Steps 1 to 5 and a late one, the shadows carried from step to step and fresh parameters at each.  Per element: bit-equal
    to the emulation, and within 2^-24 (2 d |s - p| + |s'|) (1 + 2^-22) of the float64 definition."""
    B = _lib()[0].ur_ema_block_elems()
    rng = np.random.default_rng(12)
    cases = _layout(dev, dtype, rng, False, B)
    visible = 0
    for step in (1, 2, 3, 4, 5, 12345):
        omd, d = _device_omd(dev, step)
        assert d == E.one_minus_decay32(step)
        if step > 1:
            for c in cases:  # fresh parameters (written by torch, outside the kernel)
                c["P"].t.copy_(torch.from_numpy((3.0 * rng.standard_normal(c["n"])).astype(np.float32)))
                c["p"], c["p_raw"] = E.widen(c["P"].t), c["P"].t.clone()
        assert _multi([(c["S"].t, c["P"].t, c["flags"]) for c in cases], omd) == 0
        torch.cuda.synchronize()
        _check_guards(cases, (dtype, step))
        for c in cases:
            got = E.widen(c["S"].t)
            if c["flags"] & COPY:
                assert np.array_equal(got, c["p"]), (dtype, step, c["n"])
            else:
                want = E.emulate32(c["s"], c["p"], d)
                assert np.array_equal(got, want), (dtype, step, c["n"], c["flags"], int((got != want).sum()))
                err = np.abs(got.astype(np.float64) - E.definition64(c["s"], c["p"], d))
                assert np.all(err <= E.bound64(c["s"], c["p"], d)), (dtype, step, c["n"])
                visible += int((E.contracted32(c["s"], c["p"], d) != want).sum()) if 2 <= step <= 5 else 0
            c["s"] = got
    assert visible > 10000  # an fma contraction of d * t and s - u would have failed the bit-equality above


def _mixed_params(dev, k):
    g = torch.Generator().manual_seed(20 + k)
    sizes = [(1,), (3, 5), (255,), (4096,), (16384,), (16385,), (7, 9, 11), (1025,), (64, 33)]
    ps = []
    for i in range(k):
        dt = (torch.float32, torch.float32, torch.bfloat16, torch.float16)[i % 4] if k > 1 else torch.float32
        p = torch.nn.Parameter((3.0 * torch.randn(sizes[i % len(sizes)], generator=g)).to(dev, dt))
        p.requires_grad_(i % 7 != 5)  # some frozen: copied
        ps.append(p)
    return ps, g


@pytest.mark.parametrize("k", [1, 65])
def test_every_tensor_is_updated_exactly_once(dev, k):
    from uni_renderer_amd import EMAModel

    ps, g = _mixed_params(dev, k)
    e = EMAModel(ps, decay=0.9)
    assert all(s.dtype == torch.float32 and s.is_cuda for s in e.shadow_params) and e._step.is_cuda
    s = [E.widen(x) for x in e.shadow_params]
    versions = [x._version for x in e.shadow_params]
    for step in range(1, 5):
        with torch.no_grad():
            for p in ps:
                p.add_((0.5 * torch.randn(p.shape, generator=g)).to(dev, p.dtype))
        raw = [p.detach().clone() for p in ps]
        e.step(ps)
        assert [count for _, count in e._cache[1]] == ([64, 1] if k == 65 else [1])  # two launches for 65 tensors
        s = E.replay(s, [E.widen(p) for p in ps], step, requires_grad=[p.requires_grad for p in ps], decay=0.9)
        for i, (a, b) in enumerate(zip(e.shadow_params, s)):  # a tensor updated twice, or not at all, differs
            assert np.array_equal(E.widen(a), b), (k, step, i)
        assert all(torch.equal(a.detach(), b) for a, b in zip(ps, raw))
    assert e.optimization_step == 4 and e.cur_decay_value == E.get_decay(4, decay=0.9)
    assert all(x._version > v for x, v in zip(e.shadow_params, versions))
    tables = e._cache[1]
    e.step(ps)
    assert e._cache[1] is tables  # same addresses: the item tables are reused
    ps[0].requires_grad_(not ps[0].requires_grad)  # averaged <-> copied: the tables are rebuilt
    before = [E.widen(x) for x in e.shadow_params]
    e.step(ps)
    want = E.replay(before, [E.widen(p) for p in ps], 6, requires_grad=[p.requires_grad for p in ps], decay=0.9)
    assert e._cache[1] is not tables and all(np.array_equal(E.widen(a), b) for a, b in zip(e.shadow_params, want))


def test_bad_items_launch_nothing(dev):
    lib, L = _lib()
    BAD = L.ABI.UR_E_BADARG
    omd, _ = _device_omd(dev, 5)
    s, p = torch.ones(100, device=dev), torch.zeros(100, device=dev)
    good = (s.data_ptr(), p.data_ptr(), 100, L.ABI.UR_DT_F32)

    def call(rows, n=None):
        from uni_renderer_amd.ops import _stream

        words = [w for r in rows for w in r]
        return lib.ur_ema_multi((ctypes.c_int64 * len(words))(*words), len(rows) if n is None else n, omd.data_ptr(), _stream())

    for rows in ([good, (0,) + good[1:]], [good, (good[0], 0) + good[2:]], [good, good[:2] + (0, good[3])], [good] * 65):
        assert call(rows) == BAD
    assert call([good], n=0) == BAD and lib.ur_ema_multi(None, 1, omd.data_ptr(), None) == BAD
    torch.cuda.synchronize()
    assert bool((s == 1.0).all()) and bool((p == 0.0).all())  # not even the good first row ran
    assert call([good]) == 0
    torch.cuda.synchronize()
    assert not bool((s == 1.0).any())
