"""GPU tests of ``ur_ddim_update`` / ``ur_unipc_update`` (csrc/sampler.hip) per element, on the rig of
tests/test_sde_update_gpu.py: exactly on small-integer data with dyadic table rows, on guarded buffers, for fp16 / bf16, every
layout, guidance on / off, ``round_master`` on / off; DDIM against the host scheduler bit for bit; UniPC against the float64
update of its own previous state within the dot-product bound."""
import itertools

import pytest
import torch

from util_models import ROOT  # noqa: F401  (path setup)
from util_sampler_update import HALF_ULP, SHAPES, Case, combine

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16]
IDS = ["f16", "bf16"]


def _advance(c, n):
    from uni_renderer_amd import ops

    ops.sampler_advance(c.step, torch.zeros(n, device=c.step.device), n)


def _fits(v, dtype):
    """``v`` (float64) is exact in fp32 and in the storage dtype."""
    return torch.equal(v.float().double(), v) and torch.equal(v.to(dtype).double(), v)


@pytest.mark.parametrize("with_master", [True, False], ids=["master", "nomaster"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_ddim_update_is_exact_on_small_integer_data(dev, dtype, with_master):
    """Rows (sqrt a_t, sqrt(1 - a_t), sqrt a_prev, sqrt(1 - a_prev)) of powers of two, integer data in [-2, 2] (guided
    predictions 2 p_cond - p_uncond in [-6, 6]).  With x the sample and m the prediction the three rows give
        (1, 1/2, 2, 1/2)    eps = 2 (x - m)        x' = 2 m + (x - m) = x + m        |x'| <= 8
        (2, 1, 1, 1)        eps = x - 2 m          x' = m + (x - 2 m) = x - m        |x'| <= 14
        (1/2, 1/4, 2, 1/2)  eps = 4 (x - m / 2)    x' = 2 m + (2 x - m) = 2 x + m    |x'| <= 34, then <= 74 (fourth call: row 2 again)
    and every intermediate (|.| <= 148, multiples of 1/2) is exact in fp32 and fits the 8-bit significand of bf16 -- checked
    here in float64 -- so the kernel must reproduce the float64 recurrence bit for bit: ``lat`` (both halves), ``master``, the
    clamp of ``*step`` (4 calls against 3 rows), the guards and the channels outside the slice.  Without ``master`` the sample
    is read back from ``lat``."""
    from uni_renderer_amd import ops

    rows = torch.tensor([[1, 0.5, 2, 0.5], [2, 1, 1, 1], [0.5, 0.25, 2, 0.5]], dtype=torch.float32)
    gen = torch.Generator().manual_seed(11)
    for (B, C, hw), cfg, rm in itertools.product(SHAPES, (False, True), (False, True)):
        c = Case(dev, dtype, B, C, hw, cfg, 3, gen, integer=True)
        cc = C // 2  # cfg_channels < C
        if not with_master:
            c.lat.copy_(torch.cat([c.x0, c.x0] if cfg else [c.x0]).to(dtype))
        x = c.x0.double()
        for i in range(4):  # the fourth call has *step = 3 >= nsteps: row 2 again
            k = min(i, 2)
            ops.ddim_update(c.preds[k], 4, c.lat, rows.to(dev), c.step, 3, master=c.master if with_master else None,
                            round_master=rm, guidance=2.0 if cfg else None, cfg_channels=cc if cfg else 0)
            _advance(c, 3)
            m = combine(c.preds[k], cfg, 2.0, cc, B, C).double().cpu()
            s_at, s_1mat, s_ap, s_1map = (float(v) for v in rows[k])
            t0 = s_at * m
            t1 = x - t0
            eps = t1 / s_1mat
            a, e = s_ap * m, s_1map * eps
            x = a + e
            assert all(_fits(v, dtype) for v in (t0, t1, eps, a, e, x)), "the test's data is not exact"
            tag = (B, C, hw, cfg, rm, i)
            assert torch.equal(c.lat[:B].cpu().double(), x), tag
            if cfg:
                assert torch.equal(c.lat[B:], c.lat[:B]), tag
            if with_master:
                assert torch.equal(c.master.cpu().double(), x), tag
            else:
                assert torch.equal(c.master.cpu(), c.x0), tag  # not passed: not touched
            assert torch.equal(c.hist, torch.zeros_like(c.hist)) and c.intact(), tag
        assert int(c.step) == 4


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_ddim_kernel_equals_the_host_scheduler_step_bitwise(dev, dtype):
    """3 steps of ``ur_ddim_update`` on the plan's table == 3 ``DDIMScheduler.step`` calls on fp32 samples: the same fp32
    expressions in the same order, no contraction on either side, so N(0, 1) data must agree bit for bit.  With and without
    guidance (the host gets the prediction combined in its dtype, as the step-by-step loop does)."""
    from uni_renderer_amd import ops
    from uni_renderer_amd.schedulers import DDIMScheduler, device_plan

    gen = torch.Generator().manual_seed(12)
    n = 3
    s = DDIMScheduler()
    s.set_timesteps(n)
    plan = device_plan(s)
    assert plan.kind == "ddim" and tuple(plan.coef.shape) == (n, 4)
    for (B, C, hw), cfg in itertools.product(SHAPES, (False, True)):
        c = Case(dev, dtype, B, C, hw, cfg, n, gen, integer=False)
        x = c.master.clone()  # fp32 samples
        for i, t in enumerate(s.timesteps):
            ops.ddim_update(c.preds[i], 4, c.lat, plan.coef.to(dev), c.step, n, master=c.master, round_master=False,
                            guidance=2.5 if cfg else None, cfg_channels=C // 2 if cfg else 0)
            _advance(c, n)
            x = s.step(combine(c.preds[i], cfg, 2.5, C // 2, B, C), t, x)[0]
            assert x.dtype == torch.float32 and torch.equal(c.master, x), (B, C, hw, cfg, i)
            assert torch.equal(c.lat[:B], x.to(dtype)), (B, C, hw, cfg, i)
            if cfg:
                assert torch.equal(c.lat[B:], c.lat[:B])
        assert c.intact()


def _ring(st):
    """(slot read as m_{i-1}, slot read as m_{i-2} and then overwritten with m_i) at the device step ``st``."""
    return (st + 1) & 1, st & 1


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_unipc_update_is_exact_on_small_integer_data(dev, dtype):
    """Rows (c0 c1 c2 c3 | p0 p1 p2 -) of +-1/2, +-1, +-2 with non-zero c2 and p2, integer data in [-2, 2] (guided predictions
    in [-6, 6]):  L = c0 L + c1 m_{i-1} + c2 m_{i-2} + c3 m_i,  x = p0 L + p1 m_i + p2 m_{i-1}.  Over the five calls (four rows;
    the fifth has *step = 4 >= nsteps: row 3 again, on the ring slots of step 3) |L| <= 8, 26, 37, 58, 79 and |x| <= 14, 25, 52,
    70, 91 in multiples of 1/2: at most 182 half-units, inside the 8-bit significand of bf16 -- checked here in float64.  Exact
    data makes the result independent of fma contraction and of ``round_master``.  Both ring slots are read as m_{i-1} and as
    m_{i-2} and overwritten; ``last``, ``xmaster``, both slots, ``lat`` and the guards are compared exactly."""
    from uni_renderer_amd import ops

    rows = torch.tensor([[1, 1, 1, 1, 1, -1, 1, 0], [-1, 1, -1, 1, 0.5, 1, -1, 0], [0.5, -1, 1, 2, 1, 2, -0.5, 0],
                         [1, 0.5, -2, 1, -1, 1, 1, 0]], dtype=torch.float32)
    n = 4
    gen = torch.Generator().manual_seed(13)
    for (B, C, hw), cfg, rm in itertools.product(SHAPES, (False, True), (False, True)):
        c = Case(dev, dtype, B, C, hw, cfg, n, gen, integer=True, ring=True)
        cc = C // 2
        c.master.fill_(3.0)  # xmaster is written, never read: its initial value must not matter
        L = c.x0.double()
        slots = [torch.zeros_like(L), torch.zeros_like(L)]
        for i in range(5):
            k = min(i, n - 1)
            ops.unipc_update(c.preds[k], 4, c.lat, rows.to(dev), c.step, n, c.last, c.master, c.hist, round_master=rm,
                             guidance=2.0 if cfg else None, cfg_channels=cc if cfg else 0)
            _advance(c, n)
            m = combine(c.preds[k], cfg, 2.0, cc, B, C).double().cpu()
            r = rows[k].double()
            s1, s2 = _ring(k)
            terms = [r[0] * L, r[1] * slots[s1], r[2] * slots[s2], r[3] * m]
            L = terms[0] + terms[1] + terms[2] + terms[3]
            x = r[4] * L + r[5] * m + r[6] * slots[s1]
            assert all(_fits(v, dtype) for v in (L, x, terms[0] + terms[1], terms[0] + terms[1] + terms[2], r[4] * L + r[5] * m)), \
                "the test's data is not exact"
            slots[s2] = m
            tag = (B, C, hw, cfg, rm, i)
            assert torch.equal(c.last.cpu().double(), L) and torch.equal(c.master.cpu().double(), x), tag
            assert torch.equal(c.hist[0].cpu().double(), slots[0]) and torch.equal(c.hist[1].cpu().double(), slots[1]), tag
            assert torch.equal(c.lat[:B].cpu().double(), x), tag
            if cfg:
                assert torch.equal(c.lat[B:], c.lat[:B]), tag
            assert c.intact(), tag
        assert int(c.step) == 5


def _gamma(k):
    return k * 2.0 ** -24 / (1 - k * 2.0 ** -24)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_unipc_update_against_float64_on_guarded_buffers(dev, dtype):
    """N(0, 1) data, all seven weights non-zero.  Each step is compared with the float64 update of the kernel's OWN previous
    state (``last``, both ``hist`` slots), so no error accumulates and the bound is one step's: a dot product of k terms
    evaluated in fp32 in any order, with or without fma, is within gamma_k * sum |c_j v_j| of the exact one, gamma_k =
    k 2^-24 / (1 - k 2^-24) (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., eq. 3.5):
        |L - L64| <= gamma_4 * sum |c_j v_j|                                            = err_L
        |x - x64| <= |p0| * err_L + gamma_3 * (|p0| (|L64| + err_L) + |p1 m| + |p2 m1|)
    With ``round_master`` L, and ``xmaster``, are rounded through the storage dtype where the scheduler casts them: one more
    rounding, half an ulp of that dtype (2^-11 / 2^-8 relative; 2^-25 absolute below fp16's normal range), which ``lat`` always
    has.  The slot that receives m_i holds it exactly; the other slot is unchanged."""
    from uni_renderer_amd import ops

    rows = torch.tensor([[0.9, 0.3, -0.2, 0.5, 0.8, 0.6, -0.4, 0], [0.7, 1.4, -0.6, 0.8, 1.1, -0.3, 0.25, 0],
                         [-0.2, 1.1, -0.3, 0.05, 0.6, 0.9, -0.7, 0], [1.2, -0.4, 0.15, 0.35, 0.95, 0.45, -0.55, 0]], dtype=torch.float32)
    n = 4
    gen = torch.Generator().manual_seed(14)
    u = HALF_ULP[dtype]
    tiny = 2.0 ** -25 if dtype == torch.float16 else 0.0
    store = lambda want, err: u * want.abs() + err * (1 + u) + tiny  # a value known to ``err``, then rounded to the dtype
    worst = 0.0
    for (B, C, hw), cfg, rm in itertools.product(SHAPES, (False, True), (False, True)):
        c = Case(dev, dtype, B, C, hw, cfg, n, gen, integer=False, ring=True)
        c.hist.copy_(torch.randn(c.hist.shape, generator=gen))  # step 0 reads both slots too
        cc = C - 1
        for i in range(n):
            L_prev, h_prev = c.last.double().cpu(), c.hist.double().cpu()
            ops.unipc_update(c.preds[i], 4, c.lat, rows.to(dev), c.step, n, c.last, c.master, c.hist, round_master=rm,
                             guidance=1.5 if cfg else None, cfg_channels=cc if cfg else 0)
            _advance(c, n)
            m = combine(c.preds[i], cfg, 1.5, cc, B, C).double().cpu()
            r = rows[i].double()
            s1, s2 = _ring(i)
            cterms = [r[0] * L_prev, r[1] * h_prev[s1], r[2] * h_prev[s2], r[3] * m]
            L = cterms[0] + cterms[1] + cterms[2] + cterms[3]
            err_L = _gamma(4) * sum(t.abs() for t in cterms) + 1e-30
            if rm:
                err_L = store(L, err_L)
            x = r[4] * L + r[5] * m + r[6] * h_prev[s1]
            err_x = r[4].abs() * err_L + _gamma(3) * (r[4].abs() * (L.abs() + err_L) + (r[5] * m).abs() + (r[6] * h_prev[s1]).abs())
            err_lat = store(x, err_x)
            e_L = (c.last.double().cpu() - L).abs()
            e_x = (c.master.double().cpu() - x).abs()
            e_lat = (c.lat[:B].double().cpu() - x).abs()
            worst = max(worst, float((e_L / err_L).max()), float((e_x / (err_lat if rm else err_x)).max()), float((e_lat / err_lat).max()))
            tag = (B, C, hw, cfg, rm, i)
            assert bool((e_L <= err_L).all()), tag
            assert bool((e_x <= (err_lat if rm else err_x)).all()), tag
            assert bool((e_lat <= err_lat).all()), tag
            assert torch.equal(c.hist[s2].cpu().double(), m) and torch.equal(c.hist[s1].cpu().double(), h_prev[s1]), tag
            assert torch.equal(c.lat[:B].float(), c.master) if rm else torch.equal(c.lat[:B], c.master.to(dtype)), tag
            if rm:
                assert torch.equal(c.last.to(dtype).float(), c.last), tag
            if cfg:
                assert torch.equal(c.lat[B:], c.lat[:B]), tag
            assert c.intact(), tag
    print("max err / bound", worst)
