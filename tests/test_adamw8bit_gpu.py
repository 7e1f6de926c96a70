"""GPU tests of the 8-bit AdamW (csrc/adamw8.hip, optim.AdamW8bit) against the float64 restatement of tests/util_adamw8bit.py:
per element, on guarded buffers, with the tolerances derived where they are used."""
import numpy as np
import pytest
import torch

import util_adamw8bit as U
from util_models import O, build_product_from_oracle

pytestmark = pytest.mark.gpu

F32 = lambda x: float(np.float32(x))  # noqa: E731  the kernel receives fp32 hyper-parameters: the restatement gets the same values
LR, B1, B2, EPS, WD = F32(1e-3), F32(0.9), F32(0.999), F32(1e-8), F32(1e-2)
CANARY_F, CANARY_B, PAD = -6.02e23, 0xA5, 64


class Guarded:
    """n elements with PAD canaries on both sides (PAD keeps the 16-byte / 4-byte alignment of the allocation; ``offset``
    shifts the payload by that many further elements)."""

    def __init__(self, values, dtype, dev, offset=0):
        values = torch.as_tensor(values).reshape(-1)
        self.canary = CANARY_B if dtype == torch.uint8 else CANARY_F
        self.buf = torch.full((2 * PAD + offset + values.numel(),), self.canary, dtype=dtype, device=dev)
        self.t = self.buf[PAD + offset:PAD + offset + values.numel()]
        self.t.copy_(values.to(dtype))
        self.lo, self.hi = PAD + offset, PAD + offset + values.numel()

    def intact(self):
        return bool((self.buf[:self.lo] == self.canary).all()) and bool((self.buf[self.hi:] == self.canary).all())

    def np(self):
        return self.t.cpu().numpy()


def _assert_nearest(codes, r, dr, signed, positive=None, what=""):
    """Every stored code is a nearest entry for r, up to the fp32 rounding dr of r: a value within dr of the midpoint of two
    entries may take either, which puts its entry at most 2 dr further away than the nearest one."""
    b = U.BOOKS[signed]
    want = U.nearest(r, signed, positive=positive)
    excess = np.abs(b[codes] - r) - np.abs(b[want] - r)
    bad = excess > 2 * dr
    assert not bad.any(), (what, int(bad.sum()), np.flatnonzero(bad)[:5], codes[bad][:5], want[bad][:5], r[bad][:5])
    if positive is not None:
        assert not (positive & (codes == 0)).any(), what  # the code-1 rule
    return int((codes != want).sum())


def _edge_data(n, signed, rng):
    x = rng.standard_normal(n) * np.repeat(np.exp(2 * rng.standard_normal(U.nblocks(n))), 256)[:n]
    if n >= 1024:
        x[0:256] = 0.0                               # a zero block
        x[256:512] = 0.0
        x[300] = 3.5e-4                              # a block with one non-zero
        x[512:768] = -np.abs(x[512:768]) - 1e-3      # an all-negative block
        x[768:1024] = 1.0
        x[771] = 1e-8                                # 1e-8 of its block's maximum
    x = x if signed else x * x
    return x.astype(np.float32)


@pytest.mark.parametrize("signed", [True, False])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 4099])
def test_quantize_dequantize_per_element(dev, n, signed):
    from uni_renderer_amd import _lib
    from uni_renderer_amd.ops import _stream

    lib = _lib.load()
    x32 = _edge_data(n, signed, np.random.default_rng(n + signed))
    x = torch.from_numpy(x32).to(dev)
    codes, amax = Guarded(torch.zeros(n), torch.uint8, dev), Guarded(torch.zeros(U.nblocks(n)), torch.float32, dev)
    _lib.check(lib.ur_adam8_quantize(x.data_ptr(), codes.t.data_ptr(), amax.t.data_ptr(), n, int(signed), _stream()), "quantize")
    torch.cuda.synchronize()
    assert codes.intact() and amax.intact()
    x64 = x32.astype(np.float64)
    want_c, want_am = U.encode(x64, signed)
    assert np.array_equal(amax.np().astype(np.float64), want_am)  # a maximum of fp32 values is exact
    # the kernel rounds x / absmax once (2^-24 relative) before it compares
    r = U.normalised(x64, want_am)
    diff = _assert_nearest(codes.np(), r, 2.0 ** -24 * np.abs(r), signed, positive=None if signed else x64 > 0, what=(n, signed))
    assert diff <= 0.005 * n, (diff, n)  # near-ties are ~1e-7 of such data: any mismatch at all is unexpected at these sizes
    if n == 4099:
        c = codes.np()
        zero = U.ZERO_CODE[signed]
        assert np.all(c[0:256] == zero) and c[300] == 255 and np.all(np.delete(c[256:512], 44) == zero)
        assert signed is False or np.all(c[512:768] < 127)
        # 1e-8 of the maximum is nearest to 0; only exp_avg_sq has the code-1 rule
        assert c[771] == (127 if signed else 1) and np.all(np.delete(c[768:1024], 3) == 255)
    out = Guarded(torch.zeros(n), torch.float32, dev)
    _lib.check(lib.ur_adam8_dequantize(out.t.data_ptr(), codes.t.data_ptr(), amax.t.data_ptr(), n, int(signed), _stream()), "dequantize")
    torch.cuda.synchronize()
    assert out.intact()
    # book[code] * absmax, two fp32 factors: their float64 product is exact, its fp32 rounding is the kernel's product
    assert np.array_equal(out.np(), U.decode(codes.np(), amax.np().astype(np.float64), signed).astype(np.float32))


def _check_step(got_p, got_cm, got_am, got_cv, got_av, R, m_old, v_old, what, am_tol=None):
    """One tensor after one update against the restatement's result R (float64 from the same inputs).

    absmax: the fresh moment of the block's extreme element went through the decode product, g / grad_scale, the lerp (or
    beta2 v + (1 - beta2) g^2) -- at most four fp32 roundings of terms that do not cancel there: relative 4 * 2^-24 = 2^-22.
    p: p * decay and the final subtraction round p (2 * 2^-24 each at most: 2^-22 |p|); the update lr / bc1 * m / (sqrt(v) /
    sqrt(bc2) + eps) collects ~10 fp32 roundings and the fp32 bias corrections: 1e-5 relative is 80 * 2^-23.
    codes: fp32 error of a fresh moment <= 2^-22 (|old moment| + |gradient term|) (absolute: the lerp may cancel), of absmax
    2^-22 relative, of the division 2^-24: that is dr below.  Returns the number of codes that are not the float64-nearest.
    ``am_tol``: per-block bound on exp_avg's absmax for data whose extreme element may cancel (lerp_absmax_tolerance)."""
    assert np.all(np.abs(got_am - R["am"]) <= (2.0 ** -22 * R["am"] if am_tol is None else am_tol)), (what, "absmax_m")
    assert np.all(np.abs(got_av - R["av"]) <= 2.0 ** -22 * R["av"]), (what, "absmax_v")
    err = np.abs(got_p - R["p"])
    assert np.all(err <= 2.0 ** -22 * np.abs(R["p"]) + 1e-5 * np.abs(R["update"])), (what, "p", float(err.max()))
    n = got_p.size
    am, av = np.repeat(R["am"], 256)[:n], np.repeat(R["av"], 256)[:n]
    rm, rv = U.normalised(R["m"], R["am"]), U.normalised(R["v"], R["av"])
    dm = 2.0 ** -22 * (np.abs(m_old) + np.abs(R["g"])) / np.maximum(am, 1e-300) + (2.0 ** -22 + 2.0 ** -24) * np.abs(rm)
    dv = 2.0 ** -22 * (v_old + R["g"] ** 2) / np.maximum(av, 1e-300) + (2.0 ** -22 + 2.0 ** -24) * rv
    return (_assert_nearest(got_cm, rm, dm, True, what=(what, "m")),
            _assert_nearest(got_cv, rv, dv, False, positive=R["v"] > 0, what=(what, "v")))


def lerp_absmax_tolerance(m_old, R):
    """fp32 bound on the absmax of the fresh exp_avg that holds when the block's extreme element cancels (a one-element last
    block whose 0.9 m and 0.1 g nearly cancel: relative 2^-22 of the RESULT is then not what fp32 can give).  Per element,
    with u = 2^-24 and c = 1 - beta1 = 0.1: the decode product errs by u |m|, g / grad_scale by u |g|, their difference d by
    both plus u |d| <= u (|m| + |g|), c d by c times that plus u c |d|, the final sum by all of it plus u |m_new|:
    u (1.3 |m| + 0.3 |g| + |m_new|) (1.2 / 0.2 when the lerp contracts to an fma).  A maximum moves by at most the largest
    move of an element.  Where nothing cancels (|m_new| ~ 0.9 |m| + 0.1 |g|) this is below the relative 2^-22."""
    return U.block_absmax(2.0 ** -24 * (1.3 * np.abs(m_old) + 0.3 * np.abs(R["g"]) + np.abs(R["m"])))


def test_one_step_per_element_from_random_state(dev):
    from uni_renderer_amd import _lib, optim
    from uni_renderer_amd.ops import _stream

    rng = np.random.default_rng(7)
    sizes = [4096, 4097, 65536, 640 * 3 * 3 * 3, 1, 255, 257, 5000, 16384, 16385]
    sizes = (sizes * 7)[:70]
    sizes[12] = 20000  # (one tensor of 65536 is enough)
    sizes[22] = sizes[32] = sizes[42] = sizes[52] = sizes[62] = 9000
    T = []
    for k, n in enumerate(sizes):
        nb = U.nblocks(n)
        scale = np.repeat(np.exp(rng.standard_normal(nb)), 256)[:n]
        t = dict(n=n, p=(0.05 * rng.standard_normal(n)).astype(np.float32), g=(1.5e-3 * rng.standard_normal(n) * scale).astype(np.float32),
                 cm=rng.integers(0, 256, n, dtype=np.uint8), cv=rng.integers(0, 256, n, dtype=np.uint8),
                 am=(1e-3 * np.exp(rng.standard_normal(nb))).astype(np.float32), av=(1e-6 * np.exp(rng.standard_normal(nb))).astype(np.float32))
        t["G"] = {key: Guarded(torch.from_numpy(t[key]), torch.uint8 if key in ("cm", "cv") else torch.float32, dev,
                               offset=1 if (key == "g" and k % 5 == 1) else 0)  # an odd-offset gradient view: the scalar path
                  for key in ("p", "g", "cm", "cv", "am", "av")}
        T.append(t)
    assert T[1]["G"]["g"].t.data_ptr() % 16 == 4 and T[0]["G"]["g"].t.data_ptr() % 16 == 0
    step, gs = torch.tensor(7.0, device=dev), torch.tensor(1.5, device=dev)

    rows = [tuple(t["G"][key].t.data_ptr() for key in ("p", "g", "cm", "cv", "am", "av")) + (t["n"],) for t in T]
    tables = optim.adamw8_tables(rows)
    assert [count for _, count in tables] == [64, 6]  # 70 tensors: two launches
    for table, count in tables:
        _lib.check(_lib.load().ur_adamw8_multi(table, count, LR, B1, B2, EPS, WD, step.data_ptr(), gs.data_ptr(), None, None, _stream()),
                   "ur_adamw8_multi")
    torch.cuda.synchronize()
    diff, total = np.zeros(2), 0
    for k, t in enumerate(T):
        G = t["G"]
        assert all(G[key].intact() for key in G), (k, t["n"])
        assert np.array_equal(G["g"].np(), t["g"])
        f64 = {key: t[key].astype(np.float64) for key in ("p", "g", "am", "av")}
        R = U.adamw8_step(f64["p"], f64["g"], t["cm"], f64["am"], t["cv"], f64["av"], 7, LR, B1, B2, EPS, WD, grad_scale=1.5)
        diff += _check_step(G["p"].np().astype(np.float64), G["cm"].np(), G["am"].np().astype(np.float64), G["cv"].np(),
                            G["av"].np().astype(np.float64), R, U.decode(t["cm"], f64["am"], True), U.decode(t["cv"], f64["av"], False),
                            (k, t["n"]))
        total += t["n"]
    print(f"codes that are not the float64-nearest: exp_avg {int(diff[0])}, exp_avg_sq {int(diff[1])} of {total}")
    assert np.all(diff <= 0.005 * total), (diff, total)


def _params(dev, seed, shapes):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter((0.05 * torch.randn(s, generator=g)).to(dev)) for s in shapes]


SHAPES = [(4096,), (4097,), (640, 3, 3, 3), (65536,), (100,), (320,), (4095,)]


def _set_grads(ps, seed, dev):
    g = torch.Generator().manual_seed(seed)
    for p in ps:
        p.grad = (2e-3 * torch.randn(p.shape, generator=g) * torch.exp(torch.randn(p.shape[:1], generator=g)).reshape(
            (-1,) + (1,) * (p.dim() - 1))).to(dev)


def test_five_steps_teacher_forced_with_a_skipped_step(dev):
    """After every step the GPU's own state is the restatement's input for the next one (a legitimate code flip cannot
    compound); three groups with their own lr / weight decay read from the device pair; step 3 has found_inf = 1."""
    from uni_renderer_amd.optim import AdamW8bit

    ps = _params(dev, 3, SHAPES)
    opt = AdamW8bit([{"params": ps[:2]}, {"params": ps[2:5], "lr": F32(3e-4), "weight_decay": 0.0}, {"params": ps[5:], "lr": F32(2e-3)}],
                    lr=LR, betas=(B1, B2), eps=EPS, weight_decay=WD)
    opt.grad_scale, opt.found_inf = torch.tensor(1.5, device=dev), torch.tensor(0.0, device=dev)
    big = [p for p in ps if p.numel() >= 4096]
    group_of = {p: g for g in opt.param_groups for p in g["params"]}
    for p in ps:
        opt._init_state(p)  # fresh state: codes 127 / 0, absmax 0 -- the restatement's input of the first step
    t, diff, total = 0, np.zeros(2), 0
    for it in range(6):
        _set_grads(ps, 100 + it, dev)
        skipped = it == 2
        opt.found_inf.fill_(1.0 if skipped else 0.0)
        before = {p: (p.detach().cpu().numpy().astype(np.float64).reshape(-1),) + tuple(
            opt.state[p][k].cpu().numpy().reshape(-1) for k in ("exp_avg", "exp_avg_absmax", "exp_avg_sq", "exp_avg_sq_absmax"))
            for p in big}
        raw = {p: [p.detach().clone()] + [v.clone() for k, v in opt.state[p].items() if k != "step"] for p in ps}
        opt.step()
        torch.cuda.synchronize()
        if skipped:
            for p in ps:  # every byte untouched, and the counter did not advance
                now = [p.detach()] + [v for k, v in opt.state[p].items() if k != "step"]
                assert all(torch.equal(a, b) for a, b in zip(raw[p], now))
            assert all(float(opt.state[p]["step"]) == t for p in ps)
            continue
        t += 1
        assert all(float(opt.state[p]["step"]) == t for p in ps)
        for p in big:
            n, grp = p.numel(), group_of[p]
            p0, cm, am, cv, av = before[p]
            am, av = am.astype(np.float64), av.astype(np.float64)
            R = U.adamw8_step(p0, p.grad.cpu().numpy().astype(np.float64), cm, am, cv, av, t, grp["lr"], B1, B2, EPS,
                              F32(grp["weight_decay"]), grad_scale=1.5)
            st = opt.state[p]
            diff += _check_step(p.detach().cpu().numpy().astype(np.float64).reshape(-1), st["exp_avg"].cpu().numpy().reshape(-1),
                                st["exp_avg_absmax"].cpu().numpy().astype(np.float64), st["exp_avg_sq"].cpu().numpy().reshape(-1),
                                st["exp_avg_sq_absmax"].cpu().numpy().astype(np.float64), R, U.decode(cm, am, True),
                                U.decode(cv, av, False), (it, tuple(p.shape)), am_tol=lerp_absmax_tolerance(U.decode(cm, am, True), R))
            total += n
    assert t == 5 and np.all(diff <= 0.005 * total), (diff, total)


def test_small_tensors_are_fusedadamw_bit_for_bit(dev):
    from uni_renderer_amd.optim import AdamW8bit, FusedAdamW

    pa, pb = _params(dev, 5, SHAPES), _params(dev, 5, SHAPES)
    kw = dict(lr=LR, betas=(B1, B2), eps=EPS, weight_decay=WD)
    oa, ob = AdamW8bit(pa, **kw), FusedAdamW(pb, **kw)
    for it in range(5):
        _set_grads(pa, 200 + it, dev)
        _set_grads(pb, 200 + it, dev)
        oa.step()
        ob.step()
    small = [(a, b) for a, b in zip(pa, pb) if a.numel() < 4096]
    assert len(small) == 3 and float(oa.state[pa[0]]["step"]) == 5.0
    for a, b in small:
        assert torch.equal(a, b) and torch.equal(oa.state[a]["exp_avg"], ob.state[b]["exp_avg"])
        assert torch.equal(oa.state[a]["exp_avg_sq"], ob.state[b]["exp_avg_sq"])
        assert oa.state[a]["step"] is oa.state[pa[0]]["step"]  # one device counter for both kinds of tensor
    assert not any(torch.equal(a, b) for a, b in zip(pa, pb) if a.numel() >= 4096)  # the others did go through 8-bit state


@pytest.mark.parametrize("spread", [0.5, 1.5])
def test_trajectory_against_fp32_adamw(dev, spread):
    """65536 elements, 20 steps from fresh state, against FusedAdamW on the same gradients.  spread 0.5: rel-L2 of the
    displacement p - p0; the GPU may exceed the restatement's own figure on the same data by 10 % (single code flips at
    near-ties, nothing else).  spread 1.5: the worst element stays within 1.0 lr t of fp32 AdamW (plain nearest rounding of
    exp_avg_sq: more than 500 lr t, tests/test_adamw8bit_cpu.py)."""
    from uni_renderer_amd.optim import AdamW8bit, FusedAdamW

    p0, grads = U.trajectory_data(0, spread=spread)
    kw = dict(lr=LR, betas=(B1, B2), eps=EPS, weight_decay=WD)
    pa = torch.nn.Parameter(torch.from_numpy(p0).float().to(dev))
    pb = torch.nn.Parameter(pa.detach().clone())
    oa, ob = AdamW8bit([pa], **kw), FusedAdamW([pb], **kw)
    for g in grads:
        pa.grad = torch.from_numpy(g).float().to(dev)
        pb.grad = pa.grad.clone()
        oa.step()
        ob.step()
    gpu, ref = pa.detach().cpu().numpy().astype(np.float64), pb.detach().cpu().numpy().astype(np.float64)
    restated = U.adamw8_trajectory(p0, grads, LR, B1, B2, EPS, WD)[-1]
    if spread == 0.5:
        fig_gpu, fig_restated = U.rel_l2(gpu - p0, ref - p0), U.rel_l2(restated - p0, ref - p0)
        print(f"rel-L2 of the displacement after 20 steps against FusedAdamW: GPU {fig_gpu:.5f}, restatement {fig_restated:.5f}")
        assert fig_gpu <= 1.1 * fig_restated
    else:
        worst, worst_restated = np.abs(gpu - ref).max() / (LR * 20), np.abs(restated - ref).max() / (LR * 20)
        print(f"worst element / (lr t) after 20 steps: GPU {worst:.3f}, restatement {worst_restated:.3f}")
        assert worst <= 1.0


def _nets(dev, seed, lr=4e-4):
    from uni_renderer_amd.optim import AdamW8bit

    nets = build_product_from_oracle(*O.build_triplet(O.TINY_CONFIG, seed=seed), torch.float32, dev)
    for m in nets:
        m.train()
        m.requires_grad_(True)
    ps = [p for m in nets for p in m.parameters()]
    opt = AdamW8bit(ps, lr=lr, betas=(0.9, 0.99), weight_decay=1e-2)
    assert any(opt._is_8bit(p) for p in ps) and not all(opt._is_8bit(p) for p in ps)  # both kernels are in the step
    return nets, opt


def _batch(dev, it):
    x, c, ehs, ti, ta = [t.to(dev) for t in O.make_inputs(2, 16, 64, seed=70 + it)]
    g = torch.Generator().manual_seed(71 + it)
    return dict(x_t=x, cond=c, ehs=ehs, t_img=ti, t_attr=ta, target_img=torch.randn(2, 4, 16, 16, generator=g).to(dev),
                target_attr=torch.randn(2, 28, 16, 16, generator=g).to(dev))


def _state(nets, opt):
    ps = [p for m in nets for p in m.parameters()]
    return [p.detach().clone() for p in ps] + [v.clone() for p in ps for k, v in sorted(opt.state[p].items())]


def _equal(a, b):
    return len(a) == len(b) and all(x.dtype == y.dtype and torch.equal(x, y) for x, y in zip(a, b))


def test_graph_replays_equal_eager_steps_and_follow_a_schedule(dev):
    from uni_renderer_amd.train_step import GraphedTrainStep, train_step

    def run(graphed):
        nets, opt = _nets(dev, 38)
        sch = torch.optim.lr_scheduler.LambdaLR(opt, lambda it: 1.0 / (1.0 + it))
        step = GraphedTrainStep(nets, _batch(dev, 0), opt, dtype=torch.bfloat16, warmup=0) if graphed else None
        first, losses = (step.g_fb if graphed else None), []
        for it in range(3):
            if graphed:
                losses.append(float(step.step(_batch(dev, it))["loss"]))
            else:
                losses.append(train_step(nets, _batch(dev, it), optimizer=opt, dtype=torch.bfloat16)["loss"])
            sch.step()
        assert not graphed or step.g_fb is first, "the step was re-captured although only lr changed"
        assert opt.param_groups[0]["lr"] == 4e-4 / 4
        return losses, _state(nets, opt)

    eager, g1, g2 = run(False), run(True), run(True)
    assert eager[0] == g1[0] == g2[0]
    assert _equal(g1[1], g2[1]), "two identical graphed runs differ"
    assert _equal(eager[1], g1[1]), "three replays are not three eager steps"


def test_checkpoint_round_trip_and_layout_conversions(dev, tmp_path):
    from uni_renderer_amd import checkpointing as C
    from uni_renderer_amd.optim import AdamW8bit, FusedAdamW, dequantize_blockwise
    from uni_renderer_amd.train_step import GraphedTrainStep

    out = str(tmp_path / "run")
    nets_a, opt_a = _nets(dev, 60)
    step_a = GraphedTrainStep(nets_a, _batch(dev, 0), opt_a, dtype=torch.bfloat16, warmup=0)
    loss_a = [float(step_a.step(_batch(dev, it))["loss"]) for it in range(3)]
    want = _state(nets_a, opt_a)

    nets_b, opt_b = _nets(dev, 60)
    step_b = GraphedTrainStep(nets_b, _batch(dev, 0), opt_b, dtype=torch.bfloat16, warmup=0)
    assert [float(step_b.step(_batch(dev, it))["loss"]) for it in range(2)] == loss_a[:2]
    saved = _state(nets_b, opt_b)
    C.save_state(nets_b, out, 2, optimizer=opt_b)
    sd = torch.load(str(tmp_path / "run" / "checkpoint-2" / C.OPTIMIZER_NAME), map_location="cpu")
    ps_b = [p for m in nets_b for p in m.parameters()]
    k8 = next(i for i, p in enumerate(ps_b) if opt_b._is_8bit(p))
    assert sd["state"][k8]["exp_avg"].dtype == torch.uint8 and sd["state"][k8]["exp_avg"].shape == ps_b[k8].shape
    assert sd["state"][k8]["exp_avg_sq_absmax"].shape == (-(-ps_b[k8].numel() // 256),)
    for it in (5, 6):  # training runs on, then the live objects are rolled back
        step_b.step(_batch(dev, it))
    graph, gen = step_b.g_fb, opt_b.generation
    addr = [v.data_ptr() for p in ps_b for k, v in sorted(opt_b.state[p].items())]
    assert C.resume_from_checkpoint(nets_b, out, "latest", opt_b) == 2
    assert opt_b.generation == gen and addr == [v.data_ptr() for p in ps_b for k, v in sorted(opt_b.state[p].items())]
    assert _equal(_state(nets_b, opt_b), saved)
    assert float(step_b.step(_batch(dev, 2))["loss"]) == loss_a[2] and step_b.g_fb is graph
    assert _equal(_state(nets_b, opt_b), want)

    # fp32 export -> FusedAdamW
    nets_c, _ = _nets(dev, 60)
    ps_c = [p for m in nets_c for p in m.parameters()]
    opt_c = FusedAdamW(ps_c, lr=4e-4, betas=(0.9, 0.99), weight_decay=1e-2)
    opt_c.load_state_dict(opt_b.dequantized_state_dict())
    for pb, pc in zip(ps_b, ps_c):
        sb, sc = opt_b.state[pb], opt_c.state[pc]
        assert sc["exp_avg"].dtype == sc["exp_avg_sq"].dtype == torch.float32 and float(sc["step"]) == 3.0
        if opt_b._is_8bit(pb):
            assert torch.equal(sc["exp_avg"], dequantize_blockwise(sb["exp_avg"], sb["exp_avg_absmax"], True))
            assert torch.equal(sc["exp_avg_sq"], dequantize_blockwise(sb["exp_avg_sq"], sb["exp_avg_sq_absmax"], False))
        else:
            assert torch.equal(sc["exp_avg"], sb["exp_avg"]) and torch.equal(sc["exp_avg_sq"], sb["exp_avg_sq"])
    # a FusedAdamW state dict -> AdamW8bit: quantised on load; decodes to within half the widest gap of each book (section 1
    # of the scheme: 0.00703 / 0.00352 of the block's absmax, + 1e-7 for the fp32 entries)
    nets_d, opt_d = _nets(dev, 61)
    ps_d = [p for m in nets_d for p in m.parameters()]
    gen = opt_d.generation
    opt_d.load_state_dict(opt_c.state_dict())
    assert opt_d.generation == gen + 1  # fresh optimizer: the state tensors are new
    for pc, pd in zip(ps_c, ps_d):
        sc, sd_ = opt_c.state[pc], opt_d.state[pd]
        assert float(sd_["step"]) == 3.0
        if not opt_d._is_8bit(pd):
            assert torch.equal(sd_["exp_avg"], sc["exp_avg"]) and torch.equal(sd_["exp_avg_sq"], sc["exp_avg_sq"])
            continue
        for key, signed, bound in (("exp_avg", True, 0.00703125), ("exp_avg_sq", False, 0.003515625)):
            assert sd_[key].dtype == torch.uint8 and sd_[key].shape == pd.shape
            am = sd_[key + "_absmax"]
            x = sc[key].reshape(-1).double()
            blocks = torch.nn.functional.pad(x.abs(), (0, am.numel() * 256 - x.numel())).reshape(-1, 256)
            assert torch.equal(am.double(), blocks.max(dim=1).values)
            err = (dequantize_blockwise(sd_[key], am, signed).reshape(-1).double() - x).abs()
            assert bool((err <= (bound + 1e-6) * am.double().repeat_interleave(256)[:x.numel()]).all()), key
