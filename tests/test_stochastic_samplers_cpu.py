"""CPU tests of the stochastic samplers (uni_renderer_amd/schedulers.py: DDIM with eta, DDPMScheduler,
DPMSolverMultistepScheduler, philox_normal).  diffusers is not available, so the schedulers are pinned by PROPERTIES of the
published algorithms, checked in float64 (a ``step`` on float64 samples uses the float64 rows, not their fp32 rounding),
against the textbook restatements of tests/util_stochastic.py, and the noise stream by Random123's known answers."""
import json
import math

import numpy as np
import pytest
import torch

from util_models import ROOT  # noqa: F401  (path setup)
import util_stochastic as R

F64 = 1e-12  # float64 rounding bound: every quantity below is O(1) and a few dozen operations deep (2^-52 * 100 = 2e-14)

KAT = (((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
       ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
       ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1"))


def test_philox_known_answers():
    from uni_renderer_amd.schedulers import philox4x32_10

    for ctr, key, out in KAT:
        want = [int(w, 16) for w in out.split()]
        assert R.philox4x32_10_int(ctr, key) == want
        assert [int(v) for v in R.philox4x32_10_np(np.array([ctr], dtype=np.uint64), key[0], key[1])[0]] == want
        assert [int(v) for v in philox4x32_10(np.array(ctr, dtype=np.uint64), np.array(key, dtype=np.uint64))] == want


def test_philox_normal_is_the_restated_stream_with_normal_moments():
    from uni_renderer_amd.schedulers import philox_normal

    n = 65536
    z = [R.normal_f64(1234, s, n) for s in range(3)]
    for s in range(3):
        got = philox_normal(1234, s, (4, 16, 32, 32)).double().numpy().reshape(-1)
        assert np.abs(got - z[s]).max() <= 2.0 ** -24 * 6.0  # the float32 rounding of |z| < 5.9
    # shape-independent: an odd size is a prefix (35 = 8 groups + a tail of 3)
    assert np.array_equal(philox_normal(1234, 1, (5, 7)).numpy().reshape(-1), philox_normal(1234, 1, (n,)).numpy()[:35])
    allz = np.concatenate(z)
    N = allz.size
    assert N == 196608
    print("mean", allz.mean(), "std", allz.std())
    assert abs(allz.mean()) <= 4 / math.sqrt(N) and abs(allz.std() - 1) <= 4 / math.sqrt(2 * N)
    assert np.all(z[0] != z[1])
    assert np.abs(allz).max() <= 5.9 and not np.array_equal(R.normal_f64(1235, 0, n), z[0])


# ---- the schedulers under test, on a common schedule ----------------------------------------------------------------
def _ddim(n=10, **kw):
    from uni_renderer_amd.schedulers import DDIMScheduler

    s = DDIMScheduler(**kw)
    s.set_timesteps(n)
    return s


def _ddpm(n=10, **kw):
    from uni_renderer_amd.schedulers import DDPMScheduler

    s = DDPMScheduler(**dict(dict(prediction_type="sample", beta_schedule="scaled_linear", beta_start=0.00085, beta_end=0.012,
                                  steps_offset=1), **kw))
    s.set_timesteps(n)
    return s


def _dpm(n=10, **kw):
    from uni_renderer_amd.schedulers import DPMSolverMultistepScheduler

    s = DPMSolverMultistepScheduler(**dict(dict(prediction_type="sample", beta_schedule="scaled_linear", beta_start=0.00085,
                                                beta_end=0.012), **kw))
    s.set_timesteps(n)
    return s


def _grid(s, i):
    """(alpha, sigma) with x = alpha x0 + sigma eps at the input and at the output of step i."""
    from uni_renderer_amd.schedulers import DDIMScheduler, DDPMScheduler

    if isinstance(s, (DDIMScheduler, DDPMScheduler)):
        t = int(s.timesteps[i])
        prev_t = t - s.num_train_timesteps // s.num_inference_steps
        a_t = float(s.alphas_cumprod[t])
        final = float(s.final_alpha_cumprod) if isinstance(s, DDIMScheduler) else 1.0
        a_p = float(s.alphas_cumprod[prev_t]) if prev_t >= 0 else final
        return (math.sqrt(a_t), math.sqrt(1 - a_t)), (math.sqrt(a_p), math.sqrt(1 - a_p))
    return R.alpha_sigma(float(s.sigmas[i])), R.alpha_sigma(float(s.sigmas[i + 1]))


CASES = [("ddim", dict(eta=0.3)), ("ddim", dict(eta=1.0)), ("ddpm", {}), ("ddpm", dict(variance_type="fixed_large")),
         ("sde1", {}), ("sde2", {})]


@pytest.mark.parametrize("kind,kw", CASES, ids=[c[0] + "".join(f"-{v}" for v in c[1].values()) for c in CASES])
def test_a_step_under_a_perfect_predictor_keeps_the_marginal(kind, kw):
    """x_s = a_s x0 + s_s eps and the model returns x0: every update gives x_t - a_t x0 = s_t (c_e eps + c_n xi).  For the
    samplers whose one-step transition IS the diffusion's (DDIM any eta, DDPM fixed_small, SDE-DPM++) c_e^2 + c_n^2 = 1;
    fixed_large (variance beta_t instead of the posterior's) exceeds 1 by construction and is only checked for c_e."""
    n = 8
    for i in range(n - 1):  # the last step of DDPM (t -> "a_prev = 1") and of DDIM has s_t ~ 0: covered by the table tests
        if kind == "ddim":
            s, step_kw = _ddim(n), dict(eta=kw["eta"])
        elif kind == "ddpm":
            s, step_kw = _ddpm(n, **kw), {}
        else:
            s, step_kw = _dpm(n, algorithm_type="sde-dpmsolver++", solver_order=int(kind[-1])), {}
        x0 = torch.tensor([0.7, -1.3, 0.0, 2.0], dtype=torch.float64)
        res = {}
        for name, (eps, xi) in dict(zero=(0.0, 0.0), e=(1.0, 0.0), n=(0.0, 1.0)).items():
            s.set_timesteps(n)
            for j in range(i + 1):  # walk the multistep history with the perfect predictor
                (a_s, s_s), (a_t, s_t) = _grid(s, j)
                x = a_s * x0 + s_s * eps
                out = s.step(x0, s.timesteps[j], x, variance_noise=torch.full_like(x0, xi), **step_kw)[0]
            res[name] = (out - a_t * x0) / s_t
        assert float(res["zero"].abs().max()) < F64 / s_t
        c_e, c_n = float(res["e"][0]), float(res["n"][0])
        assert float((res["e"] - c_e).abs().max()) < F64 / s_t and float((res["n"] - c_n).abs().max()) < F64 / s_t
        assert c_n > 0 and 0 < c_e < 1
        if kw.get("variance_type") != "fixed_large":
            assert abs(c_e * c_e + c_n * c_n - 1) < 10 * F64 / s_t, (i, c_e, c_n)


def test_ddpm_fixed_small_step_is_a_ddim_eta_one_step():
    n = 10
    d, p = _ddim(n, set_alpha_to_one=True), _ddpm(n)
    p.alphas_cumprod = d.alphas_cumprod  # one table: the classes build theirs in different precisions
    assert d.timesteps.tolist() == p.timesteps.tolist()
    g = torch.Generator().manual_seed(1)
    for i, t in enumerate(d.timesteps):
        x, m, xi = (torch.randn(3, 5, generator=g, dtype=torch.float64) for _ in range(3))
        a = d.step(m, t, x, eta=1.0, variance_noise=xi)[0]
        b = p.step(m, t, x, variance_noise=xi)[0]
        # last step (a_prev = 1): DDIM's sigma is 0, DDPM's is the clamp sqrt(1e-20) = 1e-10
        assert float((a - b).abs().max()) < (F64 if i < n - 1 else 1.01e-10 * float(xi.abs().max()) + F64), i


def test_dpmpp_first_order_is_the_ddim_step_between_the_same_noise_levels():
    s = _dpm(12, solver_order=1)
    g = torch.Generator().manual_seed(2)
    for i, t in enumerate(s.timesteps):
        x, m = torch.randn(3, 5, generator=g, dtype=torch.float64), torch.randn(3, 5, generator=g, dtype=torch.float64)
        (a0, s0), (a1, s1) = _grid(s, i)
        ddim = a1 * m + s1 * (x - a0 * m) / s0
        assert float((s.step(m, t, x)[0] - ddim).abs().max()) < F64 * 20  # |x| / s0 up to ~ 20 at the last grid point


def _flow_error(n, order, s2=0.25, frac=0.8):
    """tests/test_schedulers_cpu.py::_run for DPM-Solver++: the probability-flow ODE of N(0, s2) data over the first
    n * frac steps of an n-step grid against the closed form x_t = x_T std_t / std_T."""
    s = _dpm(n, solver_order=order, lower_order_final=False)
    s.sigmas = s.sigmas.double()
    a0, g0 = R.alpha_sigma(float(s.sigmas[0]))
    x = torch.linspace(-2, 2, 9, dtype=torch.float64) * (a0 * a0 * s2 + g0 * g0) ** 0.5
    x_start, k = x.clone(), int(n * frac)
    for i, t in enumerate(s.timesteps[:k]):
        a, sg = R.alpha_sigma(float(s.sigmas[i]))
        x = s.step(x * (a * s2 / (a * a * s2 + sg * sg)), t, x)[0]
    a1, g1 = R.alpha_sigma(float(s.sigmas[k]))
    exact = x_start * ((a1 * a1 * s2 + g1 * g1) / (a0 * a0 * s2 + g0 * g0)) ** 0.5
    return float((x - exact).abs().max() / exact.abs().max())


def test_dpmpp_2m_converges_with_order_two_on_gaussian_data():
    e = [_flow_error(n, 2) for n in (10, 20, 40)]
    f = [_flow_error(n, 1) for n in (10, 20, 40)]
    print(dict(order2=e, order1=f))
    assert 1.6 < f[0] / f[1] < 2.6 and 1.6 < f[1] / f[2] < 2.6  # first order
    assert e[0] / e[1] > 3.5 and e[1] / e[2] > 3.5              # 2M: second order
    assert e[1] < 0.2 * f[1]


def test_sde_dpmpp_without_its_noise_is_an_exponential_contraction_towards_the_prediction():
    """The restatement with its noise weight forced to 0, a constant prediction x0 and x_s = a_s x0 + s_s eps:
    x_t = a_t x0 + s_t e^-h eps for both orders -- the deterministic part of the SDE step contracts the noise by e^-h (the ODE
    step keeps it: e^0)."""
    s = _dpm(9, algorithm_type="sde-dpmsolver++")
    sg = [float(v) for v in s.sigmas]
    x0, eps = 0.8, -1.1
    for i in range(1, 8):
        for order in (1, 2):
            (a_s, s_s), (a_t, s_t) = R.alpha_sigma(sg[i]), R.alpha_sigma(sg[i + 1])
            h = math.log(a_t / s_t) - math.log(a_s / s_s)
            out = R.dpmpp_update(a_s * x0 + s_s * eps, x0, x0, 123.0, sg[i - 1], sg[i], sg[i + 1], order, True, noise_weight=0.0)
            assert abs(out - (a_t * x0 + s_t * math.exp(-h) * eps)) < F64
            ode = R.dpmpp_update(a_s * x0 + s_s * eps, x0, x0, 123.0, sg[i - 1], sg[i], sg[i + 1], order, False)
            assert abs(ode - (a_t * x0 + s_t * eps)) < F64


# ---- tables ------------------------------------------------------------------------------------------------------
def _schedulers_with_tables(n):
    yield "ddim-eta0.5", _ddim(n), dict(eta=0.5), lambda s: s.coefficient_table(0.5)
    yield "ddim-eta1", _ddim(n), dict(eta=1.0), lambda s: s.coefficient_table(1.0)
    yield "ddpm", _ddpm(n), {}, lambda s: s.coefficient_table()
    yield "ddpm-large", _ddpm(n, variance_type="fixed_large", timestep_spacing="trailing"), {}, lambda s: s.coefficient_table()
    for alg in ("dpmsolver++", "sde-dpmsolver++"):
        for order in (1, 2):
            for karras in (False, True):
                yield (f"{alg}-{order}-{karras}", _dpm(n, algorithm_type=alg, solver_order=order, use_karras_sigmas=karras), {},
                       lambda s: s.coefficient_table())


def _textbook_rows(name, s):
    """The float64 rows of scheduler ``s`` from the textbook updates of util_stochastic (probed with unit inputs)."""
    rows = []
    for i, t in enumerate(s.timesteps.tolist()):
        if name.startswith("dd"):
            ac = s.alphas_cumprod.double()
            prev_t = t - s.num_train_timesteps // s.num_inference_steps
            a_t = float(ac[t])
            if name.startswith("ddim"):
                a_p = float(ac[prev_t]) if prev_t >= 0 else float(s.final_alpha_cumprod)
                eta = float(name.split("eta")[1])
                rows.append(R.row_of(lambda x, m, mp, xi: R.ddim_update(x, m, xi, a_t, a_p, eta)))
            else:
                a_p = float(ac[prev_t]) if prev_t >= 0 else 1.0
                rows.append(R.row_of(lambda x, m, mp, xi: R.ddpm_update(x, m, xi, a_t, a_p, t, s.config["variance_type"])))
        else:
            sg = [float(v) for v in s.sigmas.double()]
            n = len(s.timesteps)
            final = i == n - 1 and n < 15
            order = 1 if (s.solver_order == 1 or i == 0 or final) else 2
            if sg[i + 1] == sg[i]:
                rows.append((1.0, 0.0, 0.0, 0.0))
                continue
            rows.append(R.row_of(lambda x, m, mp, xi: R.dpmpp_update(x, m, mp, xi, sg[i - 1], sg[i], sg[i + 1], order,
                                                                        name.startswith("sde"))))
    return rows


@pytest.mark.parametrize("n", [6, 20])
def test_coefficient_tables_equal_the_step_arithmetic_and_the_textbook_updates(n):
    g = torch.Generator().manual_seed(3)
    for name, s, step_kw, table in _schedulers_with_tables(n):
        tab = table(s)
        assert tab.shape == (n, 4) and tab.dtype == torch.float32 and float(tab[0, 2]) == 0.0, name
        if name.startswith("dpmsolver++") or name.startswith("dd"):
            assert bool((tab[:, 3] == 0).all()) == name.startswith("dpmsolver++"), name
        # (a) the rows are the textbook update's, to float64 rounding before the cast
        want = torch.tensor(_textbook_rows(name, s), dtype=torch.float64)
        assert torch.equal(tab, want.float()) or float((tab.double() - want).abs().max()) < 2.0 ** -23 * float(want.abs().max()), name
        # (b) fp32 samples: step() == the table recurrence in the kernel's order, bit for bit
        x0 = torch.randn(2, 4, 5, 7, generator=g)
        outs = [torch.randn(2, 4, 5, 7, generator=g) for _ in range(n)]
        noise = [torch.randn(2, 4, 5, 7, generator=g) for _ in range(n)]
        xa, xb, m1 = x0.clone(), x0.clone(), torch.zeros_like(x0)
        for i, t in enumerate(s.timesteps):
            xa = s.step(outs[i], t, xa, variance_noise=noise[i], **step_kw)[0]
            p0, p1, p2, pn = (float(v) for v in tab[i])
            xb = p0 * xb
            xb = xb + p1 * outs[i]
            xb = xb + p2 * m1
            if pn != 0:
                xb = xb + pn * noise[i]
            m1 = outs[i]
            assert torch.equal(xa, xb), (name, i)
        # (c) float64 samples run the float64 rows: the fp32 table is their rounding
        s.set_timesteps(n)
        xc, m1 = x0.double(), torch.zeros_like(x0).double()
        xd = x0.double()
        for i, t in enumerate(s.timesteps):
            xc = s.step(outs[i].double(), t, xc, variance_noise=noise[i].double(), **step_kw)[0]
            xd = want[i, 0] * xd + want[i, 1] * outs[i].double() + want[i, 2] * m1 + want[i, 3] * noise[i].double()
            m1 = outs[i].double()
        assert float((xc - xd).abs().max()) < 1e-10 * max(1.0, float(xd.abs().max())), name


def test_ddim_eta_zero_is_todays_ddim_bit_for_bit():
    """``step(eta=0)`` keeps its code path: the expression below is DDIMScheduler.step as it stood before eta existed.  The
    eta = 0 rows of ``coefficient_table`` are the same update as a linear form (to fp32 rounding), with no noise weight."""
    s = _ddim(7)
    g = torch.Generator().manual_seed(4)
    tab = s.coefficient_table()
    assert torch.equal(tab, s.coefficient_table(0.0)) and bool((tab[:, 2:] == 0).all())
    for i, t in enumerate(s.timesteps):
        x, m = torch.randn(2, 4, 8, 8, generator=g), torch.randn(2, 4, 8, 8, generator=g)
        prev_t = int(t) - 1000 // 7
        a_t = s.alphas_cumprod[int(t)]
        a_prev = s.alphas_cumprod[prev_t] if prev_t >= 0 else s.final_alpha_cumprod
        eps = (x - a_t.sqrt() * m) / (1 - a_t).sqrt()
        today = a_prev.sqrt() * m + (1 - a_prev).sqrt() * eps
        for got in (s.step(m, t, x)[0], s.step(m, t, x, eta=0.0, generator=g, variance_noise=torch.ones_like(x))[0]):
            assert torch.equal(got, today)
        lin = float(tab[i, 0]) * x + float(tab[i, 1]) * m
        assert float((lin - today).abs().max()) < 2e-5  # |x| <= 5, |coef| <= ~4 at the noisy end: ~20 x 2^-24 x a few roundings


# ---- plumbing -----------------------------------------------------------------------------------------------------
def test_unsupported_options_are_refused_by_name():
    from uni_renderer_amd import schedulers as S

    for kw in (dict(algorithm_type="dpmsolver"), dict(algorithm_type="sde-dpmsolver"), dict(solver_order=3),
               dict(solver_type="heun"), dict(euler_at_final=True), dict(thresholding=True), dict(variance_type="learned_range"),
               dict(prediction_type="v_prediction"), dict(beta_schedule="squaredcos_cap_v2"), dict(lambda_min_clipped=-5.1)):
        with pytest.raises(NotImplementedError):
            S.DPMSolverMultistepScheduler(**kw)
    for kw in (dict(variance_type="learned"), dict(variance_type="learned_range"), dict(variance_type="fixed_small_log"),
               dict(clip_sample=True), dict(thresholding=True), dict(prediction_type="v_prediction")):
        with pytest.raises(NotImplementedError):
            S.DDPMScheduler(**kw)
    for name in ("EulerDiscreteScheduler", "EulerAncestralDiscreteScheduler", "HeunDiscreteScheduler", "PNDMScheduler"):
        with pytest.raises(NotImplementedError):
            getattr(S, name)()
        with pytest.raises(NotImplementedError):
            getattr(S, name).from_config(S.UniPCMultistepScheduler().config)
    with pytest.raises(NotImplementedError):
        S.DDIMScheduler().step(torch.zeros(1, 4, 2, 2), 981, torch.zeros(1, 4, 2, 2), eta=0.5, use_clipped_model_output=True)


def test_noise_sources_and_argument_checks():
    from uni_renderer_amd import ops
    from uni_renderer_amd import schedulers as S

    s = _ddpm(5)
    x, m = torch.zeros(1, 4, 3, 3), torch.zeros(1, 4, 3, 3)
    t = s.timesteps[0]
    a = s.step(m, t, x, generator=torch.Generator().manual_seed(7))[0]
    b = s.step(m, t, x, generator=torch.Generator().manual_seed(7))[0]
    pn = float(s.coefficient_table()[0, 3])
    want = pn * torch.randn(x.shape, generator=torch.Generator().manual_seed(7))
    assert torch.equal(a, b) and torch.equal(a, want) and pn > 0
    assert torch.equal(s.step(m, t, x, variance_noise=torch.ones_like(x))[0], torch.full_like(x, pn))
    with pytest.raises(ValueError):
        s.step(m, t, x, variance_noise=torch.ones(1, 4, 3, 2))
    # the last DDPM step (t = 0 under "leading" without an offset) draws nothing
    p = S.DDPMScheduler(prediction_type="sample")
    p.set_timesteps(4)
    assert int(p.timesteps[-1]) == 0 and float(p.coefficient_table()[-1, 3]) == 0.0
    g = torch.Generator().manual_seed(9)
    before = g.get_state()
    p.step(m, 0, x, generator=g)
    assert torch.equal(before, g.get_state())
    # epsilon prediction is converted to the data prediction first
    e, q = S.DDPMScheduler(), S.DDPMScheduler(prediction_type="sample")
    e.set_timesteps(5), q.set_timesteps(5)
    g = torch.Generator().manual_seed(10)
    xs, eps, xi = (torch.randn(2, 4, 3, 3, generator=g) for _ in range(3))
    a_t = float(e.alphas_cumprod[int(e.timesteps[1])])
    x0 = (xs - (1 - a_t) ** 0.5 * eps) / a_t ** 0.5
    assert torch.equal(e.step(eps, e.timesteps[1], xs, variance_noise=xi)[0], q.step(x0, q.timesteps[1], xs, variance_noise=xi)[0])
    # the device ops refuse host tensors: there is no CPU fallback of the kernels
    seed = torch.zeros(1, dtype=torch.int64)
    with pytest.raises(RuntimeError):
        ops.sampler_noise(seed, 0, (4,))
    with pytest.raises(RuntimeError):
        ops.sde_update(torch.zeros(1, 2, 2, 4), 0, torch.zeros(1, 4, 2, 2), torch.zeros(1, 4), torch.zeros(1, dtype=torch.int32), 1,
                       seed, torch.zeros(1, 4, 2, 2), torch.zeros(1, 4, 2, 2))


def test_ddpm_from_pretrained_round_trip_and_from_config(tmp_path):
    import uni_renderer_amd as U
    from uni_renderer_amd import schedulers as S

    assert U.DDPMScheduler is S.DDPMScheduler and U.DPMSolverMultistepScheduler is S.DPMSolverMultistepScheduler
    cfg = {"_class_name": "DDPMScheduler", "_diffusers_version": "0.24.0", "beta_end": 0.012, "beta_schedule": "scaled_linear",
           "beta_start": 0.00085, "clip_sample": False, "num_train_timesteps": 1000, "prediction_type": "epsilon",
           "set_alpha_to_one": False, "skip_prk_steps": True, "steps_offset": 1, "trained_betas": None,
           "variance_type": "fixed_small", "timestep_spacing": "leading"}
    (tmp_path / "scheduler").mkdir()
    (tmp_path / "scheduler" / "scheduler_config.json").write_text(json.dumps(cfg))
    s = S.DDPMScheduler.from_pretrained(str(tmp_path), subfolder="scheduler")
    assert s.config["beta_schedule"] == "scaled_linear" and s.config["steps_offset"] == 1 and s.prediction_type == "epsilon"
    again = S.DDPMScheduler.from_config(s.config)
    assert again.config == s.config and torch.equal(again.alphas_cumprod, s.alphas_cumprod)
    # the training use: add_noise at random timesteps == the closed form
    g = torch.Generator().manual_seed(11)
    x0, eps = torch.randn(3, 4, 2, 2, generator=g), torch.randn(3, 4, 2, 2, generator=g)
    ts = torch.tensor([0, 500, 999])
    a = s.alphas_cumprod[ts].reshape(3, 1, 1, 1)
    assert torch.equal(s.add_noise(x0, eps, ts), a.sqrt() * x0 + (1 - a).sqrt() * eps)
    with pytest.raises(NotImplementedError):
        S.DDPMScheduler.from_config(dict(cfg, clip_sample=True))
    # the scheduler class is the caller's choice (X.from_config(pipeline.scheduler.config)): configs carry over
    u = S.UniPCMultistepScheduler()
    d = S.DPMSolverMultistepScheduler.from_config(u.config, algorithm_type="sde-dpmsolver++")
    assert d.prediction_type == "sample" and d.config["beta_schedule"] == "scaled_linear" and d.config["solver_type"] == "midpoint"
    d.set_timesteps(20)
    u.set_timesteps(20)
    assert d.timesteps.tolist() == u.timesteps.tolist() and torch.equal(d.sigmas, u.sigmas)
    k = S.DPMSolverMultistepScheduler.from_config(d.config, use_karras_sigmas=True)
    k.set_timesteps(20)
    assert all(a >= b for a, b in zip(k.timesteps.tolist(), k.timesteps.tolist()[1:])) and float(k.sigmas[-1]) == float(k.sigmas[-2])
    assert S.DDPMScheduler.from_config(S.DDIMScheduler().config).config["beta_schedule"] == "scaled_linear"
