"""Minimal sampler used when the caller does not attach diffusers scheduler objects.

The reference attaches eight ``UniPCMultistepScheduler`` instances to the pipeline (eval/test_real.py:485-492)
and BASELINE.json's config 3 names a 50-step DDIM; both come from diffusers, which is not available here.  The
pipeline only needs the diffusers scheduler *protocol* -- ``set_timesteps``, ``timesteps``, ``order``,
``init_noise_sigma``, ``scale_model_input``, ``step(...)[0]``, ``add_noise``.  The schedulers of this module are
restatements of the published algorithms as diffusers 0.24 parameterises them, pinned by properties (parity with
diffusers itself is unpinned): ``DDIMScheduler`` (eta = 0 and eta != 0) with the model's x0 ("sample") prediction
 on the SD scaled-linear beta schedule, ``UniPCMultistepScheduler``, ``DDPMScheduler`` and
``DPMSolverMultistepScheduler`` (DPM-Solver++ 1 / 2M and its SDE variant).  All of them run inside the fused sampling
loop (one update kernel per step: ``ur_ddim_update``, ``ur_unipc_update``, ``ur_sde_update``); an object of another
class that follows the protocol with ``init_noise_sigma == 1`` takes the step-by-step loop.  The Euler / Heun / PNDM
families are refused by name (``NotImplementedError``).  ``device_plan(scheduler, eta)`` is the one description of a
scheduler the pipeline reads: which update kernel, its coefficient table, the timesteps, whether it draws noise, and the
keywords of its ``step``.

Noise: a stochastic sampler inside the pipeline draws from the package's own counter-based stream (``philox_normal``
here, ``ops.sampler_noise`` / ``ur_sde_update`` on the device), keyed by ONE int64 drawn from the caller's generator
per call -- not from ``torch.randn``'s stream.  A ``step`` called directly takes ``variance_noise`` or draws with
``torch.randn(..., generator=generator)``.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Tuple, Union

import torch


def _betas(beta_schedule: str, beta_start: float, beta_end: float, n: int) -> torch.Tensor:
    if beta_schedule == "scaled_linear":
        return torch.linspace(beta_start ** 0.5, beta_end ** 0.5, n, dtype=torch.float32) ** 2
    if beta_schedule == "linear":
        return torch.linspace(beta_start, beta_end, n, dtype=torch.float32)
    raise NotImplementedError(f"beta_schedule {beta_schedule!r}: scaled_linear and linear are implemented")


def _config_of(config):
    c = dict(getattr(config, "config", config))
    return {k: v for k, v in c.items() if not k.startswith("_")}


class _Scheduler:
    """What the four schedulers share: the variance-preserving protocol constants, ``add_noise``, the eps -> x0 conversion,
    the timestep grid of the multistep solvers and ``from_config``."""

    order = 1
    init_noise_sigma = 1.0
    _config_drop: Tuple[str, ...] = ()  # config keys the constructor does not take

    @classmethod
    def from_config(cls, config, **overrides):
        """``config``: a dict (the SD-1.x scheduler config) or a scheduler object of any class of this module."""
        c = {k: v for k, v in _config_of(config).items() if k not in cls._config_drop}
        c.update(overrides)
        return cls(**c)

    def scale_model_input(self, sample: torch.Tensor, timestep=None) -> torch.Tensor:
        return sample

    def add_noise(self, original: torch.Tensor, noise: torch.Tensor, timesteps: torch.Tensor) -> torch.Tensor:
        a = self.alphas_cumprod.to(original.device)[timesteps.long()].to(original.dtype)
        while a.dim() < original.dim():
            a = a[..., None]
        return a.sqrt() * original + (1 - a).sqrt() * noise

    def _to_x0(self, model_output, sample, alpha, sigma):
        """The model's output as an x0 prediction: itself, or (x - sigma eps) / alpha for an eps-predicting model, in fp32
        (float64 for a float64 sample)."""
        if self.prediction_type == "sample":
            return model_output
        cd = torch.float64 if sample.dtype == torch.float64 else torch.float32
        return (sample.to(cd) - sigma * model_output.to(cd)) / alpha

    @staticmethod
    def _alpha_sigma(sigma):
        alpha_t = 1.0 / ((sigma ** 2 + 1.0) ** 0.5)
        return alpha_t, sigma * alpha_t

    def _index_for(self, timestep):
        t = int(torch.as_tensor(timestep).flatten()[0].item())
        idx = (self.timesteps.cpu() == t).nonzero()
        return int(idx[1 if len(idx) > 1 else 0]) if len(idx) else len(self.timesteps) - 1

    def _multistep_timesteps(self, num_inference_steps: int):
        """The int64 numpy grid of UniPC and DPM-Solver++: ``num_inference_steps + 1`` points, the last (t = 0) dropped."""
        import numpy as np

        n_train, sp = self.num_train_timesteps, self.config["timestep_spacing"]
        if sp == "linspace":
            return np.linspace(0, n_train - 1, num_inference_steps + 1).round()[::-1][:-1].copy().astype(np.int64)
        if sp == "leading":
            ratio = n_train // (num_inference_steps + 1)
            ts = (np.arange(0, num_inference_steps + 1) * ratio).round()[::-1][:-1].copy().astype(np.int64)
            return ts + self.config["steps_offset"]
        if sp == "trailing":
            return (np.arange(n_train, 0, -n_train / num_inference_steps).round() - 1).astype(np.int64)
        raise ValueError(sp)


class DDIMScheduler(_Scheduler):
    _config_drop = ("beta_schedule", "clip_sample")  # constants of this class that its config records

    def __init__(self, num_train_timesteps: int = 1000, beta_start: float = 0.00085, beta_end: float = 0.012,
                 prediction_type: str = "sample", steps_offset: int = 1, set_alpha_to_one: bool = False):
        if prediction_type not in ("sample", "epsilon"):
            raise ValueError(prediction_type)
        self.config = dict(num_train_timesteps=num_train_timesteps, beta_start=beta_start, beta_end=beta_end,
                           beta_schedule="scaled_linear", prediction_type=prediction_type, steps_offset=steps_offset,
                           set_alpha_to_one=set_alpha_to_one, clip_sample=False)
        self.num_train_timesteps = num_train_timesteps
        self.prediction_type = prediction_type
        self.steps_offset = steps_offset
        # float64 betas, alphas_cumprod rounded to fp32 (the other classes build theirs in fp32: _betas)
        betas = torch.linspace(beta_start ** 0.5, beta_end ** 0.5, num_train_timesteps, dtype=torch.float64) ** 2
        self.alphas_cumprod = torch.cumprod(1.0 - betas, dim=0).float()
        self.final_alpha_cumprod = torch.tensor(1.0) if set_alpha_to_one else self.alphas_cumprod[0]
        self.timesteps = torch.arange(num_train_timesteps - 1, -1, -1)
        self.num_inference_steps = None

    def set_timesteps(self, num_inference_steps: int, device=None):
        self.num_inference_steps = num_inference_steps
        ratio = self.num_train_timesteps // num_inference_steps
        ts = (torch.arange(0, num_inference_steps) * ratio).flip(0) + self.steps_offset
        self.timesteps = ts.clamp_max(self.num_train_timesteps - 1).to(device)

    def _alpha(self, t, device):
        t = torch.as_tensor(t, device="cpu").long().clamp(0, self.num_train_timesteps - 1)
        return self.alphas_cumprod[t].to(device)

    def _alphas_at(self, t: int):
        """(a_t, a_prev) as float64 Python numbers: the fp32 table values, exactly."""
        prev_t = t - self.num_train_timesteps // (self.num_inference_steps or self.num_train_timesteps)
        a_t = float(self._alpha(t, "cpu"))
        a_prev = float(self._alpha(prev_t, "cpu")) if prev_t >= 0 else float(self.final_alpha_cumprod)
        return a_t, a_prev

    def _row64(self, t: int, eta: float):
        """(p0, p1, p2, pn) of ``x_prev = p0 x + p1 x0 + p2 x0_prev + pn xi`` at timestep ``t`` in float64: DDIM (Song et al.
        2021, eq. 12 / 16) with sigma = eta sqrt((1 - a_prev) / (1 - a_t)) sqrt(1 - a_t / a_prev), written for the x0 prediction
        (eps = (x - sqrt(a_t) x0) / sqrt(1 - a_t) substituted)."""
        a_t, a_prev = self._alphas_at(t)
        sigma = float(eta) * ((1 - a_prev) / (1 - a_t)) ** 0.5 * max(1 - a_t / a_prev, 0.0) ** 0.5
        p0 = max(1 - a_prev - sigma * sigma, 0.0) ** 0.5 / (1 - a_t) ** 0.5
        return (p0, a_prev ** 0.5 - a_t ** 0.5 * p0, 0.0, sigma)

    def _sqrt_rows(self) -> torch.Tensor:
        """[n, 4] fp32 rows sqrt(a_t), sqrt(1 - a_t), sqrt(a_prev), sqrt(1 - a_prev) over ``timesteps``: what ``ur_ddim_update``
        consumes at ``eta == 0`` -- the same fp32 torch expressions as ``step``."""
        rows = []
        for t in self.timesteps.cpu().tolist():
            prev_t = int(t) - self.num_train_timesteps // (self.num_inference_steps or self.num_train_timesteps)
            a_t = self._alpha(int(t), "cpu")
            a_prev = self._alpha(prev_t, "cpu") if prev_t >= 0 else self.final_alpha_cumprod.to("cpu")
            rows.append(torch.stack([a_t.sqrt(), (1 - a_t).sqrt(), a_prev.sqrt(), (1 - a_prev).sqrt()]).float())
        return torch.stack(rows)

    def coefficient_table(self, eta: float = 0.0) -> torch.Tensor:
        """[n, 4] fp32 rows (p0, p1, p2, pn) over ``timesteps``: what ``ur_sde_update`` consumes and what ``step`` with
        ``eta != 0`` evaluates (p2 = 0: DDIM is a one-step method).  The fused loop runs ``eta == 0`` on ``ur_ddim_update``."""
        return torch.tensor([self._row64(int(t), eta) for t in self.timesteps.cpu().tolist()], dtype=torch.float32).reshape(-1, 4)

    def step(self, model_output: torch.Tensor, timestep, sample: torch.Tensor, eta: float = 0.0, use_clipped_model_output=False,
             generator=None, variance_noise: Optional[torch.Tensor] = None, return_dict: bool = False, **_):
        """``eta == 0``: the deterministic step, unchanged.  ``eta != 0`` (a restatement of the published algorithm as
        diffusers 0.24 parameterises it; parity with diffusers is unpinned, diffusers is not available here): the fp32 row of
        ``coefficient_table(eta)`` evaluated left to right like ``ur_sde_update``; the noise is ``variance_noise`` if given,
        else ``torch.randn(..., generator=generator)``."""
        t = int(torch.as_tensor(timestep).flatten()[0].item())
        if eta != 0.0:
            if use_clipped_model_output:
                raise NotImplementedError("DDIMScheduler: use_clipped_model_output")
            a_t = self._alphas_at(t)[0]
            m = self._to_x0(model_output, sample, a_t ** 0.5, (1 - a_t) ** 0.5)
            prev = _linear_step(self._row64(t, eta), m, sample, None, generator, variance_noise)
            return (prev,) if not return_dict else {"prev_sample": prev}
        prev_t = t - self.num_train_timesteps // (self.num_inference_steps or self.num_train_timesteps)
        a_t = self._alpha(t, sample.device)
        a_prev = self._alpha(prev_t, sample.device) if prev_t >= 0 else self.final_alpha_cumprod.to(sample.device)
        out = model_output.to(torch.float32)
        x = sample.to(torch.float32)
        if self.prediction_type == "sample":
            x0 = out
            eps = (x - a_t.sqrt() * x0) / (1 - a_t).sqrt()
        else:
            eps = out
            x0 = (x - (1 - a_t).sqrt() * eps) / a_t.sqrt()
        prev = a_prev.sqrt() * x0 + (1 - a_prev).sqrt() * eps
        prev = prev.to(sample.dtype)
        return (prev,) if not return_dict else {"prev_sample": prev}


def retrieve_timesteps(scheduler, num_inference_steps: Optional[int] = None, device=None, timesteps=None, **kw
                       ) -> Tuple[torch.Tensor, int]:
    """models/pipeline.py:80-121."""
    if timesteps is not None:
        scheduler.set_timesteps(timesteps=timesteps, device=device, **kw)
        return scheduler.timesteps, len(scheduler.timesteps)
    scheduler.set_timesteps(num_inference_steps, device=device, **kw)
    return scheduler.timesteps, num_inference_steps


class UniPCMultistepScheduler(_Scheduler):
    """UniPC (Zhao et al. 2023) multistep predictor-corrector, restated from the published algorithm as diffusers 0.24's
    ``UniPCMultistepScheduler`` implements it (the scheduler eval/test_real.py:485-492 attaches eight times and runs for
    20 steps): B(h) variant ``bh2``, data prediction (``predict_x0=True``), ``solver_order`` 2 with first-order warm-up
    and ``lower_order_final``, corrector after every step but the first, ``linspace`` timestep spacing, sigmas
    interpolated from the training schedule.  diffusers itself is not available here, so this restatement
    is pinned by properties only (tests/test_schedulers_cpu.py): exact recovery of x0 under a perfect x0 predictor,
    first step == DDIM, order-2 convergence on a linear ODE, coefficient tables == step-by-step arithmetic.

    ``from_config`` takes the SD-1.x scheduler config (scaled_linear betas 0.00085 .. 0.012, ``prediction_type``
    "sample" for the x0 model).  Every update is a LINEAR combination of tensors with data-independent
    scalar weights; ``coefficient_table()`` exposes them so the pipeline can run the update as one HIP kernel
    (``ur_unipc_update``) inside the step graph."""

    def __init__(self, num_train_timesteps: int = 1000, beta_start: float = 0.00085, beta_end: float = 0.012,
                 beta_schedule: str = "scaled_linear", solver_order: int = 2, prediction_type: str = "sample",
                 predict_x0: bool = True, solver_type: str = "bh2", lower_order_final: bool = True,
                 disable_corrector=(), timestep_spacing: str = "linspace", steps_offset: int = 0, **_ignored):
        if solver_order not in (1, 2) or not predict_x0 or solver_type != "bh2":
            raise NotImplementedError("UniPC: solver_order 1 / 2, predict_x0, bh2 (the diffusers defaults) are implemented")
        if prediction_type not in ("sample", "epsilon"):
            raise ValueError(prediction_type)
        betas = _betas(beta_schedule, beta_start, beta_end, num_train_timesteps)
        self.config = dict(num_train_timesteps=num_train_timesteps, beta_start=beta_start, beta_end=beta_end,
                           beta_schedule=beta_schedule, solver_order=solver_order, prediction_type=prediction_type,
                           predict_x0=predict_x0, solver_type=solver_type, lower_order_final=lower_order_final,
                           disable_corrector=tuple(disable_corrector), timestep_spacing=timestep_spacing,
                           steps_offset=steps_offset)
        self.num_train_timesteps = num_train_timesteps
        self.prediction_type = prediction_type
        self.solver_order = solver_order
        self.alphas_cumprod = torch.cumprod(1.0 - betas, dim=0)
        self.timesteps = torch.arange(num_train_timesteps - 1, -1, -1)
        self.num_inference_steps = None
        self.sigmas = None
        self._reset()

    def _reset(self):
        self.model_outputs = [None] * self.solver_order
        self.lower_order_nums = 0
        self.last_sample = None
        self.this_order = 1
        self._step_index = None

    def set_timesteps(self, num_inference_steps: int, device=None):
        import numpy as np

        ts = self._multistep_timesteps(num_inference_steps)
        ac = self.alphas_cumprod.numpy().astype(np.float64)
        sig = ((1 - ac) / ac) ** 0.5
        sigmas = np.interp(ts, np.arange(0, len(sig)), sig)
        sigma_last = ((1 - ac[0]) / ac[0]) ** 0.5
        self.sigmas = torch.from_numpy(np.concatenate([sigmas, [sigma_last]]).astype(np.float32))
        self.timesteps = torch.from_numpy(ts).to(device=device, dtype=torch.int64)
        self.num_inference_steps = len(ts)
        self._reset()

    def _lambda(self, i):
        a, s = self._alpha_sigma(self.sigmas[i])
        return torch.log(a) - torch.log(s)

    # ---- the data-independent scalars of one update ------------------------------------------------------------
    def _bh_terms(self, i_from: int, i_to: int, order: int, corrector: bool):
        """Scalars of the update from grid point ``i_from`` to ``i_to`` (indices into ``sigmas``):
        returns (sigma_t / sigma_s0, alpha_t * h_phi_1, alpha_t * B_h, rhos) with rhos = the weights of
        [D1(m_{-1}) .. , D1_t]: predictor ``order - 1`` of them, corrector ``order``; and the r_k of the older points."""
        a_t, s_t = self._alpha_sigma(self.sigmas[i_to])
        a_0, s_0 = self._alpha_sigma(self.sigmas[i_from])
        lam_t, lam_0 = torch.log(a_t) - torch.log(s_t), torch.log(a_0) - torch.log(s_0)
        h = lam_t - lam_0
        rks = []
        for k in range(1, order):
            rks.append((self._lambda(i_from - k) - lam_0) / h)
        rks.append(torch.tensor(1.0))
        rks = torch.stack([torch.as_tensor(r).to(h.dtype) for r in rks])
        hh = -h
        h_phi_1 = torch.expm1(hh)
        h_phi_k = h_phi_1 / hh - 1
        B_h = torch.expm1(hh)
        R, b, fact = [], [], 1
        for k in range(1, order + 1):
            R.append(torch.pow(rks, k - 1))
            b.append(h_phi_k * fact / B_h)
            fact *= k + 1
            h_phi_k = h_phi_k / hh - 1 / fact
        R, b = torch.stack(R), torch.stack(b)
        if corrector:
            rhos = torch.tensor([0.5]) if order == 1 else torch.linalg.solve(R, b)
        else:
            rhos = torch.tensor([0.5]) if order == 2 else (torch.linalg.solve(R[:-1, :-1], b[:-1]) if order > 2 else torch.zeros(0))
        return s_t / s_0, a_t * h_phi_1, a_t * B_h, rhos, rks

    def _orders(self):
        """this_order of the predictor at every step index (warm-up + lower_order_final)."""
        n, out, low = self.num_inference_steps, [], 0
        for i in range(n):
            o = min(self.solver_order, n - i) if self.config["lower_order_final"] else self.solver_order
            out.append(min(o, low + 1))
            if low < self.solver_order:
                low += 1
        return out

    def coefficient_table(self) -> torch.Tensor:
        """[n, 8] fp32.  With m_i the (converted) model output of step i, L the corrected sample ("last_sample") and
        x_next the next model input:
            L_i      = c0 * L_{i-1} + c1 * m_{i-1} + c2 * m_{i-2} + c3 * m_i     (step 0: L_0 = the initial sample)
            x_{i+1}  = p0 * L_i     + p1 * m_i     + p2 * m_{i-1}
        row i = (c0, c1, c2, c3, p0, p1, p2, 0)."""
        n, orders = self.num_inference_steps, self._orders()
        rows = []
        for i in range(n):
            c = [1.0, 0.0, 0.0, 0.0]
            if i > 0 and (i - 1) not in self.config["disable_corrector"]:
                o = orders[i - 1]
                ratio, ah1, aB, rhos, rks = self._bh_terms(i - 1, i, o, corrector=True)
                # x = ratio*L - ah1*m0 - aB*(sum_k rho_k (m_k - m0)/r_k + rho_last (m_t - m0))
                c0, c1, c2, c3 = float(ratio), -float(ah1), 0.0, -float(aB * rhos[-1])
                c1 += float(aB * rhos[-1])
                if o == 2:
                    w = float(aB * rhos[0] / rks[0])
                    c2 -= w
                    c1 += w
                c = [c0, c1, c2, c3]
            o = orders[i]
            ratio, ah1, aB, rhos, rks = self._bh_terms(i, i + 1, o, corrector=False)
            p0, p1, p2 = float(ratio), -float(ah1), 0.0
            if o == 2:
                w = float(aB * rhos[0] / rks[0])
                p2 -= w
                p1 += w
            rows.append(c + [p0, p1, p2, 0.0])
        return torch.tensor(rows, dtype=torch.float32)

    # ---- diffusers protocol: one step on tensors ------------------------------------------------------------------
    def convert_model_output(self, model_output, sample):
        return self._to_x0(model_output, sample, *self._alpha_sigma(self.sigmas[self._step_index]))

    def step(self, model_output: torch.Tensor, timestep, sample: torch.Tensor, return_dict: bool = False, **_):
        """One predictor-corrector step.  Arithmetic in fp32 whatever the input dtypes, the two samples (corrected
        ``last_sample``, returned ``prev_sample``) rounded through ``sample.dtype`` -- the precision contract of the
        fused kernel (``ur_unipc_update`` with ``round_master``).  diffusers evaluates the same expressions in the
        tensors' own dtype, i.e. with an fp16 rounding after every op when the model runs in fp16."""
        if self._step_index is None:
            self._step_index = self._index_for(timestep)
        i = self._step_index
        out_dtype = sample.dtype
        cd = torch.float64 if sample.dtype == torch.float64 else torch.float32
        m_t = self.convert_model_output(model_output.to(cd), sample.to(cd))
        sample = sample.to(cd)
        use_corrector = i > 0 and (i - 1) not in self.config["disable_corrector"] and self.last_sample is not None
        if use_corrector:
            o = self.this_order
            ratio, ah1, aB, rhos, rks = self._bh_terms(i - 1, i, o, corrector=True)
            m0 = self.model_outputs[-1]
            x = ratio * self.last_sample - ah1 * m0
            res = rhos[-1] * (m_t - m0)
            if o == 2:
                res = res + rhos[0] * ((self.model_outputs[-2] - m0) / rks[0])
            sample = (x - aB * res).to(out_dtype).to(cd)
        for k in range(self.solver_order - 1):
            self.model_outputs[k] = self.model_outputs[k + 1]
        self.model_outputs[-1] = m_t
        o = min(self.solver_order, len(self.timesteps) - i) if self.config["lower_order_final"] else self.solver_order
        self.this_order = min(o, self.lower_order_nums + 1)
        self.last_sample = sample
        ratio, ah1, aB, rhos, rks = self._bh_terms(i, i + 1, self.this_order, corrector=False)
        x = ratio * sample - ah1 * m_t
        if self.this_order == 2:
            x = x - aB * (rhos[0] * ((self.model_outputs[-2] - m_t) / rks[0]))
        prev = x.to(out_dtype)
        if self.lower_order_nums < self.solver_order:
            self.lower_order_nums += 1
        self._step_index += 1
        return (prev,) if not return_dict else {"prev_sample": prev}


# ---------------------------------------------------------------------------------------------------------------------
# Samplers that are one linear multistep recurrence with a noise term (ur_sde_update):
#     x_{i+1} = p0 x_i + p1 m_i + p2 m_{i-1} + pn xi_i          m_i = the model's x0 prediction at step i
# DDIM with eta, DDPM, DPM-Solver++ (1, 2M) and SDE-DPM-Solver++ (1, 2M).  Each class computes its rows in float64
# (``_rows64``), hands the kernel their fp32 rounding (``coefficient_table``) and evaluates ``step`` from the SAME fp32 row in
# the kernel's order, so that the fused loop and the step-by-step loop agree bit for bit.
# ---------------------------------------------------------------------------------------------------------------------
def _linear_step(row64, m, sample, m_prev, generator, variance_noise):
    """``p0 x + p1 m + p2 m_prev + pn xi``: products added left to right, separate multiply and add (no fma), in fp32 from
    the fp32 rounding of ``row64`` -- float64 from ``row64`` itself when ``sample`` is float64 (the property tests) -- and one
    rounding to ``sample.dtype``.  ``m_prev`` None = zeros.  ``pn == 0``: three terms, no noise drawn."""
    import numpy as np

    f64 = sample.dtype == torch.float64
    cd = torch.float64 if f64 else torch.float32
    p0, p1, p2, pn = (float(v) if f64 else float(np.float32(v)) for v in row64)
    x, m = sample.to(cd), m.to(cd)
    out = p0 * x
    out = out + p1 * m
    out = out + p2 * (torch.zeros_like(m) if m_prev is None else m_prev.to(cd))
    if pn != 0.0:
        if variance_noise is None:
            gdev = generator.device if generator is not None else sample.device
            variance_noise = torch.randn(sample.shape, generator=generator, device=gdev, dtype=cd)
        if tuple(variance_noise.shape) != tuple(sample.shape):
            raise ValueError(f"variance_noise has shape {tuple(variance_noise.shape)}, the sample {tuple(sample.shape)}")
        out = out + pn * variance_noise.to(device=sample.device, dtype=cd)
    return out.to(sample.dtype)


class DDPMScheduler(_Scheduler):
    """DDPM ancestral sampling (Ho et al. 2020, eq. 7 and 11), restated from the published algorithm as diffusers 0.24's
    ``DDPMScheduler`` parameterises it: ``variance_type`` ``fixed_small`` (the posterior variance, clamped at 1e-20) /
    ``fixed_large`` (beta_t), no noise at t = 0, ``leading`` / ``linspace`` / ``trailing`` timestep spacing,
    ``prediction_type`` ``epsilon`` / ``sample``.  diffusers is not available here, so parity with it is unpinned; the class is
    pinned by properties (tests/test_stochastic_samplers_cpu.py): a ``fixed_small`` step == a DDIM eta = 1 step, the marginal
    of a step under a perfect predictor, table == step arithmetic.  This is the noise scheduler the reference's training
    script builds with ``DDPMScheduler.from_pretrained(path, subfolder="scheduler")`` (``add_noise``).

    NOT implemented (``NotImplementedError``): ``clip_sample=True`` (so the default here is False, diffusers' is True),
    ``thresholding``, the learned variance types, ``v_prediction``, custom timestep lists."""

    def __init__(self, num_train_timesteps: int = 1000, beta_start: float = 0.0001, beta_end: float = 0.02,
                 beta_schedule: str = "linear", variance_type: str = "fixed_small", clip_sample: bool = False,
                 prediction_type: str = "epsilon", thresholding: bool = False, timestep_spacing: str = "leading",
                 steps_offset: int = 0, trained_betas=None, **_ignored):
        if variance_type not in ("fixed_small", "fixed_large"):
            raise NotImplementedError(f"DDPMScheduler: variance_type {variance_type!r} (fixed_small / fixed_large are implemented)")
        if clip_sample or thresholding or trained_betas is not None:
            raise NotImplementedError("DDPMScheduler: clip_sample, thresholding and trained_betas are not implemented")
        if prediction_type not in ("sample", "epsilon"):
            raise NotImplementedError(f"DDPMScheduler: prediction_type {prediction_type!r}")
        if timestep_spacing not in ("leading", "linspace", "trailing"):
            raise ValueError(timestep_spacing)
        self.config = dict(num_train_timesteps=num_train_timesteps, beta_start=beta_start, beta_end=beta_end,
                           beta_schedule=beta_schedule, variance_type=variance_type, clip_sample=False,
                           prediction_type=prediction_type, thresholding=False, timestep_spacing=timestep_spacing,
                           steps_offset=steps_offset)
        self.num_train_timesteps = num_train_timesteps
        self.prediction_type = prediction_type
        self.alphas_cumprod = torch.cumprod(1.0 - _betas(beta_schedule, beta_start, beta_end, num_train_timesteps), dim=0)
        self.timesteps = torch.arange(num_train_timesteps - 1, -1, -1)
        self.num_inference_steps = None

    @classmethod
    def from_pretrained(cls, pretrained_model_name_or_path: str, subfolder: Optional[str] = None, **overrides):
        """Reads ``<path>/<subfolder>/scheduler_config.json`` (the diffusers layout)."""
        import json
        import os

        with open(os.path.join(pretrained_model_name_or_path, subfolder or "", "scheduler_config.json")) as f:
            return cls.from_config(json.load(f), **overrides)

    def set_timesteps(self, num_inference_steps: int, device=None):
        import numpy as np

        n_train, sp = self.num_train_timesteps, self.config["timestep_spacing"]
        if num_inference_steps > n_train:
            raise ValueError("num_inference_steps > num_train_timesteps")
        if sp == "linspace":  # n points: not the (n + 1)-point grid of the multistep solvers
            ts = np.linspace(0, n_train - 1, num_inference_steps).round()[::-1].copy().astype(np.int64)
        elif sp == "leading":
            ts = (np.arange(0, num_inference_steps) * (n_train // num_inference_steps)).round()[::-1].copy().astype(np.int64)
            ts += self.config["steps_offset"]
        else:
            ts = (np.round(np.arange(n_train, 0, -n_train / num_inference_steps)) - 1).astype(np.int64)
        self.num_inference_steps = num_inference_steps
        self.timesteps = torch.from_numpy(ts).to(device)

    def _row64(self, t: int):
        ac = self.alphas_cumprod
        prev_t = t - self.num_train_timesteps // (self.num_inference_steps or self.num_train_timesteps)
        a_t = float(ac[t])
        a_prev = float(ac[prev_t]) if prev_t >= 0 else 1.0
        cur_alpha = a_t / a_prev
        cur_beta = 1 - cur_alpha
        p1 = a_prev ** 0.5 * cur_beta / (1 - a_t)               # weight of the predicted x0 (eq. 7)
        p0 = cur_alpha ** 0.5 * (1 - a_prev) / (1 - a_t)        # weight of the current sample
        pn = 0.0
        if t > 0:
            var = max((1 - a_prev) / (1 - a_t) * cur_beta, 1e-20) if self.config["variance_type"] == "fixed_small" else cur_beta
            pn = var ** 0.5
        return (p0, p1, 0.0, pn)

    def coefficient_table(self) -> torch.Tensor:
        """[n, 4] fp32 rows (p0, p1, 0, pn) over ``timesteps`` for ``ur_sde_update``."""
        return torch.tensor([self._row64(int(t)) for t in self.timesteps.cpu().tolist()], dtype=torch.float32).reshape(-1, 4)

    def step(self, model_output: torch.Tensor, timestep, sample: torch.Tensor, generator=None,
             variance_noise: Optional[torch.Tensor] = None, return_dict: bool = False, **_):
        t = int(torch.as_tensor(timestep).flatten()[0].item())
        a_t = float(self.alphas_cumprod[t])
        m = self._to_x0(model_output, sample, a_t ** 0.5, (1 - a_t) ** 0.5)
        prev = _linear_step(self._row64(t), m, sample, None, generator, variance_noise)
        return (prev,) if not return_dict else {"prev_sample": prev}


class DPMSolverMultistepScheduler(_Scheduler):
    """DPM-Solver++ (Lu et al. 2022, arXiv 2211.01095: Algorithm 1 = first order, Algorithm 2 = 2M) and its SDE variant
    (Sec. 5 / eq. 18 of the same paper's v2), restated from the published algorithms as diffusers 0.24's
    ``DPMSolverMultistepScheduler`` parameterises them: data prediction, ``algorithm_type`` ``dpmsolver++`` /
    ``sde-dpmsolver++``, ``solver_order`` 1 / 2 with ``solver_type="midpoint"``, first-order warm-up, ``lower_order_final``
    (the last step of a loop of fewer than 15 steps is first order), ``use_karras_sigmas`` (Karras et al. 2022, rho = 7; the
    last sigma is repeated as in 0.24, so the last step is the identity), ``timestep_spacing`` as UniPC has it.  diffusers is
    not available here, so parity with it is unpinned; the class is pinned by properties
    (tests/test_stochastic_samplers_cpu.py): order 1 == DDIM, order-2 convergence on the Gaussian flow, the marginal of an SDE
    step under a perfect predictor, table == step arithmetic.

    With lambda = log(alpha / sigma), h = lambda_t - lambda_s, r = (lambda_s - lambda_s') / h, m the newest and m' the previous
    x0 prediction:
        dpmsolver++       x_t = (sigma_t / sigma_s) x        + alpha_t (1 - e^-h)  [m + (m - m') / (2 r)]
        sde-dpmsolver++   x_t = (sigma_t / sigma_s) e^-h x   + alpha_t (1 - e^-2h) [m + (m - m') / (2 r)] + sigma_t sqrt(1 - e^-2h) xi
    (first order: without the bracket's second term).  The deterministic variant is the same recurrence with pn = 0.

    NOT implemented (``NotImplementedError``): ``algorithm_type`` ``dpmsolver`` / ``sde-dpmsolver``, ``solver_order`` 3,
    ``solver_type="heun"``, ``euler_at_final``, ``thresholding``, ``lambda_min_clipped``, the learned ``variance_type``s,
    ``v_prediction``."""

    _config_drop = ("predict_x0", "disable_corrector")  # a UniPC config names these; they have no meaning here

    def __init__(self, num_train_timesteps: int = 1000, beta_start: float = 0.0001, beta_end: float = 0.02,
                 beta_schedule: str = "linear", solver_order: int = 2, prediction_type: str = "epsilon",
                 thresholding: bool = False, algorithm_type: str = "dpmsolver++", solver_type: str = "midpoint",
                 lower_order_final: bool = True, euler_at_final: bool = False, use_karras_sigmas: bool = False,
                 lambda_min_clipped: float = -float("inf"), variance_type=None, timestep_spacing: str = "linspace",
                 steps_offset: int = 0, trained_betas=None, **_ignored):
        if algorithm_type not in ("dpmsolver++", "sde-dpmsolver++"):
            raise NotImplementedError(f"DPMSolverMultistepScheduler: algorithm_type {algorithm_type!r} "
                                      "(dpmsolver++ / sde-dpmsolver++ are implemented)")
        if solver_order not in (1, 2):
            raise NotImplementedError("DPMSolverMultistepScheduler: solver_order 1 / 2 are implemented")
        if solver_type != "midpoint":
            raise NotImplementedError(f"DPMSolverMultistepScheduler: solver_type {solver_type!r} (midpoint is implemented)")
        if euler_at_final or thresholding or variance_type is not None or trained_betas is not None \
                or lambda_min_clipped != -float("inf"):
            raise NotImplementedError("DPMSolverMultistepScheduler: euler_at_final, thresholding, learned variance types, "
                                      "trained_betas and lambda_min_clipped are not implemented")
        if prediction_type not in ("sample", "epsilon"):
            raise NotImplementedError(f"DPMSolverMultistepScheduler: prediction_type {prediction_type!r}")
        if timestep_spacing not in ("leading", "linspace", "trailing"):
            raise ValueError(timestep_spacing)
        self.config = dict(num_train_timesteps=num_train_timesteps, beta_start=beta_start, beta_end=beta_end,
                           beta_schedule=beta_schedule, solver_order=solver_order, prediction_type=prediction_type,
                           algorithm_type=algorithm_type, solver_type=solver_type, lower_order_final=lower_order_final,
                           use_karras_sigmas=use_karras_sigmas, timestep_spacing=timestep_spacing, steps_offset=steps_offset)
        self.num_train_timesteps = num_train_timesteps
        self.prediction_type = prediction_type
        self.solver_order = solver_order
        self.alphas_cumprod = torch.cumprod(1.0 - _betas(beta_schedule, beta_start, beta_end, num_train_timesteps), dim=0)
        self.timesteps = torch.arange(num_train_timesteps - 1, -1, -1)
        self.num_inference_steps = None
        self.sigmas = None
        self._reset()

    @classmethod
    def from_config(cls, config, **overrides):
        c = _config_of(config)
        if c.get("solver_type") in ("bh1", "bh2"):  # UniPC's B(h) variant, not a DPM-Solver type
            del c["solver_type"]
        return super().from_config(c, **overrides)

    def _reset(self):
        self._m_prev = None
        self._step_index = None

    def set_timesteps(self, num_inference_steps: int, device=None):
        import numpy as np

        ts = self._multistep_timesteps(num_inference_steps)
        ac = self.alphas_cumprod.numpy().astype(np.float64)
        sig = ((1 - ac) / ac) ** 0.5
        if self.config["use_karras_sigmas"]:
            rho, ramp = 7.0, np.linspace(0, 1, num_inference_steps)
            lo, hi = sig[0] ** (1 / rho), sig[-1] ** (1 / rho)
            sigmas = (hi + ramp * (lo - hi)) ** rho
            # the (fractional, then rounded) training timestep of each sigma: linear interpolation in log sigma
            ts = np.interp(np.log(np.maximum(sigmas, 1e-10)), np.log(sig), np.arange(len(sig))).round().astype(np.int64)
            sigmas = np.concatenate([sigmas, sigmas[-1:]])
        else:
            sigmas = np.concatenate([np.interp(ts, np.arange(0, len(sig)), sig), [sig[0]]])
        self.sigmas = torch.from_numpy(sigmas.astype(np.float32))
        self.timesteps = torch.from_numpy(ts).to(device=device, dtype=torch.int64)
        self.num_inference_steps = len(ts)
        self._reset()

    def _orders(self):
        """The order of the update at every step index (first-order warm-up, lower_order_final)."""
        n, out = self.num_inference_steps, []
        for i in range(n):
            final = i == n - 1 and self.config["lower_order_final"] and n < 15
            out.append(1 if (self.solver_order == 1 or i < 1 or final) else 2)
        return out

    def _rows64(self):
        import math

        sde = self.config["algorithm_type"] == "sde-dpmsolver++"
        sg = [float(s) for s in self.sigmas.double().tolist()]
        lam = lambda s: -math.log(s)  # log(alpha / sigma_t) = -log(sigma) with alpha = 1 / sqrt(sigma^2 + 1), sigma_t = sigma alpha
        rows = []
        for i, o in enumerate(self._orders()):
            a_t, s_t = self._alpha_sigma(sg[i + 1])
            _, s_0 = self._alpha_sigma(sg[i])
            h = lam(sg[i + 1]) - lam(sg[i])
            if h == 0.0:  # the repeated last sigma of the Karras grid: the identity
                rows.append((1.0, 0.0, 0.0, 0.0))
                continue
            if sde:
                p0, d0, pn = s_t / s_0 * math.exp(-h), a_t * -math.expm1(-2.0 * h), s_t * (-math.expm1(-2.0 * h)) ** 0.5
            else:
                p0, d0, pn = s_t / s_0, a_t * -math.expm1(-h), 0.0
            p1, p2 = d0, 0.0
            if o == 2:
                r = (lam(sg[i]) - lam(sg[i - 1])) / h
                w = 0.5 * d0 / r  # weight of D1 = (m - m') / r
                p1, p2 = d0 + w, -w
            rows.append((p0, p1, p2, pn))
        return rows

    def coefficient_table(self) -> torch.Tensor:
        """[n, 4] fp32 rows (p0, p1, p2, pn) for ``ur_sde_update``; pn = 0 throughout for ``dpmsolver++``."""
        return torch.tensor(self._rows64(), dtype=torch.float32).reshape(-1, 4)

    def step(self, model_output: torch.Tensor, timestep, sample: torch.Tensor, generator=None,
             variance_noise: Optional[torch.Tensor] = None, return_dict: bool = False, **_):
        """One multistep update: the fp32 row of ``coefficient_table`` in the kernel's order, one rounding to
        ``sample.dtype``; the previous x0 prediction is kept in the computation dtype."""
        if self.num_inference_steps is None:
            raise ValueError("DPMSolverMultistepScheduler.step: call set_timesteps first")
        if self._step_index is None:
            self._step_index = self._index_for(timestep)
        i = min(self._step_index, self.num_inference_steps - 1)
        cd = torch.float64 if sample.dtype == torch.float64 else torch.float32
        m = self._to_x0(model_output.to(cd), sample, *self._alpha_sigma(float(self.sigmas[i])))
        prev = _linear_step(self._rows64()[i], m, sample, self._m_prev, generator, variance_noise)
        self._m_prev = m
        self._step_index += 1
        return (prev,) if not return_dict else {"prev_sample": prev}


# ---------------------------------------------------------------------------------------------------------------------
# What the on-device sampling loop needs to know about a scheduler, in one place.
# ---------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class DevicePlan:
    """A scheduler's loop as the update kernels run it.  ``kind``: ``"ddim"`` (``ur_ddim_update``, [n, 4] square-root rows),
    ``"unipc"`` (``ur_unipc_update``, [n, 8]) or ``"sde-<ClassName>"`` (``ur_sde_update``, [n, 4] rows p0 p1 p2 pn); ``coef``:
    that table, fp32 on the CPU; ``tvals``: the timesteps as fp32 [n]; ``noisy``: some row has a noise weight.  Plans are
    shared between calls: read-only."""
    kind: str
    coef: torch.Tensor
    tvals: torch.Tensor
    noisy: bool

    def step_kwargs(self, eta: float, noise) -> dict:
        """The keywords of the scheduler's own ``step`` in a step-by-step loop (the reference's
        ``prepare_extra_step_kwargs``): ``eta`` for DDIM only, the step's noise for the three classes that take it."""
        kw = {}
        if self.kind == "sde-DDIMScheduler":
            kw["eta"] = eta
        if noise is not None and self.kind != "unipc":
            kw["variance_noise"] = noise
        return kw


_PLANS: dict = {}  # schedule -> plan: the eight equal schedulers of a pipeline share one table, and so do its calls


def device_plan(sched, eta: float = 0.0) -> Optional[DevicePlan]:
    """The plan of ``sched`` (after ``set_timesteps``) with DDIM's ``eta``, or None for an object that is not exactly one of
    this module's four classes (subclasses and foreign protocol objects take the step-by-step loop).  THE place that maps a
    scheduler to its kernel, table and state.  A UniPC table costs milliseconds, so plans are kept per schedule (class,
    config, eta, timesteps, alphas_cumprod / sigmas by value)."""
    cls = type(sched)
    if cls not in (DDIMScheduler, UniPCMultistepScheduler, DDPMScheduler, DPMSolverMultistepScheduler):
        return None
    eta = float(eta) if cls is DDIMScheduler else 0.0
    raw = lambda t: None if t is None else t.detach().cpu().numpy().tobytes()
    key = (cls, eta, sched.num_inference_steps, tuple(sorted(sched.config.items())), raw(sched.timesteps),
           raw(sched.alphas_cumprod), raw(getattr(sched, "sigmas", None)), raw(getattr(sched, "final_alpha_cumprod", None)))
    plan = _PLANS.get(key)
    if plan is None:
        if cls is DDIMScheduler and eta == 0.0:
            kind, coef = "ddim", sched._sqrt_rows()
        elif cls is UniPCMultistepScheduler:
            kind, coef = "unipc", sched.coefficient_table()
        else:
            kind, coef = "sde-" + cls.__name__, (sched.coefficient_table(eta) if cls is DDIMScheduler else sched.coefficient_table())
        noisy = kind.startswith("sde-") and bool((coef[:, 3] != 0).any())
        plan = DevicePlan(kind, coef, sched.timesteps.detach().cpu().to(torch.float32), noisy)
        if len(_PLANS) >= 64:
            _PLANS.clear()
        _PLANS[key] = plan
    return plan


def _refused(name: str, why: str):
    def __init__(self, *a, **k):
        raise NotImplementedError(f"{name}: {why}")

    return type(name, (), {"__init__": __init__, "from_config": classmethod(lambda cls, *a, **k: cls()),
                           "from_pretrained": classmethod(lambda cls, *a, **k: cls()),
                           "__doc__": f"Not implemented: {why}"})


_SIGMA_SPACE = ("works on sigma-scaled inputs (init_noise_sigma != 1, scale_model_input); the sampling loops here keep the "
                "latents in the variance-preserving parameterisation.  DDIM, DDPM, DPM-Solver++ and UniPC are implemented")
EulerDiscreteScheduler = _refused("EulerDiscreteScheduler", _SIGMA_SPACE)
EulerAncestralDiscreteScheduler = _refused("EulerAncestralDiscreteScheduler", _SIGMA_SPACE)
HeunDiscreteScheduler = _refused("HeunDiscreteScheduler", _SIGMA_SPACE)
PNDMScheduler = _refused("PNDMScheduler", "the PNDM / PLMS family is not implemented.  DDIM, DDPM, DPM-Solver++ and UniPC are")


# ---------------------------------------------------------------------------------------------------------------------
# The noise of the stochastic samplers on the host: the stream ur_sde_update / ur_sampler_noise draw on the device, so
# that CPU pipelines and CPU tests see the same numbers (to the fp32 accuracy of the device's log / sqrt / sin / cos).  It is
# the package's own stream, NOT torch.randn's.
# ---------------------------------------------------------------------------------------------------------------------
def philox4x32_10(counter, key):
    """Philox4x32-10 (Salmon et al., SC'11; Random123) in numpy ``uint64``: ``counter`` [..., 4] and ``key`` [..., 2] hold
    32-bit words; returns the four output words [..., 4] as ``uint64``."""
    import numpy as np

    c = np.asarray(counter, dtype=np.uint64) & np.uint64(0xFFFFFFFF)
    k = np.asarray(key, dtype=np.uint64) & np.uint64(0xFFFFFFFF)
    c0, c1, c2, c3 = (c[..., j].copy() for j in range(4))
    k0, k1 = k[..., 0].copy(), k[..., 1].copy()
    M0, M1, W0, W1, MASK, S32 = (np.uint64(v) for v in (0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85, 0xFFFFFFFF, 32))
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2  # 32 x 32 -> 64 bits: exact in uint64
        c0, c1, c2, c3 = (p1 >> S32) ^ c1 ^ k0, p1 & MASK, (p0 >> S32) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return np.stack(np.broadcast_arrays(c0, c1, c2, c3), axis=-1)


def philox_normal(seed: int, step: int, shape) -> torch.Tensor:
    """fp32 CPU tensor of ``shape``: the standard normals ``ur_sde_update`` draws at step ``step`` under ``seed`` for a latent
    of that logical contiguous shape (include/ur_kernels.h: group g = e // 4, counter (g lo, g hi, step, 0), key (seed lo,
    seed hi), u = ((w >> 8) + 0.5) 2^-24, Box-Muller on (w0, w1) and (w2, w3)), evaluated in float64."""
    import numpy as np

    n = 1
    for d in shape:
        n *= int(d)
    seed, groups = int(seed) & 0xFFFFFFFFFFFFFFFF, (n + 3) // 4
    g = np.arange(groups, dtype=np.uint64)
    ctr = np.stack([g & np.uint64(0xFFFFFFFF), g >> np.uint64(32), np.full(groups, int(step), dtype=np.uint64),
                    np.zeros(groups, dtype=np.uint64)], axis=-1)
    w = philox4x32_10(ctr, np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64))
    u = ((w >> np.uint64(8)).astype(np.float64) + 0.5) * 2.0 ** -24
    r0, r1 = np.sqrt(-2.0 * np.log(u[:, 0])), np.sqrt(-2.0 * np.log(u[:, 2]))
    t0, t1 = 2.0 * np.pi * u[:, 1], 2.0 * np.pi * u[:, 3]
    z = np.stack([r0 * np.cos(t0), r0 * np.sin(t0), r1 * np.cos(t1), r1 * np.sin(t1)], axis=-1).reshape(-1)[:n]
    return torch.from_numpy(z.astype(np.float32)).reshape(tuple(int(d) for d in shape))
