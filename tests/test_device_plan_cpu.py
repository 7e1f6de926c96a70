"""``schedulers.device_plan``: the one place that maps a scheduler object to the update kernel, table and noise flag of the
on-device sampling loop."""
import pytest
import torch

from util_models import ROOT  # noqa: F401  (path setup)
from uni_renderer_amd import schedulers as S

N = 7
KW = dict(prediction_type="sample", beta_schedule="scaled_linear", beta_start=0.00085, beta_end=0.012)


class _SubDDIM(S.DDIMScheduler):
    pass


class _Foreign:
    """Follows the protocol, belongs to nobody."""
    order, init_noise_sigma, prediction_type = 1, 1.0, "sample"

    def __init__(self):
        self.timesteps = torch.arange(N - 1, -1, -1)

    def set_timesteps(self, n, device=None):
        self.timesteps = torch.arange(n - 1, -1, -1)

    def scale_model_input(self, sample, timestep=None):
        return sample

    def step(self, model_output, timestep, sample, **_):
        return (sample,)


CASES = [
    ("ddim-eta0", lambda: S.DDIMScheduler(), 0.0, "ddim", 4, False),
    ("ddim-eta0.5", lambda: S.DDIMScheduler(), 0.5, "sde-DDIMScheduler", 4, True),
    ("unipc", lambda: S.UniPCMultistepScheduler(), 0.0, "unipc", 8, False),
    ("ddpm", lambda: S.DDPMScheduler(steps_offset=1, **KW), 0.0, "sde-DDPMScheduler", 4, True),
    ("dpm++", lambda: S.DPMSolverMultistepScheduler(**KW), 0.0, "sde-DPMSolverMultistepScheduler", 4, False),
    ("sde-dpm++", lambda: S.DPMSolverMultistepScheduler(algorithm_type="sde-dpmsolver++", **KW), 0.0,
     "sde-DPMSolverMultistepScheduler", 4, True),
]


@pytest.mark.parametrize("name,make,eta,kind,width,noisy", CASES, ids=[c[0] for c in CASES])
def test_plan_of_every_scheduler_configuration(name, make, eta, kind, width, noisy):
    s = make()
    s.set_timesteps(N)
    plan = S.device_plan(s, eta)
    assert plan.kind == kind and plan.noisy is noisy
    assert plan.coef.dtype == torch.float32 and plan.coef.device.type == "cpu" and tuple(plan.coef.shape) == (N, width)
    assert plan.tvals.dtype == torch.float32 and torch.equal(plan.tvals, s.timesteps.float())
    if kind.startswith("sde-"):  # the table the scheduler itself steps from
        assert torch.equal(plan.coef, s.coefficient_table(eta) if "eta" in name else s.coefficient_table())
    if kind == "unipc":
        assert torch.equal(plan.coef, s.coefficient_table())
    assert S.device_plan(make_again(make), eta) is plan  # an equal schedule shares its plan ...
    s.set_timesteps(N + 1)
    assert tuple(S.device_plan(s, eta).coef.shape) == (N + 1, width)  # ... another one does not


def make_again(make):
    s = make()
    s.set_timesteps(N)
    return s


def test_subclasses_and_foreign_objects_have_no_plan():
    sub = _SubDDIM()
    sub.set_timesteps(N)
    assert S.device_plan(sub) is None and S.device_plan(sub, 1.0) is None
    assert S.device_plan(_Foreign()) is None and S.device_plan(object()) is None


def test_eta_belongs_to_ddim_only():
    u = S.UniPCMultistepScheduler()
    u.set_timesteps(N)
    assert S.device_plan(u, 0.7) is S.device_plan(u, 0.0)
    d = S.DDIMScheduler()
    d.set_timesteps(N)
    assert S.device_plan(d, 0.7).kind == "sde-DDIMScheduler" and S.device_plan(d, 0.0).kind == "ddim"
    assert not torch.equal(S.device_plan(d, 0.7).coef, S.device_plan(d, 0.3).coef)


def test_step_keywords_come_from_the_plan():
    """``eta`` goes to DDIM only (and only when it is not 0), the step's noise to the three classes that take it."""
    noise = torch.zeros(1)
    kws = {}
    for name, make, eta, *_ in CASES:
        s = make_again(make)
        kws[name] = (S.device_plan(s, eta).step_kwargs(eta, noise), S.device_plan(s, eta).step_kwargs(eta, None))
    assert kws["ddim-eta0"] == ({"variance_noise": noise}, {})
    assert kws["ddim-eta0.5"] == ({"eta": 0.5, "variance_noise": noise}, {"eta": 0.5})
    assert kws["unipc"] == ({}, {})
    for name in ("ddpm", "dpm++", "sde-dpm++"):
        assert kws[name] == ({"variance_noise": noise}, {})


@pytest.mark.parametrize("set_alpha_to_one", [False, True])
@pytest.mark.parametrize("n", [1, 3, 50])
def test_ddim_plan_row_in_the_kernels_order_is_the_scheduler_step(n, set_alpha_to_one):
    """Row i of the ``"ddim"`` plan applied in fp32 in ``ur_ddim_update``'s operation order == ``DDIMScheduler.step``, bit for
    bit, on N(0, 1) data -- including the last step, which reads
    ``final_alpha_cumprod``."""
    s = S.DDIMScheduler(set_alpha_to_one=set_alpha_to_one)
    s.set_timesteps(n)
    plan = S.device_plan(s)
    assert plan.kind == "ddim"
    gen = torch.Generator().manual_seed(n)
    x = torch.randn(2, 4, 5, 7, generator=gen)
    for i, t in enumerate(s.timesteps):
        x0 = torch.randn(2, 4, 5, 7, generator=gen)
        s_at, s_1mat, s_ap, s_1map = plan.coef[i]
        eps = (x - s_at * x0) / s_1mat
        a = s_ap * x0
        e = s_1map * eps
        want = s.step(x0, t, x)[0]
        x = a + e
        assert x.dtype == torch.float32 and torch.equal(x, want), (n, i)
