"""Helpers of the LoRA training tests: a float64 reference of ur_lora_grad_multi with its per-element error bound, problem
builders, a launcher over guarded outputs, and the CPU oracle whose UNet holds ``W + s * rscale * up @ down`` as differentiable
expressions of leaf factors."""
import torch

import util_lora as L
from util_models import O  # noqa: F401  (re-exported for the tests)

SHAPES = [(1, 1, 1), (5, 7, 3), (32, 128, 16), (33, 130, 17), (64, 257, 1), (320, 320, 4), (320, 768, 8), (40, 1280, 33)]
DW_DTYPES = [torch.float16, torch.bfloat16, torch.float32]


# ---------------------------------------------------------------------------------------------------------------------
# reference and bound of the factor gradients
# ---------------------------------------------------------------------------------------------------------------------
def ref_grad(dw, up, down, rscale, scale):
    """float64: d_up[n][r] = scale rscale[r] sum_k dw[n][k] down[r][k], d_down[r][k] = scale rscale[r] sum_n up[n][r] dw[n][k],
    and the magnitudes |scale rscale[r]| sum |dw| |factor| the bound is stated in."""
    g, u, d = dw.double().cpu(), up.double().cpu(), down.double().cpu()
    rs = torch.ones(u.shape[1], dtype=torch.float64) if rscale is None else rscale.double().cpu()
    f = scale * rs
    d_up, m_up = (g @ d.t()) * f[None], (g.abs() @ d.abs().t()) * f.abs()[None]
    d_down, m_down = (u.t() @ g) * f[:, None], (u.abs().t() @ g.abs()) * f.abs()[:, None]
    return d_up, d_down, m_up, m_down


def grad_bound(dw, up, down, rscale, scale):
    """Per element ``(n + 3) 2^-24 |scale rscale[r]| sum |dW| |factor|`` with n = K for d_up and n = N for d_down.

    Derivation.  Each result is a sum of n products followed by one scaling.  However the n terms are associated -- a chain
    per thread, a tree across lanes, a chain across waves -- a term passes through at most n roundings on its way to the
    total: one per fma or addition it takes part in, and no tree over n leaves has a path with more than n - 1 additions
    beside the fma that formed the term; additions of the zero padding are exact.  With the unit roundoff u = 2^-24 of fp32
    the accumulated sum therefore differs from the exact one by at most n u sum |dW| |factor| to first order.  Three more
    roundings follow: of ``rscale * up`` where an implementation forms that product first (or of ``scale * rscale``, the
    factor the finished sum is multiplied with), of the scaling itself, and of the store -- each at most u times the
    magnitude.  Together (n + 3) u |scale rscale[r]| sum |dW| |factor|."""
    N, K = dw.shape
    _, _, m_up, m_down = ref_grad(dw, up, down, rscale, scale)
    return (K + 3) * 2.0 ** -24 * m_up, (N + 3) * 2.0 ** -24 * m_down


def int_grad_problem(N, K, R, dtype, seed, scale, rscale_none=False):
    """dw in [-8, 8] (exact in every dtype), up / down in {-1, 0, 1}, rscale in {1, 2}: with scale in {0.5, 2} every partial
    sum stays far below 2^24 in any order, so fp32 arithmetic is exact whatever the summation order."""
    g = torch.Generator().manual_seed(seed)
    dw = torch.randint(-8, 9, (N, K), generator=g).to(dtype)
    up = torch.randint(-1, 2, (N, R), generator=g).float()
    down = torch.randint(-1, 2, (R, K), generator=g).float()
    rscale = None if rscale_none else torch.randint(1, 3, (R,), generator=g).float()
    return dw, up, down, rscale, scale


def rand_grad_problem(N, K, R, dtype, seed, scale):
    g = torch.Generator().manual_seed(seed)
    dw = (torch.randn(N, K, generator=g) * 0.05).to(dtype)
    up = torch.randn(N, R, generator=g)
    down = torch.randn(R, K, generator=g) * 0.1
    rscale = torch.rand(R, generator=g) * 2 - 0.5
    return dw, up, down, rscale, scale


def launch_grad(problems, dtype, dev, dw_offset=None, out_offset=0):
    """One ``lora.grad_items`` call (one launch per lora.multi_max() items) over ``problems`` = (dw, up, down, rscale, scale)
    held on the CPU.  Every d_up / d_down sits in ONE guarded fp32 buffer (L.Guarded), ``out_offset`` elements behind its
    guard; ``dw_offset[i]`` elements shift item i's dw off its allocation's alignment.  Returns ([(d_up, d_down)] on the device, the guard, the device inputs)."""
    from uni_renderer_amd import lora

    guard = L.Guarded(torch.float32, dev)
    for dw, up, down, _, _ in problems:
        guard.reserve(up.numel(), offset=out_offset)
        guard.reserve(down.numel(), offset=out_offset)
    guard.allocate()
    rows, outs, inputs = [], [], []
    for i, (dw, up, down, rscale, scale) in enumerate(problems):
        off = 0 if dw_offset is None else dw_offset[i]
        hold = torch.empty(dw.numel() + off, dtype=dtype, device=dev)
        g = hold[off:].view(dw.shape)
        g.copy_(dw)
        u, d = up.to(dev).contiguous(), down.to(dev).contiguous()
        rs = None if rscale is None else rscale.to(dev).contiguous()
        du, dd = guard.view(2 * i, tuple(up.shape)), guard.view(2 * i + 1, tuple(down.shape))
        rows.append((g, u, d, rs, du, dd, float(scale)))
        outs.append((du, dd))
        inputs.append((g, u, d, rs))
    lora.grad_items(rows, dtype)
    torch.cuda.synchronize()
    return outs, guard, inputs


# ---------------------------------------------------------------------------------------------------------------------
# the oracle with differentiable merged weights
# ---------------------------------------------------------------------------------------------------------------------
def set_up_factors(unet, seed, mag=0.5):
    """Seeded ``up`` factors for the trainable adapter of ``unet``, scaled as util_lora.make_adapter scales them: the update's
    Frobenius norm is ``mag`` times the weight's (with up = 0, d_down is identically zero and would test nothing)."""
    st = unet._lora
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, (down, up, factor) in st.adapters[st.trainable].items():
            w = unet.get_submodule(name).weight.detach().float().cpu()
            u = torch.randn(up.shape, generator=g)
            delta = factor * (u @ down.detach().float().cpu())
            u = u * (mag * w.norm() / delta.norm().clamp_min(1e-12))
            up.copy_(u.to(up.device))


def factors_of(unet):
    """{module name: (down, up, rscale)} of the trainable adapter, fp32 CPU copies."""
    st = unet._lora
    return {n: (d.detach().float().cpu().clone(), u.detach().float().cpu().clone(), float(f))
            for n, (d, u, f) in st.adapters[st.trainable].items()}


def oracle_factor_leaves(factors):
    return {n: (d.clone().requires_grad_(True), u.clone().requires_grad_(True), f) for n, (d, u, f) in factors.items()}


def oracle_unet_call(unet_o, leaves, scale):
    """``unet_o`` as a function whose adapted weights are ``W + scale * rscale * up @ down`` of the leaf factors."""
    params = {k: v.detach() for k, v in unet_o.named_parameters()}
    for n, (d, u, f) in leaves.items():
        w = params[n + ".weight"]
        params[n + ".weight"] = w + (scale * f) * (u @ d).reshape(w.shape)
    buffers = dict(unet_o.named_buffers())
    return lambda *a, **kw: torch.func.functional_call(unet_o, {**params, **buffers}, a, kw)
