"""Float64 restatements for the stochastic-sampler tests: the noise stream of ``ur_sde_update`` (include/ur_kernels.h) and
the textbook forms of the DDIM (eta), DDPM, DPM-Solver++ and SDE-DPM-Solver++ updates.  They share no code with
uni_renderer_amd/schedulers.py: the updates are written as the papers write them (x0 / eps / direction terms, D0 / D1), not
as coefficient rows, and the rows are recovered by probing them with unit inputs."""
import math

import numpy as np

M32 = 0xFFFFFFFF


def philox4x32_10_int(counter, key):
    """Philox4x32-10 on Python integers (Salmon et al., SC'11, Fig. 2 / Random123 philox.h): one counter, one key."""
    c, k = [int(v) & M32 for v in counter], [int(v) & M32 for v in key]
    for r in range(10):
        if r:
            k = [(k[0] + 0x9E3779B9) & M32, (k[1] + 0xBB67AE85) & M32]
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & M32, (p0 >> 32) ^ c[3] ^ k[1], p0 & M32]
    return c


def philox4x32_10_np(c, k0, k1):
    """The same over an [N, 4] uint64 array of counters (32-bit words) with one key."""
    c = [c[:, j].astype(np.uint64) for j in range(4)]
    k0, k1 = np.uint64(k0), np.uint64(k1)
    for r in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & np.uint64(M32), (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & np.uint64(M32)]
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & np.uint64(M32), (k1 + np.uint64(0xBB67AE85)) & np.uint64(M32)
    return np.stack(c, axis=1)


def noise_words(seed: int, step: int, n: int):
    """[ceil(n / 4), 4] output words of the groups of an n-element latent."""
    seed &= 0xFFFFFFFFFFFFFFFF
    g = np.arange((n + 3) // 4, dtype=np.uint64)
    ctr = np.stack([g & np.uint64(M32), g >> np.uint64(32), np.full_like(g, step), np.zeros_like(g)], axis=1)
    return philox4x32_10_np(ctr, seed & M32, seed >> 32)


def normal_f64(seed: int, step: int, n: int, parts: bool = False):
    """float64 [n]: u = ((w >> 8) + 0.5) 2^-24; (z0, z1) = sqrt(-2 ln u0) (cos, sin)(2 pi u1); (z2, z3) from (u2, u3).
    ``parts``: also the radius of every element (what the error bound of the fp32 evaluation scales with)."""
    w = noise_words(seed, step, n)
    u = ((w >> np.uint64(8)).astype(np.float64) + 0.5) / 16777216.0
    z, rr = np.empty((len(w), 4)), np.empty((len(w), 4))
    for a in (0, 2):
        r, t = np.sqrt(-2.0 * np.log(u[:, a])), 2.0 * np.pi * u[:, a + 1]
        z[:, a], z[:, a + 1] = r * np.cos(t), r * np.sin(t)
        rr[:, a] = rr[:, a + 1] = r
    return (z.reshape(-1)[:n], rr.reshape(-1)[:n]) if parts else z.reshape(-1)[:n]


# ---- textbook updates, float64 scalars or arrays ----------------------------------------------------------------
def ddim_update(x, x0, xi, a_t, a_prev, eta):
    """Song et al. 2021 eq. 12 with eq. 16's sigma; a_* = alpha-bar (cumulative products)."""
    eps = (x - math.sqrt(a_t) * x0) / math.sqrt(1 - a_t)
    sigma = eta * math.sqrt((1 - a_prev) / (1 - a_t)) * math.sqrt(1 - a_t / a_prev)
    return math.sqrt(a_prev) * x0 + math.sqrt(1 - a_prev - sigma ** 2) * eps + sigma * xi


def ddpm_update(x, x0, xi, a_t, a_prev, t, variance_type="fixed_small"):
    """Ho et al. 2020 eq. 7 (posterior mean from x0) and eq. 6 / Sec. 3.2 (variance beta-tilde or beta); no noise at t = 0."""
    alpha = a_t / a_prev
    beta = 1 - alpha
    mean = math.sqrt(a_prev) * beta / (1 - a_t) * x0 + math.sqrt(alpha) * (1 - a_prev) / (1 - a_t) * x
    if t == 0:
        return mean
    var = max((1 - a_prev) / (1 - a_t) * beta, 1e-20) if variance_type == "fixed_small" else beta
    return mean + math.sqrt(var) * xi


def alpha_sigma(sigma):
    a = 1.0 / math.sqrt(sigma * sigma + 1.0)
    return a, sigma * a


def dpmpp_update(x, m, m_prev, xi, sig_prev, sig_s, sig_t, order, sde, noise_weight=None):
    """Lu et al. 2022 (arXiv 2211.01095) Algorithm 1 (order 1) / Algorithm 2 (2M) with D0 = m, D1 = (m - m_prev) / r, and
    the SDE variant; sig_* are sigma / alpha ratios of the grid points s' (previous), s (current), t (next)."""
    a_t, s_t = alpha_sigma(sig_t)
    a_s, s_s = alpha_sigma(sig_s)
    lam = lambda sg: math.log(alpha_sigma(sg)[0]) - math.log(alpha_sigma(sg)[1])
    h = lam(sig_t) - lam(sig_s)
    D0, D1 = m, 0.0
    if order == 2:
        r = (lam(sig_s) - lam(sig_prev)) / h
        D1 = (m - m_prev) / r
    if sde:
        nw = s_t * math.sqrt(1 - math.exp(-2 * h)) if noise_weight is None else noise_weight
        return (s_t / s_s) * math.exp(-h) * x + a_t * (1 - math.exp(-2 * h)) * (D0 + 0.5 * D1) + nw * xi
    return (s_t / s_s) * x - a_t * (math.exp(-h) - 1) * (D0 + 0.5 * D1)


def row_of(update):
    """(p0, p1, p2, pn) of a linear ``update(x, m, m_prev, xi)`` by probing it with unit inputs."""
    return tuple(update(*e) for e in ((1.0, 0.0, 0.0, 0.0), (0.0, 1.0, 0.0, 0.0), (0.0, 0.0, 1.0, 0.0), (0.0, 0.0, 0.0, 1.0)))
