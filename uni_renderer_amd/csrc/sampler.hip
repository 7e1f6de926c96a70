// The device side of the sampling loops (include/ur_kernels.h): the three update kernels -- ur_ddim_update (DDIM, eta = 0),
// ur_unipc_update (UniPC), ur_sde_update (DDIM with eta, DDPM, (SDE-)DPM-Solver++, noise drawn on the device) -- with
// ur_sampler_noise and ur_sampler_advance.  A sampling loop is replays of ONE captured graph (step + update kernel +
// ur_sampler_advance): the per-step scalars come from a device table indexed by a device-side step counter, so there is no host
// round trip.  schedulers.device_plan names the kernel of a scheduler and builds its table.
//
// Written once for the three kernels: the element -> (b, c, p) decomposition (elem_of), the classifier-free-guidance combine in
// the prediction's dtype (guided_pred) and the store of the next network input (store_latent).  Their ARITHMETIC stays separate
// and literal, because each reproduces its host scheduler's fp32 expression bit for bit: DDIM's eps / division form and the
// left-to-right adds of ur_sde_update without fma contraction, UniPC's two sums under the compiler's default contraction.
//
// Layout: pred NHWC [B][HW][pred_ld], channels pred_c0 .. pred_c0 + C.  lat NCHW [B][C][HW] with batch stride lat_bs.  The fp32
// state buffers (master, last, hist) are contiguous [B][C][HW]: the reference keeps its latents in the caller's dtype (fp32 in
// eval) between steps and only the network input is rounded to fp16 / bf16.  Under guidance pred / lat hold cond = samples
// [0, B) and uncond = [B, 2B), the state B.
//
// Noise of ur_sde_update: the noise of step i of a replayed graph can come neither from the host nor from an RNG launch whose
// state the graph does not own.  Here it is a pure FUNCTION of (seed, step, element index): a counter-based generator
// (Philox4x32-10, Salmon et al., SC'11) keyed by a seed the kernel reads from device memory and counted by the device-side step
// counter the loop already has.  Nothing of it is baked into a graph.
//
// Noise (normative; tests/util_stochastic.py restates it in numpy): element e of the logical contiguous [B][C][HW] latent
// belongs to group g = e / 4.  Philox4x32-10 with counter (g lo, g hi, step, 0) and key (seed lo, seed hi) gives w0..w3;
// u_k = ((w_k >> 8) + 0.5) * 2^-24 lies in (0, 1); Box-Muller: (z0, z1) = sqrt(-2 ln u_0) * (cos, sin)(2 pi u_1), (z2, z3)
// likewise from (u_2, u_3); element e takes z[e % 4].  Independent of layout, launch geometry and the cond / uncond halves.
//
// Accuracy of the fp32 evaluation: (w >> 8) + 0.5 needs 25 bits.  For the radius that matters near u = 1, where ln u ~ u - 1
// and a rounding of u by 2^-25 would be as large as the result, so ln u is taken from an argument that IS exact in fp32:
//     k = w >> 8 <  2^23:  ln u = logf((2k + 1) * 2^-25)                         (2k + 1 < 2^24)
//     k          >= 2^23:  ln u = log1pf(-(2^25 - 2k - 1) * 2^-25)               (the integer is < 2^24)
// For the angle the rounding of 2 u_1 (relative 2^-24) moves the angle by at most 2 pi 2^-24; sincospif reduces the argument
// exactly.  logf / log1pf / sqrtf / sincospif are the accurate library functions, not the fast intrinsics: this is a few
// thousand elements per step.
#include "ur_launch.h"

namespace ur {

struct Elem { int b, c, p; };  // sample, channel, pixel

// element i of the logical contiguous [B][C][HW] latent
__device__ __forceinline__ Elem elem_of(int64_t i, int C, int HW) {
    const int p = (int)(i % HW);
    const int64_t bc = i / HW;
    return {(int)(bc / C), (int)(bc % C), p};
}

// The prediction of element e.  Channels [0, cfg_channels) under guidance: pred = p_uncond + g * (p_cond - p_uncond) as the
// reference's loop evaluates it in the prediction's dtype, every operation rounded.
template <typename T>
__device__ __forceinline__ T guided_pred(const T* __restrict__ pred, int pred_ld, int pred_c0, Elem e, int B, int HW, int cfg,
                                         float guidance, int cfg_channels) {
#pragma clang fp contract(off)
    T mt = pred[((int64_t)e.b * HW + e.p) * pred_ld + pred_c0 + e.c];
    if (cfg && e.c < cfg_channels) {
        const T pu = pred[((int64_t)(e.b + B) * HW + e.p) * pred_ld + pred_c0 + e.c];
        const T d = (T)((float)mt - (float)pu);
        const T m = (T)((float)d * guidance);
        mt = (T)((float)pu + (float)m);
    }
    return mt;
}

template <typename T>
__device__ __forceinline__ T* latent_ptr(T* lat, int64_t lat_bs, Elem e, int HW) {
    return lat + (int64_t)e.b * lat_bs + (int64_t)e.c * HW + e.p;
}

// the next network input; the uncond half of it is the same latent
template <typename T>
__device__ __forceinline__ void store_latent(T* xp, T v, int cfg, int B, int64_t lat_bs) {
    *xp = v;
    if (cfg) xp[(int64_t)B * lat_bs] = v;
}

// DDIM (eta = 0) for a model that predicts x0 ("sample"), models/pipeline.py:2691-2730 / 1645-1649 of the reference, in the
// operation order of DDIMScheduler.step:
//     eps  = (x - sqrt(a_t) * x0) / sqrt(1 - a_t);   x' = sqrt(a_prev) * x0 + sqrt(1 - a_prev) * eps
// coef row i = (sqrt(a_t), sqrt(1 - a_t), sqrt(a_prev), sqrt(1 - a_prev)).  master is optional: without it x is read from lat.
template <typename T>
__global__ void __launch_bounds__(256) ddim_update_kernel(const T* __restrict__ pred, int pred_ld, int pred_c0,
                                                          T* __restrict__ lat, int64_t lat_bs, int C, int B, int HW,
                                                          const float* __restrict__ coef, const int* __restrict__ step,
                                                          int nsteps, float* __restrict__ master, int round_master,
                                                          int cfg, float guidance, int cfg_channels) {
#pragma clang fp contract(off)
    const int st = min(*step, nsteps - 1);
    const float s_at = coef[4 * st + 0], s_1mat = coef[4 * st + 1], s_ap = coef[4 * st + 2], s_1map = coef[4 * st + 3];
    const int64_t total = (int64_t)B * C * HW;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const Elem e = elem_of(i, C, HW);
        T* xp = latent_ptr(lat, lat_bs, e, HW);
        const float x = master ? master[i] : (float)*xp;
        const float x0 = (float)guided_pred(pred, pred_ld, pred_c0, e, B, HW, cfg, guidance, cfg_channels);
        const float eps = (x - s_at * x0) / s_1mat;
        const float a = s_ap * x0;
        const float ee = s_1map * eps;
        const float v = a + ee;
        store_latent(xp, (T)v, cfg, B, lat_bs);
        if (master) master[i] = round_master ? (float)(T)v : v;
    }
}

// UniPC (order <= 2, x0 / data prediction, B(h) = bh2) predictor-corrector update as ONE pass (schedulers.py
// UniPCMultistepScheduler.coefficient_table): with m_i the model's x0 prediction at step i,
//     L_i     = c0 L_{i-1} + c1 m_{i-1} + c2 m_{i-2} + c3 m_i      corrected sample ("last_sample"; step 0: L_0 = x_0)
//     x_{i+1} = p0 L_i     + p1 m_i     + p2 m_{i-1}               next model input
// coef row i = (c0, c1, c2, c3, p0, p1, p2, -).  `last` holds L, `xmaster` the evolving x (what the loop returns), `hist`
// the two previous predictions in a 2-slot ring indexed by the device step counter (m_{i-1} in slot (i+1)&1, m_{i-2}
// in slot i&1, which m_i then overwrites).  All fp32; with round_master the samples are rounded through the latent dtype
// where the reference's scheduler casts them (`x_t.to(x.dtype)`).  NOT under `fp contract(off)`: the two sums compile
// with the compiler's default contraction, as they always have.
template <typename T>
__global__ void __launch_bounds__(256) unipc_update_kernel(const T* __restrict__ pred, int pred_ld, int pred_c0, T* __restrict__ lat,
                                                           int64_t lat_bs, int C, int B, int HW, const float* __restrict__ coef,
                                                           const int* __restrict__ step, int nsteps, float* __restrict__ last,
                                                           float* __restrict__ xmaster, float* __restrict__ hist, int round_master,
                                                           int cfg, float guidance, int cfg_channels) {
    const int st = min(*step, nsteps - 1);
    const float* cr = coef + (int64_t)st * 8;
    const float c0 = cr[0], c1 = cr[1], c2 = cr[2], c3 = cr[3], p0 = cr[4], p1 = cr[5], p2 = cr[6];
    const int64_t total = (int64_t)B * C * HW;
    float* h1 = hist + (int64_t)((st + 1) & 1) * total;  // m_{i-1}
    float* h2 = hist + (int64_t)(st & 1) * total;        // m_{i-2}, then m_i
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const Elem e = elem_of(i, C, HW);
        const float m = (float)guided_pred(pred, pred_ld, pred_c0, e, B, HW, cfg, guidance, cfg_channels), m1 = h1[i], m2 = h2[i];
        float L = c0 * last[i] + c1 * m1 + c2 * m2 + c3 * m;
        if (round_master) L = (float)(T)L;
        float x = p0 * L + p1 * m + p2 * m1;
        const T xt = (T)x;
        if (round_master) x = (float)xt;
        last[i] = L;
        xmaster[i] = x;
        h2[i] = m;
        store_latent(latent_ptr(lat, lat_bs, e, HW), xt, cfg, B, lat_bs);
    }
}

__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                              uint32_t w[4]) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        const uint32_t n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
        c0 = n0, c1 = lo1, c2 = n2, c3 = lo0;
        k0 += 0x9E3779B9u, k1 += 0xBB67AE85u;
    }
    w[0] = c0, w[1] = c1, w[2] = c2, w[3] = c3;
}

// sqrt(-2 ln u) * (cos, sin)(2 pi v) with u, v the uniforms of the words wu, wv
__device__ __forceinline__ void box_muller(uint32_t wu, uint32_t wv, float& zc, float& zs) {
#pragma clang fp contract(off)
    const uint32_t k = wu >> 8;
    float lnu;
    if (k < (1u << 23))
        lnu = logf((float)(2u * k + 1u) * 0x1p-25f);
    else
        lnu = log1pf(-((float)((1u << 25) - 2u * k - 1u) * 0x1p-25f));
    const float r = sqrtf(-2.0f * lnu);
    const float v2 = ((float)(wv >> 8) + 0.5f) * 0x1p-23f;  // 2 v, in (0, 2]
    float s, c;
    sincospif(v2, &s, &c);
    zc = r * c;
    zs = r * s;
}

// the four normals of group g at step `step` under `seed`: THE noise function, shared by both kernels below
__device__ __forceinline__ void sampler_normal4(int64_t seed, int step, int64_t g, float z[4]) {
    uint32_t w[4];
    philox4x32_10((uint32_t)((uint64_t)g & 0xffffffffu), (uint32_t)((uint64_t)g >> 32), (uint32_t)step, 0u,
                  (uint32_t)((uint64_t)seed & 0xffffffffu), (uint32_t)((uint64_t)seed >> 32), w);
    box_muller(w[0], w[1], z[0], z[1]);
    box_muller(w[2], w[3], z[2], z[3]);
}

// The linear recurrence with a noise term, for an x0-predicting model (schedulers.py: DDIM with eta, DDPM, DPM-Solver++ 1 / 2M
// and their SDE variants all reduce to it; coefficient_table() row i = p0 p1 p2 pn):
//     m_i     = pred at step i (after the guidance combine)
//     x_{i+1} = p0 * x_i + p1 * m_i + p2 * m_{i-1} + pn * xi_i
// evaluated in fp32, the products added left to right WITHOUT fma contraction, so the host scheduler's torch expression gives
// the same bits.  A row with pn == 0 has three terms: it draws nothing and does not read the seed.
// Mapping: one thread owns one Philox group = 4 consecutive logical elements.  HW need not be a multiple of 4, so a group may
// straddle two channel planes (or two samples): every element computes its own (b, c, p) and its own lat / pred address.
template <typename T>
__global__ void __launch_bounds__(256) sde_update_kernel(const T* __restrict__ pred, int pred_ld, int pred_c0, T* __restrict__ lat,
                                                         int64_t lat_bs, int C, int B, int HW, const float* __restrict__ coef,
                                                         const int* __restrict__ step, int nsteps, const int64_t* __restrict__ seed,
                                                         float* __restrict__ master, float* __restrict__ hist, int round_master,
                                                         int cfg, float guidance, int cfg_channels) {
#pragma clang fp contract(off)
    const int st = min(max(*step, 0), nsteps - 1);
    const float* cr = coef + (int64_t)st * 4;
    const float p0 = cr[0], p1 = cr[1], p2 = cr[2], pn = cr[3];
    const bool noisy = pn != 0.0f;
    const int64_t sd = noisy ? *seed : 0;  // a deterministic row never touches the seed
    const int64_t total = (int64_t)B * C * HW;
    const int64_t groups = (total + 3) >> 2;
    for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += (int64_t)gridDim.x * blockDim.x) {
        float z[4] = {0.f, 0.f, 0.f, 0.f};
        if (noisy) sampler_normal4(sd, st, g, z);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int64_t i = 4 * g + j;
            if (i >= total) break;  // the tail group
            const Elem e = elem_of(i, C, HW);
            const float m = (float)guided_pred(pred, pred_ld, pred_c0, e, B, HW, cfg, guidance, cfg_channels);
            float x = p0 * master[i];
            x = x + p1 * m;
            x = x + p2 * hist[i];
            if (noisy) x = x + pn * z[j];
            const T xt = (T)x;
            master[i] = round_master ? (float)xt : x;
            hist[i] = m;
            store_latent(latent_ptr(lat, lat_bs, e, HW), xt, cfg, B, lat_bs);
        }
    }
}

__global__ void __launch_bounds__(256) sampler_noise_kernel(const int64_t* __restrict__ seed, int step, float* __restrict__ out,
                                                            int64_t n) {
    const int64_t sd = *seed;
    const int64_t groups = (n + 3) >> 2;
    for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += (int64_t)gridDim.x * blockDim.x) {
        float z[4];
        sampler_normal4(sd, step, g, z);
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (4 * g + j < n) out[4 * g + j] = z[j];
    }
}

// step += 1; t_out[0..B) = tsteps[step] (the timestep the NEXT replay denoises at)
__global__ void sampler_advance_kernel(int* step, const float* __restrict__ tsteps, int nsteps, float* t_out, int B) {
    // ONE thread reads the counter and shares it through LDS: with every thread reading *step, waves 1-3 could see
    // the value thread 0 had already incremented and write tsteps[st + 1] for the samples beyond the first 64
    __shared__ int st_sh;
    if (threadIdx.x == 0) {
        st_sh = *step + 1;
        *step = st_sh;
    }
    __syncthreads();
    const int st = st_sh;
    if (t_out && (int)threadIdx.x < B) t_out[threadIdx.x] = tsteps[min(st, nsteps - 1)];
}

template <typename T>
static int launch_sde(const void* pred, int pred_ld, int pred_c0, void* lat, int64_t lat_bs, int C, int B, int HW, const float* coef,
                      const int* step, int nsteps, const int64_t* seed, float* master, float* hist, int round_master, int cfg,
                      float guidance, int cfg_channels, hipStream_t s) {
    const int64_t groups = ((int64_t)B * C * HW + 3) >> 2;
    hipLaunchKernelGGL((sde_update_kernel<T>), dim3(grid_for(groups, 2048)), dim3(256), 0, s, (const T*)pred, pred_ld, pred_c0,
                       (T*)lat, lat_bs, C, B, HW, coef, step, nsteps, seed, master, hist, round_master, cfg, guidance, cfg_channels);
    return last_error();
}

}  // namespace ur

using namespace ur;

extern "C" int ur_ddim_update(const void* pred, int pred_ld, int pred_c0, void* lat, int64_t lat_bstride, int C, int B,
                              int HW, const float* coef, const int* step, int nsteps, float* master, int round_master,
                              int cfg, float guidance, int cfg_channels, int dtype, void* stream) {
    if (!pred || !lat || !coef || !step || C <= 0 || B <= 0 || HW <= 0 || nsteps <= 0 || pred_c0 < 0 ||
        pred_c0 + C > pred_ld)
        return UR_E_BADARG;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int grid = grid_for((int64_t)B * C * HW, 2048);
    UR_DISPATCH(dtype, hipLaunchKernelGGL((ddim_update_kernel<T>), dim3(grid), dim3(256), 0, s, (const T*)pred, pred_ld,
                       pred_c0, (T*)lat, lat_bstride, C, B, HW, coef, step, nsteps, master, round_master, cfg, guidance,
                       cfg_channels));
    return last_error();
}

extern "C" int ur_unipc_update(const void* pred, int pred_ld, int pred_c0, void* lat, int64_t lat_bstride, int C, int B,
                               int HW, const float* coef, const int* step, int nsteps, float* last, float* xmaster,
                               float* hist, int round_master, int cfg, float guidance, int cfg_channels, int dtype,
                               void* stream) {
    if (!pred || !lat || !coef || !step || !last || !xmaster || !hist || C <= 0 || B <= 0 || HW <= 0 || nsteps <= 0 ||
        pred_c0 < 0 || pred_c0 + C > pred_ld)
        return UR_E_BADARG;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int grid = grid_for((int64_t)B * C * HW, 2048);
    UR_DISPATCH(dtype, hipLaunchKernelGGL((unipc_update_kernel<T>), dim3(grid), dim3(256), 0, s, (const T*)pred, pred_ld,
                       pred_c0, (T*)lat, lat_bstride, C, B, HW, coef, step, nsteps, last, xmaster, hist, round_master, cfg,
                       guidance, cfg_channels));
    return last_error();
}

extern "C" int ur_sde_update(const void* pred, int pred_ld, int pred_c0, void* lat, int64_t lat_bstride, int C, int B, int HW,
                             const float* coef, const int* step, int nsteps, const int64_t* seed, float* master, float* hist,
                             int round_master, int cfg, float guidance, int cfg_channels, int dtype, void* stream) {
    if (!pred || !lat || !coef || !step || !seed || !master || !hist || C <= 0 || B <= 0 || HW <= 0 || nsteps <= 0 || pred_c0 < 0 ||
        pred_c0 + C > pred_ld || lat_bstride < (int64_t)C * HW || cfg_channels < 0 || cfg_channels > C)
        return UR_E_BADARG;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
#define UR_SDE_ARGS pred, pred_ld, pred_c0, lat, lat_bstride, C, B, HW, coef, step, nsteps, seed, master, hist, round_master, cfg, guidance, cfg_channels, s
    if (dtype == UR_DT_F32) return launch_sde<float>(UR_SDE_ARGS);
    UR_DISPATCH(dtype, return launch_sde<T>(UR_SDE_ARGS));
#undef UR_SDE_ARGS
}

extern "C" int ur_sampler_noise(const int64_t* seed, int step, float* out, int64_t n, void* stream) {
    if (!seed || !out || n <= 0 || step < 0) return UR_E_BADARG;
    hipLaunchKernelGGL(sampler_noise_kernel, dim3(grid_for((n + 3) >> 2, 2048)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                       seed, step, out, n);
    return last_error();
}

extern "C" int ur_sampler_advance(int* step, const float* tsteps, int nsteps, float* t_out, int B, void* stream) {
    if (!step || !tsteps || nsteps <= 0 || B < 0 || B > 256) return UR_E_BADARG;
    hipLaunchKernelGGL(sampler_advance_kernel, dim3(1), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), step, tsteps,
                       nsteps, t_out, B);
    return last_error();
}
