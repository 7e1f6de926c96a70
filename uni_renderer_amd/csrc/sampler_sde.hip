// Stochastic sampler update with the noise drawn on the device (include/ur_kernels.h, ur_sde_update / ur_sampler_noise).
//
// A sampling loop is replays of one captured graph (step + update kernel + ur_sampler_advance), so the noise of step i can
// come neither from the host nor from an RNG launch whose state the graph does not own.  Here it is a pure FUNCTION of
// (seed, step, element index): a counter-based generator (Philox4x32-10, Salmon et al., SC'11) keyed by a seed the kernel reads
// from device memory and counted by the device-side step counter the loop already has.  Nothing of it is baked into a graph.
//
// Update, for an x0-predicting model (schedulers.py: DDIM with eta, DDPM, DPM-Solver++ 1 / 2M and their SDE variants all
// reduce to it; coefficient_table() row i = p0 p1 p2 pn):
//     m_i     = pred at step i (after the classifier-free-guidance combine, in the prediction's dtype)
//     x_{i+1} = p0 * x_i + p1 * m_i + p2 * m_{i-1} + pn * xi_i
// evaluated in fp32, the products added left to right WITHOUT fma contraction, so the host scheduler's torch expression gives
// the same bits.  A row with pn == 0 has three terms: it draws nothing and does not read the seed.
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
//
// Mapping: one thread owns one Philox group = 4 consecutive logical elements.  HW need not be a multiple of 4, so a group may
// straddle two channel planes (or two samples): every element computes its own (b, c, p) and its own lat / pred address.
#include "ur_launch.h"

namespace ur {

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
            const int p = (int)(i % HW);
            const int64_t bc = i / HW;
            const int c = (int)(bc % C), b = (int)(bc / C);
            T mt = pred[((int64_t)b * HW + p) * pred_ld + pred_c0 + c];
            if (cfg && c < cfg_channels) {  // as in ddim_update_kernel: the reference's guidance arithmetic in the prediction's dtype
                const T pu = pred[((int64_t)(b + B) * HW + p) * pred_ld + pred_c0 + c];
                const T d = (T)((float)mt - (float)pu);
                const T m = (T)((float)d * guidance);
                mt = (T)((float)pu + (float)m);
            }
            const float m = (float)mt;
            float x = p0 * master[i];
            x = x + p1 * m;
            x = x + p2 * hist[i];
            if (noisy) x = x + pn * z[j];
            const T xt = (T)x;
            master[i] = round_master ? (float)xt : x;
            hist[i] = m;
            T* xp = lat + (int64_t)b * lat_bs + (int64_t)c * HW + p;
            *xp = xt;
            if (cfg) xp[(int64_t)B * lat_bs] = xt;  // the uncond half of the next input is the same latent
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
