// Direct 3x3 convolution (pad 1, stride 1 | 2) over NHWC maps with FEW channels: the seven narrow layers of diffusers'
// ControlNetConditioningEmbedding (3 -> 16 -> 16 -> 32 -> 32 -> 96 -> 96 -> 256 at 512^2 ... 64^2; reference
// models/controlnet.py, `controlnet_cond_embedding`).  ur_igemm walks K in 64-channel chunks and 64-column tiles, so it
// would move 4x / 2x the bytes of a 16- / 32-channel map and multiply mostly zeros; here K is walked in chunks of CC = 8
// (image), 16 or 32 channels and N in blocks of 16.
//
// One workgroup (4 waves) owns a 16 x 16 rectangle of output pixels of one sample and ALL output channels:
//   for each pass of up to 6 blocks of 16 output channels (96 channels: the accumulators of a wave, 4 x 6 MFMA tiles)
//     for each chunk of CC input channels
//       stage   the input rectangle with its halo, (15 S + 3)^2 pixels x CC channels, into LDS -- every element comes from
//               global memory once per pass, taps outside the image are zero-filled here (the sample index is fixed per
//               workgroup, so a halo row never comes from the neighbouring sample) -- and beside it the packed weights of
//               (pass, chunk), a contiguous run per block of 16 output channels;
//       multiply  wave w owns output rows 4 w .. 4 w + 3 of the rectangle (one row of 16 pixels = one MFMA column block).
//               v_mfma_f32_16x16x32: A = weights [16 output channels][32 k], B = input [32 k][16 pixels], so a lane ends up
//               with 4 CONSECUTIVE output channels of one pixel (an 8-byte store).  k runs over (tap, channel) of the
//               chunk, k = tap * CC + c, padded with zero weights to a multiple of 32 (CC = 16: 144 -> 160, CC = 8:
//               72 -> 96); a lane's 8 consecutive k are 8 consecutive channels of one tap = one 16-byte LDS read.
//     epilogue  + bias (fp32), optional SiLU (fp32), ONE rounding to the storage type.
// LDS: stride 1 / CC = 32: 20.3 KB input + 54 KB weights; stride 2 / CC = 16: 34 KB + 30 KB; two workgroups per CU fit in
// every build.  The sums are taken in a fixed order by the MFMA chain (no atomics, no split): a launch is bit-reproducible.
// All global offsets are 64-bit.
#include "ur_launch.h"

namespace ur {

constexpr int CC_TH = 16, CC_TW = 16;  // output pixels of a workgroup
constexpr int CC_NBW = 6;              // blocks of 16 output channels per pass

struct CondConvArgs {
    const void* x;
    const void* w;
    const float* bias;
    void* out;
    int B, H, W, Cin, Cout, Ho, Wo;
    int tiles_x, tiles_y;
    int x_dtype, act;
    int nchunks;  // chunks of CC input channels
};

template <int S, int CC>
struct CondGeom {
    static constexpr int RH = (CC_TH - 1) * S + 3, RW = (CC_TW - 1) * S + 3;  // staged input rectangle
    static constexpr int STEPS = (9 * CC + 31) / 32;                          // MFMA k steps per chunk
    static constexpr int IN_ELEMS = RH * RW * CC;
    static constexpr int W_ELEMS = CC_NBW * STEPS * 512;
    static constexpr int LDS_BYTES = (IN_ELEMS + W_ELEMS) * 2;
    static_assert((IN_ELEMS * 2) % 16 == 0, "the weight image starts 16-byte aligned");
};

// one element of the caller's NCHW image, rounded to the storage type
template <typename T>
__device__ __forceinline__ T cond_img_load(const void* x, int dt, int64_t i) {
    const float f = dt == UR_F32 ? ((const float*)x)[i] : dt == UR_F16 ? (float)((const f16*)x)[i] : (float)((const bf16*)x)[i];
    return (T)f;
}

template <typename T, int S, int CC, bool IMG>
__global__ void __launch_bounds__(256) cond_conv_kernel(const CondConvArgs a) {
    using G = CondGeom<S, CC>;
    typedef typename Vec8<T>::type vec8;
    extern __shared__ __attribute__((aligned(16))) unsigned char cond_smem[];
    T* xs = reinterpret_cast<T*>(cond_smem);  // [RH][RW][CC]
    T* ws = xs + G::IN_ELEMS;                 // [block][step][lane][8]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, m = lane & 15, g = lane >> 4;
    int bid = blockIdx.x;
    const int tx = bid % a.tiles_x;
    bid /= a.tiles_x;
    const int ty = bid % a.tiles_y, b = bid / a.tiles_y;
    const int oy0 = ty * CC_TH, ox0 = tx * CC_TW;
    const int iy0 = oy0 * S - 1, ix0 = ox0 * S - 1;
    const int H = a.H, W = a.W, Cin = a.Cin, Cout = a.Cout;

    // where this lane's 8 k of step kk lie inside the staged rectangle, relative to its pixel's top-left tap
    int aoff[G::STEPS];
    bool aval[G::STEPS];
#pragma unroll
    for (int kk = 0; kk < G::STEPS; ++kk) {
        const int k0 = kk * 32 + 8 * g;
        const int tap = k0 / CC, c = k0 % CC;
        aval[kk] = tap < 9;  // the zero-weight padding of k
        const int t = tap < 9 ? tap : 8;
        aoff[kk] = ((t / 3) * G::RW + t % 3) * CC + c;
    }
    int prow[4];
#pragma unroll
    for (int mi = 0; mi < 4; ++mi) prow[mi] = (((wave * 4 + mi) * S) * G::RW + m * S) * CC;

    const int NB = Cout >> 4;
    const int nsteps = a.nchunks * G::STEPS;
    for (int nb0 = 0; nb0 < NB; nb0 += CC_NBW) {
        const int nbw = NB - nb0 < CC_NBW ? NB - nb0 : CC_NBW;
        f32x4 acc[4][CC_NBW];
#pragma unroll
        for (int mi = 0; mi < 4; ++mi)
#pragma unroll
            for (int n = 0; n < CC_NBW; ++n) acc[mi][n] = f32x4{0.f, 0.f, 0.f, 0.f};

        for (int ch = 0; ch < a.nchunks; ++ch) {
            __syncthreads();  // the previous chunk has been read
            if constexpr (IMG) {
                for (int pix = tid; pix < G::RH * G::RW; pix += 256) {
                    const int r = pix / G::RW, c = pix - r * G::RW;
                    const int iy = iy0 + r, ix = ix0 + c;
                    vec8 v;
#pragma unroll
                    for (int j = 0; j < 8; ++j) v[j] = (T)0.f;
                    if ((unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W) {
                        const int64_t p = ((int64_t)b * Cin * H + iy) * W + ix;
#pragma unroll
                        for (int j = 0; j < 4; ++j)
                            if (j < Cin) v[j] = cond_img_load<T>(a.x, a.x_dtype, p + (int64_t)j * H * W);
                    }
                    *reinterpret_cast<vec8*>(xs + pix * 8) = v;
                }
            } else {
                constexpr int PP = CC / 8;  // 16-byte pieces per pixel
                const T* xg = (const T*)a.x + (int64_t)b * H * W * Cin + ch * CC;
                for (int i = tid; i < G::RH * G::RW * PP; i += 256) {
                    const int pix = i / PP, p = i - pix * PP;
                    const int r = pix / G::RW, c = pix - r * G::RW;
                    const int iy = iy0 + r, ix = ix0 + c;
                    vec8 v;
#pragma unroll
                    for (int j = 0; j < 8; ++j) v[j] = (T)0.f;
                    if ((unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W)
                        v = *reinterpret_cast<const vec8*>(xg + ((int64_t)iy * W + ix) * Cin + p * 8);
                    *reinterpret_cast<vec8*>(xs + i * 8) = v;
                }
            }
            {
                constexpr int PER = G::STEPS * 64;  // 16-byte pieces per block of 16 output channels
                const T* wg = (const T*)a.w + ((int64_t)nb0 * nsteps + ch * G::STEPS) * 512;
                for (int i = tid; i < nbw * PER; i += 256) {
                    const int n = i / PER, q = i - n * PER;
                    *reinterpret_cast<vec8*>(ws + i * 8) = *reinterpret_cast<const vec8*>(wg + ((int64_t)n * nsteps * 64 + q) * 8);
                }
            }
            __syncthreads();

#pragma unroll
            for (int kk = 0; kk < G::STEPS; ++kk) {
                vec8 xb[4];
#pragma unroll
                for (int mi = 0; mi < 4; ++mi) {
                    xb[mi] = *reinterpret_cast<const vec8*>(xs + prow[mi] + aoff[kk]);
                    if constexpr ((9 * CC) % 32 != 0) {
                        if (kk == G::STEPS - 1 && !aval[kk]) {
#pragma unroll
                            for (int j = 0; j < 8; ++j) xb[mi][j] = (T)0.f;
                        }
                    }
                }
#pragma unroll
                for (int n = 0; n < CC_NBW; ++n) {
                    if (n < nbw) {
                        const vec8 wa = *reinterpret_cast<const vec8*>(ws + (n * G::STEPS + kk) * 512 + lane * 8);
#pragma unroll
                        for (int mi = 0; mi < 4; ++mi) acc[mi][n] = mfma16(wa, xb[mi], acc[mi][n]);
                    }
                }
            }
        }

        // lane: output channels (nb0 + n) * 16 + 4 g .. + 3 of pixel (oy0 + 4 wave + mi, ox0 + m)
        const int ox = ox0 + m;
#pragma unroll
        for (int mi = 0; mi < 4; ++mi) {
            const int oy = oy0 + wave * 4 + mi;
            if (oy < a.Ho && ox < a.Wo) {
                T* o = (T*)a.out + (((int64_t)b * a.Ho + oy) * a.Wo + ox) * Cout;
#pragma unroll
                for (int n = 0; n < CC_NBW; ++n) {
                    if (n < nbw) {
                        const int co = (nb0 + n) * 16 + 4 * g;
                        const float4 bi = *reinterpret_cast<const float4*>(a.bias + co);
                        float v[4] = {acc[mi][n][0] + bi.x, acc[mi][n][1] + bi.y, acc[mi][n][2] + bi.z, acc[mi][n][3] + bi.w};
                        T r[4];
#pragma unroll
                        for (int j = 0; j < 4; ++j) r[j] = (T)(a.act == ACT_SILU ? silu_f(v[j]) : v[j]);
                        uint2 pk;
                        __builtin_memcpy(&pk, r, 8);
                        *reinterpret_cast<uint2*>(o + co) = pk;
                    }
                }
            }
        }
    }
}

template <typename T, int S, int CC, bool IMG>
static int cond_conv_launch(const CondConvArgs& a, int blocks, hipStream_t s) {
    static std::atomic<uint64_t> done{0};
    constexpr int lds = CondGeom<S, CC>::LDS_BYTES;
    set_lds_limit_once(done, reinterpret_cast<const void*>(&cond_conv_kernel<T, S, CC, IMG>), lds);
    hipLaunchKernelGGL((cond_conv_kernel<T, S, CC, IMG>), dim3(blocks), dim3(256), lds, s, a);
    return last_error();
}

template <typename T>
static int cond_conv_dispatch(const CondConvArgs& a, int stride, int cc, int blocks, hipStream_t s) {
    if (cc == 8) return stride == 1 ? cond_conv_launch<T, 1, 8, true>(a, blocks, s) : cond_conv_launch<T, 2, 8, true>(a, blocks, s);
    if (cc == 32) return cond_conv_launch<T, 1, 32, false>(a, blocks, s);
    return stride == 1 ? cond_conv_launch<T, 1, 16, false>(a, blocks, s) : cond_conv_launch<T, 2, 16, false>(a, blocks, s);
}

}  // namespace ur

using namespace ur;

extern "C" int ur_cond_conv3x3_kchunk(int Cin, int stride, int x_nchw) {
    if (stride != 1 && stride != 2) return UR_E_UNSUPPORTED;
    if (x_nchw) return Cin >= 1 && Cin <= 4 ? 8 : UR_E_UNSUPPORTED;
    if (Cin <= 0 || (Cin & 15) || Cin > 256) return UR_E_UNSUPPORTED;
    return stride == 2 || (Cin & 31) ? 16 : 32;
}

extern "C" int ur_cond_conv3x3(const void* x, int x_dtype, int x_nchw, const void* w, const float* bias, void* out, int B,
                               int H, int W, int Cin, int Cout, int stride, int act, int dtype, void* stream) {
    if (!x || !w || !bias || !out || B <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0) return UR_E_BADARG;
    if (dtype != UR_DT_F16 && dtype != UR_DT_BF16) return UR_E_BADARG;
    if (x_nchw ? (x_dtype != UR_DT_F16 && x_dtype != UR_DT_BF16 && x_dtype != UR_DT_F32) : x_dtype != dtype) return UR_E_BADARG;
    if (act != UR_ACT_NONE && act != UR_ACT_SILU) return UR_E_BADARG;
    if (((uintptr_t)w | (uintptr_t)bias | (uintptr_t)out) & 15) return UR_E_BADARG;
    if ((uintptr_t)x & (x_nchw ? (x_dtype == UR_DT_F32 ? 3 : 1) : 15)) return UR_E_BADARG;
    const int cc = ur_cond_conv3x3_kchunk(Cin, stride, x_nchw);
    if (cc < 0) return cc;
    if ((Cout & 15) || Cout > 256) return UR_E_UNSUPPORTED;
    CondConvArgs a{};
    a.x = x; a.w = w; a.bias = bias; a.out = out;
    a.B = B; a.H = H; a.W = W; a.Cin = Cin; a.Cout = Cout;
    a.Ho = (H - 1) / stride + 1;
    a.Wo = (W - 1) / stride + 1;
    a.tiles_x = (a.Wo + CC_TW - 1) / CC_TW;
    a.tiles_y = (a.Ho + CC_TH - 1) / CC_TH;
    a.x_dtype = x_dtype; a.act = act;
    a.nchunks = x_nchw ? 1 : Cin / cc;
    const int64_t blocks = (int64_t)B * a.tiles_x * a.tiles_y;
    if (blocks > 0x7fffffff || H > (1 << 24) || W > (1 << 24)) return UR_E_UNSUPPORTED;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    UR_DISPATCH(dtype, return cond_conv_dispatch<T>(a, stride, cc, (int)blocks, st));
}
