// Backward of the direct narrow-channel 3x3 convolution of condconv.hip (pad 1, stride 1 | 2, NHWC, channels in multiples of
// 16 up to 256): the seven narrow layers of the ControlNet conditioning embedding, whose backward through the 64-channel
// implicit GEMM would save 64-channel activations at 512^2 and write a zero-inserted dy to memory for the stride-2 layers.
//
// INPUT GRADIENT (ur_cond_conv3x3_dgrad).  dx = conv3x3(Z(dy), W_rot), stride 1, where W_rot[c][n][ky][kx] = W[n][c][2 - ky][2 - kx]
// and Z is the zero insertion of a stride-2 layer (Z[2 oy][2 ox] = dy[oy][ox], zero elsewhere; the identity for stride 1).  The
// kernel is the forward's mapping (one workgroup = 16 x 16 pixels of dx of one sample and all input channels in passes of 6
// blocks of 16; K = (tap, dy channel) walked in chunks of CC = 16 | 32 channels; v_mfma_f32_16x16x32 with A = weights, B =
// staged pixels), with ONE difference: the staged 18 x 18 rectangle is filled from dy THROUGH Z -- a position with an odd
// coordinate, or one outside dy, is written as zero in LDS and never read from memory.  So the zero-inserted tensor exists
// only in LDS: dy is read from global memory once per pass, dx is written once.  The parity decomposition (1 / 2 / 2 / 4 taps
// per parity class of dx) was NOT built: it needs four k layouts of the weight image and four pixel mappings of the MFMA
// columns, and what it saves is MFMA time on a kernel whose cost is the traffic of dy and dx (at most 9 * 256 k per 96
// outputs; the zero taps cost 3 / 4 of that MFMA time and no bytes).  Stride 1 is the same kernel with Z = identity.
//
// WEIGHT / BIAS GRADIENT (ur_cond_conv3x3_wgrad).  dw[n][c][tap] = sum over output pixels p of dy[p][n] * x[p * stride + tap - 1][c]:
// both operands are pixel-major, the contraction index is their slow dimension.  A workgroup owns a tile of 32 output channels
// x 32 input channels (x 9 taps) and a contiguous range of UNITS (one unit = 4 output rows x 32 output columns of one sample);
// per unit it stages the dy tile [4][32][n] and the x rectangle with its halo [3 S + 3][31 S + 3][c] into LDS as they lie in
// memory (zero-filled outside the map, so a halo never reads the neighbouring sample) and wave w contracts output row w: the
// MFMA fragments (8 pixels of one channel per lane) are gathered with the LDS transpose read, as in wgrad.hip -- in a 16-lane
// group lane 4 r + q supplies the address of pixel r, channels 4 q .. 4 q + 3 and lane i receives channel i of the 4 pixels --
// so a stride-2 tap is only a different address stride.  A = x^T (rows = input channel), B = dy (columns = output channel): a
// lane ends up with dw[n][4 g .. 4 g + 3][0 .. 8] = 36 CONSECUTIVE floats of the parameter's own layout.  db comes from one
// more MFMA per step with A = ones (workgroups of input-channel tile 0).  The four waves' sums are added in wave order through
// LDS, the workgroup writes ONE fp32 partial per split into the caller's workspace, and a second pass adds the partials in a
// fixed tree into dw / db: no atomics, bit-reproducible for a given `splits`.  All global offsets are 64-bit.
#include "ur_launch.h"

namespace ur {

// =================================================================================================== dgrad
constexpr int CD_TH = 16, CD_TW = 16;  // pixels of dx per workgroup
constexpr int CD_NBW = 6;              // blocks of 16 input channels per pass

struct CondDgradArgs {
    const void* dy;
    const void* w;
    void* dx;
    int B, H, W, Cin, Cout, Ho, Wo;
    int tiles_x, tiles_y;
    int nchunks;  // chunks of CC dy channels
};

template <int CC>
struct CondDgradGeom {
    static constexpr int RH = CD_TH + 2, RW = CD_TW + 2;  // staged rectangle of Z(dy)
    static constexpr int STEPS = (9 * CC + 31) / 32;
    static constexpr int IN_ELEMS = RH * RW * CC;
    static constexpr int W_ELEMS = CD_NBW * STEPS * 512;
    static constexpr int LDS_BYTES = (IN_ELEMS + W_ELEMS) * 2;
    static_assert((IN_ELEMS * 2) % 16 == 0, "the weight image starts 16-byte aligned");
};

template <typename T, int S, int CC>
__global__ void __launch_bounds__(256) cond_dgrad_kernel(const CondDgradArgs a) {
    using G = CondDgradGeom<CC>;
    typedef typename Vec8<T>::type vec8;
    extern __shared__ __attribute__((aligned(16))) unsigned char cond_bwd_smem[];
    T* zs = reinterpret_cast<T*>(cond_bwd_smem);  // [RH][RW][CC]
    T* ws = zs + G::IN_ELEMS;                     // [block][step][lane][8]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, m = lane & 15, g = lane >> 4;
    int bid = blockIdx.x;
    const int tx = bid % a.tiles_x;
    bid /= a.tiles_x;
    const int ty = bid % a.tiles_y, b = bid / a.tiles_y;
    const int y0 = ty * CD_TH, x0 = tx * CD_TW;
    const int H = a.H, W = a.W, Cin = a.Cin, Cout = a.Cout, Ho = a.Ho, Wo = a.Wo;

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
    for (int mi = 0; mi < 4; ++mi) prow[mi] = ((wave * 4 + mi) * G::RW + m) * CC;

    const int NB = Cin >> 4;
    const int nsteps = a.nchunks * G::STEPS;
    for (int nb0 = 0; nb0 < NB; nb0 += CD_NBW) {
        const int nbw = NB - nb0 < CD_NBW ? NB - nb0 : CD_NBW;
        f32x4 acc[4][CD_NBW];
#pragma unroll
        for (int mi = 0; mi < 4; ++mi)
#pragma unroll
            for (int n = 0; n < CD_NBW; ++n) acc[mi][n] = f32x4{0.f, 0.f, 0.f, 0.f};

        for (int ch = 0; ch < a.nchunks; ++ch) {
            __syncthreads();  // the previous chunk has been read
            {
                constexpr int PP = CC / 8;  // 16-byte pieces per pixel
                const T* yg = (const T*)a.dy + (int64_t)b * Ho * Wo * Cout + ch * CC;
                for (int i = tid; i < G::RH * G::RW * PP; i += 256) {
                    const int pix = i / PP, p = i - pix * PP;
                    const int r = pix / G::RW, c = pix - r * G::RW;
                    const int v = y0 - 1 + r, u = x0 - 1 + c;  // position in Z(dy)
                    int oy = v, ox = u;
                    bool ok = v >= 0 && u >= 0;
                    if constexpr (S == 2) {
                        ok = ok && !((v | u) & 1);
                        oy = v >> 1;
                        ox = u >> 1;
                    }
                    ok = ok && oy < Ho && ox < Wo;
                    vec8 val;
#pragma unroll
                    for (int j = 0; j < 8; ++j) val[j] = (T)0.f;
                    if (ok) val = *reinterpret_cast<const vec8*>(yg + ((int64_t)oy * Wo + ox) * Cout + p * 8);
                    *reinterpret_cast<vec8*>(zs + i * 8) = val;
                }
            }
            {
                constexpr int PER = G::STEPS * 64;  // 16-byte pieces per block of 16 input channels
                const T* wg = (const T*)a.w + ((int64_t)nb0 * nsteps + ch * G::STEPS) * 512;
                for (int i = tid; i < nbw * PER; i += 256) {
                    const int n = i / PER, q = i - n * PER;
                    *reinterpret_cast<vec8*>(ws + i * 8) = *reinterpret_cast<const vec8*>(wg + ((int64_t)n * nsteps * 64 + q) * 8);
                }
            }
            __syncthreads();

#pragma unroll
            for (int kk = 0; kk < G::STEPS; ++kk) {
                vec8 zb[4];
#pragma unroll
                for (int mi = 0; mi < 4; ++mi) {
                    zb[mi] = *reinterpret_cast<const vec8*>(zs + prow[mi] + aoff[kk]);
                    if constexpr ((9 * CC) % 32 != 0) {
                        if (kk == G::STEPS - 1 && !aval[kk]) {
#pragma unroll
                            for (int j = 0; j < 8; ++j) zb[mi][j] = (T)0.f;
                        }
                    }
                }
#pragma unroll
                for (int n = 0; n < CD_NBW; ++n) {
                    if (n < nbw) {
                        const vec8 wa = *reinterpret_cast<const vec8*>(ws + (n * G::STEPS + kk) * 512 + lane * 8);
#pragma unroll
                        for (int mi = 0; mi < 4; ++mi) acc[mi][n] = mfma16(wa, zb[mi], acc[mi][n]);
                    }
                }
            }
        }

        // lane: input channels (nb0 + n) * 16 + 4 g .. + 3 of pixel (y0 + 4 wave + mi, x0 + m) of dx
        const int x = x0 + m;
#pragma unroll
        for (int mi = 0; mi < 4; ++mi) {
            const int y = y0 + wave * 4 + mi;
            if (y < H && x < W) {
                T* o = (T*)a.dx + (((int64_t)b * H + y) * W + x) * Cin;
#pragma unroll
                for (int n = 0; n < CD_NBW; ++n) {
                    if (n < nbw) {
                        T r[4];
#pragma unroll
                        for (int j = 0; j < 4; ++j) r[j] = (T)acc[mi][n][j];
                        uint2 pk;
                        __builtin_memcpy(&pk, r, 8);
                        *reinterpret_cast<uint2*>(o + (nb0 + n) * 16 + 4 * g) = pk;
                    }
                }
            }
        }
    }
}

template <typename T, int S, int CC>
static int cond_dgrad_launch(const CondDgradArgs& a, int blocks, hipStream_t s) {
    static std::atomic<uint64_t> done{0};
    constexpr int lds = CondDgradGeom<CC>::LDS_BYTES;
    set_lds_limit_once(done, reinterpret_cast<const void*>(&cond_dgrad_kernel<T, S, CC>), lds);
    hipLaunchKernelGGL((cond_dgrad_kernel<T, S, CC>), dim3(blocks), dim3(256), lds, s, a);
    return last_error();
}

template <typename T>
static int cond_dgrad_dispatch(const CondDgradArgs& a, int stride, int cc, int blocks, hipStream_t s) {
    if (cc == 32) return stride == 1 ? cond_dgrad_launch<T, 1, 32>(a, blocks, s) : cond_dgrad_launch<T, 2, 32>(a, blocks, s);
    return stride == 1 ? cond_dgrad_launch<T, 1, 16>(a, blocks, s) : cond_dgrad_launch<T, 2, 16>(a, blocks, s);
}

// =================================================================================================== wgrad
constexpr int CW_ROWS = 4, CW_PX = 32;  // output rows (one per wave) x output columns of a unit
constexpr int CW_CH = 32;               // channels of a tile, and the channel pitch of both LDS images
constexpr int CW_ACC = 9 * 2 * 2 + 2;   // f32x4 accumulators of a lane: (tap, c block, n block) + db per n block

typedef short cw_s16x4 __attribute__((ext_vector_type(4)));

struct CondWgradArgs {
    const void* x;
    const void* dy;
    float* ws;
    int B, H, W, Cin, Cout, Ho, Wo;
    int Cp;        // channel count of the partial's layout: Cin, or 16 in image mode
    int oyb, oxb;  // units per sample along y / x
    int units, splits;
    int ntc;       // input-channel tiles
    int x_dtype;
    int64_t pstride;  // floats per partial
};

template <int S>
struct CondWgradGeom {
    static constexpr int RH = (CW_ROWS - 1) * S + 3, RW = (CW_PX - 1) * S + 3;
    static constexpr int X_BYTES = RH * RW * CW_CH * 2;
    static constexpr int Y_BYTES = CW_ROWS * CW_PX * CW_CH * 2;
    static constexpr int RED_BYTES = CW_ACC * 4 * 64 * 4;  // one wave's accumulators
    static constexpr int LDS_BYTES = X_BYTES + Y_BYTES > RED_BYTES ? X_BYTES + Y_BYTES : RED_BYTES;
    static_assert(X_BYTES % 16 == 0, "the dy image starts 16-byte aligned");
};

// 8 contraction values of one channel: two LDS transpose reads, 4 pixels each; `jump` = bytes between pixel r and pixel r + 4
template <typename T>
__device__ __forceinline__ typename Vec8<T>::type cw_frag(const unsigned char* p, int jump) {
    const cw_s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) cw_s16x4*)p);
    const cw_s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) cw_s16x4*)(p + jump));
    return __builtin_bit_cast(typename Vec8<T>::type, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
}

template <typename T>
__device__ __forceinline__ T cw_img_load(const void* x, int dt, int64_t i) {
    const float f = dt == UR_F32 ? ((const float*)x)[i] : dt == UR_F16 ? (float)((const f16*)x)[i] : (float)((const bf16*)x)[i];
    return (T)f;
}

template <typename T, int S, bool IMG>
__global__ void __launch_bounds__(256) cond_wgrad_kernel(const CondWgradArgs a) {
    using G = CondWgradGeom<S>;
    typedef typename Vec8<T>::type vec8;
    extern __shared__ __attribute__((aligned(16))) unsigned char cond_bwd_smem[];
    T* xs = reinterpret_cast<T*>(cond_bwd_smem);               // [RH][RW][CW_CH]
    T* ys = reinterpret_cast<T*>(cond_bwd_smem + G::X_BYTES);  // [CW_ROWS][CW_PX][CW_CH]
    float* red = reinterpret_cast<float*>(cond_bwd_smem);      // [CW_ACC * 4][64], after the last unit
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, m = lane & 15, g = lane >> 4;
    const int H = a.H, W = a.W, Cin = a.Cin, Cout = a.Cout, Ho = a.Ho, Wo = a.Wo;
    const int ntiles = ((Cout + CW_CH - 1) / CW_CH) * a.ntc;
    const int tile = blockIdx.x % ntiles, split = blockIdx.x / ntiles;
    const int tn = tile / a.ntc, tc = tile - tn * a.ntc;
    const int n0 = tn * CW_CH, c0 = tc * CW_CH;
    const int nnb = (Cout - n0) >= CW_CH ? 2 : 1;
    const int ncb = (a.Cp - c0) >= CW_CH ? 2 : 1;
    const int u0 = (int)((int64_t)a.units * split / a.splits), u1 = (int)((int64_t)a.units * (split + 1) / a.splits);

    f32x4 acc[9][2][2], accb[2];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int cb = 0; cb < 2; ++cb)
#pragma unroll
            for (int nb = 0; nb < 2; ++nb) acc[t][cb][nb] = f32x4{0.f, 0.f, 0.f, 0.f};
    accb[0] = accb[1] = f32x4{0.f, 0.f, 0.f, 0.f};
    vec8 ones;
#pragma unroll
    for (int j = 0; j < 8; ++j) ones[j] = (T)1.f;

    // this lane's address inside a fragment: pixel 8 g + (m >> 2) (+ 4 for the second read), channels 4 (m & 3) .. + 3
    const int fpx = 8 * g + (m >> 2), fch = 4 * (m & 3);
    const unsigned char* yfrag = reinterpret_cast<const unsigned char*>(ys) + ((wave * CW_PX + fpx) * CW_CH + fch) * 2;
    const unsigned char* xfrag = reinterpret_cast<const unsigned char*>(xs) + (((wave * S) * G::RW + fpx * S) * CW_CH + fch) * 2;

    for (int u = u0; u < u1; ++u) {
        const int oxblk = u % a.oxb;
        const int t = u / a.oxb;
        const int oyblk = t % a.oyb, b = t / a.oyb;
        const int oy0 = oyblk * CW_ROWS, ox0 = oxblk * CW_PX;
        const int iy0 = oy0 * S - 1, ix0 = ox0 * S - 1;
        __syncthreads();  // the previous unit has been read
        if constexpr (IMG) {
            for (int pix = tid; pix < G::RH * G::RW; pix += 256) {
                const int r = pix / G::RW, c = pix - r * G::RW;
                const int iy = iy0 + r, ix = ix0 + c;
                vec8 v, z;
#pragma unroll
                for (int j = 0; j < 8; ++j) v[j] = z[j] = (T)0.f;
                if ((unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W) {
                    const int64_t p = ((int64_t)b * Cin * H + iy) * W + ix;
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (j < Cin) v[j] = cw_img_load<T>(a.x, a.x_dtype, p + (int64_t)j * H * W);
                }
                *reinterpret_cast<vec8*>(xs + pix * CW_CH) = v;
                *reinterpret_cast<vec8*>(xs + pix * CW_CH + 8) = z;
            }
        } else {
            const int PP = ncb * 2;  // 16-byte pieces per pixel
            const T* xg = (const T*)a.x + (int64_t)b * H * W * Cin + c0;
            for (int i = tid; i < G::RH * G::RW * PP; i += 256) {
                const int pix = i / PP, p = i - pix * PP;
                const int r = pix / G::RW, c = pix - r * G::RW;
                const int iy = iy0 + r, ix = ix0 + c;
                vec8 v;
#pragma unroll
                for (int j = 0; j < 8; ++j) v[j] = (T)0.f;
                if ((unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W)
                    v = *reinterpret_cast<const vec8*>(xg + ((int64_t)iy * W + ix) * Cin + p * 8);
                *reinterpret_cast<vec8*>(xs + pix * CW_CH + p * 8) = v;
            }
        }
        {
            const int PP = nnb * 2;
            const T* yg = (const T*)a.dy + (int64_t)b * Ho * Wo * Cout + n0;
            for (int i = tid; i < CW_ROWS * CW_PX * PP; i += 256) {
                const int pix = i / PP, p = i - pix * PP;
                const int oy = oy0 + pix / CW_PX, ox = ox0 + pix % CW_PX;
                vec8 v;
#pragma unroll
                for (int j = 0; j < 8; ++j) v[j] = (T)0.f;
                if (oy < Ho && ox < Wo) v = *reinterpret_cast<const vec8*>(yg + ((int64_t)oy * Wo + ox) * Cout + p * 8);
                *reinterpret_cast<vec8*>(ys + pix * CW_CH + p * 8) = v;
            }
        }
        __syncthreads();

        vec8 yb[2];
#pragma unroll
        for (int nb = 0; nb < 2; ++nb)
            if (nb < nnb) yb[nb] = cw_frag<T>(yfrag + nb * 32, 4 * CW_CH * 2);
        if (tc == 0) {
#pragma unroll
            for (int nb = 0; nb < 2; ++nb)
                if (nb < nnb) accb[nb] = mfma16(ones, yb[nb], accb[nb]);
        }
#pragma unroll
        for (int t9 = 0; t9 < 9; ++t9) {
            const int off = ((t9 / 3) * G::RW + t9 % 3) * CW_CH * 2;
#pragma unroll
            for (int cb = 0; cb < 2; ++cb) {
                if (cb < ncb) {
                    const vec8 xa = cw_frag<T>(xfrag + off + cb * 32, 4 * S * CW_CH * 2);
#pragma unroll
                    for (int nb = 0; nb < 2; ++nb)
                        if (nb < nnb) acc[t9][cb][nb] = mfma16(xa, yb[nb], acc[t9][cb][nb]);
                }
            }
        }
    }

    // the four waves' sums, added in wave order
    __syncthreads();
    for (int w = 1; w < 4; ++w) {
        if (wave == w) {
#pragma unroll
            for (int t = 0; t < 9; ++t)
#pragma unroll
                for (int cb = 0; cb < 2; ++cb)
#pragma unroll
                    for (int nb = 0; nb < 2; ++nb)
#pragma unroll
                        for (int j = 0; j < 4; ++j) red[(((t * 2 + cb) * 2 + nb) * 4 + j) * 64 + lane] = acc[t][cb][nb][j];
#pragma unroll
            for (int nb = 0; nb < 2; ++nb) red[(144 + nb) * 64 + lane] = accb[nb][0];
        }
        __syncthreads();
        if (wave == 0) {
#pragma unroll
            for (int t = 0; t < 9; ++t)
#pragma unroll
                for (int cb = 0; cb < 2; ++cb)
#pragma unroll
                    for (int nb = 0; nb < 2; ++nb)
#pragma unroll
                        for (int j = 0; j < 4; ++j) acc[t][cb][nb][j] += red[(((t * 2 + cb) * 2 + nb) * 4 + j) * 64 + lane];
#pragma unroll
            for (int nb = 0; nb < 2; ++nb) accb[nb][0] += red[(144 + nb) * 64 + lane];
        }
        __syncthreads();
    }
    if (wave != 0) return;

    // lane: partial[n0 + 16 nb + m][c0 + 16 cb + 4 g .. + 3][0 .. 8], 36 consecutive floats
    float* pw = a.ws + (int64_t)split * a.pstride;
#pragma unroll
    for (int cb = 0; cb < 2; ++cb) {
        if (cb < ncb) {
#pragma unroll
            for (int nb = 0; nb < 2; ++nb) {
                if (nb < nnb) {
                    const int n = n0 + nb * 16 + m, c = c0 + cb * 16 + 4 * g;
                    float4* o = reinterpret_cast<float4*>(pw + ((int64_t)n * a.Cp + c) * 9);
#pragma unroll
                    for (int q = 0; q < 9; ++q) {
                        float f[4];
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            const int k = 4 * q + e;  // = j * 9 + tap
                            f[e] = acc[k % 9][cb][nb][k / 9];
                        }
                        o[q] = make_float4(f[0], f[1], f[2], f[3]);
                    }
                }
            }
        }
    }
    if (tc == 0 && g == 0) {
#pragma unroll
        for (int nb = 0; nb < 2; ++nb)
            if (nb < nnb) pw[(int64_t)Cout * a.Cp * 9 + n0 + nb * 16 + m] = accb[nb][0];
    }
}

// second pass: the partials added in split order; dw in the parameter's layout [Cout][Cin][3][3] (image mode: the real channels only)
// A workgroup owns 64 consecutive outputs; wave w adds the splits k = w, w + 4, ... in four interleaved chains (k, k + 16, ...:
// independent loads in flight, the pass is latency bound), the chains and then the waves are combined in a fixed tree.
__global__ void __launch_bounds__(256) cond_wgrad_sum_kernel(const float* ws, float* dw, float* db, int Cout, int Cin, int Cp,
                                                             int splits, int64_t pstride) {
    __shared__ float part[4][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t nw = (int64_t)Cout * Cin * 9, total = nw + Cout;
    const int64_t i = (int64_t)blockIdx.x * 64 + lane;
    int64_t src = 0;
    float* dst = nullptr;
    if (i < nw) {
        const int64_t n = i / (Cin * 9), r = i - n * (Cin * 9);
        src = n * Cp * 9 + r;
        dst = dw ? dw + i : nullptr;
    } else if (i < total) {
        src = (int64_t)Cout * Cp * 9 + (i - nw);
        dst = db ? db + (i - nw) : nullptr;
    }
    float s[4] = {0.f, 0.f, 0.f, 0.f};
    if (dst) {
        const float* p = ws + src;
        int k = w;
        for (; k + 12 < splits; k += 16) {
#pragma unroll
            for (int j = 0; j < 4; ++j) s[j] += p[(int64_t)(k + 4 * j) * pstride];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (k + 4 * j < splits) s[j] += p[(int64_t)(k + 4 * j) * pstride];
    }
    part[w][lane] = (s[0] + s[1]) + (s[2] + s[3]);
    __syncthreads();
    if (w == 0 && dst) *dst = (part[0][lane] + part[1][lane]) + (part[2][lane] + part[3][lane]);
}

struct CondWgradPlan {
    int Ho, Wo, Cp, oyb, oxb, units, ntn, ntc, splits;
    int64_t pstride;
};

// 0, or the code of the refusal
static int cond_wgrad_plan(int B, int H, int W, int Cin, int Cout, int stride, int x_nchw, int splits, CondWgradPlan& p) {
    if (B <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0 || splits < 0) return UR_E_BADARG;
    if (stride != 1 && stride != 2) return UR_E_UNSUPPORTED;
    if (x_nchw ? Cin > 4 : ((Cin & 15) || Cin > 256)) return UR_E_UNSUPPORTED;
    if ((Cout & 15) || Cout > 256 || H > (1 << 24) || W > (1 << 24) || splits > 65536) return UR_E_UNSUPPORTED;
    p.Ho = (H - 1) / stride + 1;
    p.Wo = (W - 1) / stride + 1;
    p.Cp = x_nchw ? 16 : Cin;
    p.oyb = (p.Ho + CW_ROWS - 1) / CW_ROWS;
    p.oxb = (p.Wo + CW_PX - 1) / CW_PX;
    const int64_t units = (int64_t)B * p.oyb * p.oxb;
    if (units > 0x7fffffff) return UR_E_UNSUPPORTED;
    p.units = (int)units;
    p.ntn = (Cout + CW_CH - 1) / CW_CH;
    p.ntc = (p.Cp + CW_CH - 1) / CW_CH;
    p.pstride = (int64_t)Cout * p.Cp * 9 + Cout;
    if (splits == 0) {  // ~4 workgroups per CU, at least one unit each, at most 64 MiB of partials
        const int tiles = p.ntn * p.ntc;
        int64_t s = 1024 / tiles;
        if (s > units) s = units;
        while (s > 1 && s * p.pstride * 4 > ((int64_t)64 << 20)) s >>= 1;
        splits = (int)(s < 1 ? 1 : s);
    }
    p.splits = splits;
    if ((int64_t)splits * p.ntn * p.ntc > 0x7fffffff) return UR_E_UNSUPPORTED;
    return 0;
}

template <typename T>
static int cond_wgrad_dispatch(const CondWgradArgs& a, int stride, int x_nchw, int blocks, hipStream_t s) {
    if (x_nchw) {
        if (stride == 1) hipLaunchKernelGGL((cond_wgrad_kernel<T, 1, true>), dim3(blocks), dim3(256), CondWgradGeom<1>::LDS_BYTES, s, a);
        else hipLaunchKernelGGL((cond_wgrad_kernel<T, 2, true>), dim3(blocks), dim3(256), CondWgradGeom<2>::LDS_BYTES, s, a);
    } else {
        if (stride == 1) hipLaunchKernelGGL((cond_wgrad_kernel<T, 1, false>), dim3(blocks), dim3(256), CondWgradGeom<1>::LDS_BYTES, s, a);
        else hipLaunchKernelGGL((cond_wgrad_kernel<T, 2, false>), dim3(blocks), dim3(256), CondWgradGeom<2>::LDS_BYTES, s, a);
    }
    return last_error();
}

}  // namespace ur

using namespace ur;

extern "C" int ur_cond_conv3x3_dgrad(const void* dy, const void* w_rot, void* dx, int B, int H, int W, int Cin, int Cout, int stride,
                                     int dtype, void* stream) {
    if (!dy || !w_rot || !dx || B <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0) return UR_E_BADARG;
    if (dtype != UR_DT_F16 && dtype != UR_DT_BF16) return UR_E_BADARG;
    if (((uintptr_t)dy | (uintptr_t)w_rot | (uintptr_t)dx) & 15) return UR_E_BADARG;
    if (stride != 1 && stride != 2) return UR_E_UNSUPPORTED;
    if ((Cin & 15) || Cin > 256 || (Cout & 15) || Cout > 256) return UR_E_UNSUPPORTED;
    const int cc = ur_cond_conv3x3_kchunk(Cout, 1, 0);
    if (cc < 0) return cc;
    CondDgradArgs a{};
    a.dy = dy; a.w = w_rot; a.dx = dx;
    a.B = B; a.H = H; a.W = W; a.Cin = Cin; a.Cout = Cout;
    a.Ho = (H - 1) / stride + 1;
    a.Wo = (W - 1) / stride + 1;
    a.tiles_x = (W + CD_TW - 1) / CD_TW;
    a.tiles_y = (H + CD_TH - 1) / CD_TH;
    a.nchunks = Cout / cc;
    const int64_t blocks = (int64_t)B * a.tiles_x * a.tiles_y;
    if (blocks > 0x7fffffff || H > (1 << 24) || W > (1 << 24)) return UR_E_UNSUPPORTED;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    UR_DISPATCH(dtype, return cond_dgrad_dispatch<T>(a, stride, cc, (int)blocks, st));
}

extern "C" int64_t ur_cond_conv3x3_wgrad_workspace(int B, int H, int W, int Cin, int Cout, int stride, int x_nchw, int splits) {
    CondWgradPlan p{};
    const int rc = cond_wgrad_plan(B, H, W, Cin, Cout, stride, x_nchw, splits, p);
    if (rc) return rc;
    return (int64_t)p.splits * p.pstride * 4;
}

extern "C" int ur_cond_conv3x3_wgrad(const void* x, int x_dtype, int x_nchw, const void* dy, float* dw, float* db, void* workspace,
                                     int64_t workspace_bytes, int B, int H, int W, int Cin, int Cout, int stride, int splits,
                                     int dtype, void* stream) {
    if (!x || !dy || !workspace || (!dw && !db)) return UR_E_BADARG;
    if (dtype != UR_DT_F16 && dtype != UR_DT_BF16) return UR_E_BADARG;
    if (x_nchw ? (x_dtype != UR_DT_F16 && x_dtype != UR_DT_BF16 && x_dtype != UR_DT_F32) : x_dtype != dtype) return UR_E_BADARG;
    if (((uintptr_t)dy | (uintptr_t)workspace) & 15) return UR_E_BADARG;
    if (((uintptr_t)dw | (uintptr_t)db) & 3) return UR_E_BADARG;
    if ((uintptr_t)x & (x_nchw ? (x_dtype == UR_DT_F32 ? 3 : 1) : 15)) return UR_E_BADARG;
    CondWgradPlan p{};
    const int rc = cond_wgrad_plan(B, H, W, Cin, Cout, stride, x_nchw, splits, p);
    if (rc) return rc;
    if (workspace_bytes < (int64_t)p.splits * p.pstride * 4) return UR_E_BADARG;
    CondWgradArgs a{};
    a.x = x; a.dy = dy; a.ws = (float*)workspace;
    a.B = B; a.H = H; a.W = W; a.Cin = Cin; a.Cout = Cout; a.Ho = p.Ho; a.Wo = p.Wo;
    a.Cp = p.Cp; a.oyb = p.oyb; a.oxb = p.oxb; a.units = p.units; a.splits = p.splits; a.ntc = p.ntc;
    a.x_dtype = x_dtype; a.pstride = p.pstride;
    const int blocks = p.splits * p.ntn * p.ntc;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    int err;
    if (dtype == UR_DT_F16) err = cond_wgrad_dispatch<f16>(a, stride, x_nchw, blocks, st);
    else err = cond_wgrad_dispatch<bf16>(a, stride, x_nchw, blocks, st);
    if (err) return err;
    const int64_t total = (int64_t)Cout * Cin * 9 + Cout;
    hipLaunchKernelGGL(cond_wgrad_sum_kernel, dim3((unsigned)((total + 63) / 64)), dim3(256), 0, st, (const float*)workspace, dw, db,
                       Cout, Cin, p.Cp, p.splits, p.pstride);
    return last_error();
}
