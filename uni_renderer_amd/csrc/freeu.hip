// FreeU (Si et al., arXiv 2309.11497) in front of the concat of an up-block resnet, both halves of diffusers'
// apply_freeu in ONE launch over NHWC tensors:
//   hidden[:, :, :, : Ch / 2] *= b                                     (in place)
//   skip = Re ifftn( mask * fftn(skip) ), mask = s on the shifted box [H/2-1 : H/2+1, W/2-1 : W/2+1], 1 elsewhere
// The box holds exactly the four frequencies (ky, kx) in {-1, 0}^2, so per (sample, channel) column the filter is a rank-7
// update and needs no FFT.  With t = 2 pi y / H, p = 2 pi x / W and the sums taken over the H * W pixels of the column:
//   x' = x + (s - 1) / (H W) * [ a0 + a1 cos t + a2 sin t + a3 cos p + a4 sin p + a5 cos(t + p) + a6 sin(t + p) ]
//   a0 = sum x, a1 = sum x cos t, a2 = sum x sin t, a3 = sum x cos p, a4 = sum x sin p, a5 = sum x cos(t + p), a6 = sum x sin(t + p)
// (the set is NOT conjugate-symmetric -- +1 is outside the box -- so this is not a symmetric low-pass).
//
// One workgroup owns one (sample, 32-channel slice) of the skip: 64 pixel lanes x 4 vectors of 8 channels.  It reads its whole
// strip, reduces the seven sums, and only then writes, so skip_out == skip is legal.  Maps of up to 1024 pixels (the 8x8 ...
// 32x32 levels FreeU acts on up to 1024^2 images) keep the strip in registers between the reduction and the update: one memory
// round trip, like the one-launch GroupNorm of norm.hip.  Larger maps read the strip a second time.
//
// Summation (fixed order, so the launch is bit-reproducible): the sums run over x - K, K = the hi part of the column's first
// pixel (the a0 term gets H W K back; the other six twiddle sets sum to zero), so a column whose mean is large against its
// spread loses nothing.  A thread sums its pixels in fma chains of four, chains are combined by compensated (Kahan) addition
// (maps of up to 256 pixels are one chain), then four pairwise levels over the 16 pixel lanes of a wave and a pairwise add of
// the 4 waves: at most min(4, ceil(HW / 64)) + 2 + ceil(log2 min(HW, 256)) roundings per sum for any map size.
// The row and column twiddles (H + W pairs) are computed once per workgroup into LDS when H + W <= 1024.
#include "ur_launch.h"

namespace ur {

struct FreeuArgs {
    void* hidden;
    void* hidden_lo;
    const void* skip;
    const void* skip_lo;
    void* skip_out;
    void* skip_out_lo;
    float b, s;
    int B, H, W, Ch, Cs;
    int nslices;      // 32-channel slices of the skip
    int skip_blocks;  // B * nslices workgroups filter; the rest scale hidden, 1024 vectors each
};

constexpr int FREEU_NSUM = 7;
constexpr int FREEU_TW_MAX = 1024;  // H + W up to which the twiddles come from the workgroup's LDS table

// cos / sin of 2 pi k / n for 0 <= k < n: the argument of sincospi is reduced to [-1, 1) in integers, so the quadrant points
// are exact and the division is the only rounding in front of it
__device__ __forceinline__ void unit_root(int k, int n, float& c, float& s) {
    const int k2 = 2 * k >= n ? 2 * k - 2 * n : 2 * k;
    sincospif((float)k2 / (float)n, &s, &c);
}

// (cos, sin) of the row angles [0, H) and the column angles [H, H + W): the LDS table, or computed in place for huge maps
struct FreeuTw {
    const float2* tab;  // nullptr: H + W > FREEU_TW_MAX
    int H, W;
};

// pixel p = y * W + x walked in steps of 64 without a division per pixel
struct FreeuPix {
    int y, x, dy, dx;
    __device__ __forceinline__ FreeuPix(int p, int W) : y(p / W), x(p - (p / W) * W), dy(64 / W), dx(64 - (64 / W) * W) {}
    __device__ __forceinline__ void next(int W) {
        x += dx;
        y += dy;
        if (x >= W) { x -= W; ++y; }
    }
};

// the six non-constant basis values of pixel (y, x): cos t, sin t, cos p, sin p, cos(t + p), sin(t + p)
__device__ __forceinline__ void freeu_basis(const FreeuPix& px, const FreeuTw& t, float (&tw)[FREEU_NSUM - 1]) {
    float ct, st, cp, sp;
    if (t.tab) {
        const float2 a = t.tab[px.y], b = t.tab[t.H + px.x];
        ct = a.x; st = a.y; cp = b.x; sp = b.y;
    } else {
        unit_root(px.y, t.H, ct, st);
        unit_root(px.x, t.W, cp, sp);
    }
    tw[0] = ct; tw[1] = st; tw[2] = cp; tw[3] = sp;
    tw[4] = ct * cp - st * sp;
    tw[5] = st * cp + ct * sp;
}

// v + (v of the lane n places down the row of 16), one DPP move
template <int N>
__device__ __forceinline__ float row_ror_add(float v) {
    return v + __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x120 | N, 0xF, 0xF, false));
}

template <typename T>
__device__ __forceinline__ void load_hilo8(const T* hi, const lo_t<T>* lo, int64_t off, float (&x)[8]) {
    load8(hi + off, x);
    if (lo) {
        float t[8];
        load_lo<8>(lo + off, t);
#pragma unroll
        for (int j = 0; j < 8; ++j) x[j] += t[j];
    }
}

// part[k][j] += (x[j] - K[j]) * basis_k(p)
__device__ __forceinline__ void freeu_accum(const float (&x)[8], const float (&K)[8], const FreeuPix& px, const FreeuTw& t,
                                            float (&part)[FREEU_NSUM][8]) {
    float tw[FREEU_NSUM - 1];
    freeu_basis(px, t, tw);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const float d = x[j] - K[j];
        part[0][j] += d;
#pragma unroll
        for (int k = 1; k < FREEU_NSUM; ++k) part[k][j] = fmaf(d, tw[k - 1], part[k][j]);
    }
}

// Kahan: sum += part with the running compensation cmp
__device__ __forceinline__ void freeu_flush(float (&part)[FREEU_NSUM][8], float (&sum)[FREEU_NSUM][8], float (&cmp)[FREEU_NSUM][8]) {
#pragma clang fp reassociate(off)
#pragma unroll
    for (int k = 0; k < FREEU_NSUM; ++k)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float yv = part[k][j] - cmp[k][j];
            const float tv = sum[k][j] + yv;
            cmp[k][j] = (tv - sum[k][j]) - yv;
            sum[k][j] = tv;
            part[k][j] = 0.f;
        }
}

// x + coef . basis(p) -> out (+ remainder -> out_lo)
template <typename T>
__device__ __forceinline__ void freeu_update(const float (&x)[8], const float (&coef)[FREEU_NSUM][8], const FreeuPix& px,
                                             const FreeuTw& t, T* out, lo_t<T>* out_lo, int64_t off) {
    float tw[FREEU_NSUM - 1], v[8];
    freeu_basis(px, t, tw);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        float c = coef[0][j];
#pragma unroll
        for (int k = 1; k < FREEU_NSUM; ++k) c = fmaf(coef[k][j], tw[k - 1], c);
        v[j] = x[j] + c;
    }
    store8(out + off, v);
    if (out_lo) store_lo8<T>(out_lo + off, v);
}

// hidden[..., : Ch / 2] *= b over the vectors that hold such channels; a vector that straddles Ch / 2 keeps the raw bits of
// its upper elements
template <typename T>
__device__ __forceinline__ void freeu_scale_hidden(const FreeuArgs& a, int blk) {
    T* hid = (T*)a.hidden;
    lo_t<T>* hlo = (lo_t<T>*)a.hidden_lo;
    const int half = a.Ch >> 1;
    const int nvh = (half + 7) >> 3;
    const int64_t total = (int64_t)a.B * a.H * a.W * nvh;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int64_t i = (int64_t)blk * 1024 + u * 256 + threadIdx.x;
        if (i >= total) break;
        const int64_t pix = i / nvh;
        const int v = (int)(i - pix * nvh);
        const int64_t off = pix * a.Ch + v * 8;
        const int lim = half - v * 8;  // elements of this vector below Ch / 2 (>= 8: all)
        typedef typename Vec8<T>::type vec8;
        vec8 raw = *reinterpret_cast<const vec8*>(hid + off);
        float x[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) x[j] = (float)raw[j];
        lo_t<T> rl[8];
        if (hlo) {
            float t[8];
            load_lo<8>(hlo + off, t);
            __builtin_memcpy(rl, hlo + off, sizeof(rl));
#pragma unroll
            for (int j = 0; j < 8; ++j) x[j] += t[j];
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            x[j] *= a.b;
            if (j < lim) raw[j] = (T)x[j];
        }
        *reinterpret_cast<vec8*>(hid + off) = raw;
        if (hlo) {
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (j < lim) rl[j] = lo_from_f<lo_t<T>>(x[j] - to_f(from_f<T>(x[j])));
            if constexpr (sizeof(lo_t<T>) == 1) { uint2 r; __builtin_memcpy(&r, rl, 8); *reinterpret_cast<uint2*>(hlo + off) = r; }
            else { uint4 r; __builtin_memcpy(&r, rl, 16); *reinterpret_cast<uint4*>(hlo + off) = r; }
        }
    }
}

// NP > 0: H * W <= 64 * NP and the strip stays in registers; NP == 0: any map, second read
template <typename T, int NP>
__global__ void __launch_bounds__(256) freeu_kernel(const FreeuArgs a) {
    if ((int)blockIdx.x >= a.skip_blocks) {
        freeu_scale_hidden<T>(a, (int)blockIdx.x - a.skip_blocks);
        return;
    }
    __shared__ float red[4][4][FREEU_NSUM][8];
    __shared__ float2 twtab[FREEU_TW_MAX];
    const int tid = threadIdx.x, cv = tid & 3, prow = tid >> 2, wave = tid >> 6;
    const int smp = (int)blockIdx.x / a.nslices, sl = (int)blockIdx.x - smp * a.nslices;
    const int H = a.H, W = a.W, HW = H * W, Cs = a.Cs;
    const int c0 = (sl * 4 + cv) * 8;
    const bool act = c0 < Cs;
    const int64_t base = (int64_t)smp * HW * Cs + c0;
    // no __restrict__: skip_out may be skip
    const T* in = (const T*)a.skip + base;
    const lo_t<T>* in_lo = a.skip_lo ? (const lo_t<T>*)a.skip_lo + base : nullptr;
    T* out = (T*)a.skip_out + base;
    lo_t<T>* out_lo = a.skip_out_lo ? (lo_t<T>*)a.skip_out_lo + base : nullptr;

    float K[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) K[j] = 0.f;
    if (act) load8(in, K);

    FreeuTw tw{H + W <= FREEU_TW_MAX ? twtab : nullptr, H, W};
    auto fill_table = [&]() {  // behind the strip's loads, so that the twiddles are computed while those are in flight
        if (tw.tab)
            for (int i = tid; i < H + W; i += 256) {
                float c, sn;
                if (i < H) unit_root(i, H, c, sn);
                else unit_root(i - H, W, c, sn);
                twtab[i] = make_float2(c, sn);
            }
        __syncthreads();
    };

    float sum[FREEU_NSUM][8], cmp[FREEU_NSUM][8], part[FREEU_NSUM][8];
#pragma unroll
    for (int k = 0; k < FREEU_NSUM; ++k)
#pragma unroll
        for (int j = 0; j < 8; ++j) sum[k][j] = cmp[k][j] = part[k][j] = 0.f;

    constexpr int NR = NP > 0 ? NP : 1;
    float xs[NR][8];
    if constexpr (NP > 0) {
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            const int p = prow + 64 * i;
            if (act && p < HW) load_hilo8<T>(in, in_lo, (int64_t)p * Cs, xs[i]);
        }
        fill_table();
        FreeuPix px(prow, W);
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            const int p = prow + 64 * i;
            if constexpr (NP <= 4) {  // one chain: no compensation needed
                if (act && p < HW) freeu_accum(xs[i], K, px, tw, sum);
            } else {
                if (act && p < HW) freeu_accum(xs[i], K, px, tw, part);
                if ((i & 3) == 3 || i == NP - 1) freeu_flush(part, sum, cmp);
            }
            px.next(W);
        }
    } else {
        fill_table();
        if (act) {
            FreeuPix px(prow, W);
            for (int p0 = prow; p0 < HW; p0 += 256) {
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int p = p0 + 64 * u;
                    if (p < HW) {
                        load_hilo8<T>(in, in_lo, (int64_t)p * Cs, xs[0]);
                        freeu_accum(xs[0], K, px, tw, part);
                    }
                    px.next(W);
                }
                freeu_flush(part, sum, cmp);
            }
        }
    }

    // the 16 pixel lanes of a wave (lane = 4 * (prow & 15) + cv): the 4 of a row of 16 lanes by DPP rotations, the 4 rows by
    // butterflies; lanes 0 .. 3 hold the wave's sums for cv = 0 .. 3; then the 4 waves through LDS
#pragma unroll
    for (int k = 0; k < FREEU_NSUM; ++k)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            float v = row_ror_add<8>(row_ror_add<4>(sum[k][j]));
            v += __shfl_xor(v, 16, 64);
            v += __shfl_xor(v, 32, 64);
            sum[k][j] = v;
        }
    if ((tid & 63) < 4) {
#pragma unroll
        for (int k = 0; k < FREEU_NSUM; ++k)
#pragma unroll
            for (int j = 0; j < 8; ++j) red[wave][cv][k][j] = sum[k][j];
    }
    __syncthreads();
    if (!act) return;

    // coef[k] = (s - 1) / (H W) * a_k; the pivot returns to the constant term: (s - 1) / (H W) * (sum(x - K) + H W K)
    const float g = (a.s - 1.0f) / (float)HW;
    float coef[FREEU_NSUM][8];
#pragma unroll
    for (int k = 0; k < FREEU_NSUM; ++k)
#pragma unroll
        for (int j = 0; j < 8; ++j)
            coef[k][j] = g * ((red[0][cv][k][j] + red[1][cv][k][j]) + (red[2][cv][k][j] + red[3][cv][k][j]));
#pragma unroll
    for (int j = 0; j < 8; ++j) coef[0][j] = fmaf(a.s - 1.0f, K[j], coef[0][j]);

    FreeuPix px(prow, W);
    if constexpr (NP > 0) {
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            const int p = prow + 64 * i;
            if (p < HW) freeu_update<T>(xs[i], coef, px, tw, out, out_lo, (int64_t)p * Cs);
            px.next(W);
        }
    } else {
        // every pixel is re-read and written by the one thread that owns it, after the whole column has been reduced
        for (int p = prow; p < HW; p += 64) {
            load_hilo8<T>(in, in_lo, (int64_t)p * Cs, xs[0]);
            freeu_update<T>(xs[0], coef, px, tw, out, out_lo, (int64_t)p * Cs);
            px.next(W);
        }
    }
}

template <typename T>
static int freeu_launch(const FreeuArgs& a, int blocks, hipStream_t s) {
    const int HW = a.skip ? a.H * a.W : 0;
    if (HW <= 64) hipLaunchKernelGGL((freeu_kernel<T, 1>), dim3(blocks), dim3(256), 0, s, a);
    else if (HW <= 256) hipLaunchKernelGGL((freeu_kernel<T, 4>), dim3(blocks), dim3(256), 0, s, a);
    else if (HW <= 1024) hipLaunchKernelGGL((freeu_kernel<T, 16>), dim3(blocks), dim3(256), 0, s, a);
    else hipLaunchKernelGGL((freeu_kernel<T, 0>), dim3(blocks), dim3(256), 0, s, a);
    return last_error();
}

}  // namespace ur

using namespace ur;

extern "C" int ur_freeu(void* hidden, void* hidden_lo, int Ch, float b, const void* skip, const void* skip_lo, void* skip_out,
                        void* skip_out_lo, int Cs, float s, int B, int H, int W, int dtype, void* stream) {
    if ((!hidden && !skip) || B <= 0 || H <= 0 || W <= 0) return UR_E_BADARG;
    if (hidden && (Ch <= 0 || (Ch & 7))) return UR_E_BADARG;
    if (!hidden && hidden_lo) return UR_E_BADARG;
    if (skip && (!skip_out || Cs <= 0 || (Cs & 7))) return UR_E_BADARG;
    if (!skip && (skip_lo || skip_out || skip_out_lo)) return UR_E_BADARG;
    if (dtype != UR_DT_F16 && dtype != UR_DT_BF16) return UR_E_BADARG;
    if (H < 2 || W < 2) return UR_E_UNSUPPORTED;  // the box [H/2-1 : H/2+1] needs two rows and two columns
    if ((int64_t)H * W > (1 << 24)) return UR_E_UNSUPPORTED;
    FreeuArgs a{};
    a.hidden = hidden; a.hidden_lo = hidden_lo; a.skip = skip; a.skip_lo = skip_lo; a.skip_out = skip_out; a.skip_out_lo = skip_out_lo;
    a.b = b; a.s = s; a.B = B; a.H = H; a.W = W; a.Ch = Ch; a.Cs = Cs;
    int64_t blocks = 0;
    if (skip) {
        a.nslices = (Cs / 8 + 3) / 4;
        blocks = (int64_t)B * a.nslices;
        if (blocks > (1 << 30)) return UR_E_UNSUPPORTED;
    }
    a.skip_blocks = (int)blocks;
    if (hidden) {
        const int64_t nvec = (int64_t)B * H * W * ((Ch / 2 + 7) / 8);
        blocks += (nvec + 1023) / 1024;
        if (blocks > (1 << 30)) return UR_E_UNSUPPORTED;
    }
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    UR_DISPATCH(dtype, return freeu_launch<T>(a, (int)blocks, st));
}
