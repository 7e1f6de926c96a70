// LoRA merge over a list of weight matrices in ONE launch (include/ur_kernels.h, ur_lora_merge_multi):
//     w[n][k] = cast( base[n][k] + scale * sum_{r < R} rscale[r] * up[n][r] * down[r][k] )
// A workgroup of 256 threads owns a tile of LT_N = 32 rows x LT_K = 128 columns of one item (workgroup -> (item, tile)
// through the SegTable in the kernel arguments).  Thread (ty, tx) = (tid >> 5, tid & 31) owns rows 4 ty .. 4 ty + 3 and
// columns 4 tx .. 4 tx + 3 of it: 16 fp32 accumulators.  The factors are walked in chunks of LT_R = 16 ranks staged in
// LDS -- the chunk of `down` ([16][128], one conflict-free ds_read_b128 per thread and rank) and the chunk of
// rscale[r] * up ([16][32], one broadcast ds_read_b128) -- so every factor element is read from memory once per tile and
// reused by all its rows / columns.  `base` is read once (before the rank loop, so that the loads are in flight under it)
// and `w` written once: at the ranks people use the kernel moves 2 x the bytes of the weights and little else.
//
// Arithmetic, per element: p_r = fl(rscale[r] * up[n][r]) (skipped when rscale is NULL), acc = fma(p_r, down[r][k], acc)
// for r = 0 .. R - 1 in ascending order from acc = 0, then ONE fma(scale, acc, base) and ONE rounding to the dtype.  No
// atomics, no data-dependent order: bit-reproducible.  R == 0 copies the bits of `base` (integer moves, no arithmetic).
// Rows whose byte length is no multiple of the 4-element access (K % 4 != 0, or a base / w address off that alignment)
// take the element-wise path for the whole item; no access is ever wider than its alignment.
#include "ur_launch.h"

namespace ur {

constexpr int LT_N = 32, LT_K = 128, LT_R = 16;
constexpr int LORA_MULTI_MAX = 48;   // items per launch (ur_lora_multi_max): 48 x 56 bytes + the segment table < 4 KB of arguments
constexpr int LORA_MAX_RANK = 512;   // ur_lora_max_rank: four rank-128 adapters at once
constexpr int LORA_ITEM_WORDS = 9;   // int64_t words per row of the caller's table

// one item as the kernel reads it (the caller's table row, narrowed)
struct LoraItem {
    const void* base;
    void* w;
    const float* up;
    const float* down;
    const float* rscale;
    int32_t N, K, R;
    float scale;
};

struct LoraArgs {
    LoraItem t[LORA_MULTI_MAX];
    SegTable<LORA_MULTI_MAX> seg;
};
static_assert(sizeof(LoraArgs) <= 4096, "kernel arguments");

template <typename T> struct alignas(4 * sizeof(T)) Quad { T v[4]; };
template <int BYTES> struct BitsOf;
template <> struct BitsOf<2> { typedef uint16_t type; };
template <> struct BitsOf<4> { typedef uint32_t type; };

template <typename T>
__global__ void __launch_bounds__(256) lora_merge_multi_kernel(const LoraArgs a) {
    typedef typename BitsOf<sizeof(T)>::type bits_t;
    __shared__ __attribute__((aligned(16))) float s_down[LT_R * LT_K];
    __shared__ __attribute__((aligned(16))) float s_up[LT_R * LT_N];

    const int it = a.seg.find(blockIdx.x);
    const LoraItem e = a.t[it];
    const int N = e.N, K = e.K, R = e.R;
    const int ktiles = (K + LT_K - 1) / LT_K;
    const int lb = (int)blockIdx.x - a.seg.start[it];
    const int n0 = (lb / ktiles) * LT_N, k0 = (lb % ktiles) * LT_K;
    const int tid = threadIdx.x, tx = tid & 31, ty = tid >> 5;
    const int row0 = n0 + 4 * ty, col0 = k0 + 4 * tx;
    const bool wide = (K & 3) == 0 && (((uintptr_t)e.base | (uintptr_t)e.w) & (4 * sizeof(T) - 1)) == 0;  // workgroup-uniform

    if (R == 0) {  // the copy path of unfuse / unload: bits, not values
        const bits_t* src = (const bits_t*)e.base;
        bits_t* dst = (bits_t*)e.w;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int row = row0 + j;
            if (row >= N) break;
            const int64_t o = (int64_t)row * K + col0;
            if (wide) {
                if (col0 < K) *reinterpret_cast<Quad<bits_t>*>(dst + o) = *reinterpret_cast<const Quad<bits_t>*>(src + o);
            } else {
#pragma unroll
                for (int c = 0; c < 4; ++c)
                    if (col0 + c < K) dst[o + c] = src[o + c];
            }
        }
        return;
    }

    const T* base = (const T*)e.base;
    T* w = (T*)e.w;
    float b[4][4], acc[4][4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int row = row0 + j;
        const int64_t o = (int64_t)row * K + col0;
#pragma unroll
        for (int c = 0; c < 4; ++c) { b[j][c] = 0.f; acc[j][c] = 0.f; }
        if (row < N) {
            if (wide) {
                if (col0 < K) {
                    const Quad<T> q = *reinterpret_cast<const Quad<T>*>(base + o);
#pragma unroll
                    for (int c = 0; c < 4; ++c) b[j][c] = (float)q.v[c];
                }
            } else {
#pragma unroll
                for (int c = 0; c < 4; ++c)
                    if (col0 + c < K) b[j][c] = (float)base[o + c];
            }
        }
    }

    for (int r0 = 0; r0 < R; r0 += LT_R) {
        const int rc = min(LT_R, R - r0);
        if (r0) __syncthreads();  // the previous chunk has been consumed
#pragma unroll
        for (int i = 0; i < LT_R * LT_K / 256; ++i) {
            const int idx = tid + 256 * i, rr = idx / LT_K, cc = idx % LT_K;
            float v = 0.f;
            if (rr < rc && k0 + cc < K) v = e.down[(int64_t)(r0 + rr) * K + k0 + cc];
            s_down[idx] = v;
        }
#pragma unroll
        for (int i = 0; i < LT_R * LT_N / 256; ++i) {
            const int idx = tid + 256 * i, rr = idx / LT_N, row = idx % LT_N;
            float v = 0.f;
            if (rr < rc && n0 + row < N) {
                v = e.up[(int64_t)(n0 + row) * R + r0 + rr];
                if (e.rscale) v = e.rscale[r0 + rr] * v;
            }
            s_up[idx] = v;
        }
        __syncthreads();
#pragma unroll 4
        for (int rr = 0; rr < rc; ++rr) {  // ascending r; ranks >= R are never multiplied
            const f32x4 d = *reinterpret_cast<const f32x4*>(s_down + rr * LT_K + 4 * tx);
            const f32x4 u = *reinterpret_cast<const f32x4*>(s_up + rr * LT_N + 4 * ty);
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int c = 0; c < 4; ++c) acc[j][c] = __builtin_fmaf(u[j], d[c], acc[j][c]);
        }
    }

    const float scale = e.scale;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int row = row0 + j;
        if (row >= N) break;
        const int64_t o = (int64_t)row * K + col0;
        if (wide) {
            if (col0 < K) {
                Quad<T> q;
#pragma unroll
                for (int c = 0; c < 4; ++c) q.v[c] = (T)__builtin_fmaf(scale, acc[j][c], b[j][c]);
                *reinterpret_cast<Quad<T>*>(w + o) = q;
            }
        } else {
#pragma unroll
            for (int c = 0; c < 4; ++c)
                if (col0 + c < K) w[o + c] = (T)__builtin_fmaf(scale, acc[j][c], b[j][c]);
        }
    }
}

}  // namespace ur

using namespace ur;

extern "C" int ur_lora_merge_multi(const int64_t* items, int n, int dtype, void* stream) {
    if (dtype != UR_DT_F16 && dtype != UR_DT_BF16 && dtype != UR_DT_F32) return UR_E_BADARG;
    if (!items || n <= 0 || n > LORA_MULTI_MAX) return UR_E_BADARG;
    const uintptr_t emask = (dtype == UR_DT_F32 ? 4 : 2) - 1;
    // every row is read and checked first: a bad item anywhere in the list is UR_E_BADARG, whatever else the list holds
    LoraItem rows[LORA_MULTI_MAX];
    bool over_cap = false;
    for (int i = 0; i < n; ++i) {
        const int64_t* r = items + (int64_t)i * LORA_ITEM_WORDS;
        const int64_t N = r[5], K = r[6], R = r[7];
        if (N <= 0 || N > 0x7fffffff || K <= 0 || K > 0x7fffffff || R < 0) return UR_E_BADARG;
        LoraItem& e = rows[i];
        e.base = reinterpret_cast<const void*>(r[0]);
        e.w = reinterpret_cast<void*>(r[1]);
        e.up = reinterpret_cast<const float*>(r[2]);
        e.down = reinterpret_cast<const float*>(r[3]);
        e.rscale = reinterpret_cast<const float*>(r[4]);
        if (!e.base || !e.w || e.w == e.base || (((uintptr_t)e.base | (uintptr_t)e.w) & emask)) return UR_E_BADARG;
        if (R > 0 && (!e.up || !e.down || (((uintptr_t)e.up | (uintptr_t)e.down | (uintptr_t)e.rscale) & 3))) return UR_E_BADARG;
        if (R > LORA_MAX_RANK) over_cap = true;
        e.N = (int32_t)N;
        e.K = (int32_t)K;
        e.R = R > LORA_MAX_RANK ? 0 : (int32_t)R;  // (over the limit: never launched)
        e.scale = __builtin_bit_cast(float, (uint32_t)(r[8] & 0xffffffff));
    }
    if (over_cap) return UR_E_UNSUPPORTED;
    LoraArgs a;
    const int rc = pack(rows, n, a.t, a.seg, UR_E_UNSUPPORTED, [](const LoraItem& e) -> int64_t {
        return (int64_t)((e.N + LT_N - 1) / LT_N) * ((e.K + LT_K - 1) / LT_K);
    });
    if (rc) return rc;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid(a.seg.total());
    if (dtype == UR_DT_F16) hipLaunchKernelGGL((lora_merge_multi_kernel<f16>), grid, dim3(256), 0, s, a);
    else if (dtype == UR_DT_BF16) hipLaunchKernelGGL((lora_merge_multi_kernel<bf16>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((lora_merge_multi_kernel<float>), grid, dim3(256), 0, s, a);
    return last_error();
}
extern "C" int ur_lora_multi_max(void) { return LORA_MULTI_MAX; }
extern "C" int ur_lora_max_rank(void) { return LORA_MAX_RANK; }
extern "C" int ur_lora_item_words(void) { return LORA_ITEM_WORDS; }
