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
//
// ur_lora_merge_cast_multi is the same kernel body with `base` read in one dtype and `w` written in another (the fp32 master
// weights of a training step merged straight into the compute-dtype operand): same chain, still ONE rounding.
//
// ur_lora_grad_multi is the backward of the merge with respect to the factors, from the weight gradient dW' [N][K]:
//     d_up[n][r] = scale * rscale[r] * sum_k dW'[n][k] * down[r][k],   d_down[r][k] = scale * rscale[r] * sum_n up[n][r] * dW'[n][k]
// One launch, two kinds of workgroups per item, both with the thread layout of the merge kernel (thread (ty, tx) holds a
// 4 x 4 patch of a 32 x 128 tile of dW' in registers, read straight from memory):
//   * a "row" workgroup owns 32 rows x 16 ranks of d_up and walks the K tiles of its rows in ascending order: the chunk of
//     `down` is staged in LDS, every thread keeps 4 x 16 partial sums over its own columns, and at the end the 32 column
//     lanes are added by a butterfly of lane exchanges (a fixed tree);
//   * a "column" workgroup owns 16 ranks x 32 columns of d_down and walks N in tiles of 128 rows x 32 columns in ascending
//     order (thread (ty, tx) = (tid >> 3, tid & 7): narrow and tall, so that a K = 1280 matrix has 40 of them and a walk over
//     N = 10240 rows takes 80 steps): the chunk of `up` is staged in LDS, every thread keeps 16 x 4 partial sums over its own
//     rows, and at the end the 8 row groups of a wave are added by a butterfly and the 4 waves through LDS in ascending order.
// In both, the next patch of dW' and the tile's factor chunk are requested before the barrier that frees the LDS buffer.
// dW' is therefore read twice per 16 ranks.  Every sum's order is a function of (N, K, R) alone: no atomics, nothing depends
// on the other items, their order or the grid.  The factor fl(scale * rscale[r]) multiplies the finished sum (one rounding
// each).  Items whose dW' rows do not allow the 4-element access take the element-wise loads.
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

template <typename TB, typename TO> struct SameType { static constexpr bool value = false; };
template <typename T> struct SameType<T, T> { static constexpr bool value = true; };

// TB: the dtype `base` is read in, T: the dtype `w` is written in (TB == T: ur_lora_merge_multi)
template <typename TB, typename T>
__global__ void __launch_bounds__(256) lora_merge_multi_kernel(const LoraArgs a) {
    typedef typename BitsOf<sizeof(T)>::type bits_t;
    constexpr bool same = SameType<TB, T>::value;
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
    const bool wide = (K & 3) == 0 && ((uintptr_t)e.base & (4 * sizeof(TB) - 1)) == 0 &&
                      ((uintptr_t)e.w & (4 * sizeof(T) - 1)) == 0;  // workgroup-uniform

    if (same && R == 0) {  // the copy path of unfuse / unload: bits, not values
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

    const TB* base = (const TB*)e.base;
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
                    const Quad<TB> q = *reinterpret_cast<const Quad<TB>*>(base + o);
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
    const bool plain = !same && R == 0;  // a cast of `base` alone (no arithmetic that a non-finite scale could spoil)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int row = row0 + j;
        if (row >= N) break;
        const int64_t o = (int64_t)row * K + col0;
        if (wide) {
            if (col0 < K) {
                Quad<T> q;
#pragma unroll
                for (int c = 0; c < 4; ++c) q.v[c] = (T)(plain ? b[j][c] : __builtin_fmaf(scale, acc[j][c], b[j][c]));
                *reinterpret_cast<Quad<T>*>(w + o) = q;
            }
        } else {
#pragma unroll
            for (int c = 0; c < 4; ++c)
                if (col0 + c < K) w[o + c] = (T)(plain ? b[j][c] : __builtin_fmaf(scale, acc[j][c], b[j][c]));
        }
    }
}

// ---- the factor gradients (ur_lora_grad_multi) -------------------------------------------------------------------------
constexpr int LORA_GRAD_ITEM_WORDS = 10;  // dw, up, down, rscale, d_up, d_down, N, K, R, scale bits

struct LoraGradItem {
    const void* dw;
    const float* up;
    const float* down;
    const float* rscale;
    float* d_up;
    float* d_down;
    int32_t N, K, R;
    float scale;
};

struct LoraGradArgs {
    LoraGradItem t[LORA_MULTI_MAX];
    SegTable<LORA_MULTI_MAX> seg;
};
static_assert(sizeof(LoraGradArgs) <= 4096, "kernel arguments");

// the 4 x 4 patch of dW' at (row0, col0) as fp32, zeros outside the matrix
template <typename T>
__device__ __forceinline__ void lora_load_patch(const T* dw, int N, int K, int64_t row0, int64_t col0, bool wide, float (&g)[4][4]) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int64_t row = row0 + j;  // 64-bit: a prefetch may name a patch past 2^31 - 1 (it then loads nothing)
        const int64_t o = row * K + col0;
#pragma unroll
        for (int c = 0; c < 4; ++c) g[j][c] = 0.f;
        if (row < N) {
            if (wide) {
                if (col0 < K) {
                    const Quad<T> q = *reinterpret_cast<const Quad<T>*>(dw + o);
#pragma unroll
                    for (int c = 0; c < 4; ++c) g[j][c] = (float)q.v[c];
                }
            } else {
#pragma unroll
                for (int c = 0; c < 4; ++c)
                    if (col0 + c < K) g[j][c] = (float)dw[o + c];
            }
        }
    }
}

constexpr int GD_N = 128, GD_K = 32;  // the tile of a column workgroup: 128 rows x 32 columns (thread (ty, tx) = (tid >> 3, tid & 7))

template <typename T>
__global__ void __launch_bounds__(256) lora_grad_multi_kernel(const LoraGradArgs a) {
    __shared__ __attribute__((aligned(16))) float s_fac[LT_R * LT_K];      // the chunk of `down` (row workgroups) or `up` (column ones)
    __shared__ __attribute__((aligned(16))) float s_red[4 * LT_R * GD_K];  // per-wave partial sums of a column workgroup

    const int it = a.seg.find(blockIdx.x);
    const LoraGradItem e = a.t[it];
    const int N = e.N, K = e.K, R = e.R;
    const int ntiles = (int)(((int64_t)N + LT_N - 1) / LT_N), ktiles = (int)(((int64_t)K + LT_K - 1) / LT_K);  // N, K up to 2^31 - 1
    const int rchunks = (R + LT_R - 1) / LT_R;
    const int lb = (int)blockIdx.x - a.seg.start[it];
    const int tid = threadIdx.x;
    const T* dw = (const T*)e.dw;
    const bool wide = (K & 3) == 0 && ((uintptr_t)e.dw & (4 * sizeof(T) - 1)) == 0;  // workgroup-uniform
    float g[4][4], gn[4][4], st[LT_R * LT_K / 256];

    if (lb < ntiles * rchunks) {
        // ---- d_up: rows n0 .. n0 + 31, ranks r0 .. r0 + 15, all of K (tiles of 32 x 128, thread (ty, tx) = (tid >> 5, tid & 31)) ----
        const int tx = tid & 31, ty = tid >> 5;
        const int n0 = (lb / rchunks) * LT_N, r0 = (lb % rchunks) * LT_R;
        const int rc = min(LT_R, R - r0);
        const int row0 = n0 + 4 * ty;
        float acc[4][LT_R];
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int rr = 0; rr < LT_R; ++rr) acc[j][rr] = 0.f;
        lora_load_patch(dw, N, K, row0, 4 * tx, wide, g);
        for (int kt = 0; kt < ktiles; ++kt) {
            const int k0 = kt * LT_K;
            // the next patch and this tile's chunk of `down` are requested before the barrier: their latency hides behind it
            if (kt + 1 < ktiles) lora_load_patch(dw, N, K, row0, (int64_t)k0 + LT_K + 4 * tx, wide, gn);
#pragma unroll
            for (int i = 0; i < LT_R * LT_K / 256; ++i) {
                const int idx = tid + 256 * i, rr = idx / LT_K, cc = idx % LT_K;
                st[i] = (rr < rc && k0 + cc < K) ? e.down[(int64_t)(r0 + rr) * K + k0 + cc] : 0.f;
            }
            if (kt) __syncthreads();  // the previous chunk has been consumed
#pragma unroll
            for (int i = 0; i < LT_R * LT_K / 256; ++i) s_fac[tid + 256 * i] = st[i];
            __syncthreads();
#pragma unroll
            for (int rr = 0; rr < LT_R; ++rr) {  // ranks >= R hold zeros
                const f32x4 d = *reinterpret_cast<const f32x4*>(s_fac + rr * LT_K + 4 * tx);
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int c = 0; c < 4; ++c) acc[j][rr] = __builtin_fmaf(g[j][c], d[c], acc[j][rr]);
            }
            if (kt + 1 < ktiles) {
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int c = 0; c < 4; ++c) g[j][c] = gn[j][c];
            }
        }
        // the 32 column lanes of a row group: a butterfly, every lane ends with the same sum
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int rr = 0; rr < LT_R; ++rr) {
                float v = acc[j][rr];
#pragma unroll
                for (int m = 1; m < 32; m <<= 1) v += __shfl_xor(v, m, 64);
                acc[j][rr] = v;
            }
        if (tx == 0) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int row = row0 + j;
                if (row >= N) break;
#pragma unroll
                for (int rr = 0; rr < LT_R; ++rr)
                    if (rr < rc) {
                        const float f = e.rscale ? e.scale * e.rscale[r0 + rr] : e.scale;
                        e.d_up[(int64_t)row * R + r0 + rr] = f * acc[j][rr];
                    }
            }
        }
        return;
    }

    // ---- d_down: ranks r0 .. r0 + 15, columns k0 .. k0 + 31, all of N (tiles of 128 x 32, thread (ty, tx) = (tid >> 3, tid & 7)) ----
    const int tx = tid & 7, ty = tid >> 3;
    const int lc = lb - ntiles * rchunks;
    const int k0 = (lc / rchunks) * GD_K, r0 = (lc % rchunks) * LT_R;
    const int rc = min(LT_R, R - r0);
    const int col0 = k0 + 4 * tx;
    const int ntall = (int)(((int64_t)N + GD_N - 1) / GD_N);
    float acc[LT_R][4];
#pragma unroll
    for (int rr = 0; rr < LT_R; ++rr)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[rr][c] = 0.f;
    lora_load_patch(dw, N, K, 4 * ty, col0, wide, g);
    for (int nt = 0; nt < ntall; ++nt) {
        const int n0 = nt * GD_N;
        if (nt + 1 < ntall) lora_load_patch(dw, N, K, (int64_t)n0 + GD_N + 4 * ty, col0, wide, gn);
#pragma unroll
        for (int i = 0; i < LT_R * GD_N / 256; ++i) {
            const int idx = tid + 256 * i, rr = idx / GD_N, row = idx % GD_N;
            st[i] = (rr < rc && n0 + row < N) ? e.up[(int64_t)(n0 + row) * R + r0 + rr] : 0.f;
        }
        if (nt) __syncthreads();
#pragma unroll
        for (int i = 0; i < LT_R * GD_N / 256; ++i) s_fac[tid + 256 * i] = st[i];
        __syncthreads();
#pragma unroll
        for (int rr = 0; rr < LT_R; ++rr) {
            const f32x4 u = *reinterpret_cast<const f32x4*>(s_fac + rr * GD_N + 4 * ty);
#pragma unroll
            for (int c = 0; c < 4; ++c)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[rr][c] = __builtin_fmaf(u[j], g[j][c], acc[rr][c]);
        }
        if (nt + 1 < ntall) {
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int c = 0; c < 4; ++c) g[j][c] = gn[j][c];
        }
    }
    // the eight row groups of a wave (a butterfly over lane bits 3 .. 5), then the four waves in ascending order
    const int wave = tid >> 6;
#pragma unroll
    for (int rr = 0; rr < LT_R; ++rr) {
        f32x4 v;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            float x = acc[rr][c];
#pragma unroll
            for (int m = 8; m < 64; m <<= 1) x += __shfl_xor(x, m, 64);
            v[c] = x;
        }
        if ((tid & 63) < 8) *reinterpret_cast<f32x4*>(s_red + (wave * LT_R + rr) * GD_K + 4 * tx) = v;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < LT_R * GD_K / 256; ++i) {
        const int idx = tid + 256 * i, rr = idx / GD_K, cc = idx % GD_K;
        if (rr < rc && k0 + cc < K) {
            float v = s_red[idx];
#pragma unroll
            for (int w_ = 1; w_ < 4; ++w_) v += s_red[w_ * LT_R * GD_K + idx];
            const float f = e.rscale ? e.scale * e.rscale[r0 + rr] : e.scale;
            e.d_down[(int64_t)(r0 + rr) * K + k0 + cc] = f * v;
        }
    }
}

}  // namespace ur

using namespace ur;

static bool lora_dtype_ok(int dt) { return dt == UR_DT_F16 || dt == UR_DT_BF16 || dt == UR_DT_F32; }

template <typename TB>
static void lora_merge_launch(int out_dtype, dim3 grid, hipStream_t s, const LoraArgs& a) {
    if (out_dtype == UR_DT_F16) hipLaunchKernelGGL((lora_merge_multi_kernel<TB, f16>), grid, dim3(256), 0, s, a);
    else if (out_dtype == UR_DT_BF16) hipLaunchKernelGGL((lora_merge_multi_kernel<TB, bf16>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((lora_merge_multi_kernel<TB, float>), grid, dim3(256), 0, s, a);
}

extern "C" int ur_lora_merge_cast_multi(const int64_t* items, int n, int base_dtype, int out_dtype, void* stream) {
    if (!lora_dtype_ok(base_dtype) || !lora_dtype_ok(out_dtype)) return UR_E_BADARG;
    if (!items || n <= 0 || n > LORA_MULTI_MAX) return UR_E_BADARG;
    const uintptr_t bmask = (base_dtype == UR_DT_F32 ? 4 : 2) - 1, omask = (out_dtype == UR_DT_F32 ? 4 : 2) - 1;
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
        if (!e.base || !e.w || e.w == e.base || ((uintptr_t)e.base & bmask) || ((uintptr_t)e.w & omask)) return UR_E_BADARG;
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
    if (base_dtype == UR_DT_F16) lora_merge_launch<f16>(out_dtype, grid, s, a);
    else if (base_dtype == UR_DT_BF16) lora_merge_launch<bf16>(out_dtype, grid, s, a);
    else lora_merge_launch<float>(out_dtype, grid, s, a);
    return last_error();
}
extern "C" int ur_lora_merge_multi(const int64_t* items, int n, int dtype, void* stream) {
    return ur_lora_merge_cast_multi(items, n, dtype, dtype, stream);
}

// [p, p + bytes) and [q, q + qbytes) share a byte (sizes below 2^64; an end past the address space counts as its top)
static bool lora_overlap(const void* p, uint64_t bytes, const void* q, uint64_t qbytes) {
    const uint64_t a0 = (uint64_t)(uintptr_t)p, b0 = (uint64_t)(uintptr_t)q;
    const uint64_t a1 = a0 + bytes < a0 ? ~0ull : a0 + bytes, b1 = b0 + qbytes < b0 ? ~0ull : b0 + qbytes;
    return q && a0 < b1 && b0 < a1;
}

extern "C" int ur_lora_grad_multi(const int64_t* items, int n, int dw_dtype, void* stream) {
    if (!lora_dtype_ok(dw_dtype)) return UR_E_BADARG;
    if (!items || n <= 0 || n > LORA_MULTI_MAX) return UR_E_BADARG;
    const uint64_t esz = dw_dtype == UR_DT_F32 ? 4 : 2;
    LoraGradItem rows[LORA_MULTI_MAX];
    bool over_cap = false;
    for (int i = 0; i < n; ++i) {
        const int64_t* r = items + (int64_t)i * LORA_GRAD_ITEM_WORDS;
        const int64_t N = r[6], K = r[7], R = r[8];
        if (N <= 0 || N > 0x7fffffff || K <= 0 || K > 0x7fffffff || R <= 0) return UR_E_BADARG;
        LoraGradItem& e = rows[i];
        e.dw = reinterpret_cast<const void*>(r[0]);
        e.up = reinterpret_cast<const float*>(r[1]);
        e.down = reinterpret_cast<const float*>(r[2]);
        e.rscale = reinterpret_cast<const float*>(r[3]);
        e.d_up = reinterpret_cast<float*>(r[4]);
        e.d_down = reinterpret_cast<float*>(r[5]);
        if (!e.dw || !e.up || !e.down || !e.d_up || !e.d_down) return UR_E_BADARG;
        if (((uintptr_t)e.dw & (uintptr_t)(esz - 1)) ||
            (((uintptr_t)e.up | (uintptr_t)e.down | (uintptr_t)e.rscale | (uintptr_t)e.d_up | (uintptr_t)e.d_down) & 3))
            return UR_E_BADARG;
        if (R > LORA_MAX_RANK) {  // (never launched; the sizes below would mean nothing)
            over_cap = true;
            continue;
        }
        const uint64_t bu = (uint64_t)N * R * 4, bd = (uint64_t)R * K * 4;  // N, K < 2^31, R <= 512: below 2^43
        const void* outs[2] = {e.d_up, e.d_down};
        const uint64_t osz[2] = {bu, bd};
        for (int o = 0; o < 2; ++o)
            if (lora_overlap(outs[o], osz[o], e.dw, (uint64_t)N * K * esz) || lora_overlap(outs[o], osz[o], e.up, bu) ||
                lora_overlap(outs[o], osz[o], e.down, bd) || lora_overlap(outs[o], osz[o], e.rscale, (uint64_t)R * 4))
                return UR_E_BADARG;
        if (lora_overlap(e.d_up, bu, e.d_down, bd)) return UR_E_BADARG;
        e.N = (int32_t)N;
        e.K = (int32_t)K;
        e.R = (int32_t)R;
        e.scale = __builtin_bit_cast(float, (uint32_t)(r[9] & 0xffffffff));
    }
    if (over_cap) return UR_E_UNSUPPORTED;
    LoraGradArgs a;
    const int rc = pack(rows, n, a.t, a.seg, UR_E_UNSUPPORTED, [](const LoraGradItem& e) -> int64_t {
        const int64_t rchunks = (e.R + LT_R - 1) / LT_R;
        return rchunks * (((int64_t)e.N + LT_N - 1) / LT_N) + rchunks * (((int64_t)e.K + GD_K - 1) / GD_K);
    });
    if (rc) return rc;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid(a.seg.total());
    if (dw_dtype == UR_DT_F16) hipLaunchKernelGGL((lora_grad_multi_kernel<f16>), grid, dim3(256), 0, s, a);
    else if (dw_dtype == UR_DT_BF16) hipLaunchKernelGGL((lora_grad_multi_kernel<bf16>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((lora_grad_multi_kernel<float>), grid, dim3(256), 0, s, a);
    return last_error();
}
extern "C" int ur_lora_grad_item_words(void) { return LORA_GRAD_ITEM_WORDS; }
extern "C" int ur_lora_multi_max(void) { return LORA_MULTI_MAX; }
extern "C" int ur_lora_max_rank(void) { return LORA_MAX_RANK; }
extern "C" int ur_lora_item_words(void) { return LORA_ITEM_WORDS; }
