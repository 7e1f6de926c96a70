// AdamW with block-wise dynamic 8-bit moments (ABI 17, include/ur_kernels.h; Dettmers et al., arXiv 2110.02861): what the
// reference's --use_8bit_adam selects (train/train.py:1101-1128).  4 + 4 + 1 + 1 B read and 4 + 1 + 1 B written per
// parameter plus 16 B of block scales per 256 of them, against the 16 + 12 B of the fp32 kernel (backward.hip).
//
// One wave owns one 256-element block, each lane 4 consecutive elements: p / g are 16-byte accesses, the codes one dword per
// moment, the two block maxima wave reductions (no LDS, no barrier).  The two code books sit in 2 KB of LDS (one barrier per
// workgroup, before the first block).  Decoding is a table read.  Encoding computes its candidate: the books are uniform
// inside a decade, so the decade (six compares) and the rounded linear position give an entry that brackets the value; the
// table entry on the value's side of it is the other bracket, and the nearer of the two is the nearest entry of the book --
// two table reads per value instead of an 8-step binary search.
#include "ur_launch.h"
#include "adam8_books.inc"

using namespace ur;

namespace {

constexpr int A8_BLOCK = 256;    // elements per absmax
constexpr int A8_CHUNK = 16384;  // elements per workgroup of the multi-tensor kernel (as adamw_multi_kernel)

// [0]: unsigned (exp_avg_sq), [1]: signed (exp_avg) -- indexed by is_signed
__device__ const float d_books[2][256] = {{UR_ADAM8_BOOK_UNSIGNED}, {UR_ADAM8_BOOK_SIGNED}};
const float h_books[2][256] = {{UR_ADAM8_BOOK_UNSIGNED}, {UR_ADAM8_BOOK_SIGNED}};

// both books into LDS: books[0 .. 256) unsigned, books[256 .. 512) signed
__device__ __forceinline__ void load_books(float* books) {
    for (int i = threadIdx.x; i < 512; i += blockDim.x) books[i] = (&d_books[0][0])[i];
    __syncthreads();
}

// The magnitudes of a book are q -> h[q]: h[0] = 0, then for decade i = 0..6 the N_i = 2^i (signed) / 2^(i+1) (unsigned)
// entries (0.1 + 0.9 (j + 0.5) / N_i) 10^(i-6), then 1.  Unsigned: h = the book.  Signed: h[q] = book[127 + q], -h[q] =
// book[127 - q] (there is no -1: q <= 127 for negative values).
// guess(a): for a = |x| / absmax in [0, 1] an index q such that h[q] is one of the two entries that bracket a (the nearest
// inside a's decade [10^(i-7), 10^(i-6)); below the first decade, its first entry).
template <bool SIGNED>
__device__ __forceinline__ int guess(float a) {
    const bool c1 = a >= 1e-6f, c2 = a >= 1e-5f, c3 = a >= 1e-4f, c4 = a >= 1e-3f, c5 = a >= 1e-2f, c6 = a >= 1e-1f;
    const int i = (int)c1 + (int)c2 + (int)c3 + (int)c4 + (int)c5 + (int)c6;
    const float scale = c6 ? 1.f : c5 ? 1e1f : c4 ? 1e2f : c3 ? 1e3f : c2 ? 1e4f : c1 ? 1e5f : 1e6f;
    const int N = (SIGNED ? 1 : 2) << i;
    const float pos = (a * scale - 0.1f) * ((float)N * (1.0f / 0.9f)) - 0.5f;
    int j = (int)rintf(pos);
    j = j < 0 ? 0 : (j > N - 1 ? N - 1 : j);
    return N + j - (SIGNED ? 0 : 1);
}

// the code of x in a block of maximum `absmax`: the index of the book entry nearest to x / absmax.  absmax == 0 gives the
// zero code without a division; a strictly positive value of the unsigned book never gets code 0.
template <bool SIGNED>
__device__ __forceinline__ uint32_t encode(float x, float absmax, const float* book) {
    const float a = absmax > 0.f ? fabsf(x) / absmax : 0.f;
    constexpr int off = SIGNED ? 127 : 0;
    const int qmax = SIGNED ? (x < 0.f ? 127 : 128) : 255;
    int q = guess<SIGNED>(a);
    const float b0 = book[off + q];
    int q1 = q + (a > b0 ? 1 : -1);
    q1 = q1 < 0 ? 0 : (q1 > qmax ? qmax : q1);
    const float b1 = book[off + q1];
    if (fabsf(a - b1) < fabsf(a - b0)) q = q1;
    if (!SIGNED && x > 0.f && q == 0) q = 1;
    return (uint32_t)(SIGNED ? (x < 0.f ? 127 - q : 127 + q) : q);
}

__device__ __forceinline__ float wave_max(float x) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) x = fmaxf(x, __shfl_xor(x, d));
    return x;
}

// the arithmetic of adamw_one (backward.hip), unchanged
__device__ __forceinline__ void adamw8_one(float& p, float g, float& m, float& v, float ginv, float decay, float b1, float b2,
                                           float step_size, float rbc2, float eps) {
    g /= ginv;
    p *= decay;
    m = m + (1.0f - b1) * (g - m);
    v = b2 * v + (1.0f - b2) * g * g;
    p -= step_size * m / (sqrtf(v) * rbc2 + eps);
}

// one row of ur_adamw8_multi's item table: seven 8-byte words
struct Adamw8Tensor {
    float* p;
    const float* g;
    uint8_t* m;
    uint8_t* v;
    float* absmax_m;
    float* absmax_v;
    int64_t n;
};
static_assert(sizeof(Adamw8Tensor) == 7 * sizeof(int64_t), "item table row");

struct Adamw8Args {
    Adamw8Tensor t[UR_ADAMW_MAX_TENSORS];
    SegTable<UR_ADAMW_MAX_TENSORS> seg;
    float lr, beta1, beta2, eps, wd;
    const float *step, *grad_scale, *found_inf;
    const float* hyper;
};
static_assert(sizeof(Adamw8Args) <= 4096, "kernel arguments");

typedef float f4 __attribute__((ext_vector_type(4)));

__global__ void __launch_bounds__(256) adamw8_multi_kernel(const Adamw8Args a) {
    if (a.found_inf && *a.found_inf != 0.f) return;
    __shared__ float books[512];
    load_books(books);
    const float *book_v = books, *book_m = books + 256;
    const int k = a.seg.find(blockIdx.x);
    const Adamw8Tensor t = a.t[k];
    const int64_t beg = (int64_t)((int)blockIdx.x - a.seg.start[k]) * A8_CHUNK;
    const int64_t end = beg + A8_CHUNK < t.n ? beg + A8_CHUNK : t.n;
    const float step = *a.step;
    const float bc1 = (float)(1.0 - pow((double)a.beta1, (double)step));
    const float bc2 = (float)(1.0 - pow((double)a.beta2, (double)step));
    const float lr = a.hyper ? a.hyper[0] : a.lr, wd = a.hyper ? a.hyper[1] : a.wd;
    const float step_size = lr / bc1, rbc2 = 1.0f / sqrtf(bc2), decay = 1.0f - lr * wd;
    const float ginv = a.grad_scale ? *a.grad_scale : 1.0f;
    const bool vec = ((((uintptr_t)t.p) | ((uintptr_t)t.g)) & 15) == 0 && ((((uintptr_t)t.m) | ((uintptr_t)t.v)) & 3) == 0;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    // the chunk is a multiple of the block: a block never straddles two workgroups, and only a tensor's last one is partial
    for (int64_t b0 = beg + wave * A8_BLOCK; b0 < end; b0 += 4 * A8_BLOCK) {
        const int64_t i = b0 + 4 * lane;
        const int cnt = t.n - i >= 4 ? 4 : (t.n - i > 0 ? (int)(t.n - i) : 0);
        const bool full = vec && cnt == 4;
        float p[4] = {0.f, 0.f, 0.f, 0.f}, g[4] = {0.f, 0.f, 0.f, 0.f};
        uint32_t cm = 0x7f7f7f7fu, cv = 0u;  // lanes / elements past the end compute on zeros and store nothing
        if (full) {
            const f4 pv = __builtin_nontemporal_load(reinterpret_cast<const f4*>(t.p + i));
            const f4 gv = __builtin_nontemporal_load(reinterpret_cast<const f4*>(t.g + i));
            cm = __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(t.m + i));
            cv = __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(t.v + i));
#pragma unroll
            for (int e = 0; e < 4; ++e) { p[e] = pv[e]; g[e] = gv[e]; }
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (e < cnt) {
                    p[e] = t.p[i + e];
                    g[e] = t.g[i + e];
                    cm = (cm & ~(0xffu << (8 * e))) | ((uint32_t)t.m[i + e] << (8 * e));
                    cv |= (uint32_t)t.v[i + e] << (8 * e);
                }
        }
        const int64_t blk = b0 / A8_BLOCK;
        const float am = t.absmax_m[blk], av = t.absmax_v[blk];
        float m[4], v[4], mx_m = 0.f, mx_v = 0.f;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            m[e] = book_m[(cm >> (8 * e)) & 0xff] * am;
            v[e] = book_v[(cv >> (8 * e)) & 0xff] * av;
            adamw8_one(p[e], g[e], m[e], v[e], ginv, decay, a.beta1, a.beta2, step_size, rbc2, a.eps);
            mx_m = fmaxf(mx_m, fabsf(m[e]));
            mx_v = fmaxf(mx_v, v[e]);
        }
        mx_m = wave_max(mx_m);
        mx_v = wave_max(mx_v);
        cm = cv = 0u;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            cm |= encode<true>(m[e], mx_m, book_m) << (8 * e);
            cv |= encode<false>(v[e], mx_v, book_v) << (8 * e);
        }
        if (full) {
            f4 pv;
#pragma unroll
            for (int e = 0; e < 4; ++e) pv[e] = p[e];
            __builtin_nontemporal_store(pv, reinterpret_cast<f4*>(t.p + i));
            __builtin_nontemporal_store(cm, reinterpret_cast<uint32_t*>(t.m + i));
            __builtin_nontemporal_store(cv, reinterpret_cast<uint32_t*>(t.v + i));
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (e < cnt) {
                    t.p[i + e] = p[e];
                    t.m[i + e] = (uint8_t)(cm >> (8 * e));
                    t.v[i + e] = (uint8_t)(cv >> (8 * e));
                }
        }
        if (lane == 0) {
            t.absmax_m[blk] = mx_m;
            t.absmax_v[blk] = mx_v;
        }
    }
}

// one wave per block, grid-stride over the blocks
template <bool SIGNED>
__global__ void __launch_bounds__(256) adam8_quantize_kernel(const float* x, uint8_t* codes, float* absmax, int64_t n) {
    __shared__ float books[512];
    load_books(books);
    const float* book = books + (SIGNED ? 256 : 0);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t nblk = (n + A8_BLOCK - 1) / A8_BLOCK;
    for (int64_t blk = (int64_t)blockIdx.x * 4 + wave; blk < nblk; blk += (int64_t)gridDim.x * 4) {
        const int64_t i = blk * A8_BLOCK + 4 * lane;
        float v[4], mx = 0.f;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            v[e] = i + e < n ? x[i + e] : 0.f;
            mx = fmaxf(mx, fabsf(v[e]));
        }
        mx = wave_max(mx);
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (i + e < n) codes[i + e] = (uint8_t)encode<SIGNED>(v[e], mx, book);
        if (lane == 0) absmax[blk] = mx;
    }
}

__global__ void __launch_bounds__(256) adam8_dequantize_kernel(float* x, const uint8_t* codes, const float* absmax, int64_t n,
                                                               int is_signed) {
    __shared__ float books[512];
    load_books(books);
    const float* book = books + (is_signed ? 256 : 0);
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
        x[i] = book[codes[i]] * absmax[i / A8_BLOCK];
}

}  // namespace

extern "C" int ur_adamw8_multi(const int64_t* items, int n_tensors, float lr, float beta1, float beta2, float eps,
                               float weight_decay, const float* step, const float* grad_scale, const float* found_inf,
                               const float* hyper, void* stream) {
    if (!step || !(beta1 >= 0.f && beta1 < 1.f) || !(beta2 >= 0.f && beta2 < 1.f))  // as ur_adamw_multi
        return UR_E_BADARG;
    Adamw8Args a;
    const int rc = pack(reinterpret_cast<const Adamw8Tensor*>(items), n_tensors, a.t, a.seg, UR_E_BADARG, [](const Adamw8Tensor& t) -> int64_t {
        if (!t.p || !t.g || !t.m || !t.v || !t.absmax_m || !t.absmax_v || t.n <= 0) return 0;
        return (t.n + A8_CHUNK - 1) / A8_CHUNK;
    });
    if (rc) return rc;
    a.lr = lr; a.beta1 = beta1; a.beta2 = beta2; a.eps = eps; a.wd = weight_decay;
    a.step = step; a.grad_scale = grad_scale; a.found_inf = found_inf; a.hyper = hyper;
    hipLaunchKernelGGL(adamw8_multi_kernel, dim3(a.seg.total()), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), a);
    return last_error();
}

extern "C" int ur_adam8_quantize(const float* x, uint8_t* codes, float* absmax, int64_t n, int is_signed, void* stream) {
    if (!x || !codes || !absmax || n <= 0) return UR_E_BADARG;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int grid = grid_for((n + 3) / 4, 16384);  // 4 blocks of 256 elements per workgroup
    if (is_signed) hipLaunchKernelGGL(adam8_quantize_kernel<true>, dim3(grid), dim3(256), 0, s, x, codes, absmax, n);
    else hipLaunchKernelGGL(adam8_quantize_kernel<false>, dim3(grid), dim3(256), 0, s, x, codes, absmax, n);
    return last_error();
}

extern "C" int ur_adam8_dequantize(float* x, const uint8_t* codes, const float* absmax, int64_t n, int is_signed, void* stream) {
    if (!x || !codes || !absmax || n <= 0) return UR_E_BADARG;
    hipLaunchKernelGGL(adam8_dequantize_kernel, dim3(grid_for(n, 16384)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), x,
                       codes, absmax, n, is_signed);
    return last_error();
}

extern "C" int ur_adam8_codebook(int is_signed, float* out256) {
    if (!out256) return UR_E_BADARG;
    for (int i = 0; i < 256; ++i) out256[i] = h_books[is_signed ? 1 : 0][i];
    return 0;
}
