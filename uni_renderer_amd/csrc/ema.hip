// Exponential moving average of the weights (an addition to ABI 17, include/ur_kernels.h): what diffusers'
// training_utils.EMAModel does once per optimisation step, `s.sub_(one_minus_decay * (s - p))` per parameter tensor, as
// one launch per 64 tensors.  4 B (the fp32 parameter; 2 B for a 16-bit one) + 4 B read and 4 B written per element.
//
// The decay schedule lives on the device: ur_ema_advance (one thread) counts the step and evaluates get_decay in fp64
// into two device scalars, and ur_ema_multi reads one_minus_decay from there -- a captured graph advances its own
// schedule on every replay and holds no step number.
//
// The update is THREE separately rounded fp32 operations, t = s - p, u = d * t, s = s - u: torch's arithmetic for the
// line above.  A contraction of the last two into an fma changes a third of the elements at steps 2 to 5, so
// contraction is switched off for this whole file (here and in the Makefile).
#include "ur_launch.h"

#pragma clang fp contract(off)

using namespace ur;

namespace {

constexpr int EMA_MAX_TENSORS = 64;  // UR_EMA_MAX_TENSORS of the header's text (the constant census of the header is pinned)
constexpr int EMA_CHUNK = 16384;     // elements one workgroup owns (as adamw_multi_kernel): a multiple of 4 * 256
constexpr int64_t EMA_DTYPE_MASK = 0xff, EMA_COPY = 0x100;

// one row of ur_ema_multi's item table: four 8-byte words
struct EmaTensor {
    float* s;
    const void* p;
    int64_t n;
    int64_t flags;
};
static_assert(sizeof(EmaTensor) == 4 * sizeof(int64_t), "item table row");

struct EmaArgs {
    EmaTensor t[EMA_MAX_TENSORS];
    SegTable<EMA_MAX_TENSORS> seg;
    const float* one_minus_decay;
};
static_assert(sizeof(EmaArgs) <= 4096, "kernel arguments");

template <typename T, int N> struct VecOf { typedef T type __attribute__((ext_vector_type(N))); };

// exact: every fp16 / bf16 value is an fp32 value
template <typename T> __device__ __forceinline__ float widen(T v) { return (float)v; }

template <bool COPY>
__device__ __forceinline__ float ema_one(float s, float p, float d) {
    if (COPY) return p;
    const float t = s - p;  // (no contraction in this file: three roundings)
    const float u = d * t;
    return s - u;
}

// the elements [beg, end) of one tensor, by one workgroup.  beg is a multiple of EMA_CHUNK, so a 16-byte aligned pair of
// base addresses stays aligned at every group of four.  Both streams are touched once per step and never again before they
// have left every cache: non-temporal loads and stores (3.85 ms against 4.00 ms for the SD-1.x sized update, profiles/ema_ab.txt)
template <typename T, bool COPY>
__device__ __forceinline__ void ema_chunk(float* __restrict__ s, const T* __restrict__ p, int64_t beg, int64_t end, float d) {
    typedef typename VecOf<T, 4>::type p4;
    const bool vec = ((((uintptr_t)s) | ((uintptr_t)p)) & 15) == 0;
    int64_t done = beg;  // [beg, done) is covered by the vector loop
    if (vec) {
        done = beg + ((end - beg) & ~(int64_t)3);
        for (int64_t i = beg + 4 * (int64_t)threadIdx.x; i < done; i += 4 * 256) {
            const p4 pv = __builtin_nontemporal_load(reinterpret_cast<const p4*>(p + i));
            f32x4 sv;
            if (!COPY) sv = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(s + i));
#pragma unroll
            for (int e = 0; e < 4; ++e) sv[e] = ema_one<COPY>(COPY ? 0.f : sv[e], widen(pv[e]), d);
            __builtin_nontemporal_store(sv, reinterpret_cast<f32x4*>(s + i));
        }
    }
    for (int64_t i = done + threadIdx.x; i < end; i += 256) s[i] = ema_one<COPY>(COPY ? 0.f : s[i], widen(p[i]), d);
}

template <typename T>
__device__ __forceinline__ void ema_dispatch(const EmaTensor& t, int64_t beg, int64_t end, float d) {
    const T* p = reinterpret_cast<const T*>(t.p);
    if (t.flags & EMA_COPY) ema_chunk<T, true>(t.s, p, beg, end, d);
    else ema_chunk<T, false>(t.s, p, beg, end, d);
}

__global__ void __launch_bounds__(256) ema_multi_kernel(const EmaArgs a) {
    const int k = a.seg.find(blockIdx.x);
    const EmaTensor t = a.t[k];
    const int64_t beg = (int64_t)((int)blockIdx.x - a.seg.start[k]) * EMA_CHUNK;
    const int64_t end = beg + EMA_CHUNK < t.n ? beg + EMA_CHUNK : t.n;
    const float d = *a.one_minus_decay;
    const int dt = (int)(t.flags & EMA_DTYPE_MASK);
    if (dt == UR_DT_F32) ema_dispatch<float>(t, beg, end, d);
    else if (dt == UR_DT_F16) ema_dispatch<f16>(t, beg, end, d);
    else ema_dispatch<bf16>(t, beg, end, d);
}

// diffusers 0.24 EMAModel.get_decay, restated (include/ur_kernels.h)
__global__ void ema_advance_kernel(int64_t* step, int64_t update_after_step, int use_ema_warmup, double inv_gamma, double power,
                                   double min_decay, double decay, double* cur_decay, float* one_minus_decay) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const int64_t now = *step + 1;
    *step = now;
    const int64_t k = now - update_after_step - 1 > 0 ? now - update_after_step - 1 : 0;
    double v = 0.0;
    if (k > 0) {
        v = use_ema_warmup ? 1.0 - pow(1.0 + (double)k / inv_gamma, -power) : (1.0 + (double)k) / (10.0 + (double)k);
        v = v < decay ? v : decay;          // min(., decay)
        v = v > min_decay ? v : min_decay;  // max(., min_decay)
    }
    *cur_decay = v;
    *one_minus_decay = (float)(1.0 - v);
}

}  // namespace

extern "C" int ur_ema_multi_max(void) { return EMA_MAX_TENSORS; }
extern "C" int ur_ema_item_words(void) { return (int)(sizeof(EmaTensor) / sizeof(int64_t)); }
extern "C" int ur_ema_block_elems(void) { return EMA_CHUNK; }

extern "C" int ur_ema_advance(int64_t* step, int64_t update_after_step, int use_ema_warmup, const double* schedule,
                              double* cur_decay, float* one_minus_decay, void* stream) {
    if (!step || !schedule || !cur_decay || !one_minus_decay) return UR_E_BADARG;
    const double inv_gamma = schedule[0], power = schedule[1], min_decay = schedule[2], decay = schedule[3];
    if (!(inv_gamma > 0.0) || !(min_decay >= 0.0 && min_decay <= 1.0) || !(decay >= 0.0 && decay <= 1.0) || power != power)
        return UR_E_BADARG;
    hipLaunchKernelGGL(ema_advance_kernel, dim3(1), dim3(1), 0, reinterpret_cast<hipStream_t>(stream), step, update_after_step,
                       use_ema_warmup, inv_gamma, power, min_decay, decay, cur_decay, one_minus_decay);
    return last_error();
}

extern "C" int ur_ema_multi(const int64_t* items, int n_tensors, const float* one_minus_decay, void* stream) {
    if (!one_minus_decay) return UR_E_BADARG;
    EmaArgs a;
    const int rc = pack(reinterpret_cast<const EmaTensor*>(items), n_tensors, a.t, a.seg, UR_E_BADARG, [](const EmaTensor& t) -> int64_t {
        const int64_t dt = t.flags & EMA_DTYPE_MASK;
        if (!t.s || !t.p || t.n <= 0 || (t.flags & ~(EMA_DTYPE_MASK | EMA_COPY))) return 0;
        if (dt != UR_DT_F32 && dt != UR_DT_F16 && dt != UR_DT_BF16) return 0;
        if (((uintptr_t)t.s & 3) || ((uintptr_t)t.p & (dt == UR_DT_F32 ? 3 : 1))) return 0;  // element alignment
        return (t.n + EMA_CHUNK - 1) / EMA_CHUNK;
    });
    if (rc) return rc;
    a.one_minus_decay = one_minus_decay;
    hipLaunchKernelGGL(ema_multi_kernel, dim3(a.seg.total()), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), a);
    return last_error();
}
