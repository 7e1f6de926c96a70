// Small HBM-bound helpers: elementwise add (the enc->unet skip exchange), sinusoidal timestep
// embedding, and NCHW <-> NHWC layout glue at the module boundary.
#include "ur_launch.h"

namespace ur {

template <typename T>
__global__ void __launch_bounds__(256) add_kernel(const T* __restrict__ a, const T* __restrict__ b, float alpha,
                                                  T* __restrict__ out, int64_t nvec) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nvec; i += (int64_t)gridDim.x * blockDim.x) {
        float x[8], y[8];
        load8(a + i * 8, x);
        load8(b + i * 8, y);
#pragma unroll
        for (int k = 0; k < 8; ++k) x[k] += alpha * y[k];
        store8(out + i * 8, x);
    }
}

// diffusers get_timestep_embedding: emb = t * exp(-ln(1e4) * i / (half - shift)); [sin | cos], flipped
// to [cos | sin] when flip_sin_to_cos.
template <typename T>
__global__ void timestep_kernel(const float* __restrict__ t, int nt, int B, int dim, int flip, float shift,
                                T* __restrict__ out) {
    const int half = dim / 2;
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= B * half) return;
    const int b = idx / half, i = idx - b * half;
    const float tv = t[nt == 1 ? 0 : b];
    const float freq = expf(-9.210340371976184f * (float)i / ((float)half - shift));
    const float arg = tv * freq;
    const float s = sinf(arg), c = cosf(arg);
    T* o = out + (int64_t)b * dim;
    if (flip) { o[i] = (T)c; o[half + i] = (T)s; }
    else { o[i] = (T)s; o[half + i] = (T)c; }
    if ((dim & 1) && i == 0) o[dim - 1] = (T)0.f;
}

template <typename S> __device__ __forceinline__ float ld_any(const S* p, int64_t i) { return (float)p[i]; }

template <typename S, typename T>
__global__ void __launch_bounds__(256) nchw_to_nhwc_kernel(const S* __restrict__ src, int B, int C, int H, int W,
                                                           T* __restrict__ dst, int Cpad) {
    const int64_t total = (int64_t)B * H * W * Cpad;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % Cpad);
        const int64_t pix = i / Cpad;
        const int x = (int)(pix % W);
        const int y = (int)((pix / W) % H);
        const int b = (int)(pix / ((int64_t)W * H));
        float v = 0.f;
        if (c < C) v = (float)src[(((int64_t)b * C + c) * H + y) * W + x];
        dst[i] = (T)v;
    }
}

template <typename T, typename S>
__global__ void __launch_bounds__(256) nhwc_to_nchw_kernel(const T* __restrict__ src, int B, int C, int H, int W,
                                                           S* __restrict__ dst) {
    const int64_t total = (int64_t)B * C * H * W;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int x = (int)(i % W);
        const int y = (int)((i / W) % H);
        const int c = (int)((i / ((int64_t)W * H)) % C);
        const int b = (int)(i / ((int64_t)W * H * C));
        dst[i] = (S)(float)src[(((int64_t)b * H + y) * W + x) * C + c];
    }
}

constexpr int EW_BLOCKS = 2048;  // most workgroups of this file's grid-stride kernels (grid_for)

// out[b][oy][ox][:] = in[b][sy(oy)][sx(ox)][:] with PyTorch's 'nearest' rule: s(o) = min(floor(o * (float)in / out), in - 1)
// (F.interpolate(size=...) of Upsample2D when the latent side is not a multiple of 8, controlnet.py:1129-1130).
template <typename T>
__global__ void __launch_bounds__(256) resize_nearest_kernel(const T* __restrict__ in, T* __restrict__ out, int B, int Hin,
                                                             int Win, int Hout, int Wout, int C) {
    const int nvec = C >> 3;
    const int64_t total = (int64_t)B * Hout * Wout * nvec;
    const float sh = (float)Hin / (float)Hout, sw = (float)Win / (float)Wout;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int cv = (int)(i % nvec);
        const int64_t pix = i / nvec;
        const int ox = (int)(pix % Wout);
        const int oy = (int)((pix / Wout) % Hout);
        const int b = (int)(pix / ((int64_t)Wout * Hout));
        const int sy = min((int)floorf(oy * sh), Hin - 1), sx = min((int)floorf(ox * sw), Win - 1);
        typedef typename Vec8<T>::type vec8;
        *reinterpret_cast<vec8*>(out + pix * C + cv * 8) =
            *reinterpret_cast<const vec8*>(in + (((int64_t)b * Hin + sy) * Win + sx) * C + cv * 8);
    }
}

}  // namespace ur

using namespace ur;

extern "C" int ur_add(const void* a, const void* b, float alpha, void* out, int64_t n, int dtype, void* stream) {
    if (!a || !b || !out || n <= 0 || (n & 7)) return UR_E_BADARG;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int64_t nvec = n / 8;
    UR_DISPATCH(dtype, hipLaunchKernelGGL((add_kernel<T>), dim3(grid_for(nvec, EW_BLOCKS)), dim3(256), 0, s, (const T*)a,
                       (const T*)b, alpha, (T*)out, nvec));
    return last_error();
}

template <typename T>
__global__ void __launch_bounds__(256) add_hilo_kernel(const T* __restrict__ a, const lo_t<T>* __restrict__ a_lo,
                                                       const T* __restrict__ b, const lo_t<T>* __restrict__ b_lo, float alpha,
                                                       T* __restrict__ out, lo_t<T>* __restrict__ out_lo, int64_t nvec) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nvec; i += (int64_t)gridDim.x * blockDim.x) {
        float x[8], y[8], t[8];
        load8(a + i * 8, x);
        load8(b + i * 8, y);
        if (a_lo) {
            load_lo<8>(a_lo + i * 8, t);
#pragma unroll
            for (int k = 0; k < 8; ++k) x[k] += t[k];
        }
        if (b_lo) {
            load_lo<8>(b_lo + i * 8, t);
#pragma unroll
            for (int k = 0; k < 8; ++k) y[k] += t[k];
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) x[k] = x[k] + alpha * y[k];
        store8(out + i * 8, x);
        if (out_lo) store_lo8<T>(out_lo + i * 8, x);
    }
}

extern "C" int ur_add_hilo(const void* a, const void* a_lo, const void* b, const void* b_lo, float alpha, void* out,
                           void* out_lo, int64_t n, int dtype, void* stream) {
    if (!a || !b || !out || n <= 0 || (n & 7)) return UR_E_BADARG;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int64_t nvec = n / 8;
    UR_DISPATCH(dtype, hipLaunchKernelGGL((add_hilo_kernel<T>), dim3(grid_for(nvec, EW_BLOCKS)), dim3(256), 0, s, (const T*)a,
                       (const lo_t<T>*)a_lo, (const T*)b, (const lo_t<T>*)b_lo, alpha, (T*)out, (lo_t<T>*)out_lo, nvec));
    return last_error();
}

// ur_add_hilo over up to UR_ADD_MULTI_MAX tensor triples in ONE launch: the 13 exchange adds of a sampling step whose
// 1x1-conv operand is loop-invariant (hoist.py).  Workgroup -> (item, chunk of 1024 8-element vectors) through a prefix table
// in the kernel arguments; same per-element arithmetic as add_hilo_kernel with alpha = 1.
struct AddMultiArgs {
    ur_add_item t[UR_ADD_MULTI_MAX];
    SegTable<UR_ADD_MULTI_MAX> seg;
};

template <typename T>
__global__ void __launch_bounds__(256) add_hilo_multi_kernel(const AddMultiArgs a) {
    const int it = a.seg.find(blockIdx.x);
    const ur_add_item e = a.t[it];
    const T* pa = (const T*)e.a;
    const T* pb = (const T*)e.b;
    const lo_t<T>* la = (const lo_t<T>*)e.a_lo;
    const lo_t<T>* lb = (const lo_t<T>*)e.b_lo;
    T* po = (T*)e.out;
    lo_t<T>* lo = (lo_t<T>*)e.out_lo;
    const int64_t nvec = e.n / 8;
    const int64_t v0 = (int64_t)((int)blockIdx.x - a.seg.start[it]) * 1024;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int64_t i = v0 + u * 256 + threadIdx.x;
        if (i >= nvec) break;
        float x[8], y[8], t[8];
        load8(pa + i * 8, x);
        load8(pb + i * 8, y);
        if (la) {
            load_lo<8>(la + i * 8, t);
#pragma unroll
            for (int k = 0; k < 8; ++k) x[k] += t[k];
        }
        if (lb) {
            load_lo<8>(lb + i * 8, t);
#pragma unroll
            for (int k = 0; k < 8; ++k) y[k] += t[k];
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) x[k] = x[k] + 1.0f * y[k];
        store8(po + i * 8, x);
        if (lo) store_lo8<T>(lo + i * 8, x);
    }
}

extern "C" int ur_add_hilo_multi(const ur_add_item* items, int n, int dtype, void* stream) {
    AddMultiArgs a;
    const int rc = pack(items, n, a.t, a.seg, UR_E_UNSUPPORTED, [](const ur_add_item& e) -> int64_t {
        if (!e.a || !e.b || !e.out || e.n <= 0 || (e.n & 7)) return 0;
        return (e.n / 8 + 1023) / 1024;
    });
    if (rc) return rc;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    UR_DISPATCH(dtype, hipLaunchKernelGGL((add_hilo_multi_kernel<T>), dim3(a.seg.total()), dim3(256), 0, s, a));
    return last_error();
}
extern "C" int ur_sizeof_add_item(void) { return (int)sizeof(ur_add_item); }

extern "C" int ur_timestep_embedding(const float* t, int nt, int B, int dim, int flip_sin_to_cos, float freq_shift,
                                     void* out, int dtype, void* stream) {
    if (!t || !out || B <= 0 || dim < 2 || (nt != 1 && nt != B)) return UR_E_BADARG;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int n = B * (dim / 2);
    dim3 grid((n + 255) / 256);
    UR_DISPATCH(dtype, hipLaunchKernelGGL((timestep_kernel<T>), grid, dim3(256), 0, s, t, nt, B, dim, flip_sin_to_cos,
                       freq_shift, (T*)out));
    return last_error();
}

template <typename S>
static int to_nhwc_src(const void* src, int B, int C, int H, int W, void* dst, int Cpad, int dtype, hipStream_t s) {
    const int64_t total = (int64_t)B * H * W * Cpad;
    UR_DISPATCH(dtype, hipLaunchKernelGGL((nchw_to_nhwc_kernel<S, T>), dim3(grid_for(total, EW_BLOCKS)), dim3(256), 0, s,
                       (const S*)src, B, C, H, W, (T*)dst, Cpad));
    return last_error();
}

extern "C" int ur_resize_nearest(const void* in, void* out, int B, int Hin, int Win, int Hout, int Wout, int C, int dtype,
                                 void* stream) {
    if (!in || !out || B <= 0 || Hin <= 0 || Win <= 0 || Hout <= 0 || Wout <= 0 || C <= 0 || (C & 7)) return UR_E_BADARG;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int64_t total = (int64_t)B * Hout * Wout * (C >> 3);
    UR_DISPATCH(dtype, hipLaunchKernelGGL((resize_nearest_kernel<T>), dim3(grid_for(total, EW_BLOCKS)), dim3(256), 0, s,
                       (const T*)in, (T*)out, B, Hin, Win, Hout, Wout, C));
    return last_error();
}

extern "C" int ur_nchw_to_nhwc(const void* src, int src_dtype, int B, int C, int H, int W, void* dst, int Cpad,
                               int dtype, void* stream) {
    if (!src || !dst || B <= 0 || C <= 0 || H <= 0 || W <= 0 || Cpad < C) return UR_E_BADARG;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (src_dtype == 0) return to_nhwc_src<f16>(src, B, C, H, W, dst, Cpad, dtype, s);
    if (src_dtype == 1) return to_nhwc_src<bf16>(src, B, C, H, W, dst, Cpad, dtype, s);
    if (src_dtype == 2) return to_nhwc_src<float>(src, B, C, H, W, dst, Cpad, dtype, s);
    return UR_E_BADARG;
}

template <typename T>
static int to_nchw_dst(const void* src, int B, int C, int H, int W, void* dst, int dst_dtype, hipStream_t s) {
    const dim3 grid(grid_for((int64_t)B * C * H * W, EW_BLOCKS));
    if (dst_dtype == 0)
        hipLaunchKernelGGL((nhwc_to_nchw_kernel<T, f16>), grid, dim3(256), 0, s, (const T*)src, B, C, H, W, (f16*)dst);
    else if (dst_dtype == 1)
        hipLaunchKernelGGL((nhwc_to_nchw_kernel<T, bf16>), grid, dim3(256), 0, s, (const T*)src, B, C, H, W, (bf16*)dst);
    else if (dst_dtype == 2)
        hipLaunchKernelGGL((nhwc_to_nchw_kernel<T, float>), grid, dim3(256), 0, s, (const T*)src, B, C, H, W, (float*)dst);
    else
        return UR_E_BADARG;
    return last_error();
}

extern "C" int ur_nhwc_to_nchw(const void* src, int dtype, int B, int C, int H, int W, void* dst, int dst_dtype,
                               void* stream) {
    if (!src || !dst || B <= 0 || C <= 0 || H <= 0 || W <= 0) return UR_E_BADARG;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    UR_DISPATCH(dtype, return to_nchw_dst<T>(src, B, C, H, W, dst, dst_dtype, s));
}

// dst[k][0..bytes_k) = src[k][*step][0..bytes_k) for up to 4 tables: the rows of the CURRENT step of per-step tables a sampling
// loop's prologue computed for all its steps (the time projections of every resnet: a function of the timestep only).
struct StepRows { const char* src[4]; char* dst[4]; int64_t bytes[4]; };
__global__ void __launch_bounds__(256) select_step_rows_kernel(StepRows a, int ntab, const int* __restrict__ step, int nsteps) {
    const int k = blockIdx.y;
    if (k >= ntab) return;
    const int st = min(max(*step, 0), nsteps - 1);
    const uint4* s = reinterpret_cast<const uint4*>(a.src[k] + (int64_t)st * a.bytes[k]);
    uint4* d = reinterpret_cast<uint4*>(a.dst[k]);
    const int64_t n = a.bytes[k] >> 4;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) d[i] = s[i];
}

extern "C" int ur_select_step_rows(const void* const* src, void* const* dst, const int64_t* bytes, int ntab, const int* step,
                                   int nsteps, void* stream) {
    if (!src || !dst || !bytes || !step || ntab <= 0 || ntab > 4 || nsteps <= 0) return UR_E_BADARG;
    StepRows a{};
    int64_t most = 0;
    for (int k = 0; k < ntab; ++k) {
        if (!src[k] || !dst[k] || bytes[k] <= 0 || (bytes[k] & 15) || ((uintptr_t)src[k] & 15) || ((uintptr_t)dst[k] & 15)) return UR_E_BADARG;
        a.src[k] = reinterpret_cast<const char*>(src[k]);
        a.dst[k] = reinterpret_cast<char*>(dst[k]);
        a.bytes[k] = bytes[k];
        most = bytes[k] > most ? bytes[k] : most;
    }
    int blocks = (int)((most / 16 + 255) / 256);
    blocks = blocks < 1 ? 1 : (blocks > 64 ? 64 : blocks);
    hipLaunchKernelGGL(select_step_rows_kernel, dim3(blocks, ntab), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), a, ntab, step,
                       nsteps);
    return last_error();
}

// One 4-byte load per 128-byte line, grid-strided; the value is consumed by an empty asm so the load is not dropped.
__global__ void __launch_bounds__(256) prefetch_kernel(const char* __restrict__ p, int64_t lines) {
    unsigned acc = 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < lines; i += (int64_t)gridDim.x * blockDim.x)
        acc ^= __builtin_nontemporal_load(reinterpret_cast<const unsigned*>(p + i * 128));
    asm volatile("" ::"v"(acc));
}

extern "C" int ur_prefetch(const void* ptr, int64_t bytes, int wgs, void* stream) {
    if (!ptr || bytes < 0 || wgs <= 0) return UR_E_BADARG;
    const int64_t lines = bytes / 128;
    if (lines == 0) return 0;
    hipLaunchKernelGGL(prefetch_kernel, dim3(wgs), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                       reinterpret_cast<const char*>(ptr), lines);
    return last_error();
}

extern "C" int ur_abi_version(void) { return UR_ABI_VERSION; }
#define UR_STR2(x) #x
#define UR_STR(x) UR_STR2(x)
extern "C" const char* ur_build_info(void) {
    return "liburhip gfx950 (hipcc, MFMA 16x16x32 + 32x32x16, LDS-DMA) abi " UR_STR(UR_ABI_VERSION);
}
extern "C" int ur_sizeof_igemm_desc(void) { return (int)sizeof(ur_igemm_desc); }
extern "C" int ur_sizeof_attn_desc(void) { return (int)sizeof(ur_attn_desc); }
extern "C" int ur_sizeof_attn_bwd_desc(void) { return (int)sizeof(ur_attn_bwd_desc); }
