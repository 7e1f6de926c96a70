// MultiDiffusion view blend (include/ur_kernels.h, ur_view_blend; an addition to ABI 17): the per-step average of the
// overlapping windows ("views") a large latent is denoised in (arXiv 2302.08113; diffusers' StableDiffusionPanoramaPipeline:
// `value[window_v] += view_v; count[window_v] += 1` over the views, `latents = value / count`, then every view cut out of
// `latents` again for the next step).  In torch that is V slice-adds, a division and V gathers per step; here it is ONE
// in-place launch behind the sampler update kernel, inside the captured sampling graph.
//
// Data: master [N*V][C][wh][ww] fp32 (what the update kernel just wrote), lat = the network's input slice (same samples,
// `halves` copies of them under classifier-free guidance, batch stride free, fp16 / bf16 / fp32), glob [N][C][H][W] fp32.
// Window (r, c) of the rows x cols grid starts at (r * sy, c * sx); view index v = r * cols + c; sample n's view v is batch
// row n * V + v.
//
// Arithmetic per global element (normative; uni_renderer_amd/multidiffusion.py blend_views_reference is the same in torch,
// tests/util_multidiffusion.py restates it in numpy): s = 0; for the covering views in ascending v: s = s + master entry (fp32,
// in that order); g = s / (float)count, correctly rounded (__fdiv_rn; no flag of this file's build relaxes division); with
// round_master g is rounded once to lat's dtype and widened again.  g goes to glob, to every covering master entry and,
// rounded once to lat's dtype, to every covering lat entry of every half.
//
// Why ONE in-place launch is race-free: one thread (or, vectorised, one thread per four consecutive x) owns a global
// element.  It reads and writes only the (view, local pixel) entries of master / lat that map to that element, and every
// such entry maps to exactly one global element -- so no entry is touched by two threads, and a thread has read all of its
// entries before it writes the first.  Nothing else is touched: not the channels of the lat buffer outside the slice (the
// four mask channels of the 28-channel cond buffer), not other samples.
//
// Vectorisation: with ww, sx (and so W) multiples of 4, four consecutive x starting at a multiple of 4 have the same covering
// columns and sit at a multiple of 4 inside every covering window row: 16-byte loads / stores of master and glob, 8- or
// 16-byte stores of lat (when its address and batch stride allow).  Otherwise one element per thread.  The sizes are 0.1 to
// 1.6 M elements: the launch is latency-bound, nothing more is built.
#include "ur_launch.h"

#pragma clang fp contract(off)

namespace ur {

constexpr int VIEW_BLEND_MAX_COVER = 64;

template <typename T, int N> struct VbVec { typedef T type __attribute__((ext_vector_type(N))); };
template <typename T> struct VbVec<T, 1> { typedef T type; };

template <int VEC> __device__ __forceinline__ void vb_load(const float* p, float v[VEC]) {
    if constexpr (VEC == 4) {
        const f32x4 q = *reinterpret_cast<const f32x4*>(p);
        v[0] = q[0], v[1] = q[1], v[2] = q[2], v[3] = q[3];
    } else {
        v[0] = *p;
    }
}

template <typename T, int VEC> __device__ __forceinline__ void vb_store(T* p, const T v[VEC]) {
    if constexpr (VEC == 4) {
        typename VbVec<T, 4>::type q;
        q[0] = v[0], q[1] = v[1], q[2] = v[2], q[3] = v[3];
        *reinterpret_cast<typename VbVec<T, 4>::type*>(p) = q;
    } else {
        *p = v[0];
    }
}

// covering windows [lo, hi] of coordinate y along an axis of `n` windows of length w at stride s: k * s <= y < k * s + w
__device__ __forceinline__ void vb_cover(int y, int n, int w, int s, int& lo, int& hi) {
    lo = y < w ? 0 : (y - w) / s + 1;
    hi = min(n - 1, y / s);
}

template <typename T, int VEC>
__global__ void __launch_bounds__(256) view_blend_kernel(float* master, T* lat, int64_t lat_bs, float* __restrict__ glob, int N, int C,
                                                         int rows, int cols, int wh, int ww, int sy, int sx, int halves,
                                                         int round_master) {
    const int H = (rows - 1) * sy + wh, W = (cols - 1) * sx + ww, Wg = W / VEC, V = rows * cols;
    const int64_t plane = (int64_t)wh * ww;
    const int64_t NV = (int64_t)N * V;
    const int64_t total = (int64_t)N * C * H * Wg;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int x = (int)(i % Wg) * VEC;
        int64_t t = i / Wg;
        const int y = (int)(t % H);
        t /= H;
        const int c = (int)(t % C), n = (int)(t / C);
        int r0, r1, c0, c1;
        vb_cover(y, rows, wh, sy, r0, r1);
        vb_cover(x, cols, ww, sx, c0, c1);  // the same for x .. x + VEC - 1 (see above)
        float s[VEC];
#pragma unroll
        for (int j = 0; j < VEC; ++j) s[j] = 0.0f;
        for (int r = r0; r <= r1; ++r)
            for (int q = c0; q <= c1; ++q) {  // ascending view index
                const int64_t b = (int64_t)n * V + r * cols + q;
                float m[VEC];
                vb_load<VEC>(master + (b * C + c) * plane + (int64_t)(y - r * sy) * ww + (x - q * sx), m);
#pragma unroll
                for (int j = 0; j < VEC; ++j) s[j] = s[j] + m[j];
            }
        const float count = (float)((r1 - r0 + 1) * (c1 - c0 + 1));
        float g[VEC];
        T gt[VEC];
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
            const float d = __fdiv_rn(s[j], count);
            gt[j] = (T)d;
            g[j] = round_master ? (float)gt[j] : d;
        }
        vb_store<float, VEC>(glob + (((int64_t)n * C + c) * H + y) * W + x, g);
        for (int r = r0; r <= r1; ++r)
            for (int q = c0; q <= c1; ++q) {
                const int64_t b = (int64_t)n * V + r * cols + q;
                const int64_t off = (int64_t)(y - r * sy) * ww + (x - q * sx);
                vb_store<float, VEC>(master + (b * C + c) * plane + off, g);
                if (lat)
                    for (int h = 0; h < halves; ++h) vb_store<T, VEC>(lat + (b + h * NV) * lat_bs + c * plane + off, gt);
            }
    }
}

template <typename T>
static int launch_view_blend(float* master, void* lat, int64_t lat_bs, float* glob, int N, int C, int rows, int cols, int wh, int ww,
                             int sy, int sx, int halves, int round_master, hipStream_t s) {
    const int64_t H = (int64_t)(rows - 1) * sy + wh, W = (int64_t)(cols - 1) * sx + ww;
    bool vec = ww % 4 == 0 && (cols == 1 || sx % 4 == 0) && ((uintptr_t)master & 15) == 0 && ((uintptr_t)glob & 15) == 0;
    if (lat) vec = vec && ((uintptr_t)lat % (4 * sizeof(T))) == 0 && (lat_bs % 4) == 0;
#define UR_VB_ARGS master, (T*)lat, lat_bs, glob, N, C, rows, cols, wh, ww, sy, sx, halves, round_master
    if (vec)
        hipLaunchKernelGGL((view_blend_kernel<T, 4>), dim3(grid_for((int64_t)N * C * H * (W / 4), 2048)), dim3(256), 0, s, UR_VB_ARGS);
    else
        hipLaunchKernelGGL((view_blend_kernel<T, 1>), dim3(grid_for((int64_t)N * C * H * W, 2048)), dim3(256), 0, s, UR_VB_ARGS);
#undef UR_VB_ARGS
    return last_error();
}

}  // namespace ur

using namespace ur;

extern "C" int ur_view_blend_max_cover(void) { return VIEW_BLEND_MAX_COVER; }

extern "C" int ur_view_blend(float* master, void* lat, int64_t lat_bstride, float* global, int N, int C, int rows, int cols, int wh,
                             int ww, int sy, int sx, int halves, int round_master, int dtype, void* stream) {
    if (!master || !global || N <= 0 || C <= 0 || rows <= 0 || cols <= 0 || wh <= 0 || ww <= 0 || sy <= 0 || sx <= 0 ||
        halves < 1 || halves > 2)
        return UR_E_BADARG;
    if ((rows > 1 && sy > wh) || (cols > 1 && sx > ww)) return UR_E_BADARG;  // pixels between two windows: count 0
    const int64_t H = (int64_t)(rows - 1) * sy + wh, W = (int64_t)(cols - 1) * sx + ww;
    if (H * W > 0x7fffffff || (int64_t)rows * cols > 0x7fffffff || (int64_t)N * rows * cols > 0x7fffffff) return UR_E_BADARG;
    if (lat && lat_bstride < (int64_t)C * wh * ww) return UR_E_BADARG;
    if (dtype != UR_DT_F32 && dtype != UR_DT_F16 && dtype != UR_DT_BF16) return UR_E_BADARG;
    const int64_t cy = (wh + sy - 1) / sy < rows ? (wh + sy - 1) / sy : rows, cx = (ww + sx - 1) / sx < cols ? (ww + sx - 1) / sx : cols;
    if (cy * cx > VIEW_BLEND_MAX_COVER) return UR_E_UNSUPPORTED;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
#define UR_VB_CALL master, lat, lat_bstride, global, N, C, rows, cols, wh, ww, sy, sx, halves, round_master, s
    if (dtype == UR_DT_F32) return launch_view_blend<float>(UR_VB_CALL);
    UR_DISPATCH(dtype, return launch_view_blend<T>(UR_VB_CALL));
#undef UR_VB_CALL
}
