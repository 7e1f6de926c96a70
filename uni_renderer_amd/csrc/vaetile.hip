// The stitch of a tiled VAE decode / encode in ONE launch (include/ur_kernels.h, ur_blend_tiles): a grid of NHWC tiles ->
// one NCHW tensor, with diffusers 0.24's blend_v / blend_h (AutoencoderKL.tiled_decode / tiled_encode) evaluated per output
// pixel from the RAW tiles.
//
// diffusers walks the grid row by row, left to right, and blends IN PLACE: blend_v(above, tile) then blend_h(left, tile), both
// writing `tile`, both reading a neighbour that has been blended already.  With lerp(a, b, w) = a (1 - w) + b w, ev / eh the
// vertical / horizontal extent of tile (i, j), wy = y / ev, wx = x / eh, and (ya, xl) = (h_above - ev + y, w_left - eh + x):
//     y >= ev, x >= eh     T[y][x]                                                                    one tile
//     y <  ev, x >= eh     lerp(A[ya][x], T[y][x], wy)                                                two
//     y >= ev, x <  eh     lerp(L[y][xl], T[y][x], wx)                                                two
//     y <  ev, x <  eh     lerp( lerp(AL[ya][xl], L[y][xl], wy),                                      four:
//                                lerp( lerp(AL[ya][xl], A[ya][x], wx), T[y][x], wy ), wx )
// In the corner the tile above was itself blended with ITS left neighbour before the vertical blend read it, and the left tile
// with the tile above it before the horizontal blend read it: AL enters twice (weight (1 - wy)(1 - wx)(1 + wx)), A with
// (1 - wy) wx^2.  The rows / columns read from A, L and AL are their LAST ev / eh ones; those are raw as long as every tile
// that has a successor is at least 2 * blend long (its own blends touch its first `blend` rows / columns only): the launcher
// returns UR_E_UNSUPPORTED otherwise.
//
// Arithmetic per element: the tile values in fp32, w = fl(fl(y) / fl(e)) (IEEE division), lerp(a, b, w) = fma(b, w, fl(a *
// fl(1 - w))), nested exactly as written above, ONE rounding to the output dtype.  No atomics, no order that depends on
// data or scheduling: bit-reproducible.
//
// Mapping: a workgroup is 256 consecutive output x of one output row of one sample (grid = x blocks, rows, samples), x
// fastest, so neighbouring lanes read neighbouring NHWC pixels and every one of the C output planes is written as one
// contiguous run.  The tile row is workgroup-uniform, the tile column per lane (a linear scan of at most `cols` prefix sums
// in the kernel arguments).  A pixel of 8 channels whose tiles are all 16-byte aligned is one 16-byte load.
#include "ur_launch.h"

namespace ur {

constexpr int BT_MAX = 64;        // tiles per launch (ur_blend_tiles_max), a read-only row above included
constexpr int BT_ITEM_WORDS = 4;  // int64_t words per tile of the caller's table: address, sample stride, h, w
constexpr int BT_MAX_C = 8;       // channels: 3 (images) and 8 (posterior moments) are what the VAE needs

struct BtTile {
    const void* p;
    int64_t bstride;  // elements between two samples
};

struct BtArgs {
    BtTile t[BT_MAX];     // [trows][cols]
    int rh[BT_MAX];       // height of tile row i
    int ry[BT_MAX + 1];   // first output row of tile row i (rows of the read-only row above: 0 wide, ry[0] == ry[1])
    int cw[BT_MAX];       // width of tile column j
    int cx[BT_MAX + 1];   // first output column of tile column j
    int trows, cols, blend, C, vec;
    int Wout;
    int64_t plane;        // elements between two channel planes of the output
};
static_assert(sizeof(BtArgs) <= 4096, "kernel arguments");

template <typename T>
__device__ __forceinline__ void bt_load(const T* p, int C, bool vec, float (&v)[BT_MAX_C]) {
    if (vec) {
        load8(p, v);
    } else {
#pragma unroll
        for (int c = 0; c < BT_MAX_C; ++c) v[c] = c < C ? (float)p[c] : 0.f;
    }
}

// a (1 - w) + b w for every channel
__device__ __forceinline__ void bt_lerp(const float (&a)[BT_MAX_C], const float (&b)[BT_MAX_C], float w, float (&o)[BT_MAX_C]) {
    const float u = 1.0f - w;
#pragma unroll
    for (int c = 0; c < BT_MAX_C; ++c) o[c] = __builtin_fmaf(b[c], w, a[c] * u);
}

template <typename T, typename S>
__global__ void __launch_bounds__(256) blend_tiles_kernel(const BtArgs a, S* __restrict__ out) {
    const int X = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (X >= a.Wout) return;
    const int Y = (int)blockIdx.y, b = (int)blockIdx.z;
    const int C = a.C, cols = a.cols;
    const bool vec = a.vec != 0;

    int i = 0;  // workgroup-uniform: the last tile row with ry[i] <= Y that is not empty
    while (i + 1 < a.trows && a.ry[i + 1] <= Y) ++i;
    int j = 0;
    while (j + 1 < cols && a.cx[j + 1] <= X) ++j;
    const int y = Y - a.ry[i], x = X - a.cx[j];
    const int h = a.rh[i], w = a.cw[j];
    const int ev = i > 0 ? min(min(a.rh[i - 1], h), a.blend) : 0;
    const int eh = j > 0 ? min(min(a.cw[j - 1], w), a.blend) : 0;
    const bool in_v = y < ev, in_h = x < eh;

    float v[BT_MAX_C];
    {
        const BtTile t = a.t[i * cols + j];
        bt_load((const T*)t.p + b * t.bstride + ((int64_t)y * w + x) * C, C, vec, v);
    }
    if (in_v | in_h) {
        const float wy = in_v ? (float)y / (float)ev : 0.f;
        const float wx = in_h ? (float)x / (float)eh : 0.f;
        const int ha = in_v ? a.rh[i - 1] : 0, wl = in_h ? a.cw[j - 1] : 0;
        const int ya = ha - ev + y, xl = wl - eh + x;
        float al[BT_MAX_C];
        if (in_v & in_h) {
            const BtTile t = a.t[(i - 1) * cols + j - 1];
            bt_load((const T*)t.p + b * t.bstride + ((int64_t)ya * wl + xl) * C, C, vec, al);
        }
        if (in_v) {  // blend_v(above, tile); the tile above was blended with its left neighbour first
            const BtTile t = a.t[(i - 1) * cols + j];
            float ab[BT_MAX_C];
            bt_load((const T*)t.p + b * t.bstride + ((int64_t)ya * w + x) * C, C, vec, ab);
            if (in_h) bt_lerp(al, ab, wx, ab);
            bt_lerp(ab, v, wy, v);
        }
        if (in_h) {  // blend_h(left, tile); the left tile was blended with the tile above it first
            const BtTile t = a.t[i * cols + j - 1];
            float lf[BT_MAX_C];
            bt_load((const T*)t.p + b * t.bstride + ((int64_t)y * wl + xl) * C, C, vec, lf);
            if (in_v) bt_lerp(al, lf, wy, lf);
            bt_lerp(lf, v, wx, v);
        }
    }
    S* o = out + (int64_t)b * C * a.plane + (int64_t)Y * a.Wout + X;
#pragma unroll
    for (int c = 0; c < BT_MAX_C; ++c)
        if (c < C) o[c * a.plane] = (S)v[c];
}

template <typename T>
static void bt_launch(const BtArgs& a, void* out, int out_dtype, dim3 grid, hipStream_t s) {
    if (out_dtype == UR_DT_F16) hipLaunchKernelGGL((blend_tiles_kernel<T, f16>), grid, dim3(256), 0, s, a, (f16*)out);
    else if (out_dtype == UR_DT_BF16) hipLaunchKernelGGL((blend_tiles_kernel<T, bf16>), grid, dim3(256), 0, s, a, (bf16*)out);
    else hipLaunchKernelGGL((blend_tiles_kernel<T, float>), grid, dim3(256), 0, s, a, (float*)out);
}

}  // namespace ur

using namespace ur;

extern "C" int ur_blend_tiles(const int64_t* items, int rows, int cols, int above, int B, int C, int blend, int limit,
                              void* out, int Hout, int Wout, int64_t out_plane, int tile_dtype, int out_dtype, void* stream) {
    if (tile_dtype != UR_DT_F16 && tile_dtype != UR_DT_BF16) return UR_E_BADARG;
    if (out_dtype != UR_DT_F16 && out_dtype != UR_DT_BF16 && out_dtype != UR_DT_F32) return UR_E_BADARG;
    if (!items || !out || rows < 1 || cols < 1 || (above != 0 && above != 1) || B < 1 || C < 1 || blend < 0 || limit < 1)
        return UR_E_BADARG;
    if (Hout < 1 || Wout < 1 || out_plane < (int64_t)Hout * Wout) return UR_E_BADARG;
    if (((uintptr_t)out & (out_dtype == UR_DT_F32 ? 3 : 1)) != 0) return UR_E_BADARG;
    const int64_t trows = (int64_t)rows + above;
    const bool over_cap = trows * cols > BT_MAX;
    // every tile is read and checked first, whatever the list's length: a bad tile anywhere is UR_E_BADARG
    BtArgs a;
    int64_t hsum = 0, wsum = 0;
    bool vec = C == 8, short_tile = false;
    for (int64_t i = 0; i < trows; ++i) {
        for (int64_t j = 0; j < cols; ++j) {
            const int64_t* r = items + (i * cols + j) * BT_ITEM_WORDS;
            const int64_t h = r[2], w = r[3];
            if (!r[0] || (r[0] & 1) || r[1] < 0 || h < 1 || w < 1 || h > 0x3fffffff || w > 0x3fffffff) return UR_E_BADARG;
            const int64_t* r0 = items + (i * cols) * BT_ITEM_WORDS;  // first tile of the row: its height is the row's
            const int64_t* c0 = items + j * BT_ITEM_WORDS;           // first tile of the column
            if (h != r0[2] || w != c0[3]) return UR_E_BADARG;
            if ((r[0] & 15) || (r[1] & 7)) vec = false;
            if (!over_cap) {
                a.t[i * cols + j].p = reinterpret_cast<const void*>(r[0]);
                a.t[i * cols + j].bstride = r[1];
            }
            if (j == 0) {
                const int64_t kept = (above && i == 0) ? 0 : (h < limit ? h : limit);
                if (!over_cap) { a.rh[i] = (int)h; a.ry[i] = (int)hsum; }
                hsum += kept;
                if (i + 1 < trows && h < 2 * (int64_t)blend) short_tile = true;
            }
            if (i == 0) {
                if (!over_cap) { a.cw[j] = (int)w; a.cx[j] = (int)wsum; }
                wsum += w < limit ? w : limit;
                if (j + 1 < cols && w < 2 * (int64_t)blend) short_tile = true;
            }
        }
    }
    if (hsum != Hout || wsum != Wout) return UR_E_BADARG;
    if (over_cap || short_tile || C > BT_MAX_C || Hout > 65535 || B > 65535) return UR_E_UNSUPPORTED;
    a.ry[trows] = (int)hsum;
    a.cx[cols] = (int)wsum;
    a.trows = (int)trows;
    a.cols = cols;
    a.blend = blend;
    a.C = C;
    a.vec = vec ? 1 : 0;
    a.Wout = Wout;
    a.plane = out_plane;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid((Wout + 255) / 256, Hout, B);
    if (tile_dtype == UR_DT_F16) bt_launch<f16>(a, out, out_dtype, grid, s);
    else bt_launch<bf16>(a, out, out_dtype, grid, s);
    return last_error();
}
extern "C" int ur_blend_tiles_max(void) { return BT_MAX; }
extern "C" int ur_blend_tiles_item_words(void) { return BT_ITEM_WORDS; }
