// The host launch layer shared by every .hip that launches: the dtype dispatch, the launch epilogue, the grid size of the
// grid-stride kernels, and the ONE "workgroup -> (item, local block)" table of the multi-tensor kernels.
#pragma once
#include "ur_common.h"
#include "../../include/ur_kernels.h"

// CALL with T = the 16-bit type `dtype` names; any other dtype returns UR_E_BADARG from the enclosing function.
#define UR_DISPATCH(dtype, CALL)                                  \
    if ((dtype) == UR_DT_F16) { typedef ur::f16 T; CALL; }        \
    else if ((dtype) == UR_DT_BF16) { typedef ur::bf16 T; CALL; } \
    else return UR_E_BADARG;

namespace ur {

// what every launcher returns after its last launch: 0, or the negated hipError_t
static inline int last_error() {
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : -(int)e;
}

// workgroups of 256 threads for n work items of a grid-stride kernel, at most max_blocks of them
static inline int grid_for(int64_t n, int max_blocks) {
    int64_t g = (n + 255) / 256;
    return (int)(g < 1 ? 1 : (g > max_blocks ? max_blocks : g));
}

// Segment table of a multi-tensor launch, passed by value inside the kernel arguments: item i owns the workgroups
// start[i] .. start[i + 1) of a one-dimensional grid of total() workgroups.
template <int MAX>
struct SegTable {
    int start[MAX + 1];
    int n;

    void clear() { n = 0; start[0] = 0; }
    // appends an item of `blocks` workgroups; false (table unchanged) when the grid would pass 2^31 - 1 workgroups
    bool push(int64_t blocks) {
        const int64_t end = start[n] + blocks;
        if (end > 0x7fffffff) return false;
        start[++n] = (int)end;
        return true;
    }
    int total() const { return start[n]; }

    // the item i that owns workgroup `block` (wave-uniform binary search: the last i with start[i] <= block); the workgroup
    // is that item's block - start[i]
    __device__ __forceinline__ int find(int block) const {
        int lo = 0, hi = n;
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (start[mid] <= block) lo = mid; else hi = mid;
        }
        return lo;
    }
};

// The host loop of a multi-tensor launcher: copies items[0 .. n) into dst and records their workgroup counts in seg.
// blocks_of(item) holds the launcher's own validation: it returns the item's workgroup count, or 0 for an item it rejects.
// Returns 0, UR_E_BADARG (bad list or item) or rc_overflow (more workgroups than one grid holds).
template <int MAX, typename Item, typename F>
static int pack(const Item* items, int n, Item* dst, SegTable<MAX>& seg, int rc_overflow, F blocks_of) {
    if (!items || n <= 0 || n > MAX) return UR_E_BADARG;
    seg.clear();
    for (int i = 0; i < n; ++i) {
        const int64_t blocks = blocks_of(items[i]);
        if (blocks <= 0) return UR_E_BADARG;
        dst[i] = items[i];
        if (!seg.push(blocks)) return rc_overflow;
    }
    return 0;
}

}  // namespace ur
