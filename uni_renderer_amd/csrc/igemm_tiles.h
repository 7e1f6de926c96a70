// The tile builds of ur_igemm: ONE row per UR_TILE_* id (include/ur_kernels.h owns the numbers: the tuning tables store
// them).  Everything that has to know a build reads this list: the host's kTiles table (split-K slab pitch, pick_tile,
// ur_igemm_partial_floats, ur_igemm_tile_info -> the Python side), the launch switch of igemm.hip and the dx-tap-sharing
// conv's tile height (igemm_dxs.hip).  A new build = one #define in ur_kernels.h, one row here, UR_TILE_COUNT + 1.
//
//   LS(id, BM, BN, WM, WN, NSTAGE, MF, NL, label)   lock-step build: the template arguments of launch_cfg / igemm_kernel
//                                                   (NSTAGE < 0: register-staged loader; MF: MFMA shape; NL: loader waves)
//   EXT(id, family, BM, BN, label)                  kernels chosen elsewhere (wsconv.hip, igemm_pp.hip) or a reserved id:
//                                                   only the geometry the host needs
// label: what ops.py puts into its profile keys, igemm_{BM}x{BN}s{label}_... (ring depth + what distinguishes the build).
#pragma once

#include "../../include/ur_kernels.h"

// clang-format off
#define UR_IGEMM_TILES(LS, EXT)                                                \
    LS(UR_TILE_128x128,         128, 128, 2, 2,  2, 16, 0, "2")                \
    LS(UR_TILE_128x64,          128,  64, 4, 1,  3, 16, 0, "3")                \
    LS(UR_TILE_64x64,            64,  64, 4, 1,  3, 16, 0, "3")                \
    LS(UR_TILE_128x128_S3,      128, 128, 2, 2,  3, 16, 0, "3")                \
    LS(UR_TILE_128x64_S2,       128,  64, 4, 1,  2, 16, 0, "2")                \
    LS(UR_TILE_64x64_S4,         64,  64, 4, 1,  4, 16, 0, "4")                \
    LS(UR_TILE_64x64_S2,         64,  64, 4, 1,  2, 16, 0, "2")                \
    LS(UR_TILE_256x128,         256, 128, 4, 2,  2, 16, 0, "2")                \
    LS(UR_TILE_128x320,         128, 320, 2, 5,  2, 16, 0, "2")                \
    LS(UR_TILE_128x256,         128, 256, 2, 4,  2, 16, 0, "2")                \
    LS(UR_TILE_256x256,         256, 256, 4, 4,  2, 16, 0, "2")                \
    LS(UR_TILE_64x64_R,          64,  64, 4, 1, -2, 16, 0, "r")                \
    LS(UR_TILE_128x64_R,        128,  64, 4, 1, -2, 16, 0, "r")                \
    LS(UR_TILE_128x128_R,       128, 128, 2, 2, -2, 16, 0, "r")                \
    LS(UR_TILE_128x320_R,       128, 320, 2, 5, -2, 16, 0, "r")                \
    LS(UR_TILE_256x128_R,       256, 128, 4, 2, -2, 16, 0, "r")                \
    LS(UR_TILE_64x64_W1,         64,  64, 1, 1,  2, 16, 0, "2w1")              \
    LS(UR_TILE_128x64_W2,       128,  64, 2, 1,  2, 16, 0, "2w2")              \
    LS(UR_TILE_64x64_W1_S3,      64,  64, 1, 1,  3, 16, 0, "3w1")              \
    LS(UR_TILE_64x128_W2,        64, 128, 1, 2,  2, 16, 0, "2w2n")             \
    LS(UR_TILE_64x64_W1_S4,      64,  64, 1, 1,  4, 16, 0, "4w1")              \
    LS(UR_TILE_128x320_M32,     128, 320, 2, 5,  2, 32, 0, "2m32")             \
    LS(UR_TILE_128x128_M32,     128, 128, 2, 2,  2, 32, 0, "2m32")             \
    LS(UR_TILE_128x64_M32,      128,  64, 4, 1,  2, 32, 0, "2m32")             \
    LS(UR_TILE_128x64_S3_M32,   128,  64, 4, 1,  3, 32, 0, "3m32")             \
    LS(UR_TILE_64x64_M32,        64,  64, 2, 2,  2, 32, 0, "2m32")             \
    LS(UR_TILE_64x64_S3_M32,     64,  64, 2, 2,  3, 32, 0, "3m32")             \
    LS(UR_TILE_256x256_M32,     256, 256, 4, 4,  2, 32, 0, "2m32")             \
    LS(UR_TILE_256x128_M32,     256, 128, 4, 2,  2, 32, 0, "2m32")             \
    LS(UR_TILE_128x256_M32,     128, 256, 2, 4,  2, 32, 0, "2m32")             \
    LS(UR_TILE_128x320_L2,      128, 320, 2, 5,  2, 16, 2, "2L2")              \
    LS(UR_TILE_128x320_L4,      128, 320, 2, 5,  2, 16, 4, "2L4")              \
    LS(UR_TILE_128x128_L2,      128, 128, 2, 2,  2, 16, 2, "2L2")              \
    LS(UR_TILE_128x128_S3_L2,   128, 128, 2, 2,  3, 16, 2, "3L2")              \
    LS(UR_TILE_128x64_L1,       128,  64, 4, 1,  2, 16, 1, "2L1")              \
    LS(UR_TILE_128x64_S3_L2,    128,  64, 4, 1,  3, 16, 2, "3L2")              \
    LS(UR_TILE_64x64_S3_L1,      64,  64, 4, 1,  3, 16, 1, "3L1")              \
    LS(UR_TILE_256x128_L2,      256, 128, 4, 2,  2, 16, 2, "2L2")              \
    EXT(UR_TILE_256x256_L0, UR_TILE_FAMILY_RESERVED, 256, 256, "2L0") /* 16 consumer waves already fill the 1024-thread limit */ \
    LS(UR_TILE_128x256_L2,      128, 256, 2, 4,  2, 16, 2, "2L2")              \
    LS(UR_TILE_128x256_S3,      128, 256, 2, 4,  3, 16, 0, "3")                \
    LS(UR_TILE_128x320_W8_M32,  128, 320, 4, 2,  2, 32, 0, "2w8m32")           \
    LS(UR_TILE_256x320_W16_M32, 256, 320, 8, 2,  2, 32, 0, "2w16m32")          \
    LS(UR_TILE_128x160_M32,     128, 160, 4, 1,  2, 32, 0, "2m32")             \
    LS(UR_TILE_128x160_S3_M32,  128, 160, 4, 1,  3, 32, 0, "3m32")             \
    LS(UR_TILE_64x320_M32,       64, 320, 2, 2,  2, 32, 0, "2m32")             \
    EXT(UR_TILE_WS320,          UR_TILE_FAMILY_WS, 128, 320, "ws")             \
    EXT(UR_TILE_WS320_W8,       UR_TILE_FAMILY_WS, 128, 320, "ws8")            \
    EXT(UR_TILE_PP_128x320,     UR_TILE_FAMILY_PP, 128, 320, "pp5")            \
    EXT(UR_TILE_PP_128x320_S4,  UR_TILE_FAMILY_PP, 128, 320, "pp4")            \
    EXT(UR_TILE_PP_256x128,     UR_TILE_FAMILY_PP, 256, 128, "pp5")            \
    EXT(UR_TILE_PP_128x256,     UR_TILE_FAMILY_PP, 128, 256, "pp5")            \
    EXT(UR_TILE_PP_256x256,     UR_TILE_FAMILY_PP, 256, 256, "pp4")            \
    EXT(UR_TILE_PP_128x128,     UR_TILE_FAMILY_PP, 128, 128, "pp5")            \
    EXT(UR_TILE_PP_256x320,     UR_TILE_FAMILY_PP, 256, 320, "pp4")            \
    LS(UR_TILE_256x160_W4_M32,  256, 160, 4, 1,  2, 32, 0, "2w4m32")           \
    LS(UR_TILE_256x320_W8_M32,  256, 320, 4, 2,  2, 32, 0, "2w8m32")           \
    LS(UR_TILE_128x320_W4_M32,  128, 320, 2, 2,  2, 32, 0, "2w4m32")           \
    LS(UR_TILE_256x128_W4_M32,  256, 128, 4, 1,  2, 32, 0, "2w4m32")           \
    LS(UR_TILE_256x256_W8_M32,  256, 256, 4, 2,  2, 32, 0, "2w8m32")           \
    LS(UR_TILE_256x320_W10,     256, 320, 2, 5,  2, 16, 0, "2w10")
// clang-format on

namespace ur {

struct TileCfg {
    int bm, bn, family;
    char label[16];  // (a longer one does not compile)
    int rows;        // rows of the list that name this id: exactly one, checked below
};
struct TileTable {
    TileCfg t[UR_TILE_COUNT];
    constexpr const TileCfg& operator[](int tile) const { return t[tile]; }
};

// filled BY ID: the order of the rows above means nothing (an id >= UR_TILE_COUNT does not compile: out-of-bounds write in a
// constant expression)
constexpr TileTable make_tile_table() {
    TileTable tb{};
#define UR_TILE_ROW_LS(id, BM, BN, WM, WN, NSTAGE, MF, NL, label) tb.t[id] = TileCfg{BM, BN, UR_TILE_FAMILY_LOCKSTEP, label, tb.t[id].rows + 1};
#define UR_TILE_ROW_EXT(id, family, BM, BN, label) tb.t[id] = TileCfg{BM, BN, family, label, tb.t[id].rows + 1};
    UR_IGEMM_TILES(UR_TILE_ROW_LS, UR_TILE_ROW_EXT)
#undef UR_TILE_ROW_LS
#undef UR_TILE_ROW_EXT
    return tb;
}
constexpr TileTable kTiles = make_tile_table();

constexpr bool tile_table_complete() {
    if (kTiles[UR_TILE_AUTO].rows != 0) return false;
    for (int t = 1; t < UR_TILE_COUNT; ++t)
        if (kTiles[t].rows != 1) return false;
    return true;
}
static_assert(tile_table_complete(), "igemm_tiles.h: every id in [1, UR_TILE_COUNT) needs exactly one row (and UR_TILE_AUTO none)");

}  // namespace ur
