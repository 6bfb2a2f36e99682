// mx2d_span.hpp — the work units of allred_plan_all_gather_shards_mxfp8_2d (allred.h; k_ag_group_mxfp8_2d
// in mx2d_kernels.hip) and their index arithmetic.
//
// A bucket is ONE row-major matrix W[nrows][cols] in `total` shard blocks of R = nrows / total rows.  The
// work unit is a PATCH of one shard block: 32 sh rows by 32 sw columns, sh and sw powers of two — whole
// 32 x 32 squares, each of which holds 32 row-wise and 32 column-wise MX blocks.  A block has
// (R / 32 sh) row groups of (cols / 32 sw) column groups; unit `rem` of a block is row group rem / cgs,
// column group rem % cgs, cgs = cols / 32 sw, split with the host's reciprocal of cgs
// (tile_span_make's idiom): no division on the device, no 64-bit division per unit anywhere.
// group_span.hpp walks the units: GroupIn.tiles / tpb are counted in units.
//
// mx2d_unit_at gives, for unit (block, rem), five 64-bit offsets of the patch's first element
// W[i0][j0], i0 = block R + 32 sh rg, j0 = 32 sw cg:
//   src      floats from the bucket's shard:        block shard_stride + 32 sh rg cols + j0
//   row      bytes into a rank's element row:       i0 cols + j0       (row i of the patch: + i cols)
//   rscale   bytes into a rank's scale row:         row / 32           (row i of the patch: + i cols / 32)
//   t        bytes into a rank's t row:             j0 nrows + i0      (column j of the patch: + j nrows)
//   tscale   bytes into a rank's t scale row:       t / 32             (column j: + j nrows / 32)
// Plain C++: mx2d_kernels.hip includes it under hipcc, tests/test_mx2d_span.py under g++.
#pragma once

#include <cstdint>

#include "tile_span.hpp"

namespace tsa {

// The patch is at most 32 << kMx2dLgSide rows and as many columns.  0 is the bare square; 1 — 64 x 64
// where cols / 32 and R / 32 are even — is what the A/B of profiles/mx2d_patch_ab.txt chose.
#ifndef TSA_MX2D_LG_SIDE
#define TSA_MX2D_LG_SIDE 1
#endif
constexpr int kMx2dLgSide = TSA_MX2D_LG_SIDE;
static_assert(kMx2dLgSide >= 0 && kMx2dLgSide <= 1, "the LDS images of mx2d_kernels.hip are sized from it: two of 4^side x 2112 bytes");

// what the kernel knows of a bucket's matrix (a part of its by-value table entry)
struct Mx2dShape {         // 32 bytes
    uint64_t cols, nrows;
    uint32_t cgs;          // column groups of a row group: cols / (32 sw)
    uint32_t rcp;          // min(floor(2^32 / cgs), 2^32 - 1), as tile_span_make computes it
    uint32_t lgh, lgw;     // sh = 1 << lgh, sw = 1 << lgw
};
static_assert(sizeof(Mx2dShape) == 32, "the kernel-argument layout");

// the largest k <= kMx2dLgSide with x % 2^k == 0 (x >= 1)
inline uint32_t mx2d_lg(uint64_t x) {
    uint32_t k = 0;
    while (k < (uint32_t)kMx2dLgSide && x % (2ull << k) == 0) ++k;
    return k;
}

// false: cols or R is not a positive multiple of 32, or a unit count that does not fit 31 bits; *s is
// then untouched.  *units: units of one shard block, *all: of the whole bucket.
inline bool mx2d_shape_make(Mx2dShape* s, uint64_t cols, uint64_t nrows, uint64_t total, uint64_t* units, uint64_t* all) {
    if (total == 0 || cols == 0 || cols % 32 || nrows == 0 || nrows % (32 * total)) return false;
    const uint64_t R = nrows / total;
    const uint32_t lgw = mx2d_lg(cols / 32), lgh = mx2d_lg(R / 32);
    const uint64_t cgs = cols >> (5 + lgw), rgs = R >> (5 + lgh);
    uint64_t per_block, n;
    if (__builtin_mul_overflow(cgs, rgs, &per_block) || __builtin_mul_overflow(per_block, total, &n) || n > kTileSpanMaxTiles)
        return false;
    TileSpan ts;
    if (!tile_span_make(&ts, 0, per_block, 1, cgs)) return false;
    *s = Mx2dShape{cols, nrows, ts.tpb, ts.rcp, lgh, lgw};
    *units = per_block;
    *all = n;
    return true;
}

struct Mx2dUnit {
    uint64_t src, row, rscale, t, tscale;
};

// unit `rem` of shard block `block`; lg_total: total = 1 << lg_total (the kernels' P), shard_stride in floats
TSA_HD inline Mx2dUnit mx2d_unit_at(const Mx2dShape& s, uint32_t block, uint32_t rem, uint64_t shard_stride, uint32_t lg_total) {
    TileSpan ts{};
    ts.tpb = s.cgs;
    ts.rcp = s.rcp;
    const TileBlock rc = tile_span_block(ts, rem);   // .block: the row group, .rem: the column group
    const uint64_t R = s.nrows >> lg_total;
    const uint64_t in_block = ((uint64_t)rc.block << (5 + s.lgh)) * s.cols;   // floats above the patch inside its block
    const uint64_t j0 = (uint64_t)rc.rem << (5 + s.lgw);
    const uint64_t i0 = (uint64_t)block * R + ((uint64_t)rc.block << (5 + s.lgh));
    Mx2dUnit u;
    u.src = (uint64_t)block * shard_stride + in_block + j0;
    u.row = i0 * s.cols + j0;
    u.rscale = u.row >> 5;
    u.t = j0 * s.nrows + i0;
    u.tscale = u.t >> 5;
    return u;
}

}  // namespace tsa
