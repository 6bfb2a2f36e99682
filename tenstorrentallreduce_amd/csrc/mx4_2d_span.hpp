// mx4_2d_span.hpp — the work units of allred_plan_all_gather_shards_mxfp4_2d (allred.h; k_ag_group_mxfp4_2d
// in mx4_2d_kernels.hip) and their index arithmetic.
//
// A bucket is ONE row-major matrix W[nrows][cols] in `total` shard blocks of R = nrows / total rows.  The
// work unit is a STRIP of the MATRIX, not a patch of one shard block: S = 1 << kMx4LgStrip consecutive
// 32-row groups of W by 32 sw columns, sw = 1 << lgw the largest power of two up to 1 << kMx4LgWidth that
// divides cols / 32.  Row group G of W (rows 32 G .. 32 G + 31) lies in exactly ONE shard block, G / rpb with
// rpb = R / 32, but the S groups of a strip may lie in several neighbouring blocks: their rows are
// consecutive in every t row, so a strip leaves in runs of 16 S bytes there whatever R is.  total >= 8 and
// nrows % (32 total) == 0 give nrows % 256 == 0: S = 4 and S = 8 tile every legal matrix, no tail class.
// group_span.hpp walks the units: GroupIn.tiles = strips x column groups, GroupIn.tpb = the column groups
// cgs = cols / 32 sw, so GroupTile.block is the STRIP and GroupTile.rem the column group.
//
// mx4_2d_unit_at gives, for unit (strip, cg), the offsets of the strip's first element W[i0][j0],
// i0 = 32 S strip, j0 = 32 sw cg — two elements per byte, (i0 cols + j0) and (j0 nrows + i0) both even:
//   row      bytes into a rank's element row:       (i0 cols + j0) / 2     (row i of the strip: + i cols / 2)
//   rscale   bytes into a rank's scale row:         (i0 cols + j0) / 32    (row i: + i cols / 32)
//   t        bytes into a rank's t row:             (j0 nrows + i0) / 2    (column j of the strip: + j nrows / 2)
//   tscale   bytes into a rank's t scale row:       (j0 nrows + i0) / 32   (column j: + j nrows / 32)
//   g0, j0   the strip's first row group S strip and its first column
// mx4_2d_group_at gives the shard block of a row group G and the floats from the bucket's shard to
// W[32 G][0]: block shard_stride + 32 (G - block rpb) cols — the quotient from the host's reciprocal of rpb
// (tile_span_make's idiom): no division on the device, no 64-bit division per unit anywhere.
// Plain C++: mx4_2d_kernels.hip includes it under hipcc, tests/test_mx4_2d_span.py under g++.
#pragma once

#include <cstdint>

#include "tile_span.hpp"

namespace tsa {

// S = 1 << TSA_MX4_2D_LG_STRIP row groups per strip: 2 — 64-byte runs in the t rows, the run length
// profiles/mx2d_patch_ab.txt measured at full rate — or 3, 128-byte runs.  The strip is at
// most 16 squares in either build (the LDS images of mx4_2d_kernels.hip are sized from it): up to 128
// columns at S = 4, up to 64 at S = 8.
#ifndef TSA_MX4_2D_LG_STRIP
#define TSA_MX4_2D_LG_STRIP 2
#endif
constexpr int kMx4LgStrip = TSA_MX4_2D_LG_STRIP;
static_assert(kMx4LgStrip == 2 || kMx4LgStrip == 3, "nrows % 256 == 0 is all the checks promise: S = 4 or 8");
constexpr int kMx4LgWidth = 4 - kMx4LgStrip;
constexpr int kMx4LgSquares = 4;   // squares of the largest strip, as a shift

// what the kernel knows of a bucket's matrix (a part of its by-value table entry)
struct Mx4Shape {          // 32 bytes
    uint64_t cols, nrows;
    uint32_t rpb;          // row groups per shard block: R / 32
    uint32_t rcp;          // min(floor(2^32 / rpb), 2^32 - 1), as tile_span_make computes it
    uint32_t lgw;          // sw = 1 << lgw
    uint32_t zero;
};
static_assert(sizeof(Mx4Shape) == 32, "the kernel-argument layout");

// false: cols or R is not a positive multiple of 32, nrows is not whole strips, or a count that does not
// fit 31 bits; *s is then untouched.  *cgs: units of one strip, *all: of the whole bucket.
inline bool mx4_2d_shape_make(Mx4Shape* s, uint64_t cols, uint64_t nrows, uint64_t total, uint64_t* cgs, uint64_t* all) {
    if (total == 0 || cols == 0 || cols % 32 || nrows == 0 || nrows % (32 * total) || nrows % (32ull << kMx4LgStrip)) return false;
    uint32_t lgw = 0;
    while (lgw < (uint32_t)kMx4LgWidth && (cols / 32) % (2ull << lgw) == 0) ++lgw;
    const uint64_t per_strip = cols >> (5 + lgw), strips = nrows >> (5 + kMx4LgStrip);
    uint64_t n;
    if (__builtin_mul_overflow(per_strip, strips, &n) || n > kTileSpanMaxTiles) return false;
    TileSpan ts;
    if (!tile_span_make(&ts, 0, nrows / 32, 1, nrows / total / 32)) return false;
    *s = Mx4Shape{cols, nrows, ts.tpb, ts.rcp, lgw, 0};
    *cgs = per_strip;
    *all = n;
    return true;
}

struct Mx4Unit {
    uint64_t row, rscale, t, tscale, j0;
    uint32_t g0;
};

// unit (strip, cg) of the bucket
TSA_HD inline Mx4Unit mx4_2d_unit_at(const Mx4Shape& s, uint32_t strip, uint32_t cg) {
    Mx4Unit u;
    u.g0 = strip << kMx4LgStrip;
    u.j0 = (uint64_t)cg << (5 + s.lgw);
    const uint64_t i0 = (uint64_t)u.g0 << 5;
    const uint64_t rw = i0 * s.cols + u.j0, tw = u.j0 * s.nrows + i0;
    u.row = rw >> 1;
    u.rscale = rw >> 5;
    u.t = tw >> 1;
    u.tscale = tw >> 5;
    return u;
}

struct Mx4Group {
    uint32_t block;   // the shard block of the row group
    uint64_t src;     // floats from the bucket's shard to the row group's first row, column 0
};

// row group G < nrows / 32 of the matrix; shard_stride in floats
TSA_HD inline Mx4Group mx4_2d_group_at(const Mx4Shape& s, uint32_t G, uint64_t shard_stride) {
    TileSpan ts{};
    ts.tpb = s.rpb;
    ts.rcp = s.rcp;
    const TileBlock b = tile_span_block(ts, G);   // .block: the shard block, .rem: the row group inside it
    return Mx4Group{b.block, (uint64_t)b.block * shard_stride + ((uint64_t)b.rem << 5) * s.cols};
}

}  // namespace tsa
