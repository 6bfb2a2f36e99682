// group_span.hpp — the tile walk of a GROUPED persistent pass: one launch over
// the concatenated tile ranges of up to 64 buckets (allred_plan_execute_group /
// allred_plan_reduce_scatter_group, k_tree_group in kernels.hip).
//
// The launch covers global tiles 0 .. T - 1, bucket i owning [first_i, end_i),
// end_i = first_{i+1}, on a grid of G workgroups; workgroup g takes tiles
// g + j * G, j = 0 .. mine - 1 — tile_span.hpp's walk with t0 = 0.  The table is
// made on the host once per launch and passed to the kernel BY VALUE (16 + 64 x
// 32 bytes of kernel arguments: no device allocation, no copy, capturable into a
// graph).  Per bucket it holds the row-0 pointer, the rank stride, the first
// global tile, the tiles per block and the host's reciprocal of that
// (tile_span_make's), so the device never divides:
//   mine   = T / G + (g < T % G)                       (q, r from the host)
//   bucket = a cursor walked FORWARD over the bucket ends: from tile j to j + 1
//            the global tile grows by G, which may pass any number of buckets
//            shorter than G; the cursor is wave-uniform (it depends on blockIdx
//            and j only)
//   block  = tile_span_block of the tile's index inside its bucket, with the
//            bucket's tpb / rcp.
// Tile indices are 32-bit: T <= 2^31 - 1 (group_span_make refuses more).  Plain
// C++: kernels.hip includes it under hipcc, tests/test_group_span.py under g++.
#pragma once

#include <cstdint>

#include "tile_span.hpp"

namespace tsa {

constexpr int kGroupMax = 64;   // ALLRED_GROUP_MAX (allred.h)

struct GroupBucket {       // 32 bytes
    uint16_t* ranks;       // rank 0's row; rank r at ranks + r * stride
    uint64_t stride;       // elements
    uint32_t first, end;   // global tiles [first, end) of this bucket
    uint32_t tpb;          // tiles per block (>= 1)
    uint32_t rcp;          // min(floor(2^32 / tpb), 2^32 - 1), as tile_span_make computes it
};

struct GroupSpan {
    uint32_t T, G;         // tiles and workgroups of the launch
    uint32_t q, r;         // T / G, T % G
    GroupBucket b[kGroupMax];   // entries past the last bucket: zero
};
static_assert(sizeof(GroupBucket) == 32 && sizeof(GroupSpan) == 16 + 32 * kGroupMax, "the kernel-argument layout");

// The shard buffers of a grouped launch (allred_plan_reduce_scatter_shards /
// allred_plan_all_gather_shards): a second by-value table next to GroupSpan, entry i for bucket
// i of the launch — block b of the bucket lives at shard + b * stride elements, or, shard ==
// nullptr, in rank b's own row (in place).  64 x 16 bytes: with the order pointer and GroupSpan
// 8 + 2064 + 1024 = 3096 bytes of kernel arguments, inside the 4 KiB limit.
struct GroupShard {        // 16 bytes
    uint16_t* shard;
    uint64_t stride;       // elements
};
struct GroupShards {
    GroupShard s[kGroupMax];    // entries past the last bucket: zero
};
static_assert(sizeof(GroupShard) == 16 && sizeof(GroupShards) == 16 * kGroupMax, "the kernel-argument layout");

// what the host knows of a bucket: `tiles` 256-element tiles per rank row in blocks of tpb tiles
struct GroupIn {
    uint16_t* ranks;
    uint64_t stride;
    uint64_t tiles, tpb;
};

// a located tile: its bucket, its index inside the bucket, its block and its index inside the block
struct GroupTile {
    uint32_t bucket, local, block, rem;
};

// false: no or too many buckets, an empty bucket, tpb == 0, G == 0 or G or the sum of the tiles
// past 2^31 - 1; *s is then untouched.
inline bool group_span_make(GroupSpan* s, const GroupIn* in, int count, uint64_t G) {
    if (count < 1 || count > kGroupMax || G == 0 || G > kTileSpanMaxTiles) return false;
    uint64_t T = 0;
    for (int i = 0; i < count; ++i) {
        if (in[i].tiles == 0 || in[i].tpb == 0 || in[i].tiles > kTileSpanMaxTiles - T) return false;
        T += in[i].tiles;
    }
    GroupSpan g{};
    g.T = (uint32_t)T;
    g.G = (uint32_t)G;
    g.q = (uint32_t)(T / G);
    g.r = (uint32_t)(T % G);
    uint32_t first = 0;
    for (int i = 0; i < count; ++i) {
        TileSpan ts;
        if (!tile_span_make(&ts, 0, in[i].tiles, 1, in[i].tpb)) return false;
        GroupBucket& e = g.b[i];
        e.ranks = in[i].ranks;
        e.stride = in[i].stride;
        e.first = first;
        first += (uint32_t)in[i].tiles;
        e.end = first;
        e.tpb = ts.tpb;
        e.rcp = ts.rcp;
    }
    *s = g;
    return true;
}

// tiles of workgroup g
TSA_HD inline uint32_t group_span_mine(const GroupSpan& s, uint32_t g) { return s.q + (g < s.r ? 1u : 0u); }

// global tile j of workgroup g (meaningful for j < mine)
TSA_HD inline uint32_t group_span_tile(const GroupSpan& s, uint32_t g, uint32_t j) { return g + j * s.G; }

// Global tile x < T located from the cursor k: the bucket of the last tile located with it (0
// before the first).  x may not go backwards.  The walk ends at the bucket whose end is above
// x — the last bucket's end is T —, passing whole buckets on the way.
TSA_HD inline GroupTile group_span_at(const GroupSpan& s, uint32_t x, uint32_t& k) {
#if defined(__clang__)
#pragma clang loop vectorize(disable) unroll(disable)   // a scalar walk of zero or one step as a rule
#endif
    while (k + 1 < (uint32_t)kGroupMax && x >= s.b[k].end) ++k;
    TileSpan ts{};
    ts.tpb = s.b[k].tpb;
    ts.rcp = s.b[k].rcp;
    const uint32_t local = x - s.b[k].first;
    const TileBlock tb = tile_span_block(ts, local);
    return GroupTile{k, local, tb.block, tb.rem};
}

}  // namespace tsa
