// shard_f32_norm_ranges.hpp — the two extra byte ranges of
// allred_plan_reduce_scatter_shards_f32_norm (allred.h) against the list's: the `total` floats of
// norm_sq and the workspace are plain intervals [p, p + bytes), and they must share no byte with
// each other, with any bucket's rank-row interval or with any fp32 shard BLOCK — the byte-exact
// rule of shard_f32_ranges.hpp, so either may live in the gap of a wide shard_stride.
//
// The list itself has passed shard_f32_lists_disjoint before (the caller's order): every row and
// block interval lies in the address space and shard_stride >= blk, which is what makes the
// block test O(1) per bucket.  For an interval [lo, hi) and blocks [at + b S, + B), S >= B, let
// b0 = floor((lo - at) / S) (0 when lo < at): the blocks before b0 end at or below lo, block b0
// is the last one that starts at or below lo (or block 0), block b0 + 1 the first that starts
// above it, and when that one starts at or past hi so does every later one.  Two blocks to test.
// Plain C++: engine.cpp includes it under hipcc, tests/test_shard_f32_norm_ranges.py under g++.
#pragma once

#include <cstdint>

#include "shard_f32_ranges.hpp"

namespace tsa {

namespace shard_f32_norm_detail {

// [lo, hi) against every interval of one bucket; true: they share a byte
inline bool hits_bucket(uint64_t lo, uint64_t hi, const ShardF32Range& s, uint64_t total) {
    const uint64_t rows = (uint64_t)(uintptr_t)s.ranks, rows_end = rows + 2 * total * s.stride;
    if (lo < rows_end && rows < hi) return true;
    const uint64_t B = 4 * (s.n / total), S = 4 * s.shard_stride, at = (uint64_t)(uintptr_t)s.shard;
    if (!s.shard || B == 0) return false;
    const uint64_t b0 = lo > at && S ? (lo - at) / S : 0;
    for (uint64_t b = b0; b < total && b <= b0 + 1; ++b) {
        const uint64_t first = at + b * S;
        if (first >= hi) break;
        if (lo < first + B) return true;
    }
    return false;
}

}  // namespace shard_f32_norm_detail

// true: [norm_sq, + sq_bytes) and [norm_ws, + ws_bytes) lie in the address space and share no byte
// with each other, with a rank-row interval or with a shard block of the list.  The list has passed
// shard_f32_lists_disjoint(list, count, total); an empty interval collides with nothing.
inline bool shard_f32_norm_disjoint(const ShardF32Range* list, int count, uint64_t total, const void* norm_sq,
                                    uint64_t sq_bytes, const void* norm_ws, uint64_t ws_bytes) {
    const uint64_t lo[2] = {(uint64_t)(uintptr_t)norm_sq, (uint64_t)(uintptr_t)norm_ws};
    uint64_t hi[2];
    if (__builtin_add_overflow(lo[0], sq_bytes, &hi[0]) || __builtin_add_overflow(lo[1], ws_bytes, &hi[1])) return false;
    if (hi[0] > (uint64_t)UINTPTR_MAX || hi[1] > (uint64_t)UINTPTR_MAX) return false;
    if (sq_bytes && ws_bytes && lo[0] < hi[1] && lo[1] < hi[0]) return false;
    if (count > 0 && (!list || total == 0)) return false;
    for (int k = 0; k < 2; ++k) {
        if (hi[k] == lo[k]) continue;
        for (int i = 0; i < count; ++i)
            if (shard_f32_norm_detail::hits_bucket(lo[k], hi[k], list[i], total)) return false;
    }
    return true;
}

}  // namespace tsa
