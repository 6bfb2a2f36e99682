// shard_f32_ranges.hpp — the disjointness rule of the grouped calls on fp32 shards
// (allred_plan_reduce_scatter_shards_f32 / allred_plan_all_gather_shards_f32, allred.h): the
// block-exact rule of shard_ranges.hpp over rank-row intervals and shard BLOCK intervals, with
// 4-byte shard elements.
//
// shard_ranges.hpp works in 2-byte elements.  An fp32 shard of blk floats per block at a stride
// of S floats occupies exactly the bytes of a 2-byte shard of 2 blk elements at stride 2 S, and
// a ShardRange whose stride is 0 contributes no row interval, so a list of `count` fp32 buckets
// is a list of 2 count ShardRanges:
//   the rows alone    {ranks, rank_stride, n, nullptr, 0}
//   the shard alone   {nullptr, 0, 2 n, shard, 2 shard_stride}
// and shard_lists_disjoint answers for it unchanged (its verdict does not depend on which entry
// an interval came from).  The two doublings are checked: a list with one that overflows is
// refused like any other address arithmetic that would.
// Plain C++: engine.cpp includes it under hipcc, tests/test_shard_f32_ranges.py under g++.
#pragma once

#include <cstdint>
#include <vector>

#include "shard_ranges.hpp"

namespace tsa {

struct ShardF32Range {
    const void* ranks;       // rank 0's row of bf16
    uint64_t stride;         // bf16 elements between rank rows
    uint64_t n;              // bf16 elements per rank row; blk = n / total
    const void* shard;       // fp32 shard (nullptr: none)
    uint64_t shard_stride;   // floats between shard blocks
};

// the 2-byte view of the list, appended to *out (two entries per bucket, one for a bucket
// without a shard); false when a doubling overflows — *out is then unspecified
inline bool shard_f32_as_ranges(const ShardF32Range* list, int count, std::vector<ShardRange>* out) {
    out->reserve(out->size() + 2 * (size_t)(count > 0 ? count : 0));
    for (int i = 0; i < count; ++i) {
        const ShardF32Range& s = list[i];
        out->push_back(ShardRange{s.ranks, s.stride, s.n, nullptr, 0});
        if (!s.shard) continue;
        uint64_t n2, stride2;
        if (__builtin_mul_overflow(s.n, (uint64_t)2, &n2) || __builtin_mul_overflow(s.shard_stride, (uint64_t)2, &stride2))
            return false;
        out->push_back(ShardRange{nullptr, 0, n2, s.shard, stride2});
    }
    return true;
}

// true: every rank-row interval and every fp32 block interval of the list lies in the address
// space and no two share a byte.  total >= 1; every n a multiple of total.
inline bool shard_f32_lists_disjoint(const ShardF32Range* list, int count, uint64_t total) {
    if (count <= 0) return true;
    if (!list || total == 0) return false;
    std::vector<ShardRange> ranges;
    if (!shard_f32_as_ranges(list, count, &ranges)) return false;
    return shard_lists_disjoint(ranges.data(), (int)ranges.size(), total);
}

}  // namespace tsa
