// shard_ranges.hpp — the disjointness rule of the grouped shard calls
// (allred_plan_reduce_scatter_shards / allred_plan_all_gather_shards, allred.h).
//
// The byte sets of one list must be pairwise disjoint:
//   a bucket's rank rows   ONE interval [ranks, ranks + 2 total stride): the stride skew counts
//                          (allred_plan_execute_group's rule);
//   a bucket's shard       its `total` SEPARATE block intervals [shard + 2 b shard_stride,
//                          + 2 blk), blk = n / total — not the range that encloses them.
// Block-exact because a sharded optimizer's buffer is rank-major: one row of F elements per
// rank, bucket i's shard at flat + off_i with shard_stride = F.  The enclosing ranges of
// different buckets then interleave — every one of them spans nearly the whole buffer — while
// no two blocks share a byte.  Blocks of another bucket in the gaps of a wide shard_stride are
// the same case.  A shard_stride below blk makes a shard's own blocks overlap: refused by the
// same rule, as is an interval that does not end at or below UINTPTR_MAX (nothing wraps: every
// product and sum is checked in 64 bits).
//
// Three steps, each exact where it answers, the cheap ones first (the check is host work on
// every call):
//   1  the enclosing ranges, count log count.  None colliding (compact shards, buffers of their
//      own): disjoint.
//   2  the rank-major flat buffer: every shard of the list has the SAME stride S and all of them
//      start inside one period, [base, base + 2 S) with base the lowest shard, block 0 included.
//      Then block b of every shard lies in period b, the periods are disjoint, and every period
//      holds period 0's pattern shifted: the blocks are disjoint exactly when the `count` blocks 0
//      are.  The shards then count as ONE range against the rank rows, count log count again.
//   3  anything else: the block intervals themselves — at most count (total + 1) — sorted and
//      compared.
// Plain C++: engine.cpp includes it under hipcc, tests/test_shard_ranges.py under g++.
#pragma once

#include <algorithm>
#include <cstdint>
#include <utility>
#include <vector>

namespace tsa {

struct ShardRange {
    const void* ranks;       // rank 0's row
    uint64_t stride;         // elements between rank rows
    uint64_t n;              // elements per rank row; blk = n / total
    const void* shard;       // nullptr: no shard
    uint64_t shard_stride;   // elements between shard blocks
};

namespace shard_ranges_detail {

typedef std::pair<uint64_t, uint64_t> Interval;   // [first, second) in bytes

// base + 2 * elems, false when that is past UINTPTR_MAX
inline bool end_of(uint64_t base, uint64_t elems, uint64_t* end) {
    uint64_t bytes;
    if (__builtin_mul_overflow(elems, (uint64_t)2, &bytes)) return false;
    if (__builtin_add_overflow(base, bytes, end)) return false;
    return *end <= (uint64_t)UINTPTR_MAX;
}

// sorts v; true when no two of its (non-empty) intervals share a byte
inline bool sorted_disjoint(std::vector<Interval>& v) {
    std::sort(v.begin(), v.end());
    for (size_t i = 1; i < v.size(); ++i)
        if (v[i].first < v[i - 1].second) return false;
    return true;
}

}  // namespace shard_ranges_detail

// true: every interval of the list lies in the address space and no two share a byte.
// total >= 1; every n a multiple of total (the callers' checks).  An empty interval (n == 0,
// or stride == 0) holds no byte and collides with nothing.
inline bool shard_lists_disjoint(const ShardRange* list, int count, uint64_t total) {
    using namespace shard_ranges_detail;
    if (count <= 0) return true;
    if (!list || total == 0) return false;
    std::vector<Interval> rows, coarse;
    rows.reserve((size_t)count);
    coarse.reserve(2 * (size_t)count);
    int shards = 0;
    bool one_stride = true;
    uint64_t S = 0, base = 0;
    for (int i = 0; i < count; ++i) {
        const ShardRange& s = list[i];
        uint64_t elems, end;
        if (__builtin_mul_overflow(total, s.stride, &elems) || !end_of((uint64_t)(uintptr_t)s.ranks, elems, &end))
            return false;
        if (end > (uint64_t)(uintptr_t)s.ranks) rows.push_back(Interval((uint64_t)(uintptr_t)s.ranks, end));
        if (!s.shard) continue;
        const uint64_t blk = s.n / total, at = (uint64_t)(uintptr_t)s.shard;
        if (blk == 0) continue;
        if (total > 1 && s.shard_stride < blk) return false;   // the shard's own blocks overlap
        // the enclosing range: (total - 1) strides and the last block
        if (__builtin_mul_overflow(total - 1, s.shard_stride, &elems) || __builtin_add_overflow(elems, blk, &elems) ||
            !end_of(at, elems, &end))
            return false;
        coarse.push_back(Interval(at, end));
        one_stride = one_stride && (shards == 0 || s.shard_stride == S);
        S = s.shard_stride;
        base = shards == 0 || at < base ? at : base;
        ++shards;
    }
    // 1: the enclosing ranges
    coarse.insert(coarse.end(), rows.begin(), rows.end());
    if (sorted_disjoint(coarse)) return true;
    if (shards == 0 || total == 1) return false;   // every interval was its own enclosing range
    // 2: one stride, every shard's block 0 inside the period that starts at the lowest shard
    // (2 S fits: 2 (total - 1) S did, above)
    if (one_stride) {
        std::vector<Interval> first;
        first.reserve((size_t)shards);
        uint64_t top = 0;   // the highest end of a last block: the end of the shards as one range
        for (int i = 0; i < count && one_stride; ++i) {
            const ShardRange& s = list[i];
            const uint64_t blk = s.n / total, at = (uint64_t)(uintptr_t)s.shard;
            if (!s.shard || blk == 0) continue;
            one_stride = at - base + 2 * blk <= 2 * S;
            first.push_back(Interval(at, at + 2 * blk));
            const uint64_t end = at + 2 * ((total - 1) * S + blk);
            top = end > top ? end : top;
        }
        if (one_stride) {
            if (!sorted_disjoint(first)) return false;
            std::vector<Interval> with(rows);
            with.push_back(Interval(base, top));
            if (sorted_disjoint(with)) return true;   // else a rank row inside the shards' range: in a gap, or on a block
        }
    }
    // 3: every interval
    std::vector<Interval> fine;
    fine.reserve(rows.size() + (size_t)shards * (size_t)total);
    fine.insert(fine.end(), rows.begin(), rows.end());
    for (int i = 0; i < count; ++i) {
        const ShardRange& s = list[i];
        const uint64_t blk = s.n / total;
        if (!s.shard || blk == 0) continue;
        for (uint64_t b = 0; b < total; ++b) {
            const uint64_t at = (uint64_t)(uintptr_t)s.shard + 2 * b * s.shard_stride;   // inside the checked range
            fine.push_back(Interval(at, at + 2 * blk));
        }
    }
    return sorted_disjoint(fine);
}

}  // namespace tsa
