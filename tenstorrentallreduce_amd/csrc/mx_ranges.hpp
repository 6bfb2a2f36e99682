// mx_ranges.hpp — the argument rules that need no plan, and the disjointness rule, of
// allred_plan_all_gather_shards_mxfp8 (allred.h): byte-exact and block-exact, on shard_ranges.hpp
// the way shard_f32_ranges.hpp is.
//
// The call WRITES the e4m3 rows and the E8M0 scale rows of every bucket and reads the fp32 shard
// while it does, so per bucket these byte sets must be pairwise disjoint, and disjoint across buckets:
//   the element rows   ONE interval [rows, rows + total * row_stride) bytes, the stride skew included;
//   the scale rows     ONE interval [scales, scales + total * scale_stride) bytes, likewise;
//   the shard          its `total` SEPARATE block intervals [shard + 4 b shard_stride, + 4 blk),
//                      blk = n / total floats.
// shard_ranges.hpp works in 2-byte elements and every byte quantity here is even (row_stride % 16,
// scale_stride % 8, n % 256), so a bucket is three ShardRanges:
//   the element rows alone   {rows, row_stride / 2, n / 2, nullptr, 0}
//   the scale rows alone     {scales, scale_stride / 2, n / 64, nullptr, 0}
//   the shard alone          {nullptr, 0, 2 n, shard, 2 shard_stride}
// (a ShardRange whose stride is 0 contributes no row interval; its verdict does not depend on which
// entry an interval came from) and shard_lists_disjoint answers for the 3 count of them unchanged.
// Rows or scales may therefore sit in the gap of a wide shard_stride, and scale rows in the skew of
// nobody: a skew belongs to its rows' interval.  The two doublings are checked: a list with one that
// overflows is refused like any other address arithmetic that would.
// Plain C++: engine.cpp includes it under hipcc, tests/test_mx_ranges.py under g++.
#pragma once

#include <cstdint>
#include <vector>

#include "shard_ranges.hpp"

namespace tsa {

constexpr uint64_t kMxMaxTiles = 0x7fffffffull;   // kTileSpanMaxTiles (tile_span.hpp): 32-bit tile indices

struct MxRange {
    const void* rows;        // rank 0's row of e4m3 bytes
    uint64_t row_stride;     // bytes between element rows
    const void* scales;      // rank 0's row of E8M0 bytes
    uint64_t scale_stride;   // bytes between scale rows
    uint64_t n;              // elements per rank row; blk = n / total
    const void* shard;       // fp32 shard
    uint64_t shard_stride;   // floats between shard blocks
};

// the 2-byte view of the list, appended to *out (three entries per bucket); false when a doubling
// overflows — *out is then unspecified
inline bool mx_as_ranges(const MxRange* list, int count, std::vector<ShardRange>* out) {
    out->reserve(out->size() + 3 * (size_t)(count > 0 ? count : 0));
    for (int i = 0; i < count; ++i) {
        const MxRange& s = list[i];
        out->push_back(ShardRange{s.rows, s.row_stride / 2, s.n / 2, nullptr, 0});
        out->push_back(ShardRange{s.scales, s.scale_stride / 2, s.n / 64, nullptr, 0});
        uint64_t n2, stride2;
        if (__builtin_mul_overflow(s.n, (uint64_t)2, &n2) || __builtin_mul_overflow(s.shard_stride, (uint64_t)2, &stride2))
            return false;
        out->push_back(ShardRange{nullptr, 0, n2, s.shard, stride2});
    }
    return true;
}

// true: every interval above lies in the address space and no two share a byte.  total >= 1; every n
// a multiple of total, every row_stride and scale_stride even (the caller's checks).
inline bool mx_lists_disjoint(const MxRange* list, int count, uint64_t total) {
    if (count <= 0) return true;
    if (!list || total == 0) return false;
    std::vector<ShardRange> ranges;
    if (!mx_as_ranges(list, count, &ranges)) return false;
    return shard_lists_disjoint(ranges.data(), (int)ranges.size(), total);
}

// The argument rules of the call that need no plan, as engine.cpp mx_check applies them (plain C++,
// so that tests/test_mx_ranges.py can hold every one of them without a device).
enum MxVerdict { kMxOk = 0, kMxArg, kMxUnsupported };

// flags with an unknown bit (ALLRED_MX_SCALE_RCEIL is bit 0)
inline bool mx_flags_ok(int flags) { return (flags & ~1) == 0; }

// kMxArg: a NULL pointer; rows not 16-byte, scales not 8-byte, the shard not 16-byte aligned; n == 0
// or not a multiple of 8 total (the grouped calls' rule for a rank row); row_stride < n or % 16 != 0;
// scale_stride < n / 32 or % 8 != 0; shard_stride < blk or % 4 != 0; more than 2^31 - 1 tiles of 256
// elements in the list; address arithmetic that would overflow; two intervals sharing a byte.  Then
// kMxUnsupported for the whole list: a bucket that is not whole tiles (total < 8 or n % (256 total)).
inline MxVerdict mx_list_verdict(const MxRange* list, int count, uint64_t total) {
    if (count <= 0) return count < 0 ? kMxArg : kMxOk;
    if (!list || total == 0) return kMxArg;
    uint64_t tiles = 0;
    for (int i = 0; i < count; ++i) {
        const MxRange& s = list[i];
        if (!s.rows || (uintptr_t)s.rows % 16 || !s.scales || (uintptr_t)s.scales % 8 || !s.shard || (uintptr_t)s.shard % 16)
            return kMxArg;
        if (s.n == 0 || total > UINT64_MAX / 8 || s.n % (8 * total)) return kMxArg;
        if (s.row_stride < s.n || s.row_stride % 16) return kMxArg;
        if (s.scale_stride < s.n / 32 || s.scale_stride % 8) return kMxArg;
        if (s.shard_stride < s.n / total || s.shard_stride % 4) return kMxArg;
        const uint64_t t = s.n / 256 + (s.n % 256 ? 1 : 0);
        if (t > kMxMaxTiles - tiles) return kMxArg;
        tiles += t;
    }
    if (!mx_lists_disjoint(list, count, total)) return kMxArg;
    for (int i = 0; i < count; ++i)
        if (total < 8 || list[i].n % (256 * total)) return kMxUnsupported;
    return kMxOk;
}

}  // namespace tsa
