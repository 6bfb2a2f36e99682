// mx2d_ranges.hpp — the argument rules that need no plan, and the disjointness rule, of
// allred_plan_all_gather_shards_mxfp8_2d (allred.h): mx_ranges.hpp's rules with two more output
// intervals per bucket.  No interval algorithm of its own: shard_lists_disjoint (shard_ranges.hpp) on
// 2-byte units answers for the list, as it does for adamw_mx_ranges.hpp.
//
// The call WRITES up to four row sets of every bucket and reads the fp32 shard while it does, so per
// bucket these byte sets must be pairwise disjoint, and disjoint across buckets:
//   the element rows     ONE interval [rows, rows + total * row_stride) bytes, the stride skew included
//   the scale rows       ONE interval [scales, scales + total * scale_stride)     (both only when given)
//   the t element rows   ONE interval [t_rows, t_rows + total * t_row_stride)
//   the t scale rows     ONE interval [t_scales, t_scales + total * t_scale_stride)
//   the shard            its `total` SEPARATE block intervals [shard + 4 b shard_stride, + 4 blk),
//                        blk = n / total floats.
// Every byte quantity is even (row strides % 16, scale strides % 8), so a bucket is three or five ShardRanges:
//   each row set alone   {p, stride / 2, 0, nullptr, 0}     (a row interval does not depend on n)
//   the shard alone      {nullptr, 0, 2 n, shard, 2 shard_stride}
// Outputs may therefore sit in the gap of a wide shard_stride.  The two doublings are checked.
// Plain C++: engine.cpp includes it under hipcc, tests/test_mx2d_ranges.py under g++.
#pragma once

#include <cstdint>
#include <vector>

#include "mx_ranges.hpp"

namespace tsa {

struct Mx2dRange {
    const void* rows;          // rank 0's row of e4m3 bytes, or nullptr with scales: no row-wise outputs
    uint64_t row_stride;       // bytes
    const void* scales;
    uint64_t scale_stride;     // bytes
    const void* t_rows;        // rank 0's row of the e4m3 bytes of W^T
    uint64_t t_row_stride;     // bytes
    const void* t_scales;
    uint64_t t_scale_stride;   // bytes
    uint64_t n;                // elements per rank row = nrows * cols; blk = n / total
    uint64_t cols;
    const void* shard;         // fp32 shard
    uint64_t shard_stride;     // floats between shard blocks
};

// the 2-byte view of the list, appended to *out; false when a doubling overflows — *out is then unspecified
inline bool mx2d_as_ranges(const Mx2dRange* list, int count, std::vector<ShardRange>* out) {
    out->reserve(out->size() + 5 * (size_t)(count > 0 ? count : 0));
    for (int i = 0; i < count; ++i) {
        const Mx2dRange& s = list[i];
        if (s.rows) {
            out->push_back(ShardRange{s.rows, s.row_stride / 2, 0, nullptr, 0});
            out->push_back(ShardRange{s.scales, s.scale_stride / 2, 0, nullptr, 0});
        }
        out->push_back(ShardRange{s.t_rows, s.t_row_stride / 2, 0, nullptr, 0});
        out->push_back(ShardRange{s.t_scales, s.t_scale_stride / 2, 0, nullptr, 0});
        uint64_t n2, stride2;
        if (__builtin_mul_overflow(s.n, (uint64_t)2, &n2) || __builtin_mul_overflow(s.shard_stride, (uint64_t)2, &stride2))
            return false;
        out->push_back(ShardRange{nullptr, 0, n2, s.shard, stride2});
    }
    return true;
}

// true: every interval above lies in the address space and no two share a byte.  total >= 1; every n a
// multiple of total, every stride even, rows and scales both given or both nullptr (the caller's checks).
inline bool mx2d_lists_disjoint(const Mx2dRange* list, int count, uint64_t total) {
    if (count <= 0) return true;
    if (!list || total == 0) return false;
    std::vector<ShardRange> ranges;
    if (!mx2d_as_ranges(list, count, &ranges)) return false;
    return shard_lists_disjoint(ranges.data(), (int)ranges.size(), total);
}

// The argument rules of the call that need no plan, as engine.cpp mx2d_check applies them.
enum Mx2dVerdict { kMx2dOk = 0, kMx2dArg, kMx2dUnsupported };

// flags with an unknown bit (ALLRED_MX_SCALE_RCEIL is bit 0)
inline bool mx2d_flags_ok(int flags) { return mx_flags_ok(flags); }

// kMx2dArg: exactly one of rows and scales nullptr; t_rows, t_scales or shard nullptr; rows, t_rows or the
// shard not 16-byte, scales or t_scales not 8-byte aligned; n == 0 or not a multiple of 8 total; cols == 0
// or n % cols != 0; a row stride < n or % 16 != 0; a scale stride < n / 32 or % 8 != 0; shard_stride < blk
// or % 4 != 0; more than 2^31 - 1 squares of 1024 elements in the list (the work items of every patch
// shape are at most these); address arithmetic that would overflow; two intervals sharing a byte.  Then
// kMx2dUnsupported for the whole list, the MX necessities: total < 8, cols % 32 != 0 or
// nrows % (32 total) != 0 in a bucket.
inline Mx2dVerdict mx2d_list_verdict(const Mx2dRange* list, int count, uint64_t total) {
    if (count <= 0) return count < 0 ? kMx2dArg : kMx2dOk;
    if (!list || total == 0) return kMx2dArg;
    uint64_t squares = 0;
    for (int i = 0; i < count; ++i) {
        const Mx2dRange& s = list[i];
        if (!s.rows != !s.scales) return kMx2dArg;
        if (s.rows && ((uintptr_t)s.rows % 16 || (uintptr_t)s.scales % 8)) return kMx2dArg;
        if (!s.t_rows || (uintptr_t)s.t_rows % 16 || !s.t_scales || (uintptr_t)s.t_scales % 8 || !s.shard || (uintptr_t)s.shard % 16)
            return kMx2dArg;
        if (s.n == 0 || total > UINT64_MAX / 8 || s.n % (8 * total)) return kMx2dArg;
        if (s.cols == 0 || s.n % s.cols) return kMx2dArg;
        if (s.rows && (s.row_stride < s.n || s.row_stride % 16 || s.scale_stride < s.n / 32 || s.scale_stride % 8)) return kMx2dArg;
        if (s.t_row_stride < s.n || s.t_row_stride % 16 || s.t_scale_stride < s.n / 32 || s.t_scale_stride % 8) return kMx2dArg;
        if (s.shard_stride < s.n / total || s.shard_stride % 4) return kMx2dArg;
        const uint64_t q = s.n / 1024 + (s.n % 1024 ? 1 : 0);
        if (q > kMxMaxTiles - squares) return kMx2dArg;
        squares += q;
    }
    if (!mx2d_lists_disjoint(list, count, total)) return kMx2dArg;
    for (int i = 0; i < count; ++i) {
        const Mx2dRange& s = list[i];
        if (total < 8 || s.cols % 32 || (s.n / s.cols) % (32 * total)) return kMx2dUnsupported;
    }
    return kMx2dOk;
}

}  // namespace tsa
