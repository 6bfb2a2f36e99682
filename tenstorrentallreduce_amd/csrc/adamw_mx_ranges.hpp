// adamw_mx_ranges.hpp — the argument rules that need no plan, and the disjointness rule, of
// allred_plan_adamw_all_gather_shards_mxfp8 (allred.h): mx_ranges.hpp's rules for the element rows and
// the scale rows, adamw_ranges.hpp's for the four planes and the three small buffers, composed.  No
// interval algorithm of its own: shard_lists_disjoint (shard_ranges.hpp) on 2-byte units answers for the
// list, shard_f32_norm_ranges.hpp's two-block test for the small buffers.
//
// The call WRITES the e4m3 rows, the E8M0 scale rows and three or four fp32 planes of every bucket and
// reads hyper and norm_sq while it does, so these byte sets must be pairwise disjoint:
//   the element rows   ONE interval [rows, rows + total * row_stride) bytes, the stride skew included;
//   the scale rows     ONE interval [scales, scales + total * scale_stride) bytes, likewise;
//   the 4 P count plane blocks   [plane + 4 b shard_stride, + 4 blk), blk = n / total floats — param,
//                                grad, exp_avg and exp_avg_sq of every bucket;
//   [hyper, + 32 ngroups)   [norm_sq, + 4 total) (when given)   [info, + 16) (when given).
// Every byte quantity is even (row_stride % 16, scale_stride % 8, n % 8 total), so a bucket is six
// ShardRanges:
//   the element rows alone   {rows, row_stride / 2, n / 2, nullptr, 0}
//   the scale rows alone     {scales, scale_stride / 2, n / 64, nullptr, 0}
//   each plane alone         {nullptr, 0, 2 n, plane, 2 shard_stride}
// and shard_lists_disjoint answers for the 6 count of them unchanged.  For the small buffers the same
// six are ShardF32Ranges — a row interval of stride s 2-byte units is ShardF32Range{p, s, 0, nullptr, 0},
// a plane {nullptr, 0, n, plane, shard_stride} — and hits_bucket tests each of the three against them,
// as adamw_lists_disjoint does: rows, scales and the three small buffers may lie in the gap of a wide
// shard_stride.
// Plain C++: engine.cpp includes it under hipcc, tests/test_adamw_mx_ranges.py under g++.
#pragma once

#include <cstdint>
#include <vector>

#include "adamw_ranges.hpp"
#include "mx_ranges.hpp"

namespace tsa {

struct AdamwMxRange {
    const void* rows;        // rank 0's row of e4m3 bytes
    uint64_t row_stride;     // bytes between element rows
    const void* scales;      // rank 0's row of E8M0 bytes
    uint64_t scale_stride;   // bytes between scale rows
    uint64_t n;              // elements per rank row; blk = n / total
    const void* plane[4];    // param, grad, exp_avg, exp_avg_sq: fp32, all required
    uint64_t shard_stride;   // floats between the blocks of every plane
};

// the 2-byte view of the list, appended to *out (six entries per bucket); false when a doubling
// overflows — *out is then unspecified
inline bool adamw_mx_as_ranges(const AdamwMxRange* list, int count, std::vector<ShardRange>* out) {
    out->reserve(out->size() + 6 * (size_t)(count > 0 ? count : 0));
    for (int i = 0; i < count; ++i) {
        const AdamwMxRange& s = list[i];
        out->push_back(ShardRange{s.rows, s.row_stride / 2, s.n / 2, nullptr, 0});
        out->push_back(ShardRange{s.scales, s.scale_stride / 2, s.n / 64, nullptr, 0});
        uint64_t n2, stride2;
        if (__builtin_mul_overflow(s.n, (uint64_t)2, &n2) || __builtin_mul_overflow(s.shard_stride, (uint64_t)2, &stride2))
            return false;
        for (const void* q : s.plane) out->push_back(ShardRange{nullptr, 0, n2, q, stride2});
    }
    return true;
}

// true: every interval above lies in the address space and no two share a byte.  total >= 1; every n a
// multiple of total, every row_stride and scale_stride even, every plane non-null (the caller's checks).
// hyper / norm_sq / info: nullptr = not given.  hyper_bytes: the length of hyper's interval.
inline bool adamw_mx_lists_disjoint(const AdamwMxRange* list, int count, uint64_t total, const void* hyper, const void* norm_sq,
                                    const void* info, uint64_t hyper_bytes = kAdamwHyperBytes) {
    if (count > 0 && (!list || total == 0)) return false;
    std::vector<ShardRange> ranges;
    if (!adamw_mx_as_ranges(list, count, &ranges)) return false;
    if (!shard_lists_disjoint(ranges.data(), (int)ranges.size(), total)) return false;
    uint64_t bytes;
    if (__builtin_mul_overflow(total, (uint64_t)4, &bytes)) return false;
    const uint64_t lo[3] = {(uint64_t)(uintptr_t)hyper, (uint64_t)(uintptr_t)norm_sq, (uint64_t)(uintptr_t)info};
    const uint64_t len[3] = {hyper ? hyper_bytes : 0, norm_sq ? bytes : 0, info ? kAdamwInfoBytes : 0};
    uint64_t hi[3];
    for (int k = 0; k < 3; ++k)
        if (__builtin_add_overflow(lo[k], len[k], &hi[k]) || hi[k] > (uint64_t)UINTPTR_MAX) return false;
    for (int k = 0; k < 3; ++k) {
        if (!len[k]) continue;
        for (int j = k + 1; j < 3; ++j)
            if (len[j] && lo[k] < hi[j] && lo[j] < hi[k]) return false;
        for (int i = 0; i < count; ++i) {
            const AdamwMxRange& s = list[i];
            // the list has passed shard_lists_disjoint: none of hits_bucket's products wraps
            if (shard_f32_norm_detail::hits_bucket(lo[k], hi[k], ShardF32Range{s.rows, s.row_stride / 2, 0, nullptr, 0}, total) ||
                shard_f32_norm_detail::hits_bucket(lo[k], hi[k], ShardF32Range{s.scales, s.scale_stride / 2, 0, nullptr, 0}, total))
                return false;
            for (const void* q : s.plane)
                if (shard_f32_norm_detail::hits_bucket(lo[k], hi[k], ShardF32Range{nullptr, 0, s.n, q, s.shard_stride}, total))
                    return false;
        }
    }
    return true;
}

// The argument rules of the call that need no plan, as engine.cpp adamw_mx_check applies them (plain
// C++, so that tests/test_adamw_mx_ranges.py can hold every one of them without a device).
enum AdamwMxVerdict { kAdamwMxOk = 0, kAdamwMxArg, kAdamwMxUnsupported };

// flags with an unknown bit (ALLRED_ADAMW_ZERO_GRAD is bit 0, ALLRED_ADAMW_MX_RCEIL bit 1), hyper NULL
// (unless `dry`: the launch count's query has none) or not 16-byte aligned, norm_sq not 4-byte aligned,
// info not 16-byte aligned
inline bool adamw_mx_pointers_ok(const void* hyper, const void* norm_sq, const void* info, int flags, bool dry) {
    if (flags & ~3) return false;
    return adamw_pointers_ok(hyper, norm_sq, info, 0, dry);
}

// kAdamwMxArg: a NULL pointer; rows not 16-byte, scales not 8-byte, a plane not 16-byte aligned; n == 0
// or not a multiple of 8 total; row_stride < n or % 16 != 0; scale_stride < n / 32 or % 8 != 0;
// shard_stride < blk or % 4 != 0; more than 2^31 - 1 tiles of 256 elements in the list; address
// arithmetic that would overflow; two intervals sharing a byte.  Then kAdamwMxUnsupported for the whole
// list: a bucket that is not whole tiles (total < 8 or n % (256 total)).
inline AdamwMxVerdict adamw_mx_list_verdict(const AdamwMxRange* list, int count, uint64_t total, const void* hyper,
                                            const void* norm_sq, const void* info, uint64_t hyper_bytes = kAdamwHyperBytes) {
    if (count < 0) return kAdamwMxArg;
    if (count > 0 && (!list || total == 0)) return kAdamwMxArg;
    uint64_t tiles = 0;
    for (int i = 0; i < count; ++i) {
        const AdamwMxRange& s = list[i];
        if (!s.rows || (uintptr_t)s.rows % 16 || !s.scales || (uintptr_t)s.scales % 8) return kAdamwMxArg;
        for (const void* q : s.plane)
            if (!q || (uintptr_t)q % 16) return kAdamwMxArg;
        if (s.n == 0 || total > UINT64_MAX / 8 || s.n % (8 * total)) return kAdamwMxArg;
        if (s.row_stride < s.n || s.row_stride % 16) return kAdamwMxArg;
        if (s.scale_stride < s.n / 32 || s.scale_stride % 8) return kAdamwMxArg;
        if (s.shard_stride < s.n / total || s.shard_stride % 4) return kAdamwMxArg;
        const uint64_t t = s.n / 256 + (s.n % 256 ? 1 : 0);
        if (t > kMxMaxTiles - tiles) return kAdamwMxArg;
        tiles += t;
    }
    if (!adamw_mx_lists_disjoint(list, count, total, hyper, norm_sq, info, hyper_bytes)) return kAdamwMxArg;
    for (int i = 0; i < count; ++i)
        if (total < 8 || list[i].n % (256 * total)) return kAdamwMxUnsupported;
    return kAdamwMxOk;
}

}  // namespace tsa
