// adamw_ranges.hpp — the disjointness rule of allred_plan_adamw_all_gather_shards_f32 (allred.h):
// byte-exact and block-exact, on shard_f32_ranges.hpp and shard_ranges.hpp.
//
// The call WRITES three or four fp32 planes and the rank rows of every bucket and reads hyper and
// norm_sq while it does, so these byte sets must be pairwise disjoint:
//   every bucket's rank-row interval      [ranks, ranks + 2 total rank_stride), the skew included;
//   the 4 P count plane blocks            [plane + 4 b shard_stride, + 4 blk), blk = n / total —
//                                         param, grad, exp_avg and exp_avg_sq of every bucket;
//   [hyper, + 32)   [norm_sq, + 4 total) (when given)   [info, + 16) (when given).
// allred_plan_adamw_all_gather_shards_f32_groups reads an ARRAY of hyper sets: its interval is
// [hyper, + 32 ngroups), passed as hyper_bytes (defaulted to the one set's 32), under the same rule.
// A bucket is four ShardF32Ranges — one with the rows and the parameter plane, three with
// ranks = nullptr and stride 0 (no row interval) and one of the other planes — and
// shard_f32_lists_disjoint answers for the 4 count of them unchanged: its verdict does not depend
// on which entry an interval came from.  Four rank-major flat buffers, one per plane, bucket i at
// column off_i with shard_stride = F, are therefore accepted like one (shard_ranges.hpp, step 3).
// The three small intervals go against each other and, by shard_f32_norm_ranges.hpp's two-block
// test, against every row interval and plane block: any of them may live in the gap of a wide
// shard_stride.
// Plain C++: engine.cpp includes it under hipcc, tests/test_adamw_ranges.py under g++.
#pragma once

#include <cstdint>
#include <vector>

#include "shard_f32_norm_ranges.hpp"
#include "shard_f32_ranges.hpp"

namespace tsa {

constexpr uint64_t kAdamwHyperBytes = 32, kAdamwInfoBytes = 16;
constexpr int kAdamwParamGroupsMax = 8;   // ALLRED_ADAMW_PARAM_GROUPS_MAX (allred.h)

struct AdamwRange {
    const void* ranks;       // rank 0's row of bf16
    uint64_t stride;         // bf16 elements between rank rows
    uint64_t n;              // bf16 elements per rank row; blk = n / total
    const void* plane[4];    // param, grad, exp_avg, exp_avg_sq: fp32, all required
    uint64_t shard_stride;   // floats between the blocks of every plane
};

// the list as 4 count ShardF32Ranges, appended to *out
inline void adamw_as_f32_ranges(const AdamwRange* list, int count, std::vector<ShardF32Range>* out) {
    out->reserve(out->size() + 4 * (size_t)(count > 0 ? count : 0));
    for (int i = 0; i < count; ++i) {
        const AdamwRange& a = list[i];
        out->push_back(ShardF32Range{a.ranks, a.stride, a.n, a.plane[0], a.shard_stride});
        for (int k = 1; k < 4; ++k) out->push_back(ShardF32Range{nullptr, 0, a.n, a.plane[k], a.shard_stride});
    }
}

// true: every interval above lies in the address space and no two share a byte.  total >= 1; every
// n a multiple of total; every plane non-null (the caller's checks).  hyper / norm_sq / info:
// nullptr = not given.  hyper_bytes: the length of hyper's interval, 32 per hyper set.
inline bool adamw_lists_disjoint(const AdamwRange* list, int count, uint64_t total, const void* hyper, const void* norm_sq,
                                 const void* info, uint64_t hyper_bytes = kAdamwHyperBytes) {
    if (count > 0 && (!list || total == 0)) return false;
    std::vector<ShardF32Range> ranges;
    adamw_as_f32_ranges(list, count, &ranges);
    if (!shard_f32_lists_disjoint(ranges.data(), (int)ranges.size(), total)) return false;
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
        for (const ShardF32Range& s : ranges)
            if (shard_f32_norm_detail::hits_bucket(lo[k], hi[k], s, total)) return false;
    }
    return true;
}

// The argument rules of the call that need no plan, as engine.cpp adamw_check applies them (plain
// C++, so that tests/test_adamw_ranges.py can hold every one of them without a device).
enum AdamwVerdict { kAdamwOk = 0, kAdamwArg, kAdamwUnsupported };

// flags with an unknown bit (ALLRED_ADAMW_ZERO_GRAD is bit 0), hyper NULL (unless `dry`: the launch
// count's query has none) or not 16-byte aligned, norm_sq not 4-byte aligned, info not 16-byte aligned
inline bool adamw_pointers_ok(const void* hyper, const void* norm_sq, const void* info, int flags, bool dry) {
    if (flags & ~1) return false;
    if (!hyper && !dry) return false;
    return (uintptr_t)hyper % 16 == 0 && (uintptr_t)norm_sq % 4 == 0 && (uintptr_t)info % 16 == 0;
}

// A list whose rank rows have passed the grouped calls' rules (engine.cpp group_check: n a non-zero
// multiple of 8 total, rank_stride >= n).  kAdamwArg: a NULL plane, a plane not 16-byte aligned,
// shard_stride < blk or % 4 != 0, address arithmetic that would overflow, two intervals sharing a
// byte; then kAdamwUnsupported for the whole list: a bucket that is not whole tiles.
inline AdamwVerdict adamw_list_verdict(const AdamwRange* list, int count, uint64_t total, const void* hyper,
                                       const void* norm_sq, const void* info, uint64_t hyper_bytes = kAdamwHyperBytes) {
    if (count > 0 && (!list || total == 0)) return kAdamwArg;
    for (int i = 0; i < count; ++i) {
        const AdamwRange& a = list[i];
        for (const void* q : a.plane)
            if (!q || (uintptr_t)q % 16) return kAdamwArg;
        if (a.shard_stride < a.n / total || a.shard_stride % 4) return kAdamwArg;
    }
    if (!adamw_lists_disjoint(list, count, total, hyper, norm_sq, info, hyper_bytes)) return kAdamwArg;
    for (int i = 0; i < count; ++i)
        if (total < 8 || list[i].n % (256 * total)) return kAdamwUnsupported;
    return kAdamwOk;
}

// The two group rules of allred_plan_adamw_all_gather_shards_f32_groups: 1 <= ngroups <=
// kAdamwParamGroupsMax, and every group_of[i], i < count, below ngroups.  group_of == nullptr: every
// bucket is in group 0, which exists.  count <= 0: only ngroups is looked at.
inline bool adamw_groups_ok(const uint8_t* group_of, int count, int ngroups) {
    if (ngroups < 1 || ngroups > kAdamwParamGroupsMax) return false;
    if (!group_of) return true;
    for (int i = 0; i < count; ++i)
        if (group_of[i] >= ngroups) return false;
    return true;
}

}  // namespace tsa
