// adamw_mx2d_ranges.hpp — the argument rules that need no plan, and the disjointness rule, of
// allred_plan_adamw_all_gather_shards_mxfp8_2d (allred.h): mx2d_ranges.hpp's rules for the up to four
// output intervals and the matrix shape, adamw_ranges.hpp's for the four planes and the three small
// buffers, composed as adamw_mx_ranges.hpp composes them.  No interval algorithm of its own:
// shard_lists_disjoint (shard_ranges.hpp) on 2-byte units answers for the list,
// shard_f32_norm_ranges.hpp's two-block test for the small buffers.
//
// The call WRITES up to four row sets and three or four fp32 planes of every bucket and reads hyper and
// norm_sq while it does, so these byte sets must be pairwise disjoint:
//   each row set given   ONE interval [p, p + total * stride) bytes, the stride skew included;
//   the 4 P count plane blocks   [plane + 4 b shard_stride, + 4 blk), blk = n / total floats;
//   [hyper, + 32 ngroups)   [norm_sq, + 4 total) (when given)   [info, + 16) (when given).
// A bucket is seven or nine ShardRanges — mx2d_as_ranges' three or five, the param plane standing where
// the shard stands, and one {nullptr, 0, 2 n, plane, 2 shard_stride} for each other plane.  Outputs and
// the small buffers may lie in the gap of a wide shard_stride.
// Plain C++: engine.cpp includes it under hipcc.
#pragma once

#include <cstdint>
#include <vector>

#include "adamw_mx_ranges.hpp"
#include "mx2d_ranges.hpp"

namespace tsa {

struct AdamwMx2dRange {
    Mx2dRange out;           // the outputs, n and cols; .shard = the param plane, .shard_stride the planes' stride
    const void* plane[3];    // grad, exp_avg, exp_avg_sq
};

// true: every interval above lies in the address space and no two share a byte.  The list has passed
// mx2d_list_verdict's argument rules and every plane is non-null (the caller's checks).
inline bool adamw_mx2d_lists_disjoint(const AdamwMx2dRange* list, int count, uint64_t total, const void* hyper, const void* norm_sq,
                                      const void* info, uint64_t hyper_bytes = kAdamwHyperBytes) {
    if (count > 0 && (!list || total == 0)) return false;
    std::vector<ShardRange> ranges;
    for (int i = 0; i < count; ++i) {
        if (!mx2d_as_ranges(&list[i].out, 1, &ranges)) return false;
        const ShardRange param = ranges.back();   // {nullptr, 0, 2 n, param, 2 shard_stride}
        for (const void* q : list[i].plane) ranges.push_back(ShardRange{nullptr, 0, param.n, q, param.shard_stride});
    }
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
        // the list has passed shard_lists_disjoint: none of hits_bucket's products wraps.  A ShardRange's row
        // interval is 2 total stride bytes and its blocks 2-byte units; hits_bucket's are bf16 rows and floats
        for (const ShardRange& s : ranges)
            if (shard_f32_norm_detail::hits_bucket(lo[k], hi[k], ShardF32Range{s.ranks, s.stride, s.n / 2, s.shard, s.shard_stride / 2},
                                                   total))
                return false;
    }
    return true;
}

// kAdamwMxArg: a NULL plane or one not 16-byte aligned; every kMx2dArg rule of mx2d_list_verdict for the
// outputs, n, cols, shard_stride and the cap of 2^31 - 1 squares; two intervals sharing a byte or address
// arithmetic that would overflow.  Then kAdamwMxUnsupported for the whole list: the 2D call's MX
// necessities (total < 8, cols % 32 != 0, nrows % (32 total) != 0).
// allred_plan_adamw_all_gather_shards_mxfp4_2d takes the same list with TWO elements per byte of rows and
// t_rows: `per_byte` (1: MXFP8, the default; 2: MXFP4) is mx2d_list_verdict's, the payload n / per_byte bytes
// that row_stride and t_row_stride must cover.  The row intervals are total strides long whatever the
// payload, so the disjointness rule above serves both.
inline AdamwMxVerdict adamw_mx2d_list_verdict(const AdamwMx2dRange* list, int count, uint64_t total, const void* hyper,
                                              const void* norm_sq, const void* info, uint64_t hyper_bytes = kAdamwHyperBytes,
                                              uint64_t per_byte = 1) {
    if (count < 0) return kAdamwMxArg;
    if (count > 0 && (!list || total == 0)) return kAdamwMxArg;
    std::vector<Mx2dRange> outs((size_t)count);
    for (int i = 0; i < count; ++i) {
        for (const void* q : list[i].plane)
            if (!q || (uintptr_t)q % 16) return kAdamwMxArg;
        outs[(size_t)i] = list[i].out;   // its NULL or misaligned .shard is mx2d_list_verdict's to refuse
    }
    const Mx2dVerdict shape = mx2d_list_verdict(outs.data(), count, total, per_byte);
    if (shape == kMx2dArg) return kAdamwMxArg;
    if (!adamw_mx2d_lists_disjoint(list, count, total, hyper, norm_sq, info, hyper_bytes)) return kAdamwMxArg;
    return shape == kMx2dOk ? kAdamwMxOk : kAdamwMxUnsupported;
}

}  // namespace tsa
