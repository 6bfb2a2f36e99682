// adamw_mx_kernels.hip — AdamW on the fp32 shards inside the MXFP8 all-gather launch
// (allred_plan_adamw_all_gather_shards_mxfp8, allred.h): the MXFP8 training step in two launches.
//
//   k_adamw_ag_mxfp8<P, ZERO, RCEIL>  adamw_ag (adamw_body.hpp) — the body of k_adamw_ag_groups_f32,
//                                     always with parameter groups — with the MXFP8 output stage:
//                                     p' is quantised in wave 0's registers, once, from fp32 (there is
//                                     no bf16 in between), and every rank's element row and scale
//                                     row receives what k_ag_group_mxfp8 writes from a shard that
//                                     holds p'.  The planes receive what k_adamw_ag_groups_f32 stores.
//
// The arithmetic depends on the build's -ffp-contract=off as adamw_kernels.hip's does.
#include <type_traits>

#include "adamw_body.hpp"
#include "device.hpp"
#include "group_batch.hpp"
#include "group_span.hpp"
#include "launch_util.hpp"

namespace tsa {
namespace {

constexpr int kAdamwMxGroupMax = ALLRED_ADAMW_MX_GROUP_MAX;   // buckets of one launch
static_assert(kAdamwMxGroupMax == kAdamwGroupMax, "adamw_body.hpp's tables hold a launch");
static_assert(sizeof(allred_adamw_mx_bucket_f32) == 80, "allred.h's layout");
// GroupSpan (element rows, in bytes) 2064 + AdamwGroup 1280 + AdamwMxScales 512 + AdamwGroupOf 32 + three
// pointers and ngroups 32 = 3920 bytes of kernel arguments
static_assert(sizeof(GroupSpan) + sizeof(AdamwGroup) + sizeof(AdamwMxScales) + sizeof(AdamwGroupOf) + 3 * 8 + 8 == 3920,
              "the kernel-argument sum");
static_assert(sizeof(GroupSpan) + sizeof(AdamwGroup) + sizeof(AdamwMxScales) + sizeof(AdamwGroupOf) + 3 * 8 + 8 < 4096,
              "kernel arguments stay below 4 KiB");

// the kernel arguments handed to the body by reference (adamw_kernels.hip says why)
template <int P, bool ZERO, bool RCEIL>
__global__ __launch_bounds__(kBlock) void k_adamw_ag_mxfp8(GroupSpan span, AdamwGroup planes, AdamwMxScales scales,
                                                           AdamwGroupOf group_of, const allred_adamw_hyper* __restrict__ hyper,
                                                           int ngroups, const float* __restrict__ norm_sq, float* info) {
    adamw_ag<P, ZERO, true, RCEIL ? kOutMxRceil : kOutMxFloor, AdamwMxScales>(span, planes, group_of, hyper, ngroups, norm_sq, info,
                                                                             scales);
}
// k_ag_group_f32's resident cap kAgGroupGrid, inherited as in adamw_kernels.hip and mx_kernels.hip: the
// cap is unmeasured for this kernel (tune pipe_grid caps it lower)
constexpr uint64_t kAdamwMxGrid = kMaxGrid;

}  // namespace

// A (checked: engine.cpp adamw_mx_check) list of whole-tile buckets — four fp32 planes, element rows,
// scale rows — through k_adamw_ag_mxfp8, ALLRED_ADAMW_MX_GROUP_MAX buckets per launch in list order
// whatever the groups are.  hyper is ngroups >= 1 sets and group_of the buckets' groups (nullptr: every
// bucket in group 0); a launch's group table is indexed by the bucket's place in the LAUNCH.  info goes
// to the first launch alone: it is written once.  dry: nothing is launched and the number of launches
// is returned.
int launch_adamw_group_mxfp8(const allred_adamw_mx_bucket_f32* buckets, const uint8_t* group_of, int count, int total,
                             const allred_adamw_hyper* hyper, int ngroups, const float* norm_sq, float* info, bool zero_grad,
                             bool rceil, bool dry, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    struct Side {
        AdamwGroup planes;
        AdamwMxScales scales;
        AdamwGroupOf groups;
    } side{};
    if (ngroups < 1 || ngroups > kParamGroupsMax) return ALLRED_ERR_ARG;   // the caller's check, kept next to its use
    auto add = [&](int i, int slot) {
        const allred_adamw_mx_bucket_f32& b = buckets[i];
        const uint64_t tiles = b.elems_per_rank / 256;
        const uint32_t g = group_of ? group_of[i] : 0u;
        if (total < 8 || b.elems_per_rank % (256 * (uint64_t)total)) return BatchAdd::error(ALLRED_ERR_UNSUPPORTED);   // the caller's checks, kept next to their use
        if (g >= (uint32_t)ngroups) return BatchAdd::error(ALLRED_ERR_ARG);
        side.planes.s[slot] = AdamwPlanes{b.param, b.grad, b.exp_avg, b.exp_avg_sq, b.shard_stride};
        side.scales.s[slot] = AdamwMxScaleRows{b.scales, b.scale_stride};
        side.groups.w[slot >> 2] |= g << (8 * (slot & 3));
        return BatchAdd::member(GroupIn{reinterpret_cast<uint16_t*>(b.rows), b.row_stride, tiles, tiles / total});
    };
    auto launch = [&](const GroupSpan& span, unsigned grid, int index, uint64_t) {
        const AdamwGroup& planes = side.planes;
        const AdamwMxScales& scales = side.scales;
        const AdamwGroupOf& groups = side.groups;
        float* out = index == 0 ? info : nullptr;
        const bool found = for_ranks<8, 64>(total, [&](auto p) {
            auto go = [&](auto zero, auto rc) {
                hipLaunchKernelGGL((k_adamw_ag_mxfp8<p(), decltype(zero)::value, decltype(rc)::value>), dim3(grid), dim3(kBlock), 0, st, span,
                                   planes, scales, groups, hyper, ngroups, norm_sq, out);
                trace_launch(grid, kBlock, "k_adamw_ag_mxfp8<%d, %s, %s>", total, tf(zero_grad), tf(rceil));
            };
            if (zero_grad) {
                if (rceil) go(std::true_type{}, std::true_type{});
                else go(std::true_type{}, std::false_type{});
            } else {
                if (rceil) go(std::false_type{}, std::true_type{});
                else go(std::false_type{}, std::false_type{});
            }
        });
        return found ? last_error() : ALLRED_ERR_UNSUPPORTED;
    };
    return group_batch<kAdamwMxGroupMax>(count, dry, side, add, [](uint64_t tiles) { return persistent_grid(tiles, kAdamwMxGrid); },
                                         launch);
}

}  // namespace tsa
