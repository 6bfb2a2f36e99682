// adamw_mx4_rht_kernels.hip — AdamW on the fp32 shards inside the rotated MXFP4 all-gather launch
// (allred_plan_adamw_all_gather_shards_mxfp4_rht, allred.h): the MXFP4 training step with the random Hadamard
// rotation of the GEMM operand, still in two launches.
//
//   k_adamw_ag_mxfp4_rht<P, ZERO, RCEIL>  adamw_ag (adamw_body.hpp) as k_adamw_ag_mxfp4 instantiates it, with
//                                         the output modes kOutMx4RhtFloor / kOutMx4RhtRceil: a COPY of p' is
//                                         rotated in wave 0's registers (mx_rht.hpp; the stages across the eight
//                                         lanes of a block through DPP) and quantised to e2m1 nibbles; the
//                                         planes receive p', m', v' as k_adamw_ag_mxfp4 stores them.  LDS slot,
//                                         barrier and store split are that kernel's.
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

constexpr int kAdamwMx4RhtGroupMax = ALLRED_ADAMW_MX_GROUP_MAX;   // buckets of one launch: the MXFP4 AdamW call's
static_assert(kAdamwMx4RhtGroupMax == kAdamwGroupMax, "adamw_body.hpp's tables hold a launch");
static_assert(sizeof(allred_adamw_mx_bucket_f32) == 80, "allred.h's layout");
// k_adamw_ag_mxfp4's 3920 bytes of arguments and the sign mask (padded to 8 bytes)
static_assert(sizeof(GroupSpan) + sizeof(AdamwGroup) + sizeof(AdamwMxScales) + sizeof(AdamwGroupOf) + 3 * 8 + 8 + 8 == 3928,
              "the kernel-argument sum");
static_assert(sizeof(GroupSpan) + sizeof(AdamwGroup) + sizeof(AdamwMxScales) + sizeof(AdamwGroupOf) + 3 * 8 + 8 + 8 < 4096,
              "kernel arguments stay below 4 KiB");

// the kernel arguments handed to the body by reference (adamw_kernels.hip says why)
template <int P, bool ZERO, bool RCEIL>
__global__ __launch_bounds__(kBlock) void k_adamw_ag_mxfp4_rht(GroupSpan span, AdamwGroup planes, AdamwMxScales scales,
                                                               AdamwGroupOf group_of, const allred_adamw_hyper* __restrict__ hyper,
                                                               int ngroups, const float* __restrict__ norm_sq, float* info,
                                                               uint32_t sign_mask) {
    adamw_ag<P, ZERO, true, RCEIL ? kOutMx4RhtRceil : kOutMx4RhtFloor, AdamwMxScales>(span, planes, group_of, hyper, ngroups, norm_sq,
                                                                                     info, scales, sign_mask);
}
// k_adamw_ag_mxfp4's cap, inherited and unmeasured here (tune pipe_grid caps it lower)
constexpr uint64_t kAdamwMx4RhtGrid = kMaxGrid;

}  // namespace

// A (checked: engine.cpp adamw_mx_check with the MXFP4 payload) list of whole-tile buckets through
// k_adamw_ag_mxfp4_rht: launch_adamw_group_mxfp4's batching — ALLRED_ADAMW_MX_GROUP_MAX buckets per launch in
// list order whatever the groups are, info to the first launch alone —, so the launch count of a list is that
// call's; sign_mask goes to every launch.
int launch_adamw_group_mxfp4_rht(const allred_adamw_mx_bucket_f32* buckets, const uint8_t* group_of, int count, int total,
                                 const allred_adamw_hyper* hyper, int ngroups, const float* norm_sq, float* info, bool zero_grad,
                                 bool rceil, uint32_t sign_mask, void* stream) {
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
                hipLaunchKernelGGL((k_adamw_ag_mxfp4_rht<p(), decltype(zero)::value, decltype(rc)::value>), dim3(grid), dim3(kBlock), 0, st,
                                   span, planes, scales, groups, hyper, ngroups, norm_sq, out, sign_mask);
                trace_launch(grid, kBlock, "k_adamw_ag_mxfp4_rht<%d, %s, %s>", total, tf(zero_grad), tf(rceil));
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
    return group_batch<kAdamwMx4RhtGroupMax>(count, /*dry=*/false, side, add,
                                             [](uint64_t tiles) { return persistent_grid(tiles, kAdamwMx4RhtGrid); }, launch);
}

}  // namespace tsa
