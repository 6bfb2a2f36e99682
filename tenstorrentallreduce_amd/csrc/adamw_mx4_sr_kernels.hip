// adamw_mx4_sr_kernels.hip — AdamW on the fp32 shards inside the stochastically rounded MXFP4 all-gather launch
// (allred_plan_adamw_all_gather_shards_mxfp4_sr, allred.h): the MXFP4 training step with the unbiased backward
// operand, rotated or not, still in two launches.
//
//   k_adamw_ag_mxfp4_sr<P, ZERO, RCEIL, RHT>  adamw_ag (adamw_body.hpp) as k_adamw_ag_mxfp4 instantiates it, with
//                                             the output modes kOutMx4Sr*: p' — or, RHT, its rotated copy — is
//                                             rounded to e2m1 nibbles by mx_sr.hpp's rule with the words of ONE
//                                             Philox call per lane and tile, generated in front of the wait for
//                                             the tile's planes; the planes receive p', m', v' as
//                                             k_adamw_ag_mxfp4 stores them.  LDS slot, barrier and store split are
//                                             that kernel's.
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

constexpr int kAdamwMx4SrGroupMax = ALLRED_ADAMW_MX_GROUP_MAX;   // buckets of one launch: the MXFP4 AdamW call's
static_assert(kAdamwMx4SrGroupMax == kAdamwGroupMax, "adamw_body.hpp's tables hold a launch");
static_assert(sizeof(allred_adamw_mx_bucket_f32) == 80, "allred.h's layout");
// k_adamw_ag_mxfp4's 3920 bytes of arguments, the sign mask and the launch's first bucket (4 bytes each) and sr
static_assert(sizeof(GroupSpan) + sizeof(AdamwGroup) + sizeof(AdamwMxScales) + sizeof(AdamwGroupOf) + 3 * 8 + 8 + 8 + 8 == 3936,
              "the kernel-argument sum");
static_assert(3936 < 4096, "kernel arguments stay below 4 KiB");

constexpr AdamwOut sr_out(bool rceil, bool rht) {
    return rht ? (rceil ? kOutMx4SrRhtRceil : kOutMx4SrRhtFloor) : (rceil ? kOutMx4SrRceil : kOutMx4SrFloor);
}

// the kernel arguments handed to the body by reference (adamw_kernels.hip says why)
template <int P, bool ZERO, bool RCEIL, bool RHT>
__global__ __launch_bounds__(kBlock) void k_adamw_ag_mxfp4_sr(GroupSpan span, AdamwGroup planes, AdamwMxScales scales,
                                                              AdamwGroupOf group_of, const allred_adamw_hyper* __restrict__ hyper,
                                                              int ngroups, const float* __restrict__ norm_sq, float* info,
                                                              uint32_t sign_mask, uint32_t first_bucket,
                                                              const allred_mx_sr_state* __restrict__ sr) {
    adamw_ag<P, ZERO, true, sr_out(RCEIL, RHT), AdamwMxScales>(span, planes, group_of, hyper, ngroups, norm_sq, info, scales, sign_mask,
                                                               sr, first_bucket);
}
// k_adamw_ag_mxfp4's cap, inherited and unmeasured here (tune pipe_grid caps it lower)
constexpr uint64_t kAdamwMx4SrGrid = kMaxGrid;

}  // namespace

// A (checked: engine.cpp adamw_mx_check with the MXFP4 payload, then sr's own rules) list of whole-tile buckets
// through k_adamw_ag_mxfp4_sr: launch_adamw_group_mxfp4's batching — ALLRED_ADAMW_MX_GROUP_MAX buckets per launch in
// list order whatever the groups are, info to the first launch alone —, so the launch count of a list is that
// call's.  Every bucket is a member, so launch `index` begins at bucket index * ALLRED_ADAMW_MX_GROUP_MAX of the
// caller's list.
int launch_adamw_group_mxfp4_sr(const allred_adamw_mx_bucket_f32* buckets, const uint8_t* group_of, int count, int total,
                                const allred_adamw_hyper* hyper, int ngroups, const float* norm_sq, float* info, bool zero_grad,
                                bool rceil, bool rotate, uint32_t sign_mask, const allred_mx_sr_state* sr, void* stream) {
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
        const uint32_t first = (uint32_t)index * kAdamwMx4SrGroupMax;
        const bool found = for_ranks<8, 64>(total, [&](auto p) {
            auto go = [&](auto zero, auto rc, auto rot) {
                hipLaunchKernelGGL((k_adamw_ag_mxfp4_sr<p(), decltype(zero)::value, decltype(rc)::value, decltype(rot)::value>), dim3(grid),
                                   dim3(kBlock), 0, st, span, planes, scales, groups, hyper, ngroups, norm_sq, out, sign_mask, first, sr);
                trace_launch(grid, kBlock, "k_adamw_ag_mxfp4_sr<%d, %s, %s, %s>", total, tf(zero_grad), tf(rceil), tf(rotate));
            };
            auto scale = [&](auto zero, auto rc) {
                if (rotate) go(zero, rc, std::true_type{});
                else go(zero, rc, std::false_type{});
            };
            if (zero_grad) {
                if (rceil) scale(std::true_type{}, std::true_type{});
                else scale(std::true_type{}, std::false_type{});
            } else {
                if (rceil) scale(std::false_type{}, std::true_type{});
                else scale(std::false_type{}, std::false_type{});
            }
        });
        return found ? last_error() : ALLRED_ERR_UNSUPPORTED;
    };
    return group_batch<kAdamwMx4SrGroupMax>(count, /*dry=*/false, side, add,
                                            [](uint64_t tiles) { return persistent_grid(tiles, kAdamwMx4SrGrid); }, launch);
}

}  // namespace tsa
