// adamw_kernels.hip — AdamW on the fp32 shards inside the grouped all-gather launch
// (allred_plan_adamw_all_gather_shards_f32 and allred_plan_adamw_all_gather_shards_f32_groups,
// allred.h): the optimizer step of a sharded training step at the one point where every master
// parameter is in a register anyway.  ONE kernel body, adamw_ag (adamw_body.hpp, with its bf16 output
// stage; adamw_mx_kernels.hip puts the same body under a third kernel), under two kernels:
//
//   k_adamw_ag_group_f32<P, ZERO>   k_ag_group_f32's walk; a tile's 256 floats of the parameter,
//                                   gradient and the two moment planes loaded ONCE, the clipped
//                                   AdamW update of allred.h applied, p' m' v' stored back, p'
//                                   rounded once to bf16 (pack_rne) and written to every rank row.
//                                   ZERO: +0.0f stored over every gradient element read.
//   k_adamw_ag_groups_f32<P, ZERO>  the same with PARAMETER GROUPS: hyper is an array of ngroups x
//                                   32 bytes, lane g of wave 0 holds group g's eight uniform values,
//                                   and every tile picks its bucket's group out of those lanes with
//                                   v_readlane_b32 (form chosen: DESIGN.md §16).
//
// The arithmetic depends on the build's -ffp-contract=off (Makefile, HIPFLAGS): every operation
// allred.h writes is ONE IEEE fp32 operation, never an fma; `/` and sqrtf are hipcc's correctly
// rounded forms (v_div_scale / v_div_fmas / v_div_fixup, v_sqrt_f32 with its refinement), denormals
// are kept — the tests compare bits, the groups call also against the one-set call.
#include <type_traits>

#include "adamw_body.hpp"
#include "device.hpp"
#include "group_batch.hpp"
#include "group_span.hpp"
#include "launch_util.hpp"

namespace tsa {
namespace {

// The two kernels: each form's own kernel arguments, handed to the body by reference (handed on by
// value the tables were copied, and the code of every instance changed)
template <int P, bool ZERO>
__global__ __launch_bounds__(kBlock) void k_adamw_ag_group_f32(GroupSpan span, AdamwGroup planes,
                                                               const allred_adamw_hyper* __restrict__ hyper,
                                                               const float* __restrict__ norm_sq, float* info) {
    adamw_ag<P, ZERO, false>(span, planes, AdamwGroupOf{}, hyper, 1, norm_sq, info);
}
template <int P, bool ZERO>
__global__ __launch_bounds__(kBlock) void k_adamw_ag_groups_f32(GroupSpan span, AdamwGroup planes, AdamwGroupOf group_of,
                                                                const allred_adamw_hyper* __restrict__ hyper, int ngroups,
                                                                const float* __restrict__ norm_sq, float* info) {
    adamw_ag<P, ZERO, true>(span, planes, group_of, hyper, ngroups, norm_sq, info);
}
// k_ag_group_f32's resident cap kAgGroupGrid, inherited: the cap is unmeasured for these kernels
// (tune pipe_grid caps it lower)
constexpr uint64_t kAdamwGrid = kMaxGrid;

}  // namespace

// A (checked: engine.cpp, adamw_check and adamw_groups_ok) list of whole-tile buckets with their four
// fp32 planes, ALLRED_ADAMW_GROUP_MAX buckets per launch in list order whatever the groups are.
// ngroups == 0: the one-set call — hyper is one set, k_adamw_ag_group_f32.  ngroups >= 1: the groups
// call — hyper is ngroups sets and group_of the buckets' groups (nullptr: every bucket in group 0),
// k_adamw_ag_groups_f32, also for one group; a launch's group table is indexed by the bucket's place
// in the LAUNCH.  info goes to the first launch alone: it is written once.  dry: nothing is launched
// and the number of launches is returned.
int launch_adamw_group_f32(const allred_adamw_bucket_f32* buckets, const uint8_t* group_of, int count, int total,
                           const allred_adamw_hyper* hyper, int ngroups, const float* norm_sq, float* info, bool zero_grad,
                           bool dry, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    struct Side {
        AdamwGroup planes;
        AdamwGroupOf groups;
    } side{};
    if (ngroups < 0 || ngroups > kParamGroupsMax) return ALLRED_ERR_ARG;   // the caller's check, kept next to its use
    auto add = [&](int i, int slot) {
        const allred_adamw_bucket_f32& b = buckets[i];
        const uint64_t nv = b.elems_per_rank / 8, bv = nv / total, tiles = nv / 32;
        const uint32_t g = group_of ? group_of[i] : 0u;
        if (total < 8 || nv % 32 || bv % 32) return BatchAdd::error(ALLRED_ERR_UNSUPPORTED);   // the caller's checks, kept next to their use
        if (g >= (uint32_t)(ngroups ? ngroups : 1)) return BatchAdd::error(ALLRED_ERR_ARG);
        side.planes.s[slot] = AdamwPlanes{b.param, b.grad, b.exp_avg, b.exp_avg_sq, b.shard_stride};
        side.groups.w[slot >> 2] |= g << (8 * (slot & 3));
        return BatchAdd::member(GroupIn{b.ranks, b.rank_stride, tiles, bv / 32});
    };
    auto launch = [&](const GroupSpan& span, unsigned grid, int index, uint64_t) {
        const AdamwGroup& planes = side.planes;
        const AdamwGroupOf& groups = side.groups;
        float* out = index == 0 ? info : nullptr;
        const bool found = for_ranks<8, 64>(total, [&](auto p) {
            if (ngroups == 0) {
                if (zero_grad)
                    hipLaunchKernelGGL((k_adamw_ag_group_f32<p(), true>), dim3(grid), dim3(kBlock), 0, st, span, planes, hyper, norm_sq, out);
                else
                    hipLaunchKernelGGL((k_adamw_ag_group_f32<p(), false>), dim3(grid), dim3(kBlock), 0, st, span, planes, hyper, norm_sq, out);
                trace_launch(grid, kBlock, "k_adamw_ag_group_f32<%d, %s>", total, tf(zero_grad));
                return;
            }
            if (zero_grad)
                hipLaunchKernelGGL((k_adamw_ag_groups_f32<p(), true>), dim3(grid), dim3(kBlock), 0, st, span, planes, groups, hyper,
                                   ngroups, norm_sq, out);
            else
                hipLaunchKernelGGL((k_adamw_ag_groups_f32<p(), false>), dim3(grid), dim3(kBlock), 0, st, span, planes, groups, hyper,
                                   ngroups, norm_sq, out);
            trace_launch(grid, kBlock, "k_adamw_ag_groups_f32<%d, %s>", total, tf(zero_grad));
        });
        return found ? last_error() : ALLRED_ERR_UNSUPPORTED;
    };
    return group_batch<kAdamwGroupMax>(count, dry, side, add, [](uint64_t tiles) { return persistent_grid(tiles, kAdamwGrid); },
                                       launch);
}

}  // namespace tsa
