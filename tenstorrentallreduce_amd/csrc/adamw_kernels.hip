// adamw_kernels.hip — AdamW on the fp32 shards inside the grouped all-gather launch
// (allred_plan_adamw_all_gather_shards_f32 and allred_plan_adamw_all_gather_shards_f32_groups,
// allred.h): the optimizer step of a sharded training step at the one point where every master
// parameter is in a register anyway.  ONE kernel body, adamw_ag, under two kernels:
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

#include "device.hpp"
#include "group_batch.hpp"
#include "group_span.hpp"
#include "launch_util.hpp"

namespace tsa {
namespace {

constexpr int kAdamwGroupMax = ALLRED_ADAMW_GROUP_MAX;            // buckets of one launch
constexpr int kParamGroupsMax = ALLRED_ADAMW_PARAM_GROUPS_MAX;    // hyperparameter sets of one call

// The four fp32 planes of a grouped launch: entry i for bucket i of the launch, block b of the
// bucket at plane + b * stride floats, ONE stride for the four.  32 x 40 bytes by value next to
// GroupSpan (reused as it is, half of its table in use) and three pointers:
// 2064 + 1280 + 24 = 3368 bytes of kernel arguments, inside 4 KiB.
struct AdamwPlanes {       // 40 bytes
    float* param;
    float* grad;
    float* exp_avg;
    float* exp_avg_sq;
    uint64_t stride;       // floats
};
struct AdamwGroup {
    AdamwPlanes s[kAdamwGroupMax];   // entries past the last bucket: zero
};
// The parameter group of every bucket of the LAUNCH: one byte per bucket, byte i for bucket i of the
// launch (not of the list), four to a word so that the wave-uniform lookup is one scalar load, a
// shift and a mask.  By value next to the two tables:
// 2064 + 1280 + 32 + 24 + 8 (ngroups, padded) = 3408 bytes of kernel arguments, inside 4 KiB.
struct AdamwGroupOf {
    uint32_t w[kAdamwGroupMax / 4];   // bytes past the last bucket: zero
};
static_assert(sizeof(AdamwPlanes) == 40 && sizeof(AdamwGroup) == 40 * kAdamwGroupMax, "the kernel-argument layout");
static_assert(sizeof(AdamwGroupOf) == kAdamwGroupMax && kAdamwGroupMax % 4 == 0, "one byte per bucket of a launch");
static_assert(sizeof(GroupSpan) + sizeof(AdamwGroup) + sizeof(AdamwGroupOf) + 3 * 8 + 8 < 4096, "kernel arguments stay below 4 KiB");
static_assert(kParamGroupsMax <= 64, "a group per lane of wave 0 (and a group index fits its byte)");
static_assert(sizeof(allred_adamw_hyper) == 32 && sizeof(allred_adamw_bucket_f32) == 64, "allred.h's layouts");

// the value lane `g` of this wave holds in x, as a wave-uniform (scalar) value; g is wave-uniform
__device__ __forceinline__ float from_lane(float x, int g) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), g));
}

// The call-wide values (allred.h): the same in every lane and every launch.
struct CallWide {
    float N, c;
    bool skip;
};
// The values of a hyperparameter set.  One set: the same in every lane.  Groups: group g's in LANE g
// of wave 0 (lanes >= ngroups: a copy of the last group's, never picked).
struct PerGroup {
    float d, o1, o2, ss;
    float beta1, beta2, eps, bc2;
};

// Wave 0, all 64 lanes active.  max_norm: the one set's, or hyper[0]'s, wave-uniform; x =
// norm_sq[lane] (lane < P, else +0.0f; given: norm_sq != NULL).
__device__ __forceinline__ CallWide call_wide(float max_norm, float x, bool given) {
    CallWide u{0.0f, 1.0f, false};
    if (given) {
        u.N = add_halves(add_lanes32(x));
        u.skip = !(__builtin_fabsf(u.N) < __builtin_inff());   // NaN or +-Inf
        const float q = max_norm / (sqrtf(u.N) + 1e-6f);
        u.c = (q < 1.0f) ? q : 1.0f;
    }
    return u;
}
// a set's values from its 32 bytes of hyper: single fp32 operations
__device__ __forceinline__ PerGroup per_group(const allred_adamw_hyper& h) {
    PerGroup v;
    v.d = 1.0f - h.lr * h.weight_decay;
    v.o1 = 1.0f - h.beta1;
    v.o2 = 1.0f - h.beta2;
    v.ss = h.lr / h.bias_corr1;
    v.beta1 = h.beta1;
    v.beta2 = h.beta2;
    v.eps = h.eps;
    v.bc2 = h.bias_corr2_sqrt;
    return v;
}

// ---------------------------------------------------------------------------
// adamw_ag<P, ZERO, GROUPS>: k_ag_group_f32's walk — persistent grid, workgroup g takes tiles
// g + j * G, a forward-only wave-uniform cursor over GroupSpan, a tile = 256 floats of ONE block at
// plane + b * stride + rem * 256 — with the planes REWRITTEN.  k_ag_group_f32 lets all four waves
// and both lane halves load the same 1 KiB; here a wave that loaded p after another wave's store of
// p' had landed would update the element twice.  So (form (a) of DESIGN.md §15):
//   wave 0 alone touches the planes.  Lane l loads floats 4 l .. 4 l + 3 of the tile from each of
//   the four planes (four 16-byte loads), computes, and puts its 8 bytes of bf16 into one of two
//   512-byte LDS slots.
//   lds_barrier(): ONE barrier per tile.  Slot j & 1 is rewritten for tile j + 2, when every
//   wave has passed the barrier of tile j + 1 and with it its own LDS read of tile j (its row
//   stores of tile j, issued before that barrier, needed the data).
//   every wave then reads column c's 16 bytes from the slot and stores them to its rows
//   r = RPW w + RPI k + q, as k_ag_group_f32's store loop does; wave 0 stores p' m' v' (ZERO: and
//   +0 over g) BEHIND its row stores — the same lane that loaded an element stores it, and no other
//   lane of the grid reads or writes it (the lists are block-disjoint: engine.cpp adamw_check).
//   With the planes' stores in front of the barrier the compiler made wave 0 wait for two of them
//   there (it reuses their data registers), and every row store of the workgroup with it.
// The next tile's four loads are issued before this tile's arithmetic (registers of their own)
// and waited for behind it; the last tile of a workgroup has no loads behind it.
// skip (N non-finite): the planes keep their bits — nothing is stored to them — and the rows
// receive bf16_rne(p).  info: lane 0 of wave 0 of workgroup 0 of the call's FIRST launch (the
// host passes info to that launch alone) stores {N, c, skip, +0} as one 16-byte vector store.
// GROUPS (the other form holds none of this: if constexpr):
//   prologue, wave 0: lane g < ngroups loads hyper[g] (two 16-byte vector loads; lanes >= ngroups
//   load hyper[ngroups - 1] again: no lane reads past the array).  N, skip and c are the call's: c
//   from lane 0's max_norm, the max_norm of the other groups is loaded and never used.  Lane g
//   forms group g's d, o1, o2, ss.
//   per tile, wave 0: the tile's bucket comes from the wave-uniform cursor, its group from the
//   by-value byte table (scalar), and the eight values are read out of lane `group` with
//   v_readlane_b32 into scalar registers: the arithmetic takes them as scalar operands.  No LDS
//   table, so no hazard beyond the above.  A group index is < ngroups <= 8 (the host's check), so
//   the lane read always holds a loaded set.
// ---------------------------------------------------------------------------
template <int P, bool ZERO, bool GROUPS>
__device__ __forceinline__ void adamw_ag(const GroupSpan& span, const AdamwGroup& planes, const AdamwGroupOf& group_of,
                                         const allred_adamw_hyper* __restrict__ hyper, int ngroups,
                                         const float* __restrict__ norm_sq, float* info) {
    constexpr int TV = 32, RPI = 2, RPW = P / 4, OPS = RPW / RPI;
    static_assert(OPS >= 1, "P >= 8");
    __shared__ __attribute__((aligned(16))) uint2 slot[2][64];
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int c = lane % TV, q = lane / TV;
    struct Tile {
        uint16_t* ranks;   // the bucket's row 0
        uint64_t stride;
        uint64_t v0;       // the tile's first 16-byte vector inside a rank row
        uint64_t off;      // the tile's first float inside a plane
        uint32_t bucket;   // index within the LAUNCH
        uint32_t group;    // GROUPS: the bucket's parameter group
    };
    uint32_t cursor = 0;   // wave-uniform: it depends on blockIdx and j only
    // the group of bucket b of the launch: a scalar load from the kernel arguments, a shift, a mask
    auto group_at = [&](uint32_t b) {
        if constexpr (GROUPS) {
            const uint32_t word = group_of.w[(b >> 2) & (kAdamwGroupMax / 4 - 1)];
            return (uint32_t)__builtin_amdgcn_readfirstlane((int)((word >> (8 * (b & 3))) & 0xFF));
        } else {
            return 0u;
        }
    };
    // the group is looked up HERE, with the tile's other table reads and in front of its loads, not in
    // front of the arithmetic: its scalar load is then not behind the tile's landing (DESIGN.md §16:
    // no difference measured in the one-tile regime)
    auto locate = [&](int j) {
        const GroupTile gt = group_span_at(span, group_span_tile(span, blockIdx.x, (uint32_t)j), cursor);
        const GroupBucket& e = span.b[gt.bucket];
        return Tile{e.ranks, e.stride, (uint64_t)gt.local * TV,
                    (uint64_t)gt.block * planes.s[gt.bucket].stride + (uint64_t)gt.rem * (8 * TV), gt.bucket, group_at(gt.bucket)};
    };
    const int mine = (int)group_span_mine(span, blockIdx.x);
    if (mine <= 0) return;   // the whole workgroup: no barrier is left waiting
    const int last = mine - 1;
    auto rows = [&](const Tile& t, int j) {
        const uint4 v = reinterpret_cast<const uint4*>(&slot[j & 1][0])[c];
#pragma unroll
        for (int k = 0; k < OPS; ++k) {
            const uint32_t r = (uint32_t)(RPW * w + RPI * k + q);
            st_nt(reinterpret_cast<uint4*>(t.ranks + (uint64_t)r * t.stride) + t.v0 + c, v);
        }
    };
    struct Src {
        f32x4 p, g, m, v;
    };
    struct New {
        f32x4 p, m, v;
    };
    auto load = [&](const Tile& t) {
        const AdamwPlanes& s = planes.s[t.bucket];
        const uint64_t i = t.off + 4 * (uint32_t)lane;
        return Src{*reinterpret_cast<const f32x4*>(s.param + i), *reinterpret_cast<const f32x4*>(s.grad + i),
                   *reinterpret_cast<const f32x4*>(s.exp_avg + i), *reinterpret_cast<const f32x4*>(s.exp_avg_sq + i)};
    };
    // wave 0: the reads of hyper (GROUPS: lane g reads group g) and norm_sq go out first, the first
    // tile's loads behind them, and only then the uniform arithmetic, which waits for the former
    // under the latter's round trip
    CallWide u{0.0f, 1.0f, false};
    PerGroup lanes{};
    Tile cur = locate(0);
    Src xc{}, xn{};
    if (w == 0) {
        allred_adamw_hyper h;
        f32x4 h0{}, h1{};
        if constexpr (GROUPS) {
            // lanes >= ngroups read the LAST set again, never past the array: a clamped index, not a branch
            // (with `if (lane < ngroups)` around the loads the compiler waited for them inside the branch,
            // in front of every other load of the prologue)
            const f32x4* hp = reinterpret_cast<const f32x4*>(hyper + (lane < ngroups ? lane : ngroups - 1));
            h0 = hp[0];
            h1 = hp[1];
        } else {
            h = *hyper;   // a wave-uniform address: the compiler may go through the scalar cache, hyper is only read
        }
        float x = 0.0f;
        if (norm_sq && lane < P) x = norm_sq[lane];
        xc = load(cur);
        if constexpr (GROUPS) {
            // nothing moves across: without it the scheduler put the read of lane 0's max_norm, and with
            // it the wait for hyper, in front of the tile's fourth load
            __builtin_amdgcn_sched_barrier(0);
            h.lr = h0[0];
            h.beta1 = h0[1];
            h.beta2 = h0[2];
            h.eps = h0[3];
            h.weight_decay = h1[0];
            h.bias_corr1 = h1[1];
            h.bias_corr2_sqrt = h1[2];
            h.max_norm = h1[3];
            u = call_wide(from_lane(h.max_norm, 0), x, norm_sq != nullptr);
        } else {
            u = call_wide(h.max_norm, x, norm_sq != nullptr);
        }
        lanes = per_group(h);
        if (info && blockIdx.x == 0 && lane == 0)
            *reinterpret_cast<f32x4*>(info) = f32x4{u.N, u.c, u.skip ? 1.0f : 0.0f, 0.0f};
    }
    // a set's value for this tile: GROUPS, out of lane g; else the one there is
    auto pick = [&](float x, int g) {
        if constexpr (GROUPS) return from_lane(x, g);
        else return x;
    };
    // the update of allred.h on this lane's four elements with group g's values, and their bf16 into
    // the tile's LDS slot
    auto update = [&](const Src& x, int j, int g) {
        New y{x.p, x.m, x.v};
        if (!u.skip) {
            const float d = pick(lanes.d, g), o1 = pick(lanes.o1, g), o2 = pick(lanes.o2, g);
            const float ss = pick(lanes.ss, g), beta1 = pick(lanes.beta1, g), beta2 = pick(lanes.beta2, g);
            const float eps = pick(lanes.eps, g), bc2 = pick(lanes.bc2, g);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float g1 = x.g[e] * u.c;
                const float p1 = x.p[e] * d;
                y.m[e] = x.m[e] * beta1 + g1 * o1;
                y.v[e] = x.v[e] * beta2 + (g1 * g1) * o2;
                const float den = sqrtf(y.v[e]) / bc2 + eps;
                y.p[e] = p1 - ss * (y.m[e] / den);
            }
        }
        slot[j & 1][lane] = make_uint2(pack_rne(y.p[0], y.p[1]), pack_rne(y.p[2], y.p[3]));
        return y;
    };
    // the planes' stores, BEHIND the barrier: the other waves' row stores do not wait for them
    auto store = [&](const Tile& t, const New& y) {
        const AdamwPlanes& s = planes.s[t.bucket];
        const uint64_t i = t.off + 4 * (uint32_t)lane;
        if (!u.skip) {
            *reinterpret_cast<f32x4*>(s.param + i) = y.p;
            *reinterpret_cast<f32x4*>(s.exp_avg + i) = y.m;
            *reinterpret_cast<f32x4*>(s.exp_avg_sq + i) = y.v;
        }
        if constexpr (ZERO) *reinterpret_cast<f32x4*>(s.grad + i) = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    };
    // One tile.  NEXT: tile j + 1 exists — its loads go out before this tile's arithmetic.  The last
    // tile is peeled so that the loop's loads are unconditional: with `if (j < last)` around them the
    // compiler merged both paths and drained the next tile's loads in front of the arithmetic.
    auto tile = [&](int j, auto next) {
        constexpr bool NEXT = decltype(next)::value;
        Tile nxt = cur;
        if constexpr (NEXT) nxt = locate(j + 1);
        New y{};
        if (w == 0) {
            if constexpr (NEXT) xn = load(nxt);
            y = update(xc, j, (int)cur.group);
        }
        lds_barrier();   // wave 0's LDS write has landed (lgkmcnt(0)) before it arrives
        rows(cur, j);
        if (w == 0) store(cur, y);
        if constexpr (NEXT) {
            cur = nxt;
            xc = xn;
        }
    };
    for (int j = 0; j < last; ++j) tile(j, std::true_type{});
    tile(last, std::false_type{});
}

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
