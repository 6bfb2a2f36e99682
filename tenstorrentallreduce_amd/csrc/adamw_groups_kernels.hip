// adamw_groups_kernels.hip — AdamW PARAMETER GROUPS inside the grouped all-gather launch
// (allred_plan_adamw_all_gather_shards_f32_groups, allred.h): adamw_kernels.hip's step with the
// hyperparameter set chosen per bucket, still one launch per ALLRED_ADAMW_GROUP_MAX buckets.
//
//   k_adamw_ag_groups_f32<P, ZERO>  k_adamw_ag_group_f32's walk, tile form and arithmetic; hyper is an
//                                   array of ngroups x 32 bytes, lane g of wave 0 holds group g's
//                                   eight uniform values, and every tile picks its bucket's group
//                                   out of those lanes with v_readlane_b32 (form chosen: DESIGN.md §16).
//
// A translation unit of its own, like adamw_kernels.hip: the older objects stay what they were
// (same code, same resources).  The arithmetic depends on the build's -ffp-contract=off (Makefile,
// HIPFLAGS) exactly as adamw_kernels.hip's does: every operation allred.h writes is ONE IEEE fp32
// operation, never an fma; `/` and sqrtf are hipcc's correctly rounded forms, denormals are kept —
// the tests compare bits, also against the one-group call.
#include <type_traits>

#include "device.hpp"
#include "group_span.hpp"
#include "launch_util.hpp"

namespace tsa {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kAdamwGroupMax = ALLRED_ADAMW_GROUP_MAX;            // buckets of one launch
constexpr int kParamGroupsMax = ALLRED_ADAMW_PARAM_GROUPS_MAX;    // hyperparameter sets of one call

// adamw_kernels.hip's plane table (file-local there, and that object is not to change): entry i for
// bucket i of the launch, block b of the bucket at plane + b * stride floats, ONE stride for the four.
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
static_assert(kAdamwGroupMax <= kGroupMax, "GroupSpan's table holds a launch");
static_assert(kParamGroupsMax <= 64, "a group per lane of wave 0 (and a group index fits its byte)");
static_assert(sizeof(allred_adamw_hyper) == 32 && sizeof(allred_adamw_bucket_f32) == 64, "allred.h's layouts");

// add_halves / add_lanes32 of shard_f32_kernels.hip and adamw_kernels.hip (file-local there): the
// balanced tree over 64 values in index order.
__device__ __forceinline__ float add_halves(float x) {
#if __has_builtin(__builtin_amdgcn_permlane32_swap)
    const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    return __uint_as_float(r[0]) + __uint_as_float(r[1]);
#else
    return x + __shfl_xor(x, 32);
#endif
}
template <int CTRL>
__device__ __forceinline__ float add_dpp(float x) {
    return x + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), CTRL, 0xF, 0xF, false));
}
__device__ __forceinline__ float add_lanes32(float t) {   // every lane of the wave must be active
    t = add_dpp<0xB1>(t);    // quad_perm [1, 0, 3, 2]: lane ^ 1
    t = add_dpp<0x4E>(t);    // quad_perm [2, 3, 0, 1]: lane ^ 2
    t = add_dpp<0x141>(t);   // row_half_mirror
    t = add_dpp<0x140>(t);   // row_mirror
    return t + __shfl_xor(t, 16);
}

// the value lane `g` of this wave holds in x, as a wave-uniform (scalar) value; g is wave-uniform
__device__ __forceinline__ float from_lane(float x, int g) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), g));
}

// The call-wide values (allred.h): the same in every lane and every launch.
struct CallWide {
    float N, c;
    bool skip;
};
// The per-group values, group g's in LANE g of wave 0 (lanes >= ngroups: a copy of the last group's, never picked).
struct PerGroup {
    float d, o1, o2, ss;
    float beta1, beta2, eps, bc2;
};

// Wave 0, all 64 lanes active.  max_norm0: hyper[0].max_norm, wave-uniform; x = norm_sq[lane]
// (lane < P, else +0.0f; given: norm_sq != NULL).  adamw_kernels.hip's uniforms(), operation for operation.
__device__ __forceinline__ CallWide call_wide(float max_norm0, float x, bool given) {
    CallWide u{0.0f, 1.0f, false};
    if (given) {
        u.N = add_halves(add_lanes32(x));
        u.skip = !(__builtin_fabsf(u.N) < __builtin_inff());   // NaN or +-Inf
        const float q = max_norm0 / (sqrtf(u.N) + 1e-6f);
        u.c = (q < 1.0f) ? q : 1.0f;
    }
    return u;
}
// this lane's group from this lane's 32 bytes of hyper: the same single fp32 operations as uniforms()
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
// k_adamw_ag_groups_f32<P, ZERO>: k_adamw_ag_group_f32 (adamw_kernels.hip) — the
// persistent GroupSpan walk, wave 0 alone touching the planes, two 512-byte LDS slots and one barrier
// per tile, the planes' stores behind the row stores, the next tile's four loads in front of this
// tile's arithmetic, the last tile peeled — with the hyperparameters chosen per bucket:
//   prologue, wave 0: lane g < ngroups loads hyper[g] (two 16-byte vector loads; lanes >= ngroups
//   load hyper[ngroups - 1] again: no lane reads past the array), every lane loads norm_sq[lane],
//   tile 0's four loads go out behind these and in front of the uniform arithmetic.  N, skip and c
//   are the call's: c from lane 0's
//   max_norm, the max_norm of the other groups is loaded and never used.  Lane g forms group g's d,
//   o1, o2, ss.
//   per tile, wave 0: the tile's bucket comes from the wave-uniform cursor, its group from the
//   by-value byte table (scalar), and the eight values are read out of lane `group` with
//   v_readlane_b32 into scalar registers: the arithmetic takes them as scalar operands.  No LDS
//   table, so no hazard beyond §15's.
// A group index is < ngroups <= 8 (the host's check), so the lane read always holds a loaded set.
// info: as k_adamw_ag_group_f32 — one 16-byte vector store by lane 0 of wave 0 of workgroup 0 of the
// call's first launch.
// ---------------------------------------------------------------------------
template <int P, bool ZERO>
__global__ __launch_bounds__(kBlock) void k_adamw_ag_groups_f32(GroupSpan span, AdamwGroup planes, AdamwGroupOf group_of,
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
        uint32_t group;    // the bucket's parameter group
    };
    uint32_t cursor = 0;   // wave-uniform: it depends on blockIdx and j only
    // the group of bucket b of the launch: a scalar load from the kernel arguments, a shift, a mask
    auto group_at = [&](uint32_t b) {
        const uint32_t word = group_of.w[(b >> 2) & (kAdamwGroupMax / 4 - 1)];
        return (uint32_t)__builtin_amdgcn_readfirstlane((int)((word >> (8 * (b & 3))) & 0xFF));
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
    // wave 0: the reads of hyper (lane g: group g) and norm_sq go out first, the first tile's loads
    // behind them, and only then the uniform arithmetic
    CallWide u{0.0f, 1.0f, false};
    PerGroup lanes{};
    Tile cur = locate(0);
    Src xc{}, xn{};
    if (w == 0) {
        // lanes >= ngroups read the LAST set again, never past the array: a clamped index, not a branch
        // (with `if (lane < ngroups)` around the loads the compiler waited for them inside the branch,
        // in front of every other load of the prologue)
        const f32x4* hp = reinterpret_cast<const f32x4*>(hyper + (lane < ngroups ? lane : ngroups - 1));
        const f32x4 h0 = hp[0], h1 = hp[1];
        float x = 0.0f;
        if (norm_sq && lane < P) x = norm_sq[lane];
        xc = load(cur);
        // nothing moves across: without it the scheduler put the read of lane 0's max_norm, and with
        // it the wait for hyper, in front of the tile's fourth load
        __builtin_amdgcn_sched_barrier(0);
        allred_adamw_hyper h;
        h.lr = h0[0];
        h.beta1 = h0[1];
        h.beta2 = h0[2];
        h.eps = h0[3];
        h.weight_decay = h1[0];
        h.bias_corr1 = h1[1];
        h.bias_corr2_sqrt = h1[2];
        h.max_norm = h1[3];
        u = call_wide(from_lane(h.max_norm, 0), x, norm_sq != nullptr);
        lanes = per_group(h);
        if (info && blockIdx.x == 0 && lane == 0)
            *reinterpret_cast<f32x4*>(info) = f32x4{u.N, u.c, u.skip ? 1.0f : 0.0f, 0.0f};
    }
    // the update of allred.h on this lane's four elements with group g's values, and their bf16 into
    // the tile's LDS slot
    auto update = [&](const Src& x, int j, int g) {
        New y{x.p, x.m, x.v};
        if (!u.skip) {
            const float d = from_lane(lanes.d, g), o1 = from_lane(lanes.o1, g), o2 = from_lane(lanes.o2, g);
            const float ss = from_lane(lanes.ss, g), beta1 = from_lane(lanes.beta1, g), beta2 = from_lane(lanes.beta2, g);
            const float eps = from_lane(lanes.eps, g), bc2 = from_lane(lanes.bc2, g);
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
    // One tile.  NEXT: tile j + 1 exists — its loads go out before this tile's arithmetic; the last
    // tile is peeled so that the loop's loads are unconditional.
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
// k_adamw_ag_group_f32's grid cap, inherited and unmeasured here as there (tune pipe_grid caps it lower)
constexpr uint64_t kAdamwGroupsGrid = kMaxGrid;

}  // namespace

// A (checked: engine.cpp, adamw_check and adamw_groups_ok) list of whole-tile buckets with their four
// fp32 planes and their parameter groups (group_of == nullptr: every bucket in group 0) through
// k_adamw_ag_groups_f32, ALLRED_ADAMW_GROUP_MAX buckets per launch in list order whatever the groups
// are, enqueued when its last member is reached; a launch's group table is indexed by the bucket's
// place in the LAUNCH.  info goes to the first launch alone: it is written once.
int launch_adamw_groups_f32(const allred_adamw_bucket_f32* buckets, const uint8_t* group_of, int count, int total,
                            const allred_adamw_hyper* hyper, int ngroups, const float* norm_sq, float* info, bool zero_grad,
                            void* stream) {
    hipStream_t st = (hipStream_t)stream;
    GroupIn in[kAdamwGroupMax];
    AdamwGroup planes{};
    AdamwGroupOf groups{};
    int pending = 0, launches = 0;
    uint64_t pending_tiles = 0;
    auto flush = [&]() -> int {
        if (!pending) return ALLRED_OK;
        ++launches;
        const int members = pending;
        const uint64_t tiles = pending_tiles;
        pending = 0;
        pending_tiles = 0;
        const unsigned grid = persistent_grid(tiles, kAdamwGroupsGrid);
        GroupSpan span;
        if (!group_span_make(&span, in, members, grid)) return ALLRED_ERR_ARG;
        float* out = launches == 1 ? info : nullptr;
        const bool found = for_ranks<8, 64>(total, [&](auto p) {
            if (zero_grad)
                hipLaunchKernelGGL((k_adamw_ag_groups_f32<p(), true>), dim3(grid), dim3(kBlock), 0, st, span, planes, groups, hyper,
                                   ngroups, norm_sq, out);
            else
                hipLaunchKernelGGL((k_adamw_ag_groups_f32<p(), false>), dim3(grid), dim3(kBlock), 0, st, span, planes, groups, hyper,
                                   ngroups, norm_sq, out);
            trace_launch(grid, kBlock, "k_adamw_ag_groups_f32<%d, %s>", total, tf(zero_grad));
        });
        planes = AdamwGroup{};
        groups = AdamwGroupOf{};
        return found ? last_error() : ALLRED_ERR_UNSUPPORTED;
    };
    if (ngroups < 1 || ngroups > kParamGroupsMax) return ALLRED_ERR_ARG;   // the caller's check, kept next to its use
    for (int i = 0; i < count; ++i) {
        const allred_adamw_bucket_f32& b = buckets[i];
        const uint64_t nv = b.elems_per_rank / 8, bv = nv / total, tiles = nv / 32;
        const uint32_t g = group_of ? group_of[i] : 0u;
        if (total < 8 || nv % 32 || bv % 32) return ALLRED_ERR_UNSUPPORTED;   // the caller's checks, kept next to their use
        if (g >= (uint32_t)ngroups) return ALLRED_ERR_ARG;
        planes.s[pending] = AdamwPlanes{b.param, b.grad, b.exp_avg, b.exp_avg_sq, b.shard_stride};
        groups.w[pending >> 2] |= g << (8 * (pending & 3));
        in[pending++] = GroupIn{b.ranks, b.rank_stride, tiles, bv / 32};
        pending_tiles += tiles;
        if (pending == kAdamwGroupMax) {
            const int s = flush();
            if (s != ALLRED_OK) return s;
        }
    }
    return flush();
}

}  // namespace tsa
