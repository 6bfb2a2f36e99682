// adamw_kernels.hip — AdamW on the fp32 shards inside the grouped all-gather launch
// (allred_plan_adamw_all_gather_shards_f32, allred.h): the optimizer step of a sharded training
// step at the one point where every master parameter is in a register anyway.
//
//   k_adamw_ag_group_f32<P, ZERO>   k_ag_group_f32's walk; a tile's 256 floats of the parameter,
//                                   gradient and the two moment planes loaded ONCE, the clipped
//                                   AdamW update of allred.h applied, p' m' v' stored back, p'
//                                   rounded once to bf16 (pack_rne) and written to every rank row.
//                                   ZERO: +0.0f stored over every gradient element read.
//
// A translation unit of its own, like shard_f32_kernels.hip: the older objects stay what they were
// (same code, same resources).  The arithmetic depends on the build's -ffp-contract=off (Makefile,
// HIPFLAGS): every operation allred.h writes is ONE IEEE fp32 operation, never an fma; `/` and
// sqrtf are hipcc's correctly rounded forms (v_div_scale / v_div_fmas / v_div_fixup, v_sqrt_f32
// with its refinement), denormals are kept — the tests compare bits.
#include <type_traits>

#include "device.hpp"
#include "group_span.hpp"
#include "launch_util.hpp"

namespace tsa {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kAdamwGroupMax = ALLRED_ADAMW_GROUP_MAX;   // buckets of one launch

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
static_assert(sizeof(AdamwPlanes) == 40 && sizeof(AdamwGroup) == 40 * kAdamwGroupMax, "the kernel-argument layout");
static_assert(sizeof(GroupSpan) + sizeof(AdamwGroup) + 3 * 8 < 4096, "kernel arguments stay below 4 KiB");
static_assert(kAdamwGroupMax <= kGroupMax, "GroupSpan's table holds a launch");
static_assert(sizeof(allred_adamw_hyper) == 32 && sizeof(allred_adamw_bucket_f32) == 64, "allred.h's layouts");

// add_halves / add_lanes32 of shard_f32_kernels.hip (file-local there, and that object is not to
// change): five levels of the balanced tree over the 32 lanes of a wave half, in lane order, then
// the level across the halves — together the balanced tree over 64 values in index order.
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

// the uniform values of a call (allred.h): the same in every lane and every launch
struct Uniforms {
    float N, c, d, o1, o2, ss;
    float beta1, beta2, eps, bc2;
    bool skip;
};

// Wave 0, all 64 lanes active: the uniform values from hyper's 32 bytes (h: loaded from a wave-uniform
// address — the compiler may go through the scalar cache, hyper is only read) and this lane's
// x = norm_sq[lane] (lane < P, else +0.0f; given: norm_sq != NULL).
__device__ __forceinline__ Uniforms uniforms(const allred_adamw_hyper& h, float x, bool given) {
    Uniforms u;
    u.N = 0.0f;
    u.c = 1.0f;
    u.skip = false;
    if (given) {
        u.N = add_halves(add_lanes32(x));
        u.skip = !(__builtin_fabsf(u.N) < __builtin_inff());   // NaN or +-Inf
        const float q = h.max_norm / (sqrtf(u.N) + 1e-6f);
        u.c = (q < 1.0f) ? q : 1.0f;
    }
    u.d = 1.0f - h.lr * h.weight_decay;
    u.o1 = 1.0f - h.beta1;
    u.o2 = 1.0f - h.beta2;
    u.ss = h.lr / h.bias_corr1;
    u.beta1 = h.beta1;
    u.beta2 = h.beta2;
    u.eps = h.eps;
    u.bc2 = h.bias_corr2_sqrt;
    return u;
}

// ---------------------------------------------------------------------------
// k_adamw_ag_group_f32<P, ZERO>: k_ag_group_f32's walk — persistent grid, workgroup g takes tiles
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
// ---------------------------------------------------------------------------
template <int P, bool ZERO>
__global__ __launch_bounds__(kBlock) void k_adamw_ag_group_f32(GroupSpan span, AdamwGroup planes,
                                                               const allred_adamw_hyper* __restrict__ hyper,
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
        uint32_t bucket;
    };
    uint32_t cursor = 0;   // wave-uniform: it depends on blockIdx and j only
    auto locate = [&](int j) {
        const GroupTile gt = group_span_at(span, group_span_tile(span, blockIdx.x, (uint32_t)j), cursor);
        const GroupBucket& e = span.b[gt.bucket];
        return Tile{e.ranks, e.stride, (uint64_t)gt.local * TV,
                    (uint64_t)gt.block * planes.s[gt.bucket].stride + (uint64_t)gt.rem * (8 * TV), gt.bucket};
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
    // wave 0: the reads of hyper and norm_sq go out first, the first tile's loads behind them, and
    // only then the uniform arithmetic, which waits for the former under the latter's round trip
    Uniforms u{};
    Tile cur = locate(0);
    Src xc{}, xn{};
    if (w == 0) {
        const allred_adamw_hyper h = *hyper;
        float x = 0.0f;
        if (norm_sq && lane < P) x = norm_sq[lane];
        xc = load(cur);
        u = uniforms(h, x, norm_sq != nullptr);
        if (info && blockIdx.x == 0 && lane == 0)
            *reinterpret_cast<f32x4*>(info) = f32x4{u.N, u.c, u.skip ? 1.0f : 0.0f, 0.0f};
    }
    // the update of allred.h on this lane's four elements, and their bf16 into the tile's LDS slot
    auto update = [&](const Src& x, int j) {
        New y{x.p, x.m, x.v};
        if (!u.skip) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float g1 = x.g[e] * u.c;
                const float p1 = x.p[e] * u.d;
                y.m[e] = x.m[e] * u.beta1 + g1 * u.o1;
                y.v[e] = x.v[e] * u.beta2 + (g1 * g1) * u.o2;
                const float den = sqrtf(y.v[e]) / u.bc2 + u.eps;
                y.p[e] = p1 - u.ss * (y.m[e] / den);
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
            y = update(xc, j);
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
// k_ag_group_f32's resident cap kAgGroupGrid, inherited: the cap is unmeasured for this kernel
// (tune pipe_grid caps it lower)
constexpr uint64_t kAdamwGrid = kMaxGrid;

}  // namespace

// A (checked: engine.cpp adamw_check) list of whole-tile buckets with their four fp32 planes through
// k_adamw_ag_group_f32, ALLRED_ADAMW_GROUP_MAX buckets per launch, enqueued when its last member is
// reached.  info goes to the first launch alone: it is written once.  dry: nothing is launched and
// the number of launches is returned.
int launch_adamw_group_f32(const allred_adamw_bucket_f32* buckets, int count, int total, const allred_adamw_hyper* hyper,
                           const float* norm_sq, float* info, bool zero_grad, bool dry, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    GroupIn in[kAdamwGroupMax];
    AdamwGroup planes{};
    int pending = 0, launches = 0;
    uint64_t pending_tiles = 0;
    auto flush = [&]() -> int {
        if (!pending) return ALLRED_OK;
        ++launches;
        const int members = pending;
        const uint64_t tiles = pending_tiles;
        pending = 0;
        pending_tiles = 0;
        if (dry) return ALLRED_OK;
        const unsigned grid = persistent_grid(tiles, kAdamwGrid);
        GroupSpan span;
        if (!group_span_make(&span, in, members, grid)) return ALLRED_ERR_ARG;
        float* out = launches == 1 ? info : nullptr;
        const bool found = for_ranks<8, 64>(total, [&](auto p) {
            if (zero_grad)
                hipLaunchKernelGGL((k_adamw_ag_group_f32<p(), true>), dim3(grid), dim3(kBlock), 0, st, span, planes, hyper, norm_sq, out);
            else
                hipLaunchKernelGGL((k_adamw_ag_group_f32<p(), false>), dim3(grid), dim3(kBlock), 0, st, span, planes, hyper, norm_sq, out);
            trace_launch(grid, kBlock, "k_adamw_ag_group_f32<%d, %s>", total, tf(zero_grad));
        });
        planes = AdamwGroup{};
        return found ? last_error() : ALLRED_ERR_UNSUPPORTED;
    };
    for (int i = 0; i < count; ++i) {
        const allred_adamw_bucket_f32& b = buckets[i];
        const uint64_t nv = b.elems_per_rank / 8, bv = nv / total, tiles = nv / 32;
        if (total < 8 || nv % 32 || bv % 32) return ALLRED_ERR_UNSUPPORTED;   // the caller's check, kept next to its use
        planes.s[pending] = AdamwPlanes{b.param, b.grad, b.exp_avg, b.exp_avg_sq, b.shard_stride};
        in[pending++] = GroupIn{b.ranks, b.rank_stride, tiles, bv / 32};
        pending_tiles += tiles;
        if (pending == kAdamwGroupMax) {
            const int s = flush();
            if (s != ALLRED_OK) return s;
        }
    }
    const int s = flush();
    if (s != ALLRED_OK) return s;
    return dry ? launches : ALLRED_OK;
}

}  // namespace tsa
