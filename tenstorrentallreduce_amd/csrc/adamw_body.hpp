// adamw_body.hpp — the ONE AdamW body of the fp32-shard calls, adamw_ag, with its kernel-argument
// tables: included by adamw_kernels.hip (k_adamw_ag_group_f32, k_adamw_ag_groups_f32: bf16 rank rows)
// and adamw_mx_kernels.hip (k_adamw_ag_mxfp8: MXFP8 element rows and E8M0 scale rows).  The output
// stage — what wave 0 puts into the LDS slot for p' and what every wave stores from it — is a
// compile-time choice (AdamwOut); everything else is the same code in every instance.
#pragma once

#include <type_traits>

#include "device.hpp"
#include "group_span.hpp"
#include "mx_quant.hpp"

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

// The output stage of adamw_ag: what p' (p on a skipped step) becomes on its way to the rank rows.
//   kOutBf16     pack_rne: 8 bytes of bf16 per lane, a 512-byte slot, 16-byte row stores.
//   kOutMxFloor  MXFP8, the floor scale rule: 4 e4m3 bytes per lane and the tile's 8 E8M0 bytes, a
//   kOutMxRceil  272-byte slot, 8-byte row stores and one 8-byte scale store per rank row (RCEIL: the
//                rounded-up scale of allred.h).
enum AdamwOut { kOutBf16 = 0, kOutMxFloor, kOutMxRceil };
// The scale rows of every bucket of an MXFP8 launch: rank r's scale row at scales + r * scale_stride
// bytes.  GroupSpan then carries the ELEMENT rows in bytes (GroupBucket::ranks row 0, ::stride the
// row stride in bytes), as in mx_kernels.hip.  The bf16 kernels hand adamw_ag an AdamwNoScales.
struct AdamwMxScaleRows {   // 16 bytes
    uint8_t* scales;
    uint64_t scale_stride;  // bytes
};
struct AdamwMxScales {
    AdamwMxScaleRows s[kAdamwGroupMax];   // entries past the last bucket: zero
};
struct AdamwNoScales {};
static_assert(sizeof(AdamwMxScales) == 16 * kAdamwGroupMax, "the kernel-argument layout");
// the LDS slot of one tile: 64 lanes' 8 bytes of bf16, or 64 lanes' 4 element bytes, the tile's 8 scale
// bytes at byte 256 and 8 bytes of padding (272: a multiple of 16, so that both slots are 16-byte aligned)
template <AdamwOut OUT>
struct AdamwSlot {
    typedef uint2 type[2][64];
};
template <>
struct AdamwSlot<kOutMxFloor> {
    typedef uint32_t type[2][68];
};
template <>
struct AdamwSlot<kOutMxRceil> {
    typedef uint32_t type[2][68];
};

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
// OUT != kOutBf16 (MXFP8 rows; the bf16 forms hold none of this: if constexpr), allred.h's rule for
// allred_plan_all_gather_shards_mxfp8 applied to p' in wave 0's registers:
//   lane l holds floats 4 l .. 4 l + 3 of the tile, so an MX block — 32 consecutive floats — is EIGHT
//   aligned lanes (k_ag_group_mxfp8's is a quad: its lanes hold eight floats).  A: the integer max
//   of the lane's four abs bit patterns, then THREE DPP steps — quad_perm lane ^ 1, quad_perm lane ^
//   2, row_half_mirror (lane 7 - i of the eight, in the other quad, which holds that quad's max: the
//   control add_lanes32 uses the same way) — after which all eight lanes hold the block's A.
//   scale byte, 2^-X, one v_mul_f32, v_med3_f32 with +-448, v_cvt_pk_fp8_f32: as k_ag_group_mxfp8; one
//   dword of element bytes per lane, 0x7F7F7F7F and scale 0xFF for a block with a NaN or Inf.
//   slot (272 bytes): dword l = lane l's element bytes; bytes 256 .. 263 = the tile's eight scale
//   bytes, written by lanes 0, 8 .. 56 as BYTE writes (ds_write_b8 under one exec mask: no readlanes);
//   bytes 264 .. 271 padding, never read.  The slot rotation and its hazard argument are the above.
//   behind the barrier every wave reads column c's 8 bytes and stores them nontemporally to its rows
//   (row stride in BYTES), lanes < RPW read the 8 scale bytes and store them to scale row RPW w + lane
//   with a PLAIN store (mx_kernels.hip says why); wave 0's plane stores follow as before.
// ---------------------------------------------------------------------------
template <int P, bool ZERO, bool GROUPS, AdamwOut OUT = kOutBf16, class Scales = AdamwNoScales>
__device__ __forceinline__ void adamw_ag(const GroupSpan& span, const AdamwGroup& planes, const AdamwGroupOf& group_of,
                                         const allred_adamw_hyper* __restrict__ hyper, int ngroups,
                                         const float* __restrict__ norm_sq, float* info, const Scales& scale_rows = Scales{}) {
    constexpr int TV = 32, RPI = 2, RPW = P / 4, OPS = RPW / RPI;
    constexpr bool MX = OUT != kOutBf16;
    static_assert(OPS >= 1, "P >= 8");
    static_assert(std::is_same<Scales, AdamwMxScales>::value == MX, "the scale rows come with the MXFP8 output stage");
    __shared__ __attribute__((aligned(16))) typename AdamwSlot<OUT>::type slot;
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int c = lane % TV, q = lane / TV;
    struct Tile {
        uint16_t* ranks;   // the bucket's row 0
        uint64_t stride;
        uint64_t v0;       // the tile's first 16-byte vector inside a rank row (MX: its first 8-byte one; v0 / TV: the tile's index)
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
        if constexpr (MX) {
            const uint2 v = reinterpret_cast<const uint2*>(&slot[j & 1][0])[c];
            const uint2 sc = reinterpret_cast<const uint2*>(&slot[j & 1][64])[0];
            uint8_t* row0 = reinterpret_cast<uint8_t*>(t.ranks);
#pragma unroll
            for (int k = 0; k < OPS; ++k) {
                const uint32_t r = (uint32_t)(RPW * w + RPI * k + q);
                __builtin_nontemporal_store(u32x2{v.x, v.y}, reinterpret_cast<u32x2*>(row0 + (uint64_t)r * t.stride) + t.v0 + c);
            }
            // NOT nontemporal: 8 bytes of a line whose other fifteen sixteenths come from other workgroups
            const AdamwMxScaleRows& sr = scale_rows.s[t.bucket];
            if (lane < RPW)
                reinterpret_cast<u32x2*>(sr.scales + (uint64_t)(RPW * w + lane) * sr.scale_stride)[t.v0 / TV] = u32x2{sc.x, sc.y};
        } else {
            const uint4 v = reinterpret_cast<const uint4*>(&slot[j & 1][0])[c];
#pragma unroll
            for (int k = 0; k < OPS; ++k) {
                const uint32_t r = (uint32_t)(RPW * w + RPI * k + q);
                st_nt(reinterpret_cast<uint4*>(t.ranks + (uint64_t)r * t.stride) + t.v0 + c, v);
            }
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
        if constexpr (MX) {
            uint32_t A = umax(umax(abs_bits(y.p[0]), abs_bits(y.p[1])), umax(abs_bits(y.p[2]), abs_bits(y.p[3])));
            A = max_dpp<0xB1>(A);    // quad_perm [1, 0, 3, 2]: lane ^ 1
            A = max_dpp<0x4E>(A);    // quad_perm [2, 3, 0, 1]: lane ^ 2
            A = max_dpp<0x141>(A);   // row_half_mirror: a lane of the other quad of the 8
            const bool special = A >= 0x7f800000u;
            int sb = (int)(A >> 23) - 8;
            if constexpr (OUT == kOutMxRceil) sb += (A & 0x7fffffu) > 0x600000u ? 1 : 0;
            sb = sb > 0 ? sb : 0;
            const float inv = __uint_as_float((uint32_t)(254 - sb) << 23);
            uint32_t e = cvt2<false>(y.p[0] * inv, y.p[1] * inv, 0u);
            e = cvt2<true>(y.p[2] * inv, y.p[3] * inv, e);
            slot[j & 1][lane] = special ? 0x7f7f7f7fu : e;
            if ((lane & 7) == 0) reinterpret_cast<uint8_t*>(&slot[j & 1][64])[lane >> 3] = (uint8_t)(special ? 0xffu : (uint32_t)sb);
        } else {
            slot[j & 1][lane] = make_uint2(pack_rne(y.p[0], y.p[1]), pack_rne(y.p[2], y.p[3]));
        }
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

}  // namespace
}  // namespace tsa
