// mx4_sr_kernels.hip — the MXFP4 all-gather from fp32 shards with STOCHASTIC ROUNDING onto the e2m1 grid, with
// or without the random Hadamard rotation in front (allred_plan_all_gather_shards_mxfp4_sr, allred.h): the
// unbiased operand of the backward GEMM, written where the all-gather holds every fp32 master value in a
// register and writes ONE quantisation to all P rank rows — every rank gets the same bits with no RNG to keep
// in step between ranks and no pass over every rank's copy.
//
//   k_ag_group_mxfp4_sr<P, RCEIL, RHT>   k_ag_group_mxfp4's walk and store split (mx4_kernels.hip), the
//                                        rotation of mx_rht.hpp where RHT, and mx_sr.hpp's rounding in place of
//                                        v_cvt_scalef32_pk_fp4_f32; a tile's random words are generated while
//                                        its loads are in flight.
//
// The rule is allred.h's, integer for integer; the tests compare whole buffers.
#include "device.hpp"
#include "group_batch.hpp"
#include "group_span.hpp"
#include "launch_util.hpp"
#include "mx_quant.hpp"
#include "mx_rht.hpp"
#include "mx_sr.hpp"

namespace tsa {
namespace {

constexpr int kMxSrGroupMax = ALLRED_MX_GROUP_MAX;   // buckets of one launch: the MXFP4 call's

// k_ag_group_mxfp4's two tables, the state's address, the sign mask and the launch's first bucket
static_assert(sizeof(GroupSpan) + sizeof(MxShards) + 16 < 4096, "kernel arguments stay below 4 KiB");
static_assert(kMxSrGroupMax <= kGroupMax, "GroupSpan's table holds a launch");

// ---------------------------------------------------------------------------
// k_ag_group_mxfp4_sr<P, RCEIL, RHT>: k_ag_group_mxfp4 line for line — the persistent grid, the forward-only
// wave-uniform cursor, unconditional next-tile loads, two tiles per trip with registers of their own, tile 0
// peeled, W = min(4, P / 4) storing waves, four rows per store instruction, the plain scale store, no LDS and
// no barrier — with two differences.
//   THE WORDS.  Lane c = lane % 16 holds floats 16 c .. 16 c + 15 of a tile, elements 256 local + 16 c .. of
//   the gathered row: four Philox calls with counters g .. g + 3, g = 64 local + 4 c — g's high word, the
//   bucket, the step and the key are wave-uniform.  They depend on the tile's INDEX alone, so words(t) runs
//   between the issue of the NEXT tile's loads and the wait for tile t's own: about 330 integer operations
//   under the memory latency, not behind it (where the rotation's 130 stand: there they need the data).  Two
//   sched_barriers hold that place: one behind the loads' issue, one — store()'s — in front of the first use
//   of the loaded floats.  Sixteen words are live across the wait.
//   THE ROUNDING.  Behind A, the scale byte and 2^-X, which are k_ag_group_mxfp4's (on the rotated registers
//   where RHT, as in k_ag_group_mxfp4_rht), sr4_fp4 in place of cvt8_fp4: no clamp — the rule saturates.
// The memory operations and their vmcnt argument are k_ag_group_mxfp4's unchanged.
// ---------------------------------------------------------------------------
template <int P, bool RCEIL, bool RHT>
__global__ __launch_bounds__(kBlock) void k_ag_group_mxfp4_sr(GroupSpan span, MxShards shards,
                                                              const allred_mx_sr_state* __restrict__ sr, uint32_t sign_mask,
                                                              uint32_t first_bucket) {
    constexpr int TV = 16, RPI = 4, W = P / RPI < 4 ? P / RPI : 4, RPW = P / W, OPS = RPW / RPI;
    static_assert(P % RPI == 0 && W >= 1 && RPW * W == P && OPS * RPI == RPW, "whole store instructions per wave");
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (w >= W) return;   // wave-uniform; P = 8 only
    const int c = lane % TV, q = lane / TV;
    const SrCall call = sr_call(sr);
    RhtLane<16> rl;
    if constexpr (RHT) rl = rht_lane<16>(sign_mask, c & 1);
    struct Tile {
        uint8_t* rows;          // the bucket's element row 0
        uint64_t row_stride;    // bytes
        uint8_t* scales;        // the bucket's scale row 0
        uint64_t scale_stride;  // bytes
        uint64_t local;         // the tile's index inside a rank row: 128 element bytes, 8 scale bytes each
        const f32x4* src;       // the source tile's first 16 bytes
        uint32_t bucket;        // index in the CALLER's list
    };
    uint32_t cursor = 0;   // wave-uniform: it depends on blockIdx and j only
    auto locate = [&](int j) {
        const GroupTile gt = group_span_at(span, group_span_tile(span, blockIdx.x, (uint32_t)j), cursor);
        const GroupBucket& e = span.b[gt.bucket];
        const MxShard& sh = shards.s[gt.bucket];
        return Tile{reinterpret_cast<uint8_t*>(e.ranks), e.stride, sh.scales, sh.scale_stride, (uint64_t)gt.local,
                    reinterpret_cast<const f32x4*>(sh.shard + (uint64_t)gt.block * sh.stride) + (uint64_t)gt.rem * (4 * TV),
                    first_bucket + gt.bucket};
    };
    const int mine = (int)group_span_mine(span, blockIdx.x);
    if (mine <= 0) return;
    const int last = mine - 1;
    struct Src {
        f32x4 a, b, c, d;
    };
    struct Rnd {
        SrWords a, b, c, d;
    };
    auto load = [&](const Tile& t) {
        const Src s{t.src[4 * c], t.src[4 * c + 1], t.src[4 * c + 2], t.src[4 * c + 3]};
        __builtin_amdgcn_sched_barrier(0);   // the loads are out before any of the words below is computed
        return s;
    };
    // g = e / 4 of the lane's first element: 64 local + 4 c; 64 local's low six bits are zero, so the low word
    // takes 4 c + k without a carry and the high word is wave-uniform
    auto words = [&](const Tile& t) {
        const uint32_t g_lo = ((uint32_t)t.local << 6) + 4 * (uint32_t)c, g_hi = (uint32_t)(t.local >> 26);
        return Rnd{sr_words(call, g_lo, g_hi, t.bucket), sr_words(call, g_lo + 1, g_hi, t.bucket),
                   sr_words(call, g_lo + 2, g_hi, t.bucket), sr_words(call, g_lo + 3, g_hi, t.bucket)};
    };
    auto store = [&](const Tile& t, const Src& s, const Rnd& rnd) {
        // as in k_ag_group_mxfp4: the wait stands in front of the first use of the loaded floats — and behind
        // the words, which stand above this line
        __builtin_amdgcn_sched_barrier(0);
        f32x4 ra = s.a, rb = s.b, rc = s.c, rd = s.d;
        if constexpr (RHT) {
            float x[16];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                x[e] = s.a[e];
                x[4 + e] = s.b[e];
                x[8 + e] = s.c[e];
                x[12 + e] = s.d[e];
            }
            rht_own(x, rl);
#pragma unroll
            for (int e = 0; e < 16; ++e) x[e] = rht_norm(rht_pair(dpp_f<0xB1>(x[e]), x[e], rl.upper[0]));   // quad_perm [1, 0, 3, 2]: lane ^ 1
            ra = f32x4{x[0], x[1], x[2], x[3]};
            rb = f32x4{x[4], x[5], x[6], x[7]};
            rc = f32x4{x[8], x[9], x[10], x[11]};
            rd = f32x4{x[12], x[13], x[14], x[15]};
        }
        uint32_t A = umax(umax(amax4(ra), amax4(rb)), umax(amax4(rc), amax4(rd)));
        A = max_dpp<0xB1>(A);   // quad_perm [1, 0, 3, 2]: lane ^ 1
        const bool special = A >= 0x7f800000u;
        int sb = (int)(A >> 23) - 2;
        if constexpr (RCEIL) sb += (A & 0x7fffffu) > 0x400000u ? 1 : 0;
        sb = sb > 0 ? sb : 0;
        const float inv = __uint_as_float((uint32_t)(254 - sb) << 23);
        const uint32_t lo = sr4_fp4(ra, inv, rnd.a) | sr4_fp4(rb, inv, rnd.b) << 16;
        const uint32_t hi = sr4_fp4(rc, inv, rnd.c) | sr4_fp4(rd, inv, rnd.d) << 16;
        const u32x2 v = {special ? 0u : lo, special ? 0u : hi};
        const uint32_t sc8 = special ? 0xffu : (uint32_t)sb;
        const u32x2 sc = {lane_of(sc8, 0) | lane_of(sc8, 2) << 8 | lane_of(sc8, 4) << 16 | lane_of(sc8, 6) << 24,
                          lane_of(sc8, 8) | lane_of(sc8, 10) << 8 | lane_of(sc8, 12) << 16 | lane_of(sc8, 14) << 24};
#pragma unroll
        for (int k = 0; k < OPS; ++k) {
            const uint32_t r = (uint32_t)(RPW * w + RPI * k + q);
            __builtin_nontemporal_store(v, reinterpret_cast<u32x2*>(t.rows + (uint64_t)r * t.row_stride + t.local * 128) + c);
        }
        // NOT nontemporal: mx_kernels.hip's finding for the same 8 bytes
        if (lane < RPW) reinterpret_cast<u32x2*>(t.scales + (uint64_t)(RPW * w + lane) * t.scale_stride)[t.local] = sc;
    };
    // the "next" tile's loads are unconditional: a workgroup's last tile is loaded once more (an L2 hit)
    auto at = [&](int j) { return locate(j < last ? j : last); };
    Tile a = locate(0);
    Src xa = load(a);
    Tile b = at(1);
    Src xb = load(b);
    store(a, xa, words(a));
    // the odd tile behind the pairs is stored after the loop, not by a break out of its middle (k_ag_group_f32)
    int j = 1;
    for (; j + 1 < mine; j += 2) {
        a = at(j + 1);
        xa = load(a);
        store(b, xb, words(b));   // tile j
        b = at(j + 2);
        xb = load(b);
        store(a, xa, words(a));   // tile j + 1
    }
    if (j < mine) store(b, xb, words(b));
}
// k_ag_group_mxfp4's grid cap, inherited and unmeasured here (tune pipe_grid caps it lower)
constexpr uint64_t kAgGroupMx4SrGrid = kMaxGrid;

}  // namespace

// A (checked: engine.cpp mx_check with the MXFP4 payload, then sr's own rules) list of whole-tile buckets
// through k_ag_group_mxfp4_sr: launch_ag_group_mxfp4's batching — ALLRED_MX_GROUP_MAX buckets per launch in list
// order —, so the launch count of a list is that call's.  Every bucket is a member, so launch `index` begins at
// bucket index * ALLRED_MX_GROUP_MAX of the caller's list: the counter's third word does not depend on the batching.
int launch_ag_group_mxfp4_sr(const allred_mx_bucket_f32* buckets, int count, int total, bool rceil, bool rotate,
                             uint32_t sign_mask, const allred_mx_sr_state* sr, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    MxShards shards{};
    auto add = [&](int i, int slot) {
        const allred_mx_bucket_f32& b = buckets[i];
        const uint64_t tiles = b.elems_per_rank / 256;
        if (total < 8 || b.elems_per_rank % (256 * (uint64_t)total)) return BatchAdd::error(ALLRED_ERR_UNSUPPORTED);   // the caller's check, kept next to its use
        shards.s[slot] = MxShard{b.shard, b.shard_stride, b.scales, b.scale_stride};
        return BatchAdd::member(GroupIn{reinterpret_cast<uint16_t*>(b.rows), b.row_stride, tiles, tiles / total});
    };
    auto launch = [&](const GroupSpan& span, unsigned grid, int index, uint64_t) {
        const uint32_t first = (uint32_t)index * kMxSrGroupMax;
        const bool found = for_ranks<8, 64>(total, [&](auto p) {
            auto go = [&](auto rc, auto rot) {
                hipLaunchKernelGGL((k_ag_group_mxfp4_sr<p(), decltype(rc)::value, decltype(rot)::value>), dim3(grid), dim3(kBlock), 0, st,
                                   span, shards, sr, sign_mask, first);
                trace_launch(grid, kBlock, "k_ag_group_mxfp4_sr<%d, %s, %s>", total, tf(rceil), tf(rotate));
            };
            if (rceil) {
                if (rotate) go(std::true_type{}, std::true_type{});
                else go(std::true_type{}, std::false_type{});
            } else {
                if (rotate) go(std::false_type{}, std::true_type{});
                else go(std::false_type{}, std::false_type{});
            }
        });
        return found ? last_error() : ALLRED_ERR_UNSUPPORTED;
    };
    return group_batch<kMxSrGroupMax>(count, /*dry=*/false, shards, add,
                                      [](uint64_t tiles) { return persistent_grid(tiles, kAgGroupMx4SrGrid); }, launch);
}

}  // namespace tsa
