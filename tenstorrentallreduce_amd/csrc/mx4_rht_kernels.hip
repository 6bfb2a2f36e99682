// mx4_rht_kernels.hip — the MXFP4 all-gather from fp32 shards with a random Hadamard rotation of every MX
// block in front of the quantiser (allred_plan_all_gather_shards_mxfp4_rht, allred.h): the operand the
// published MXFP4 training recipes feed the GEMM, written where the all-gather holds every fp32 master value
// in a register anyway — no rotation pass over the masters before the call, none over every rank's copy after.
//
//   k_ag_group_mxfp4_rht<P, RCEIL>   k_ag_group_mxfp4's walk and store split (mx4_kernels.hip) with the
//                                    rotation of mx_rht.hpp between the loads and the amax.
//
// Every fp32 operation and its order are allred.h's; the tests compare whole buffers.
#include "device.hpp"
#include "group_batch.hpp"
#include "group_span.hpp"
#include "launch_util.hpp"
#include "mx_quant.hpp"
#include "mx_rht.hpp"

namespace tsa {
namespace {

constexpr int kMxRhtGroupMax = ALLRED_MX_GROUP_MAX;   // buckets of one launch: the MXFP4 call's

// k_ag_group_mxfp4's two tables and the sign mask (padded to 8 bytes)
static_assert(sizeof(GroupSpan) + sizeof(MxShards) + 8 < 4096, "kernel arguments stay below 4 KiB");
static_assert(kMxRhtGroupMax <= kGroupMax, "GroupSpan's table holds a launch");

// ---------------------------------------------------------------------------
// k_ag_group_mxfp4_rht<P, RCEIL>: k_ag_group_mxfp4 line for line — the persistent grid, the forward-only
// wave-uniform cursor, unconditional next-tile loads, two tiles per trip with registers of their own, tile 0
// peeled, W = min(4, P / 4) storing waves, four rows per store instruction, the plain scale store, no LDS and
// no barrier — except between the loads' landing and the amax:
//   lane c = lane % 16 holds floats 16 c .. 16 c + 15, so an MX block is the lane pair (c, c ^ 1): the even
//   lane holds x[0 .. 15], the odd lane x[16 .. 31].
//   signs   sixteen v_xor_b32 with the lane's masks — bit e of sign_mask >> 16 (c & 1) at bit 31 —, which are
//           the same for every tile: sixteen registers filled in front of the first load.
//   h = 1, 2, 4, 8   sixty-four v_add_f32 / v_sub_f32 on the lane's own sixteen registers.
//   h = 16  per register ONE v_add_f32 whose first operand is the partner's register through DPP quad_perm
//           [1, 0, 3, 2] and whose second is own, with its sign flipped in the odd lane (one v_xor_b32 with a
//           lane mask): own + partner in the even lane, partner - own in the odd one.
//   2^-2.5  sixteen v_mul_f32.
// Behind it A, the scale byte, 2^-X and cvt8_fp4 are k_ag_group_mxfp4's on the rotated registers; a block whose
// rotated values hold a NaN or an Inf — one that overflowed in the butterfly included — has A >= 0x7f800000.
// About 130 more VALU operations per lane and tile; the memory operations and their vmcnt argument are
// k_ag_group_mxfp4's unchanged (the rotation stands behind the same sched_barrier as the amax).
// ---------------------------------------------------------------------------
template <int P, bool RCEIL>
__global__ __launch_bounds__(kBlock) void k_ag_group_mxfp4_rht(GroupSpan span, MxShards shards, uint32_t sign_mask) {
    constexpr int TV = 16, RPI = 4, W = P / RPI < 4 ? P / RPI : 4, RPW = P / W, OPS = RPW / RPI;
    static_assert(P % RPI == 0 && W >= 1 && RPW * W == P && OPS * RPI == RPW, "whole store instructions per wave");
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (w >= W) return;   // wave-uniform; P = 8 only
    const int c = lane % TV, q = lane / TV;
    const RhtLane<16> rl = rht_lane<16>(sign_mask, c & 1);
    struct Tile {
        uint8_t* rows;          // the bucket's element row 0
        uint64_t row_stride;    // bytes
        uint8_t* scales;        // the bucket's scale row 0
        uint64_t scale_stride;  // bytes
        uint64_t local;         // the tile's index inside a rank row: 128 element bytes, 8 scale bytes each
        const f32x4* src;       // the source tile's first 16 bytes
    };
    uint32_t cursor = 0;   // wave-uniform: it depends on blockIdx and j only
    auto locate = [&](int j) {
        const GroupTile gt = group_span_at(span, group_span_tile(span, blockIdx.x, (uint32_t)j), cursor);
        const GroupBucket& e = span.b[gt.bucket];
        const MxShard& sh = shards.s[gt.bucket];
        return Tile{reinterpret_cast<uint8_t*>(e.ranks), e.stride, sh.scales, sh.scale_stride, (uint64_t)gt.local,
                    reinterpret_cast<const f32x4*>(sh.shard + (uint64_t)gt.block * sh.stride) + (uint64_t)gt.rem * (4 * TV)};
    };
    const int mine = (int)group_span_mine(span, blockIdx.x);
    if (mine <= 0) return;
    const int last = mine - 1;
    struct Src {
        f32x4 a, b, c, d;
    };
    auto load = [&](const Tile& t) { return Src{t.src[4 * c], t.src[4 * c + 1], t.src[4 * c + 2], t.src[4 * c + 3]}; };
    auto store = [&](const Tile& t, const Src& s) {
        // as in k_ag_group_mxfp4: the wait stands in front of the first use of the loaded floats
        __builtin_amdgcn_sched_barrier(0);
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
        const f32x4 ra = {x[0], x[1], x[2], x[3]}, rb = {x[4], x[5], x[6], x[7]};
        const f32x4 rc = {x[8], x[9], x[10], x[11]}, rd = {x[12], x[13], x[14], x[15]};
        uint32_t A = umax(umax(amax4(ra), amax4(rb)), umax(amax4(rc), amax4(rd)));
        A = max_dpp<0xB1>(A);   // quad_perm [1, 0, 3, 2]: lane ^ 1
        const bool special = A >= 0x7f800000u;
        int sb = (int)(A >> 23) - 2;
        if constexpr (RCEIL) sb += (A & 0x7fffffu) > 0x400000u ? 1 : 0;
        sb = sb > 0 ? sb : 0;
        const float inv = __uint_as_float((uint32_t)(254 - sb) << 23);
        const uint32_t lo = cvt8_fp4(ra, rb, inv), hi = cvt8_fp4(rc, rd, inv);
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
    store(a, xa);
    // the odd tile behind the pairs is stored after the loop, not by a break out of its middle (k_ag_group_f32)
    int j = 1;
    for (; j + 1 < mine; j += 2) {
        a = at(j + 1);
        xa = load(a);
        store(b, xb);   // tile j
        b = at(j + 2);
        xb = load(b);
        store(a, xa);   // tile j + 1
    }
    if (j < mine) store(b, xb);
}
// k_ag_group_mxfp4's grid cap, inherited and unmeasured here (tune pipe_grid caps it lower)
constexpr uint64_t kAgGroupMx4RhtGrid = kMaxGrid;

}  // namespace

// A (checked: engine.cpp mx_check with the MXFP4 payload) list of whole-tile buckets through
// k_ag_group_mxfp4_rht: launch_ag_group_mxfp4's batching — ALLRED_MX_GROUP_MAX buckets per launch in list
// order —, so the launch count of a list is that call's; sign_mask goes to every launch.
int launch_ag_group_mxfp4_rht(const allred_mx_bucket_f32* buckets, int count, int total, bool rceil, uint32_t sign_mask, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    MxShards shards{};
    auto add = [&](int i, int slot) {
        const allred_mx_bucket_f32& b = buckets[i];
        const uint64_t tiles = b.elems_per_rank / 256;
        if (total < 8 || b.elems_per_rank % (256 * (uint64_t)total)) return BatchAdd::error(ALLRED_ERR_UNSUPPORTED);   // the caller's check, kept next to its use
        shards.s[slot] = MxShard{b.shard, b.shard_stride, b.scales, b.scale_stride};
        return BatchAdd::member(GroupIn{reinterpret_cast<uint16_t*>(b.rows), b.row_stride, tiles, tiles / total});
    };
    auto launch = [&](const GroupSpan& span, unsigned grid, int, uint64_t) {
        const bool found = for_ranks<8, 64>(total, [&](auto p) {
            if (rceil) hipLaunchKernelGGL((k_ag_group_mxfp4_rht<p(), true>), dim3(grid), dim3(kBlock), 0, st, span, shards, sign_mask);
            else hipLaunchKernelGGL((k_ag_group_mxfp4_rht<p(), false>), dim3(grid), dim3(kBlock), 0, st, span, shards, sign_mask);
            trace_launch(grid, kBlock, "k_ag_group_mxfp4_rht<%d, %s>", total, tf(rceil));
        });
        return found ? last_error() : ALLRED_ERR_UNSUPPORTED;
    };
    return group_batch<kMxRhtGroupMax>(count, /*dry=*/false, shards, add,
                                       [](uint64_t tiles) { return persistent_grid(tiles, kAgGroupMx4RhtGrid); }, launch);
}

}  // namespace tsa
