// mx4_kernels.hip — the grouped all-gather from fp32 shards into MXFP4 rows
// (allred_plan_all_gather_shards_mxfp4, allred.h): OCP MX e2m1 elements, two per byte, and one E8M0
// scale byte per 32 elements — the narrowest operand of the block-scaled f8f6f4 MFMA — written where
// the all-gather holds every fp32 master value in a register anyway, rounded once from the fp32 value.
//
//   k_ag_group_mxfp4<P, RCEIL>   k_ag_group_mxfp8's walk (mx_kernels.hip) with a split of its own
//                                inside the tile: a tile's 256 floats become 128 element bytes and 8
//                                scale bytes, written to every rank's element row and scale row.
//
// The scaling is ONE fp32 multiply by a power of two with denormals kept (the build does not flush
// them), everything around it integer work: allred.h states every output bit as a function of the
// input bits and the tests compare whole buffers.
#include "device.hpp"
#include "group_batch.hpp"
#include "group_span.hpp"
#include "launch_util.hpp"
#include "mx_quant.hpp"

namespace tsa {
namespace {

constexpr int kMxGroupMax = ALLRED_MX_GROUP_MAX;   // buckets of one launch

// MxShard / MxShards (mx_quant.hpp): mx_kernels.hip's side table, entry for entry — the two calls take
// one allred_mx_bucket_f32 list.  GroupSpan carries the element rows: GroupBucket::ranks is the
// bucket's row 0 of BYTES and GroupBucket::stride its row stride in BYTES here.
static_assert(sizeof(GroupSpan) + sizeof(MxShards) < 4096, "kernel arguments stay below 4 KiB");
static_assert(kMxGroupMax <= kGroupMax, "GroupSpan's table holds a launch");

// ---------------------------------------------------------------------------
// k_ag_group_mxfp4<P, RCEIL>: k_ag_group_f32's walk — persistent grid, workgroup g takes tiles
// g + j * G, a forward-only wave-uniform cursor over GroupSpan, unconditional next-tile loads, two
// tiles per trip with registers of their own, tile 0 peeled.  A tile's source is wave-uniform: 1 KiB
// of floats in ONE block of the shard.  At four bits per element the MXFP8 split (8 floats per lane,
// a row from 32 lanes) would leave 4 bytes per lane, so the split is this file's own:
//   loads  lane c = lane % 16 loads floats 16 c .. 16 c + 15 as four 16-byte loads (all four lane
//          quarters q = lane / 16 and every storing wave load the same data), so an MX block — 32
//          consecutive floats — is one aligned PAIR of lanes;
//   A      the integer max of the lane's sixteen abs bit patterns, then ONE DPP quad_perm step
//          (lane ^ 1): both lanes of the pair hold the block's A;
//   scale  byte = max((A >> 23) - 2 + rceil, 0), rceil = RCEIL && (A & 0x7fffff) > 0x400000; that is
//          X + 127 with X clamped at -127; 2^-X = (254 - byte) << 23, a normal fp32 for every byte;
//   y      x * 2^-X, one v_mul_f32; v_med3_f32 with +-6; v_cvt_scalef32_pk_fp4_f32 at scale 1.0,
//          eight per lane: 16 floats become 8 bytes, element 2 i in the low nibble of byte i;
//   A >= 0x7f800000 (a NaN or Inf in the block): element bytes 0x00, scale byte 0xFF.
// Stores per wave and tile: the lane's 8 element bytes to its rows r = RPW w + 4 k + q, k < OPS, as
// 8-byte nontemporal stores — a row's 128 bytes from 16 lanes, contiguous, and FOUR rows per store
// instruction —, then the tile's 8 scale bytes — collected from lanes 0, 2 .. 14 by eight
// v_readlane_b32 into two wave-uniform words — by lane i < RPW to scale row RPW w + i as ONE plain
// 8-byte store (mx_kernels.hip's finding: streamed scale bytes cost 9.1 us against 5.5).
// Waves: a store instruction covers four rows, so W = min(4, P / 4) waves store RPW = P / W rows
// each; at P = 8 that is waves 0 and 1 with four rows each, and waves 2 and 3 leave before their
// first load — two full-width stores per tile rather than four half-masked ones, and half the
// redundant loads.  There is no barrier in the kernel.  Every row is written, the shard only read.
// vmcnt: k_ag_group_f32's argument with L = 4 loads and S = OPS + 1 stores per tile — issue order
// per wave L0 L1 S0 L2 S1 .., behind tile j's four loads come tile j - 1's stores and tile j + 1's
// four loads: OPS + 5 memory operations may stay in flight.  The ISA has vmcnt(OPS + 4) in the loop,
// twice, vmcnt(4) before the peeled tile 0 and vmcnt(OPS) before an odd last tile — the scale store
// stands behind a branch over exec (lane < RPW), so the compiler counts the path without it, as it
// does in k_ag_group_mxfp8: never too few waits, and in a wave that stored scales the oldest element
// store of tile j - 1 is waited for as well.  DESIGN.md §23.
// ---------------------------------------------------------------------------
template <int P, bool RCEIL>
__global__ __launch_bounds__(kBlock) void k_ag_group_mxfp4(GroupSpan span, MxShards shards) {
    constexpr int TV = 16, RPI = 4, W = P / RPI < 4 ? P / RPI : 4, RPW = P / W, OPS = RPW / RPI;
    static_assert(P % RPI == 0 && W >= 1 && RPW * W == P && OPS * RPI == RPW, "whole store instructions per wave");
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (w >= W) return;   // wave-uniform; P = 8 only
    const int c = lane % TV, q = lane / TV;
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
    auto store = [&](const Tile& t, const Src& x) {
        // as in k_ag_group_f32: the wait stands in front of the first use of the loaded floats; without
        // this barrier the scheduler lifts that use above the next tile's loads and the wait with it
        __builtin_amdgcn_sched_barrier(0);
        uint32_t A = umax(umax(amax4(x.a), amax4(x.b)), umax(amax4(x.c), amax4(x.d)));
        A = max_dpp<0xB1>(A);   // quad_perm [1, 0, 3, 2]: lane ^ 1
        const bool special = A >= 0x7f800000u;
        int sb = (int)(A >> 23) - 2;
        if constexpr (RCEIL) sb += (A & 0x7fffffu) > 0x400000u ? 1 : 0;
        sb = sb > 0 ? sb : 0;
        const float inv = __uint_as_float((uint32_t)(254 - sb) << 23);
        const uint32_t lo = cvt8_fp4(x.a, x.b, inv), hi = cvt8_fp4(x.c, x.d, inv);
        const u32x2 v = {special ? 0u : lo, special ? 0u : hi};
        const uint32_t s = special ? 0xffu : (uint32_t)sb;
        const u32x2 sc = {lane_of(s, 0) | lane_of(s, 2) << 8 | lane_of(s, 4) << 16 | lane_of(s, 6) << 24,
                          lane_of(s, 8) | lane_of(s, 10) << 8 | lane_of(s, 12) << 16 | lane_of(s, 14) << 24};
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
// k_ag_group_f32's grid cap, inherited and unmeasured here (tune pipe_grid caps it lower)
constexpr uint64_t kAgGroupMx4Grid = kMaxGrid;

}  // namespace

// A (checked: engine.cpp mx_check with the MXFP4 payload) list of whole-tile buckets — fp32 shard,
// nibble rows, scale rows — through k_ag_group_mxfp4, ALLRED_MX_GROUP_MAX buckets per launch in list
// order, enqueued when its last member is reached.  dry: nothing is launched and the number of
// launches is returned.
int launch_ag_group_mxfp4(const allred_mx_bucket_f32* buckets, int count, int total, bool rceil, bool dry, void* stream) {
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
            if (rceil) hipLaunchKernelGGL((k_ag_group_mxfp4<p(), true>), dim3(grid), dim3(kBlock), 0, st, span, shards);
            else hipLaunchKernelGGL((k_ag_group_mxfp4<p(), false>), dim3(grid), dim3(kBlock), 0, st, span, shards);
            trace_launch(grid, kBlock, "k_ag_group_mxfp4<%d, %s>", total, tf(rceil));
        });
        return found ? last_error() : ALLRED_ERR_UNSUPPORTED;
    };
    return group_batch<kMxGroupMax>(count, dry, shards, add, [](uint64_t tiles) { return persistent_grid(tiles, kAgGroupMx4Grid); },
                                    launch);
}

}  // namespace tsa
