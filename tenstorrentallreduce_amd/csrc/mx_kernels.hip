// mx_kernels.hip — the grouped all-gather from fp32 shards into MXFP8 rows
// (allred_plan_all_gather_shards_mxfp8, allred.h): what a block-scaled f8f6f4 MFMA consumer takes —
// OCP MX e4m3 element bytes and one E8M0 scale byte per 32 elements — written where the all-gather
// holds every fp32 master value in a register anyway, rounded once from the fp32 value.
//
//   k_ag_group_mxfp8<P, RCEIL>   k_ag_group_f32's walk and load / store loop (shard_f32_kernels.hip);
//                                a tile's 256 floats become 256 element bytes and 8 scale bytes,
//                                written to every rank's element row and scale row.
//
// The scaling is ONE fp32 multiply by a power of two with denormals kept (the build does not flush
// them), everything around it integer work: allred.h states every output bit as a function of the
// input bits and the tests compare whole buffers.
#include <type_traits>

#include "device.hpp"
#include "group_batch.hpp"
#include "group_span.hpp"
#include "launch_util.hpp"
#include "mx_quant.hpp"

namespace tsa {
namespace {

constexpr int kMxGroupMax = ALLRED_MX_GROUP_MAX;   // buckets of one launch

// The shard and the scale rows of every bucket of a launch: entry i for bucket i of the launch, block
// b of the bucket at shard + b * stride floats, rank r's scale row at scales + r * scale_stride bytes.
// GroupSpan carries the element rows: GroupBucket::ranks is the bucket's row 0 of BYTES and
// GroupBucket::stride its row stride in BYTES here (this file alone reads them).  Two more words per
// entry than GroupShardF32, hence 32 entries: 2064 + 1024 = 3088 bytes of kernel arguments.
struct MxShard {           // 32 bytes
    const float* shard;
    uint64_t stride;       // floats
    uint8_t* scales;
    uint64_t scale_stride; // bytes
};
struct MxShards {
    MxShard s[kMxGroupMax];   // entries past the last bucket: zero
};
static_assert(sizeof(MxShard) == 32 && sizeof(MxShards) == 32 * kMxGroupMax, "the kernel-argument layout");
static_assert(sizeof(GroupSpan) + sizeof(MxShards) < 4096, "kernel arguments stay below 4 KiB");
static_assert(kMxGroupMax <= kGroupMax, "GroupSpan's table holds a launch");
static_assert(sizeof(allred_mx_bucket_f32) == 56, "allred.h's layout");

// max_dpp, abs_bits, umax, cvt2 and lane_of: mx_quant.hpp, shared with adamw_mx_kernels.hip

// ---------------------------------------------------------------------------
// k_ag_group_mxfp8<P, RCEIL>: k_ag_group_f32's walk — persistent grid, workgroup g takes tiles
// g + j * G, a forward-only wave-uniform cursor over GroupSpan, unconditional next-tile loads, two
// tiles per trip with registers of their own, tile 0 peeled.  A tile's source is wave-uniform: 1 KiB
// of floats in ONE block of the shard.  Lane c = lane % 32 loads floats 8 c .. 8 c + 7 as two 16-byte
// loads (both lane halves q and all four waves load the same data), so an MX block — 32 consecutive
// floats — is one aligned QUAD of lanes:
//   A      the integer max of the lane's eight abs bit patterns, then two DPP quad_perm steps (lane ^
//          1, lane ^ 2): every lane of the quad holds the block's A;
//   scale  byte = max((A >> 23) - 8 + rceil, 0), rceil = RCEIL && (A & 0x7fffff) > 0x600000; that is
//          X + 127 with X clamped at -127; 2^-X = (254 - byte) << 23, a normal fp32 for every byte;
//   y      x * 2^-X, one v_mul_f32; v_med3_f32 with +-448; v_cvt_pk_fp8_f32, four per lane;
//   A >= 0x7f800000 (a NaN or Inf in the block): element bytes 0x7F, scale byte 0xFF.
// Stores per wave and tile: the lane's 8 element bytes to its rows r = RPW w + RPI k + q, k < OPS, as
// 8-byte stores (a row's 256 bytes from 32 lanes: contiguous), then the tile's 8 scale bytes —
// collected from lanes 0, 4 .. 28 by eight v_readlane_b32 into two wave-uniform words — by lane
// i < RPW to scale row RPW w + i as ONE 8-byte store, a plain one (the element stores are
// nontemporal).  Every row is written, the shard only read.
// vmcnt: k_ag_group_f32's argument with S = OPS + 1 stores per tile — issue order per wave
// L0 L1 S0 L2 S1 .., behind tile j's two loads come tile j - 1's stores and tile j + 1's two loads.
// What the ISA has: DESIGN.md §17.
// ---------------------------------------------------------------------------
template <int P, bool RCEIL>
__global__ __launch_bounds__(kBlock) void k_ag_group_mxfp8(GroupSpan span, MxShards shards) {
    constexpr int TV = 32, RPI = 2, RPW = P / 4, OPS = RPW / RPI;
    static_assert(OPS >= 1, "P >= 8");
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int c = lane % TV, q = lane / TV;
    struct Tile {
        uint8_t* rows;          // the bucket's element row 0
        uint64_t row_stride;    // bytes
        uint8_t* scales;        // the bucket's scale row 0
        uint64_t scale_stride;  // bytes
        uint64_t local;         // the tile's index inside a rank row: 256 element bytes, 8 scale bytes each
        const f32x4* src;       // the source tile's first 16 bytes
    };
    uint32_t cursor = 0;   // wave-uniform: it depends on blockIdx and j only
    auto locate = [&](int j) {
        const GroupTile gt = group_span_at(span, group_span_tile(span, blockIdx.x, (uint32_t)j), cursor);
        const GroupBucket& e = span.b[gt.bucket];
        const MxShard& sh = shards.s[gt.bucket];
        return Tile{reinterpret_cast<uint8_t*>(e.ranks), e.stride, sh.scales, sh.scale_stride, (uint64_t)gt.local,
                    reinterpret_cast<const f32x4*>(sh.shard + (uint64_t)gt.block * sh.stride) + (uint64_t)gt.rem * (2 * TV)};
    };
    const int mine = (int)group_span_mine(span, blockIdx.x);
    if (mine <= 0) return;
    const int last = mine - 1;
    struct Src {
        f32x4 a, b;
    };
    auto load = [&](const Tile& t) { return Src{t.src[2 * c], t.src[2 * c + 1]}; };
    auto store = [&](const Tile& t, const Src& x) {
        // as in k_ag_group_f32: the wait stands in front of the first use of the loaded floats; without
        // this barrier the scheduler lifts that use above the next tile's loads and the wait with it
        __builtin_amdgcn_sched_barrier(0);
        uint32_t A = umax(umax(umax(abs_bits(x.a[0]), abs_bits(x.a[1])), umax(abs_bits(x.a[2]), abs_bits(x.a[3]))),
                          umax(umax(abs_bits(x.b[0]), abs_bits(x.b[1])), umax(abs_bits(x.b[2]), abs_bits(x.b[3]))));
        A = max_dpp<0xB1>(A);   // quad_perm [1, 0, 3, 2]: lane ^ 1
        A = max_dpp<0x4E>(A);   // quad_perm [2, 3, 0, 1]: lane ^ 2
        const bool special = A >= 0x7f800000u;
        int sb = (int)(A >> 23) - 8;
        if constexpr (RCEIL) sb += (A & 0x7fffffu) > 0x600000u ? 1 : 0;
        sb = sb > 0 ? sb : 0;
        const float inv = __uint_as_float((uint32_t)(254 - sb) << 23);
        uint32_t lo = cvt2<false>(x.a[0] * inv, x.a[1] * inv, 0u);
        lo = cvt2<true>(x.a[2] * inv, x.a[3] * inv, lo);
        uint32_t hi = cvt2<false>(x.b[0] * inv, x.b[1] * inv, 0u);
        hi = cvt2<true>(x.b[2] * inv, x.b[3] * inv, hi);
        const u32x2 v = {special ? 0x7f7f7f7fu : lo, special ? 0x7f7f7f7fu : hi};
        const uint32_t s = special ? 0xffu : (uint32_t)sb;
        const u32x2 sc = {lane_of(s, 0) | lane_of(s, 4) << 8 | lane_of(s, 8) << 16 | lane_of(s, 12) << 24,
                          lane_of(s, 16) | lane_of(s, 20) << 8 | lane_of(s, 24) << 16 | lane_of(s, 28) << 24};
#pragma unroll
        for (int k = 0; k < OPS; ++k) {
            const uint32_t r = (uint32_t)(RPW * w + RPI * k + q);
            __builtin_nontemporal_store(v, reinterpret_cast<u32x2*>(t.rows + (uint64_t)r * t.row_stride + t.local * 256) + c);
        }
        // NOT nontemporal: 8 bytes are a sixteenth of a line, and the neighbouring tiles' scale bytes of the row come
        // from other workgroups — written back from the L2 they leave as whole lines (streamed: 9.1 us against 5.5)
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
constexpr uint64_t kAgGroupMxGrid = kMaxGrid;

}  // namespace

// A (checked: engine.cpp mx_check) list of whole-tile buckets — fp32 shard, element rows, scale rows —
// through k_ag_group_mxfp8, ALLRED_MX_GROUP_MAX buckets per launch in list order, enqueued when its
// last member is reached.  dry: nothing is launched and the number of launches is returned.
int launch_ag_group_mxfp8(const allred_mx_bucket_f32* buckets, int count, int total, bool rceil, bool dry, void* stream) {
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
            if (rceil) hipLaunchKernelGGL((k_ag_group_mxfp8<p(), true>), dim3(grid), dim3(kBlock), 0, st, span, shards);
            else hipLaunchKernelGGL((k_ag_group_mxfp8<p(), false>), dim3(grid), dim3(kBlock), 0, st, span, shards);
            trace_launch(grid, kBlock, "k_ag_group_mxfp8<%d, %s>", total, tf(rceil));
        });
        return found ? last_error() : ALLRED_ERR_UNSUPPORTED;
    };
    return group_batch<kMxGroupMax>(count, dry, shards, add, [](uint64_t tiles) { return persistent_grid(tiles, kAgGroupMxGrid); },
                                    launch);
}

}  // namespace tsa
