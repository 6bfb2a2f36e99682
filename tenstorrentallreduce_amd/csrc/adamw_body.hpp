// adamw_body.hpp — the ONE AdamW body of the fp32-shard calls, adamw_ag, with its kernel-argument
// tables: included by adamw_kernels.hip (k_adamw_ag_group_f32, k_adamw_ag_groups_f32: bf16 rank rows)
// adamw_mx_kernels.hip (k_adamw_ag_mxfp8: MXFP8 element rows and E8M0 scale rows) and
// adamw_mx4_kernels.hip (k_adamw_ag_mxfp4: MXFP4 nibble rows and E8M0 scale rows) and adamw_mx4_rht_kernels.hip
// (k_adamw_ag_mxfp4_rht: the same rows from a ROTATED copy of p') and adamw_mx4_sr_kernels.hip
// (k_adamw_ag_mxfp4_sr: the same rows rounded STOCHASTICALLY, rotated or not).  The output
// stage — what wave 0 puts into the LDS slot for p' and what every wave stores from it — is a
// compile-time choice (AdamwOut); everything else is the same code in every instance.
#pragma once

#include <type_traits>

#include "device.hpp"
#include "group_span.hpp"
#include "mx_quant.hpp"
#include "mx_rht.hpp"
#include "mx_sr.hpp"

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
//   kOutMx4Floor MXFP4: 2 bytes of e2m1 nibbles per lane and the tile's 8 E8M0 bytes, a 144-byte slot,
//   kOutMx4Rceil 8-byte row stores in k_ag_group_mxfp4's split (four rows per store instruction) and
//                one 8-byte scale store per rank row.
//   kOutMx4RhtFloor  the MXFP4 stage on a copy of p' that went through the random Hadamard rotation of
//   kOutMx4RhtRceil  mx_rht.hpp first; slot, barrier and stores are kOutMx4Floor's / kOutMx4Rceil's.
//   kOutMx4SrFloor / kOutMx4SrRceil        the MXFP4 stage with mx_sr.hpp's stochastic rounding in place of the
//   kOutMx4SrRhtFloor / kOutMx4SrRhtRceil  RNE conversion, on p' or on its rotated copy; slot, barrier and stores
//                                          are kOutMx4Floor's / kOutMx4Rceil's.
enum AdamwOut {
    kOutBf16 = 0, kOutMxFloor, kOutMxRceil, kOutMx4Floor, kOutMx4Rceil, kOutMx4RhtFloor, kOutMx4RhtRceil,
    kOutMx4SrFloor, kOutMx4SrRceil, kOutMx4SrRhtFloor, kOutMx4SrRhtRceil
};
// The scale rows of every bucket of an MXFP8 launch: rank r's scale row at scales + r * scale_stride
// bytes.  GroupSpan then carries the ELEMENT rows in bytes (GroupBucket::ranks row 0, ::stride the
// row stride in bytes), as in mx_kernels.hip; the MXFP4 stage takes the same table.  The bf16 kernels
// hand adamw_ag an AdamwNoScales.
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
// bytes at byte 256 and 8 bytes of padding (272: a multiple of 16, so that both slots are 16-byte aligned),
// or 64 lanes' 2 nibble bytes, the 8 scale bytes at byte 128 and 8 bytes of padding (144, likewise)
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
template <>
struct AdamwSlot<kOutMx4Floor> {
    typedef uint32_t type[2][36];
};
template <>
struct AdamwSlot<kOutMx4Rceil> {
    typedef uint32_t type[2][36];
};
template <>
struct AdamwSlot<kOutMx4RhtFloor> {
    typedef uint32_t type[2][36];
};
template <>
struct AdamwSlot<kOutMx4RhtRceil> {
    typedef uint32_t type[2][36];
};
template <>
struct AdamwSlot<kOutMx4SrFloor> : AdamwSlot<kOutMx4Floor> {};
template <>
struct AdamwSlot<kOutMx4SrRceil> : AdamwSlot<kOutMx4Floor> {};
template <>
struct AdamwSlot<kOutMx4SrRhtFloor> : AdamwSlot<kOutMx4Floor> {};
template <>
struct AdamwSlot<kOutMx4SrRhtRceil> : AdamwSlot<kOutMx4Floor> {};

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

// Wave 0, all 64 lanes active.  max_norm: the one set's, or hypey.p[0]'s, wave-uniform; x =
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
// OUT == kOutMx4Floor / kOutMx4Rceil (MXFP4 rows), allred.h's rule for allred_plan_all_gather_shards_mxfp4
// applied to p' in wave 0's registers.  In front of the barrier the stage is the MXFP8 one with other
// constants — the same eight-lane block and three DPP steps, the scale byte (A >> 23) - 2 (RCEIL: + 1
// above mantissa 0x400000), one v_mul_f32 per element, v_med3_f32 with +-6 and two
// v_cvt_scalef32_pk_fp4_f32 at scale 1.0 (mx_quant.hpp cvt2_fp4<0>, <1>): lane l's four nibbles are 16
// bits, element 4 l in bits 3:0; 0x0000 and scale 0xFF for a block with a NaN or Inf.
//   slot (144 bytes): bytes 2 l, 2 l + 1 = lane l's nibbles, ONE ds_write_b16 per lane under the full exec
//   mask (the other form — a fourth DPP step that hands the odd lane's 16 bits to the even lane, which
//   writes a dword — costs a DPP move, a shift-or and an exec change for the same 128 bytes; neither is
//   measured); bytes 128 .. 135 = the tile's eight scale bytes, byte writes from lanes 0, 8 .. 56 as
//   above; bytes 136 .. 143 padding, never read.
//   behind the barrier the split is k_ag_group_mxfp4's, not the one above: c = lane % 16, q = lane / 16,
//   a wave reads column c's 8 bytes and stores them nontemporally to rows RPW w + 4 k + q at byte
//   local * 128 + 8 c — a row's 128 bytes are one run from 16 lanes and one store instruction covers
//   FOUR rows —, so W = min(4, P / 4) waves store RPW = P / W rows each; lanes < RPW of a storing wave
//   write the scale bytes with a PLAIN store as above.
//   P = 8: W = 2, waves 2 and 3 have no rows.  k_ag_group_mxfp4 lets them return before their first
//   load; it has no barrier.  Here NO wave leaves before the workgroup's last barrier: waves 2 and 3
//   walk every tile and arrive at every lds_barrier, and skip the LDS read and the stores only (w < W, a
//   scalar branch).  The one early return stays the workgroup-uniform `mine <= 0`.  The slot-rotation
//   argument above therefore carries over unchanged: a wave without rows has no LDS read to protect,
//   and a wave with rows has passed the barrier of tile j + 1 behind its read of tile j as before.
// OUT == kOutMx4RhtFloor / kOutMx4RhtRceil: allred.h's rotation (mx_rht.hpp) on a COPY of p' in wave 0's
// registers, in front of the MXFP4 stage above, which then takes the copy; y.p, and with it the param plane,
// is untouched.  Lane l holds elements 4 (l & 7) .. 4 (l & 7) + 3 of its eight-lane block:
//   signs   four v_xor_b32 with the lane's masks (bits 4 (l & 7) .. + 3 of sign_mask at bit 31: four
//           registers filled once, in front of the tile loop);
//   h = 1, 2   eight v_add_f32 / v_sub_f32 on the lane's own four registers;
//   h = 4   lane ^ 1, quad_perm [1, 0, 3, 2];   h = 8   lane ^ 2, quad_perm [2, 3, 0, 1]: per register one
//           v_add_f32 with a DPP operand, own's sign flipped where the lane holds the upper half of the pair;
//   h = 16  lane ^ 4.  gfx9 DPP has no xor form for it: row_half_mirror (lane 7 - i of the eight) composed
//           with quad_perm [3, 2, 1, 0] (lane 3 - i of the quad) is i ^ 7 ^ 3 = i ^ 4 — a v_mov_b32 with DPP
//           and the v_add_f32 with DPP, eight VALU operations for the four registers.  ds_swizzle_b32 and
//           ds_bpermute_b32 do it in one operation each, but through the LDS queue: their results would be
//           waited for with lgkmcnt next to the slot writes and the scalar loads of the walk, in a wave that is
//           the workgroup's critical path in front of the barrier; the DPP pair stays in the VALU.
//   2^-2.5  four v_mul_f32.
// The stages and operands are in the rule's order, so the bits are k_ag_group_mxfp4_rht's.
// OUT == kOutMx4Sr*: allred.h's stochastic rounding (mx_sr.hpp) in place of the RNE conversion, behind the
// rotation where the mode has one.  Wave 0's lane l holds elements 4 l .. 4 l + 3 of the tile, elements
// 256 tile + 4 l .. of the gathered row: ONE Philox call, counter g = 64 tile + l, the bucket's index in the
// caller's list (first_bucket + its index in the launch) and the step; the key and the step are read from sr
// once, in front of the tile loop.  The words depend on indices alone: they are generated behind the issue of
// the NEXT tile's loads and in front of the first use of this tile's planes (two sched_barriers hold them
// there), about 85 integer operations under the loads' round trip.  On a skipped step y.p is p and the rows
// are its SR quantisation.
// ---------------------------------------------------------------------------
template <int P, bool ZERO, bool GROUPS, AdamwOut OUT = kOutBf16, class Scales = AdamwNoScales>
__device__ __forceinline__ void adamw_ag(const GroupSpan& span, const AdamwGroup& planes, const AdamwGroupOf& group_of,
                                         const allred_adamw_hyper* __restrict__ hyper, int ngroups,
                                         const float* __restrict__ norm_sq, float* info, const Scales& scale_rows = Scales{},
                                         uint32_t sign_mask = 0, const allred_mx_sr_state* __restrict__ sr = nullptr,
                                         uint32_t first_bucket = 0) {
    constexpr bool SR = OUT == kOutMx4SrFloor || OUT == kOutMx4SrRceil || OUT == kOutMx4SrRhtFloor || OUT == kOutMx4SrRhtRceil;
    // the rotation in front of the MXFP4 stage
    constexpr bool RHT = OUT == kOutMx4RhtFloor || OUT == kOutMx4RhtRceil || OUT == kOutMx4SrRhtFloor || OUT == kOutMx4SrRhtRceil;
    constexpr bool MX4 = OUT == kOutMx4Floor || OUT == kOutMx4Rceil || RHT || SR;
    constexpr bool MX = OUT != kOutBf16;   // any MX row format: element rows in bytes, and scale rows
    constexpr bool RCEIL = OUT == kOutMxRceil || OUT == kOutMx4Rceil || OUT == kOutMx4RhtRceil || OUT == kOutMx4SrRceil ||
                           OUT == kOutMx4SrRhtRceil;
    // TV: lanes of a row's run; RPI: rows per store instruction; W: waves with rows (MX4 at P = 8: two)
    constexpr int TV = MX4 ? 16 : 32, RPI = 64 / TV, W = (MX4 && P / RPI < 4) ? P / RPI : 4, RPW = P / W, OPS = RPW / RPI;
    constexpr int SC = MX4 ? 32 : 64;   // the slot's dword that holds the tile's scale bytes
    static_assert(OPS >= 1 && RPW * W == P && OPS * RPI == RPW, "P >= 8, whole store instructions per wave");
    static_assert(std::is_same<Scales, AdamwMxScales>::value == MX, "the scale rows come with the MXFP8 output stage");
    __shared__ __attribute__((aligned(16))) typename AdamwSlot<OUT>::type slot;
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int c = lane % TV, q = lane / TV;
    // RHT only; filled under if constexpr: computed in every form, and dead there, it moved the MX forms' registers
    RhtLane<4> rl;
    if constexpr (RHT) rl = rht_lane<4>(sign_mask, lane & 7);
    // SR only, under if constexpr for the same reason: the key and the step, and the tile's four words
    SrCall sr_state;
    SrWords rnd;
    if constexpr (SR) sr_state = sr_call(sr);
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
                    (uint64_t)gt.block * planes.s[gt.bucket].stride + (uint64_t)gt.rem * 256, gt.bucket, group_at(gt.bucket)};
    };
    const int mine = (int)group_span_mine(span, blockIdx.x);
    if (mine <= 0) return;   // the whole workgroup: no barrier is left waiting
    const int last = mine - 1;
    auto rows = [&](const Tile& t, int j) {
        if constexpr (MX) {
            if (W < 4 && w >= W) return;   // MX4 at P = 8: a wave without rows, behind the barrier (scalar branch)
            const uint2 v = reinterpret_cast<const uint2*>(&slot[j & 1][0])[c];
            const uint2 sc = reinterpret_cast<const uint2*>(&slot[j & 1][SC])[0];
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
            // RHT: the stage below quantises y.p, so the rotated values stand in y.p while it runs and p' is put
            // back behind it (register renaming, no instruction); written this way the other forms' code, and
            // with it their ISA, is untouched — with a named copy in front of the stage their registers moved
            f32x4 unrotated{};
            if constexpr (RHT) {
                unrotated = y.p;
                float x[4] = {y.p[0], y.p[1], y.p[2], y.p[3]};
                rht_own(x, rl);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    x[e] = rht_pair(dpp_f<0xB1>(x[e]), x[e], rl.upper[0]);                  // h = 4: lane ^ 1
                    x[e] = rht_pair(dpp_f<0x4E>(x[e]), x[e], rl.upper[1]);                  // h = 8: lane ^ 2
                    x[e] = rht_pair(dpp_f<0x1B>(dpp_f<0x141>(x[e])), x[e], rl.upper[2]);    // h = 16: lane ^ 4
                    y.p[e] = rht_norm(x[e]);
                }
            }
            uint32_t A = umax(umax(abs_bits(y.p[0]), abs_bits(y.p[1])), umax(abs_bits(y.p[2]), abs_bits(y.p[3])));
            A = max_dpp<0xB1>(A);    // quad_perm [1, 0, 3, 2]: lane ^ 1
            A = max_dpp<0x4E>(A);    // quad_perm [2, 3, 0, 1]: lane ^ 2
            A = max_dpp<0x141>(A);   // row_half_mirror: a lane of the other quad of the 8
            const bool special = A >= 0x7f800000u;
            int sb = (int)(A >> 23) - (MX4 ? 2 : 8);   // emax of e2m1 is 2, of e4m3 8
            if constexpr (RCEIL) sb += (A & 0x7fffffu) > (MX4 ? 0x400000u : 0x600000u) ? 1 : 0;
            sb = sb > 0 ? sb : 0;
            const float inv = __uint_as_float((uint32_t)(254 - sb) << 23);
            if constexpr (SR) {
                const uint32_t e = sr4_fp4(y.p, inv, rnd);
                reinterpret_cast<uint16_t*>(&slot[j & 1][0])[lane] = (uint16_t)(special ? 0u : e);
            } else if constexpr (MX4) {
                uint32_t e = cvt2_fp4<0>(y.p[0] * inv, y.p[1] * inv, 0u);
                e = cvt2_fp4<1>(y.p[2] * inv, y.p[3] * inv, e);   // bits 31:16 stay zero
                reinterpret_cast<uint16_t*>(&slot[j & 1][0])[lane] = (uint16_t)(special ? 0u : e);
            } else {
                uint32_t e = cvt2<false>(y.p[0] * inv, y.p[1] * inv, 0u);
                e = cvt2<true>(y.p[2] * inv, y.p[3] * inv, e);
                slot[j & 1][lane] = special ? 0x7f7f7f7fu : e;
            }
            if ((lane & 7) == 0) reinterpret_cast<uint8_t*>(&slot[j & 1][SC])[lane >> 3] = (uint8_t)(special ? 0xffu : (uint32_t)sb);
            if constexpr (RHT) y.p = unrotated;
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
            if constexpr (SR) {
                // cur.v0 / TV: the tile's index in the rank row; 64 times it has no low six bits, so the lane adds without a carry
                const uint64_t tile = cur.v0 / TV;
                __builtin_amdgcn_sched_barrier(0);   // the next tile's loads are out
                rnd = sr_words(sr_state, ((uint32_t)tile << 6) + (uint32_t)lane, (uint32_t)(tile >> 26), first_bucket + cur.bucket);
                __builtin_amdgcn_sched_barrier(0);   // the wait for this tile's planes stands behind the words
            }
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
